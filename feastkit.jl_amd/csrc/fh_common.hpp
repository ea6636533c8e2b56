// fh_common.hpp -- shared types for libfeasthip (gfx950 / CDNA4 only).
//
// Internal block-vector layout ("panel"): an N x m complex block is stored ROW-MAJOR with a
// padded row length ld in {16,32,64} c128 elements, so one row of a 64-column block is one
// contiguous 1 KiB line = one wave-wide 16 B/lane access.  Lane <-> column, so every
// per-column scalar of the batched Krylov solver (alpha_c, omega_c, ...) lives in the lane
// that owns column c, and a gathered SpMM row read is a single coalesced wave access.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include <map>

#include "fh_factor_cache.hpp"

struct __attribute__((aligned(16))) cplx { double x, y; };

__host__ __device__ inline cplx cmake(double a, double b) { cplx r; r.x = a; r.y = b; return r; }
__host__ __device__ inline cplx cadd(cplx a, cplx b) { return cmake(a.x + b.x, a.y + b.y); }
__host__ __device__ inline cplx csub(cplx a, cplx b) { return cmake(a.x - b.x, a.y - b.y); }
__host__ __device__ inline cplx cmul(cplx a, cplx b) { return cmake(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__host__ __device__ inline cplx cmulc(cplx a, cplx b) { /* conj(a)*b */ return cmake(a.x * b.x + a.y * b.y, a.x * b.y - a.y * b.x); }
__host__ __device__ inline cplx cscale(cplx a, double s) { return cmake(a.x * s, a.y * s); }
__host__ __device__ inline cplx cconj(cplx a) { return cmake(a.x, -a.y); }
__host__ __device__ inline double cabs2(cplx a) { return a.x * a.x + a.y * a.y; }
__host__ __device__ inline cplx cdiv(cplx a, cplx b) {
    double d = b.x * b.x + b.y * b.y;
    return cmake((a.x * b.x + a.y * b.y) / d, (a.y * b.x - a.x * b.y) / d);
}
// acc += a*b
__host__ __device__ inline void cfma(cplx& acc, cplx a, cplx b) {
    acc.x += a.x * b.x - a.y * b.y;
    acc.y += a.x * b.y + a.y * b.x;
}
// matrix value (real or complex) times complex
__host__ __device__ inline cplx vmul(double a, cplx b) { return cmake(a * b.x, a * b.y); }
__host__ __device__ inline cplx vmul(cplx a, cplx b) { return cmul(a, b); }

// ---- single-precision complex for the mixed-precision Krylov correction solves -------------
struct __attribute__((aligned(8))) cplxf { float x, y; };
__host__ __device__ inline cplxf cmakef(float a, float b) { cplxf r; r.x = a; r.y = b; return r; }
__host__ __device__ inline cplxf cadd(cplxf a, cplxf b) { return cmakef(a.x + b.x, a.y + b.y); }
__host__ __device__ inline cplxf csub(cplxf a, cplxf b) { return cmakef(a.x - b.x, a.y - b.y); }
__host__ __device__ inline cplxf cmul(cplxf a, cplxf b) { return cmakef(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__host__ __device__ inline void cfma(cplxf& acc, cplxf a, cplxf b) {
    acc.x += a.x * b.x - a.y * b.y;
    acc.y += a.x * b.y + a.y * b.x;
}
__host__ __device__ inline cplxf vmul(double a, cplxf b) { float f = (float)a; return cmakef(f * b.x, f * b.y); }
__host__ __device__ inline cplxf vmul(cplx a, cplxf b) { return cmul(cmakef((float)a.x, (float)a.y), b); }
// conversions: to_d widens to double complex (all reductions run in fp64); cvt<CT> narrows
__host__ __device__ inline cplx to_d(cplx a) { return a; }
__host__ __device__ inline cplx to_d(cplxf a) { return cmake((double)a.x, (double)a.y); }
template <typename CT> __host__ __device__ inline CT cvt(cplx a);
template <> __host__ __device__ inline cplx cvt<cplx>(cplx a) { return a; }
template <> __host__ __device__ inline cplxf cvt<cplxf>(cplx a) { return cmakef((float)a.x, (float)a.y); }

#define FH_MAX_LD 64

#define FH_CHECK(expr)                                                                      \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) {                                                             \
            h->last_error = std::string(#expr) + ": " + hipGetErrorString(_e);              \
            return (_e == hipErrorOutOfMemory) ? 6 : 7;                                     \
        }                                                                                   \
    } while (0)

// ---- profiling of kernel classes with HIP events on the handle's stream -----------------
struct fh_prof_class {
    double total_ms = 0.0;
    int64_t launches = 0;
};

struct fh_event_pair {
    hipEvent_t a, b;
    std::string cls;
};

// ---- device CSR (union pattern of A and B) ---------------------------------------------
struct fh_csr {
    int64_t N = 0, nnz = 0;
    int is_complex = 0;      // values are double (0) or cplx (1)
    int b_identity = 0;      // no B values: B = I
    int* rowptr = nullptr;   // N+1
    int* col = nullptr;      // nnz
    void* aval = nullptr;    // nnz x (double|cplx), A on the union pattern
    void* bval = nullptr;    // nnz x (double|cplx), B on the union pattern (null if identity)
    // rows padded to whole chunks of 8 nonzeros for the row-per-wave SpMM (real values only): chunk range of row i is
    // [rp8[i], rp8[i+1]); col8 / a8 / b8 hold 8 entries per chunk, padding = (own row, 0.0, 0.0)
    int* rp8 = nullptr; int* col8 = nullptr; double* a8 = nullptr; double* b8 = nullptr;
    int* perm = nullptr;     // N: row/column renumbering applied at ingest, perm[internal] = caller's index (null: none)
    // row blocks of the renumbered matrix (LDS-window SpMM): block b = rows [blk_start[b], blk_start[b+1]) (<= FH_SPMM_R),
    // ext_idx[ext_ptr[b] .. ext_ptr[b+1]) = the distinct rows OUTSIDE the block its nonzeros touch (<= FH_SPMM_EXT kept),
    // lcol[k] = LDS slot of nonzero k: row - blk_start[b] inside the block, FH_SPMM_R + position in the block's ext list
    // outside, 0xFFFF when the ext list was full (the kernel then gathers col[k] from global memory)
    int nblk = 0;
    int* blk_start = nullptr;
    int* ext_ptr = nullptr;
    int* ext_idx = nullptr;
    unsigned short* lcol = nullptr;
};
#define FH_SPMM_R 128        // rows per block of the ingest renumbering / the LDS-window SpMM
#define FH_SPMM_EXT 160      // outside rows a block stages next to its own: (128 + 160) x 256 B = 72 KiB of LDS, two blocks per CU

struct fh_dense {
    int64_t N = 0;
    int is_complex = 0;
    int b_identity = 0;
    void* A = nullptr;       // N x N column-major, double or cplx
    void* B = nullptr;
};

// Matrix polynomial P(lambda) = A_0 + lambda A_1 + ... + lambda^d A_d (feasthip_set_polynomial, fh_poly.hip): the d + 1
// coefficients, N x N column-major, all double or all cplx; fro[k] = ||A_k||_F.  N and is_complex live in fh_dense.
// sparse (feasthip_set_polynomial_csr): the coefficients share ONE CSR pattern that holds the whole diagonal -- device rowptr /
// col in feasthip_ctx::csr (N, nnz, is_complex; aval and bval stay null, b_identity 0), the host copy in host_rowptr / host_col
// in the caller's order -- and coef[k] is the array of nnz values of A_k on that pattern, explicit zeros included.
// terms (feasthip_set_terms / feasthip_set_terms_csr): the same storage read as the split form T(lambda) = sum_k f_k(lambda) A_k
// of degree + 1 terms, f_k arbitrary scalar functions that only the caller evaluates -- fnode[e * (degree + 1) + k] = f_k(z_e) on
// the contour fnode_z (feasthip_nep_set_node_values); the feasthip_nep_* entry points take the other scalars as tables.
#define FH_POLY_MAX_DEGREE 8
struct fh_poly {
    int degree = 0;
    int sparse = 0;
    int terms = 0;
    void* coef[FH_POLY_MAX_DEGREE + 1] = {};
    double fro[FH_POLY_MAX_DEGREE + 1] = {};
    std::vector<cplx> fnode, fnode_z;
};
// the coefficient pointers as a kernel argument (fh_poly_coef_ptrs below fills it; null past the degree)
struct fh_poly_ptrs { const void* c[FH_POLY_MAX_DEGREE + 1]; };

// A coefficient value (real or complex storage) as a complex number, and sum_{k <= d} coef(k) z^k by Horner: fully unrolled
// from the compile-time top index TOP down, so a register array of TOP + 1 entries behind coef stays in registers and no
// guarded-out step indexes past it (d <= TOP).
__device__ inline cplx poly_val(cplx v) { return v; }
__device__ inline cplx poly_val(double v) { return cmake(v, 0.0); }
template <int TOP, typename F> __device__ __forceinline__ cplx fh_horner(int d, cplx z, F&& coef) {
    cplx v = cmake(0, 0);
#pragma unroll
    for (int k = TOP; k >= 0; --k)
        if (k <= d) v = cadd(cmul(v, z), coef(k));
    return v;
}
// The table form of the same combination: sum_{k < nt} f[k] coef(k) in ascending k, for the split form of a term handle
// (fh_poly::terms), whose scalars come from a table instead of the powers of z.  f: nt values, uniform or per lane.
template <int TOP, typename FS, typename F> __device__ __forceinline__ cplx fh_term_sum(int nt, FS&& f, F&& coef) {
    cplx v = cmake(0, 0);
#pragma unroll
    for (int k = 0; k <= TOP; ++k)
        if (k < nt) cfma(v, f(k), coef(k));
    return v;
}

// Operator handle (FH_KIND_OPERATOR, feasthip_set_operator): the products A X and B X are the caller's callback
// (feasthip_apply_fn of include/feasthip.h) on whole node batches of panels; fh_operator.hip turns them into what the
// drivers read.  N, b_identity and is_complex live in fh_dense.  failed: a callback of the running entry point returned
// non-zero -- no further product is made or launched in that call (cleared by fh_check_problem at the next one).
typedef int (*fh_apply_fn)(void* user, int which, int nodes, int ld, int64_t N, const void* dX, int64_t x_node_stride, void* dY,
                           int64_t y_node_stride, void* stream);
struct fh_operator {
    fh_apply_fn apply = nullptr;
    void* user = nullptr;
    int symmetric = 0;
    int failed = 0;
};

// Term-operator handle (FH_KIND_TERM_OPERATOR, feasthip_set_term_operator, fh_termop.hip): the split form of a term handle whose
// products A_k X are the caller's callback (fh_operator::apply with which = k).  N and is_complex live in fh_dense, the term
// count (degree + 1), the node table and the norms (fro) in fh_poly with terms = 1, the callback in fh_operator.
// shift_dev / shift_z: the node shifts fh_upload_shift_coefs sent last and where -- the Krylov drivers hand the operator their
// coefB array, and the host finds the rows of the node table by these z without reading them back.  col_terms: bit k set when
// row k of the column table poly_upload_cols sent last has a non-zero entry.
struct fh_termop {
    unsigned identity_mask = 0;
    size_t scratch_bytes = 0;
    int norms_set = 0;
    const cplx* shift_dev = nullptr;
    std::vector<cplx> shift_z;
    unsigned col_terms = 0;
};

// what every refusal of a term-operator handle ends with, and the reason feasthip_set_solver and the solving entry points
// refuse a solver kind on it (null: the kind is taken; fh_problem.hip)
#define FH_TERMOP_TAKES "a term-operator handle (feasthip_set_term_operator) takes the Krylov solvers FEASTHIP_SOLVER_BICGSTAB, _GMRES or (FEASTHIP_OP_SYMMETRIC) _COCG"
struct feasthip_ctx;
const char* fh_termop_solver_why(const feasthip_ctx* h, int kind, int factor_precision);

// Per-(node,column) Krylov scalars, struct of arrays; each array is [nodes][ld].
struct fh_krylov_scalars {
    cplx* rho = nullptr;
    cplx* alpha = nullptr;
    cplx* omega = nullptr;
    cplx* beta = nullptr;
    double* r0norm = nullptr;
    double* target = nullptr;
    double* rnorm = nullptr;
    int* active = nullptr;    // 1 while the column is still iterating
    int* iters = nullptr;     // iterations performed by the column
    int* status = nullptr;    // 0 converged, 5 not converged, 8 breakdown
    int* node_active = nullptr;  // [nodes]: number of active columns of the node
    int* accum = nullptr;        // sum mode: column took an alpha step in this iteration (set by fin_alpha)
    int* node_accum = nullptr;   // [nodes]: any column of the node did
};

struct fh_comm;   // fh_comm.hip: RCCL (or shared-device) communicator attached by feasthip_comm_init_rank

// What problem a handle holds (feasthip_ctx::kind).  POLYNOMIAL: a matrix polynomial, dense or (poly.sparse) CSR, for the
// feasthip_poly_* entry points only; OPERATOR: Krylov solvers only; TERM_OPERATOR: the feasthip_nep_* entry points, Krylov
// solvers only.
enum fh_kind { FH_KIND_NONE = 0, FH_KIND_DENSE = 1, FH_KIND_CSR = 2, FH_KIND_POLYNOMIAL = 3, FH_KIND_OPERATOR = 4, FH_KIND_TERM_OPERATOR = 5 };

// Plan of the sparse direct solver (feasthip_ctx::band_plan, made by fh_banded.hip: band_make_plan): NARROW, a band of at most
// 64 diagonals in stored order (one-workgroup elimination); BAND, the blocked band LU on the dense kernels after reverse
// Cuthill-McKee; MF, the multifrontal LU on a nested-dissection tree.  The values are what the "plan %d" messages print.
enum fh_direct_plan { FH_PLAN_NONE = 0, FH_PLAN_NARROW = 1, FH_PLAN_BAND = 2, FH_PLAN_MF = 3 };

struct feasthip_ctx {
    int device = 0;
    fh_comm* comm = nullptr;
    int64_t col_block_lo = 0, col_block_hi = -1;   // feasthip_set_column_block: columns this rank sweeps (hi < 0: all)
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::string last_error;

    // problem
    fh_kind kind = FH_KIND_NONE;
    fh_poly poly;
    fh_operator op;
    fh_termop top;
    fh_csr csr;
    // conjugate transpose of `csr` (A^H, B^H on the transposed union pattern, internal numbering; rowptr / col / aval / bval only):
    // built at the first adjoint product of a CSR problem (fh_problem.hip: fh_adjoint_csr_ensure), freed with the problem
    fh_csr csr_adj;
    fh_dense dense;

    // contour
    std::vector<cplx> zne, wne;
    double weight_scale = 2.0;
    int real_projection = 0;
    int adjoint = 0;              // feasthip_set_adjoint: sweeps, solves, products and residuals act with the conjugate transposes
    int require_adjoint = 0;      // feasthip_require_adjoint: the direct plan of a CSR problem must have an adjoint substitution (the multifrontal one)
    int node_first = 0, node_count = 0;
    std::vector<int> node_ids;      // local node -> contour index (set by range or list)
    std::vector<int> node_kinds;    // feasthip_set_node_solver: per CONTOUR node, 0 = the handle's solver, FEASTHIP_SOLVER_BANDED = direct; empty = none

    // solver options
    int solver = 1;
    int shifted = 0;               // FEASTHIP_SOLVER_SHIFTED_COCG was asked for (solver then holds COCG)
    // the last contour_apply: panels swept, panels that took the shifted sweep, its seed (contour index) and seed iterations
    int shift_panels = 0, shift_used = 0, shift_seed = -1, shift_seed_iters = 0;
    int block = 0;                 // FEASTHIP_SOLVER_BLOCK_COCG was asked for (solver then holds COCG)
    // the last contour_apply: panels swept, panels that took the block sweep, most block steps of a node, nodes that broke
    // down (finished by the per-column sweep), operator node-passes that ran
    int block_panels = 0, block_used = 0, block_steps_max = 0, block_breakdowns = 0, block_passes = 0;
    double rtol = 1e-12, atol = 0.0;
    int maxit = 500, restart = 30, factor_precision = 64, cache_factors = 1;

    std::vector<int> last_col_iters;    // [local node][m] iterations per column of the last sweep
    int last_col_m = 0;
    std::vector<int> last_node_iters;   // per local node: max column iterations of the last sweep
    std::vector<int> global_node_iters; // per CONTOUR node, summed over the ranks by the packed reduce of the last sweep

    // workspace (grown lazily)
    std::map<std::string, std::pair<void*, size_t>> bufs;

    // pinned staging ring of the small host -> device uploads (per-column coefficients, weights): fh_upload_coefs
    char* pin = nullptr; size_t pin_cap = 0, pin_off = 0;

    // resident refinement loop (feasthip_contour_apply_resident / rr_reduce_resident / rr_ritz_resident): the panels of one
    // FEAST loop stay on the device in the kernels' own row-major layout between the calls; pointers into `bufs`, dropped
    // (rs_epoch bumped) whenever the problem changes
    int rs_m = 0, rs_ld = 0;                    // columns / padded row length of the projection panel
    cplx* rs_P = nullptr;                       // Q_proj of the last resident sweep, summed over the ranks
    cplx* rs_basis = nullptr;                   // what the Ritz step multiplies: rs_P, or the orthonormalised panel of the fallback
    std::vector<cplx> rs_T;                     // implicit basis Q_proj D^-1: the m diagonal entries 1 / ||column||; empty = the basis is used as is
    int rs_rank = 0;
    cplx* rs_X = nullptr; int rs_X_m = 0, rs_X_ld = 0;   // Ritz vectors of the last resident Ritz step: the next sweep's subspace
    cplx* rs_R = nullptr;                       // A X - B X diag(lambda) of that step: the next sweep's shared start residual
    std::vector<cplx> rs_R_lambda;              // the lambda it was formed with

    // LU factors + pivots per local node slot (fh_factor_cache.hpp; the sequences over them: fh_direct.hip): the dense LU's,
    // and the sparse direct solver's (CSR input, FEASTHIP_SOLVER_BANDED; complex64 factors under FH_PLAN_BAND / FH_PLAN_MF only)
    fh_factor_cache lu_cache, band_cache;
    int csr_kl = 0, csr_ku = 0;   // bandwidths of the union pattern
    // pattern of the matrix as stored on the device (ingest order), kept on the host for the band plan of the direct solver
    std::vector<int> host_rowptr, host_col;
    // plan of the sparse direct solver (fh_banded.hip); FH_PLAN_BAND works in band order (band_perm[band row] = stored row,
    // band_iperm its inverse; both on the device)
    fh_direct_plan band_plan = FH_PLAN_NONE;
    int band_kl = 0, band_ku = 0;
    int band_plan_required = 0;   // the plan was made while feasthip_require_adjoint was on (dropped when it is next needed with the requirement off)
    int* band_perm = nullptr;
    int* band_iperm = nullptr;
    void* mf = nullptr;           // multifrontal plan of the sparse direct solver (fh_dense.hip: fh_mf_state), band_plan == FH_PLAN_MF
    // feasthip_set_ortho_method / feasthip_last_ortho: what rejected panels take, and what the last orthonormalisation did
    int ortho_method = 0;         // FEASTHIP_ORTHO_MGS | FEASTHIP_ORTHO_CHOLQR_RR
    struct { int panels = 0, used = 0, stages = 0, fell_back = 0, rank = 0; std::vector<int> perm; std::vector<double> rdiag; } ortho_last;
    // feasthip_set_preconditioner: the pivot shifts, and per CONTOUR node the index of its pivot (-1: unpreconditioned); empty = none
    std::vector<cplx> pc_pivots;
    std::vector<int> pc_node_pivot;
    // feasthip_last_precond_sweep: panels of the last sweep that ran preconditioned, distinct pivots, factorisations done,
    // substitution sweeps (one per cycle start, per lock-step and per final x = M^-1 u of a batch), factor bytes held, band fallback
    struct { int panels = 0, used = 0, pivots = 0, fell_back = 0; int64_t factorizations = 0, sweeps = 0, factor_bytes = 0; } pc_last;
    std::vector<int> col_mask;    // feasthip_set_column_mask: columns with 0 are not iterated by the Krylov solvers
    int poisoned = 0;             // a Krylov deadline / queue fault returned with kernels possibly still queued: every later call fails fast
    int mask_live = 0;            // set only while a contour_apply call runs: the mask is one-shot and never reaches shifted_solve
    int sum_mode = 1;             // COCG contour_apply accumulates alpha*p into one shared panel (FH_NO_SUM_MODE=1 disables)
    int lu_outer_block = 0;       // FH_LU_KB: outer block column of the two-level LU (multiple of 32); 0 = by size (128, 256 from N = 6144)
    int lu_panel_legacy = 0;      // FH_LU_PANEL_LEGACY=1: per-column global-memory panel kernel
    int lu_solve_legacy = 0;      // FH_LU_SOLVE_32=1: 32-column one-launch substitution steps (comparison)
    int lu_lookahead = 1;         // FH_LU_LOOKAHEAD=0: no overlap of the next block column's panels with the rest of the trailing update
    hipStream_t side_stream = nullptr;            // second stream of the LU look-ahead (created on first use)
    int side_reserve = -1;                        // CUs per XCD the side stream's mask leaves to the main stream
    hipEvent_t lu_ev_next = nullptr, lu_ev_rest = nullptr;
    int lu_gemm_staged = 0;       // FH_LU_GEMM_STAGED=1: trailing update with both panels through LDS (comparison; always for complex64)

    // host-mapped progress word written by the device: (chunk tag << 32) | active columns
    volatile unsigned long long* h_progress = nullptr;   // pinned host view
    unsigned long long* d_progress = nullptr;            // device view of the same word

    // profiling
    unsigned long long* d_counters = nullptr;   // [0] spmm node-launches, [1] spmm column passes
    int profiling = 0;
    std::map<std::string, fh_prof_class> prof;
    std::map<std::string, double> prof_work;    // algorithmic work (flops) issued per class while profiling (dense MFMA classes)
    int prof_period = 0;                        // feasthip_profile_set_period: 0 = default sampling, 1 = every launch
    std::vector<fh_event_pair> pending_events;
    std::vector<hipEvent_t> event_pool;         // recycled profiling events
    int prof_mult = 1;                          // sampling period multiplier, raised when the host cost of sampling shows
    double prof_host_s = 0.0;                   // host seconds spent recording / reading events since profile_enable
    double prof_t0 = 0.0;                       // steady-clock seconds at profile_enable
};

// the handle's products are the caller's callback (an operator or a term-operator handle)
inline bool fh_callback_products(const feasthip_ctx* h) { return h->kind == FH_KIND_OPERATOR || h->kind == FH_KIND_TERM_OPERATOR; }

// workspace helper: returns a device buffer of at least `bytes`, reallocating if needed
int fh_get_buf(feasthip_ctx* h, const char* name, size_t bytes, void** out);
// the same for `count` elements of T (*out is left alone when the request fails)
template <typename T> inline int fh_buf(feasthip_ctx* h, const char* name, size_t count, T** out) {
    void* p = nullptr;
    const int rc = fh_get_buf(h, name, count * sizeof(T), &p);
    if (!rc) *out = (T*)p;
    return rc;
}
void fh_free_bufs(feasthip_ctx* h);
// frees the matrices, factors and plans of the current problem (any kind) and leaves h->kind = FH_KIND_NONE
void fh_free_problem(feasthip_ctx* h);

// What a direct solver gives the sequences of fh_direct.hip: its factor cache; at least nslots slots of the handle's factor
// precision (the sparse solver makes its plan first; keep_count: and no fewer than the cache held, whatever is dropped on the
// way); the factors of z[q] B - A into slot which[q], info[q] != 0: singular; and Y[q] = (z B - A)^-1 RHS[q] on the factors of
// slots[q] (rhs_stride 0: one right-hand side panel shared by all; h->adjoint: the conjugate-transposed substitution).
struct fh_direct_ops {
    fh_factor_cache feasthip_ctx::* cache;
    int (*ensure_slots)(feasthip_ctx* h, int nslots, bool keep_count);
    int (*factor)(feasthip_ctx* h, const std::vector<int>& which, const std::vector<cplx>& z, std::vector<int>& info);
    int (*solve)(feasthip_ctx* h, int ld, int m, const std::vector<int>& slots, const cplx* RHS, size_t rhs_stride, cplx* Y, size_t stride);
};
// fh_direct.hip: the sequences over a factor cache, on the sparse direct solver (banded) or the dense LU.  Factors are reused
// when h->cache_factors and the slot holds the shift exactly; *nfact: factorisations done; status: 0 or FEASTHIP_ERROR_LAPACK.
// Every local node, slot e for node e:  Y[e] = (z_e B - A)^-1 RHS_e
int fh_direct_solve_nodes(feasthip_ctx* h, bool banded, int ld, int m, int nodes, const std::vector<cplx>& z, const cplx* RHS, size_t rhs_stride,
                          cplx* Y, size_t stride, std::vector<int>& status, int64_t* nfact);
// One shift, in the slot fh_one_off_slot gives it; *nfact = 1 when it was factored, left alone when the factor was cached
int fh_direct_solve_single(feasthip_ctx* h, bool banded, int ld, int m, cplx z, const cplx* RHS, cplx* Y, int* status, int64_t* nfact);
// A subset of the nodes on one shared RHS panel: slots matched by shift (fh_factor_cache::match), only as many as it needs
int fh_direct_solve_subset(feasthip_ctx* h, bool banded, int ld, int m, const std::vector<cplx>& z, const cplx* RHS, cplx* Y, size_t stride,
                           std::vector<int>& status, int64_t* nfact);
// The factors of the distinct shifts z, matched by shift likewise, without a solve: slots[p] and status[p] of shift p ...
int fh_direct_factor_matched(feasthip_ctx* h, bool banded, const std::vector<cplx>& z, std::vector<int>& slots, std::vector<int>& status, int64_t* nfact);
// ... and Y_q = (z B - A)^-1 RHS_q with the factors in slots[q] (a slot may be named more than once), q < slots.size()
int fh_direct_solve_slots(feasthip_ctx* h, bool banded, int ld, int m, const std::vector<int>& slots, const cplx* RHS, size_t rhs_stride, cplx* Y, size_t stride);

// profiling helpers
void fh_prof_begin(feasthip_ctx* h, const char* cls);
void fh_prof_end(feasthip_ctx* h);
void fh_prof_collect(feasthip_ctx* h);

static inline int fh_pick_ld(int64_t m) {
    if (m <= 16) return 16;
    if (m <= 32) return 32;
    return 64;
}

// the coefficient table of a polynomial handle for a kernel launch
static inline fh_poly_ptrs fh_poly_coef_ptrs(const feasthip_ctx* h) {
    fh_poly_ptrs P;
    for (int k = 0; k <= FH_POLY_MAX_DEGREE; ++k) P.c[k] = h->poly.coef[k];
    return P;
}

// Vp (ld x ld, zero padded) = block (i, j) of the r x nc column-major host matrix V cut into ld x ld blocks -- all of V for
// r, nc <= ld -- with row k of V scaled by rowscale[k].x when rowscale != null
static inline void fh_pad_block(const cplx* V, int r, int64_t nc, int ld, int i, int64_t j, const cplx* rowscale, std::vector<cplx>& Vp) {
    const int mi = r - i * ld < ld ? r - i * ld : ld, mj = (int)(nc - j * ld < ld ? nc - j * ld : ld);
    Vp.assign((size_t)ld * ld, cmake(0, 0));
    for (int c2 = 0; c2 < mj; ++c2)
        for (int c1 = 0; c1 < mi; ++c1) {
            const cplx v = V[(size_t)(j * ld + c2) * r + i * ld + c1];
            Vp[(size_t)c2 * ld + c1] = rowscale ? cscale(v, rowscale[i * ld + c1].x) : v;
        }
}
