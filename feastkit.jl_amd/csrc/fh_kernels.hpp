// fh_kernels.hpp -- argument structs and launcher prototypes shared by the .hip units.
#pragma once
#include "fh_common.hpp"
#include <type_traits>

// ---- launch dispatch: the panel width (16 | 32 | 64) and the panel precision (64 | 32) as compile-time values -------------
//   fh_with_ld(ld, [&](auto L) { constexpr int LD = decltype(L)::value; hipLaunchKernelGGL((k_x<LD>), ...); });
//   fh_with_prec(prec, [&](auto ct) { using CT = decltype(ct); ... });
template <typename F> inline void fh_with_ld(int ld, F&& f) {
    if (ld == 16) f(std::integral_constant<int, 16>{});
    else if (ld == 32) f(std::integral_constant<int, 32>{});
    else f(std::integral_constant<int, 64>{});
}
template <typename F> inline void fh_with_prec(int prec, F&& f) {
    if (prec == 32) f(cplxf{});
    else f(cplx{});
}
// the two common launches: KERNEL<LD> and KERNEL<CT, LD> with the given grid, block and arguments, no dynamic LDS
#define FH_LAUNCH_LD(ld, KERNEL, grid, block, st, ...) \
    fh_with_ld(ld, [&](auto L) { hipLaunchKernelGGL((KERNEL<decltype(L)::value>), grid, block, 0, st, __VA_ARGS__); })
#define FH_LAUNCH_PREC_LD(prec, ld, KERNEL, grid, block, st, ...)                                                      \
    fh_with_prec(prec, [&](auto ct) {                                                                                   \
        fh_with_ld(ld, [&](auto L) { hipLaunchKernelGGL((KERNEL<decltype(ct), decltype(L)::value>), grid, block, 0, st, __VA_ARGS__); }); \
    })

// ---- sparse operator -------------------------------------------------------------------
// Panel pointers are void*: complex128 panels when prec == 64, complex64 when prec == 32.
struct fh_spmm_args {
    const int* rowptr; const int* col; const void* aval; const void* bval;
    int N; int nodes;
    const void* X; size_t x_node_stride;      // element stride between nodes (0 = shared)
    void* Y; size_t y_node_stride;
    const cplx* coefA; const cplx* coefB;     // [nodes][LD] per-column coefficients (always fp64)
    const void* Bvec; size_t b_node_stride;   // non-null: Y = Bvec - S X
    const void* U; size_t u_node_stride;      // dot_mode 1: <U, Y>
    int dot_mode;
    cplx* partial1; cplx* partial2;           // [nodes][nprow][LD], always fp64
    const int* node_active;                   // may be null
    unsigned long long* counters;             // [0] active node-launches, [1] active column x vector passes (may be null)
    int m;                                    // active width when node_active is null
    int uniform_coef;                         // coefA/coefB identical for every column of a node
    int prec;                                 // 64 | 32
    const int* rp8 = nullptr; const int* col8 = nullptr; const double* a8 = nullptr; const double* b8 = nullptr;   // chunk-of-8 rows (fh_csr)
    int use_row_kernel = 0;                   // LD = 64 and real matrix values: k_spmm_row (one wave per row); partial rows = fh_spmm_row_grid(N)
    // k_spmm_row / k_spmm (complex128 panels): X holds a panel SHARED by the nodes whose column c is to be read as colscale[node][c] * X (the lazy
    // start of the sum-mode COCG sweeps: every node's first direction is one source panel times a per-column factor).  The
    // kernel forms y = colscale * (S x) and takes its dots with colscale * x.  Null: X as is.
    const cplx* colscale = nullptr;
    // row blocks of a renumbered matrix (fh_common.hpp: fh_csr); lcol == null: not renumbered, k_spmm serves
    int nblk_rows; const int* blk_start; const int* ext_ptr; const int* ext_idx; const unsigned short* lcol;
};
int fh_spmm_grid(int N, int ld);
int fh_spmm_partials(int N, int ld);
int fh_spmm_row_grid(int N);
int fh_spmm_lds_slots(int nblk_rows, int ld);
void fh_launch_spmm(const fh_spmm_args& a, int ld, bool is_complex, bool bident, int nblk, hipStream_t st);

// ---- shift-preconditioned operator in its identity form (fh_sparse.hip: k_precond_op) -------------------------------------
// S_e M^-1 = I + c_e B M^-1 with M = z_p B - A, c_e = z_e - z_p.  T_e = M^-1 V_e comes from the substitution; the kernel forms
//   step:        Y_e = V_e + c_e B T_e                    (Bvec == null)
//   cycle start: Y_e = Bvec - V_e - c_e B T_e, partial2 = <Y, Y> in the layout of dot mode 3 ([nodes][fh_spmm_partials][LD])
// on complex128 panels; columns >= m are written as zeros.  It reads B's values only (none when B = I).
struct fh_precond_args {
    const int* rowptr; const int* col; const void* bval;
    int N; int nodes; int m;
    const cplx* V; size_t v_node_stride;
    const cplx* T; size_t t_node_stride;
    cplx* Y; size_t y_node_stride;
    const cplx* cnode;                        // [nodes] c_e
    const cplx* Bvec;                         // shared by the nodes, or null
    cplx* partial2;                           // cycle start only
    const int* node_active;                   // may be null; an inactive node is skipped (its partial rows are cleared)
};
void fh_launch_precond_op(const fh_precond_args& a, int ld, bool is_complex, bool bident, hipStream_t st);

// ---- Krylov vector kernels (BiCGStab and COCG) -------------------------------------------
struct fh_vec_args {
    int N;
    size_t node_stride;
    void *X, *R, *Rhat, *P, *V, *S, *T;
    const cplx* Q;             // init guess source (shared by all nodes, fp64)
    const double* lambda;      // [LD] Ritz values or null
    const cplx* znode;         // [nodes]
    fh_krylov_scalars s;
    cplx* partial1; cplx* partial2;
    int prec;                  // 64 | 32
    unsigned long long* counters;   // measurement: [2] += active columns of this launch (update kernels), may be null
    // sum mode (COCG inside contour_apply): the per-node solutions are never formed; every step
    // alpha p of every node goes straight into the shared accumulator  ACC += w_node alpha [scale] p
    // lazy start (first fused iteration only): residual and direction of every node are first_scale[node][c] * first_src,
    // the panels R and P do not exist yet -- the kernel reads first_src in their place and WRITES them
    const cplx* first_src;     // N x LD fp64 shared source panel, or null
    const cplx* first_scale;   // [nodes x LD]
    cplx* sum_acc;             // N x LD fp64 accumulator, or null (solutions are updated in X)
    const cplx* wnode;         // [nodes] quadrature weights
    const double* sum_scale;   // [nodes x LD] column scale of the correction (mixed precision) or null
    int nodes;
};
struct fh_fin_args {
    fh_krylov_scalars s;
    const cplx* partial1; const cplx* partial2;
    int nblk; int m;
    double rtol, atol;
    const double* atol_scale;  // per (node,column) factor on atol (mixed precision: 1/||r0||), may be null
    int mode;                  // 0 BiCGStab, 1 COCG
    const int* col_mask;       // [LD] 0 = column keeps its initial guess and is never iterated; may be null
};
void fh_launch_init_guess(const fh_vec_args& a, int ld, int nblk, int nodes, hipStream_t st);
void fh_launch_copy_r(const fh_vec_args& a, int ld, int nblk, int nodes, hipStream_t st);
void fh_launch_p_update(const fh_vec_args& a, int ld, int nblk, int nodes, hipStream_t st);
void fh_launch_s_update(const fh_vec_args& a, int ld, int nblk, int nodes, hipStream_t st);
void fh_launch_xr_update(const fh_vec_args& a, int ld, int nblk, int nodes, hipStream_t st);
void fh_launch_cocg_init(const fh_vec_args& a, int ld, int nblk, int nodes, hipStream_t st);
// sum-mode start from one shared source panel (a.Q = source, a.lambda/a.znode = warm-start factors or null)
void fh_launch_cocg_init_shared(const fh_vec_args& a, int ld, int nblk, int nodes, hipStream_t st);
// the same start without materialising R and P: only the per-node dot partials (a.Q = source, a.first_scale = per-node column
// factors); the first fused iteration then runs with fh_spmm_args::colscale / fh_vec_args::first_src
void fh_launch_cocg_init_lazy(const fh_vec_args& a, int ld, int nblk, int nodes, hipStream_t st);
// OUT = [Re](SRC * rho_c + ACC)
void fh_launch_sum_finish(const cplx* src, const cplx* rho, const cplx* acc, cplx* out, int N, int ld, int real_part, hipStream_t st);
#define FH_NODE_FINISH_MAX 64    // direct nodes one finishing launch sums (their weights sit in LDS); FH_BLOCK >= this
void fh_launch_node_finish(const cplx* src, const cplx* rho, const cplx* acc, const cplx* Yd, size_t stride, const cplx* wd, int nd,
                           cplx* out, int N, int ld, int real_part, hipStream_t st);
void fh_launch_cocg_update(const fh_vec_args& a, int ld, int nblk, int nodes, hipStream_t st);
void fh_launch_cocg_p(const fh_vec_args& a, int ld, int nblk, int nodes, hipStream_t st);
void fh_launch_cocg_p_sum(const fh_vec_args& a, int ld, int nodes, hipStream_t st);
// ---- fused COCG iteration (fh_sparse.hip, "fused COCG"): SpMM with five dots -> one finalize -> one vector kernel --------
struct fh_fused_fin_args {
    fh_krylov_scalars s;
    const cplx *sig, *kap;                    // SpMM partials [nodes][nblk_op][LD]: p^T q, q^T q (unconjugated)
    const cplx *rho, *rr;                     // partials of the last vector kernel / the init kernel [nodes][nblk_vec][LD]: r^T r, |r|^2
    int nblk_op, nblk_vec;
    unsigned long long* tickets;              // [nodes], zero between launches
    int final_check;                          // 1: only re-evaluate the stop test from (rho, rr) after the last step
    int predict_stop;                         // inexact solves: also stop on the predicted norm of the next residual
};
void fh_launch_fused_fin(const fh_fused_fin_args& a, int ld, int nodes, hipStream_t st);
// geometry of the fused vector kernel for a panel of N x ld elements: blocks per segment, segments, elements per thread
void fh_fused_vec_geometry(int N, int ld, int half, int* nblk, int* nseg, int* per_thread);
// R -= alpha Q, [ACC += w alpha P | X += alpha P], P = R + beta P, partials r^T r and |r|^2 ([nodes][nblk*nseg][LD])
void fh_launch_fused_vec(const fh_vec_args& a, int ld, hipStream_t st);
// ---- shifted COCG (fh_sparse.hip, "shifted COCG"): one Krylov space for all nodes of a B = I sweep ------------------------
// Panels are complex128.  Arrays marked [n][LD] hold one entry per (node, column), [LD] one per column.
struct fh_shift_args {
    int N, nodes, seed, m;
    size_t node_stride;
    cplx* R; cplx* Qv; cplx* P;               // seed residual, S_seed p_seed, direction panels [nodes] (P + seed * node_stride: the seed's)
    cplx* sum_acc;                            // N x LD accumulator: ACC += w_e alpha_e p_e
    const cplx* src;                          // shared start source: r_e^0 = fscale[e][c] * src
    const cplx* fscale;                       // [n][LD]
    const cplx* sigma;                        // [nodes] z_e - z_seed
    const cplx* wnode;                        // [nodes]
    cplx *pi, *pi_old;                        // [n][LD] pi_e^k, pi_e^(k-1)
    cplx *coef, *ipi, *beta_e;                // [n][LD] w_e alpha_e, 1 / pi_e^(k+1), beta_e of the step the vector kernel takes
    double *r0norm, *target, *rnorm;          // [n][LD]
    int *active, *accum, *iters, *status;     // [n][LD]
    cplx *alpha, *beta;                       // [LD] the seed's scalars of the last step taken
    int* col_step;                            // [LD] the column's seed recurrence advances in this iteration
    int* node_step;                           // [LD / 16][nodes] a column of the tile steps at this node
    int* tile_alive;                          // [LD / 16] columns of the tile with a node still iterating
    int* alive_total;                         // [1] their sum (the node_active word of the seed's operator product)
    int* passes;                              // [1] operator products that found a live column
    const cplx *sig, *kap; int nblk_op;       // SpMM partials [nblk_op][LD]: p^T q, q^T q
    cplx *rho_part, *rr_part; int nblk_vec;   // partials of the seed residual [nblk_vec][LD]: r^T r, |r|^2
    double rtol, atol;
    const int* col_mask;                      // [LD] or null
    int phase;                                // finalize: 0 first iteration (sets the start values), 1 iteration, 2 final check
};
// R = f_seed src, P_e = f_e src, partial rows of r^T r and |r|^2; returns the number of partial rows
int fh_launch_shift_init(const fh_shift_args& a, int ld, hipStream_t st);
void fh_launch_shift_fin(const fh_shift_args& a, int ld, hipStream_t st);
// r -= alpha q; ACC += sum_e w_e alpha_e p_e; p_e = r / pi_e + beta_e p_e; partial rows of the new r; returns their number
int fh_launch_shift_vec(const fh_shift_args& a, int ld, hipStream_t st);
// ---- block COCG (fh_bcocg.hip): one block Krylov space per node ---------------------------------------------------------------
// Panels are complex128.  [n][LD] arrays hold one entry per (node, ORIGINAL column); the small matrices are LD x LD, row-major,
// zero padded, one per node ([n][LD*LD]).  stop[e]: 0 running, 1 converged, 2 breakdown; every kernel skips a node that left.
struct fh_bcocg_args {
    int N, nodes, m;
    size_t node_stride;
    cplx *Q, *P, *W;                          // [nodes] panels: orthonormal residual factor, directions, S P
    cplx* sum_acc;                            // N x LD accumulator: ACC += w_e P_e (alpha_e C_e)
    const cplx* src;                          // shared start residual: R_e^0 = src diag(fscale[e])
    const cplx* fscale;                       // [n][LD]
    const cplx* wnode;                        // [nodes]
    cplx *SH, *ST;                            // [LD*LD] src^H src, src^T src
    cplx *GA, *GH, *GT;                       // P^T W ; Qh^H Qh ; Qh^T Qh
    cplx *T, *Tn, *U, *Ze, *Zi, *Cs, *Al, *M1, *Be;   // Q^T Q, its successor, scratch, zeta, zeta^-1, C, alpha, w alpha C, beta
    double *r0norm, *target, *rnorm;          // [n][LD]
    int *active, *iters, *status, *live;      // [n][LD]; live[e][j]: original column of block column j (-1 past nlive[e])
    int *node_active, *stop, *steps, *passes, *nlive;   // [nodes]; steps: block steps taken, passes: operator products that ran
    const int* col_mask;                      // [LD] or null
    double rtol, atol;
};
size_t fh_bcocg_gram_work_elems(int ld, int nodes);
// outH[e] = X_e^H Y_e and outT[e] = X_e^T Y_e (either may be null) for the nodes with stop[e] == 0 (stop null: all)
void fh_launch_bcocg_gram(const cplx* X, size_t xs, const cplx* Y, size_t ys, int N, int ld, int nodes, cplx* work, cplx* outH,
                          cplx* outT, const int* stop, hipStream_t st);
// phase 0: start; 1: alpha and w alpha C from P^T W; 2: zeta, T', beta, C, norms and the stop word from the Grams of Qh
void fh_launch_bcocg_small(const fh_bcocg_args& a, int ld, int phase, hipStream_t st);
// phase 0: Q = P = src Zi; 1: ACC += P M1, Q -= W alpha; 2: Q = Q Zi, P = Q + P beta; 3: W = Q C for the nodes that broke down
void fh_launch_bcocg_update(const fh_bcocg_args& a, int ld, int phase, hipStream_t st);

void fh_launch_fin_init(const fh_fin_args& a, int ld, int nodes, hipStream_t st);
void fh_launch_fin_alpha(const fh_fin_args& a, int ld, int nodes, hipStream_t st);
void fh_launch_fin_omega(const fh_fin_args& a, int ld, int nodes, hipStream_t st);
void fh_launch_fin_rho(const fh_fin_args& a, int ld, int nodes, hipStream_t st);
void fh_launch_count_active(const int* node_active, int nodes, int* out, hipStream_t st);
// writes (tag << 32 | active columns) to a host-mapped word with a system-scope release store
void fh_launch_publish_progress(const int* node_active, int nodes, unsigned long long* progress, unsigned tag, hipStream_t st);
// mixed precision hand-off: dst = src / ||r0||  (complex64) and X += ||r0|| * D
void fh_launch_narrow_scaled(const cplx* src, size_t src_stride, cplxf* dst, size_t dst_stride, const double* r0norm,
                             int N, int ld, int nblk, int nodes, hipStream_t st);
void fh_launch_widen_axpy(cplx* X, size_t x_stride, const cplxf* D, size_t d_stride, const double* r0norm,
                          int N, int ld, int nblk, int nodes, hipStream_t st);

// ---- device-resident restarted GMRES(m) (fh_gmres.hip) -----------------------------------------
struct fh_gmres_args {
    int N; int mr;                    // restart length
    size_t panel;                     // N * ld elements
    cplx* V; size_t v_node_stride;    // basis panels V[node][0..mr], (mr + 1) * panel apart
    cplx* W;                          // [node] work panel (residual at cycle start, then S v_k)
    cplx* partial;                    // multi-dot partials [node][chunk][blk][8][ld]
    cplx* npartial;                   // norm partials [node][blk][ld]
    cplx* H;                          // [node*ld][(mr+1) x mr] Hessenberg columns (rotated in place)
    cplx* hcur;                       // [node*ld][mr+1] coefficients of the running Gram-Schmidt pass
    cplx* cs; cplx* sn;               // [node*ld][mr] Givens rotations
    cplx* g;                          // [node*ld][mr+1] rotated right-hand side
    cplx* y;                          // [node*ld][mr] solution of the triangular system
    double* inv;                      // [node*ld] column scale of the next basis vector (0 = column finished)
    double* r0norm; double* target; double* rnorm;
    int* active; int* iters; int* status; int* kdim;   // [node*ld]
    int* node_active;                 // [nodes]
};
int fh_gm_nchunk(int k);
size_t fh_gm_partial_elems(int mr, int nblk, int nodes, int ld);
void fh_launch_gm_orthogonalize(const fh_gmres_args& a, int ld, int k, int nblk, int nodes, hipStream_t st);
void fh_launch_gm_start(const fh_gmres_args& a, int ld, int nblk_norm, int nodes, int first, double rtol, double atol, int m, hipStream_t st);
void fh_launch_gm_givens(const fh_gmres_args& a, int ld, int k, int nblk, int nodes, hipStream_t st);
void fh_launch_gm_scale_store(const fh_gmres_args& a, int ld, const cplx* src, size_t src_node_stride, int dst_index, int nblk, int nodes,
                              hipStream_t st);
void fh_launch_gm_finish_cycle(const fh_gmres_args& a, int ld, cplx* X, size_t x_node_stride, int kmax, int nblk, int nodes,
                               unsigned long long* steps_ran, hipStream_t st);

// ---- block (panel) operations ------------------------------------------------------------
// column-major (N x m, leading dim lds) <-> row-major panel (N x ld), zero padded
// perm != null: panel row i holds the caller's row perm[i] (block order of a renumbered sparse matrix)
void fh_launch_to_panel(const cplx* src, int64_t lds, int N, int m, cplx* dst, int ld, hipStream_t st, const int* perm = nullptr);
void fh_launch_from_panel(const cplx* src, int ld, int N, int m, cplx* dst, int64_t ldd, hipStream_t st, const int* perm = nullptr);
// resident refinement loop: dst (N x ldd panel, zero padded) = columns [c0, c0 + w) of the N x lds panel src; and the same
// columns written into columns [c0, c0 + w) of an N x ldd array of reals / interleaved complex values (zeros elsewhere)
void fh_launch_panel_cols(const cplx* src, int lds, int c0, int w, int N, cplx* dst, int ldd, hipStream_t st);
void fh_launch_pack_cols(const cplx* src, int lds, int c0, int w, int N, double* dst, int ldd, int real_only, hipStream_t st);
// real column-major source -> complex panel
void fh_launch_to_panel_real(const double* src, int64_t lds, int N, int m, cplx* dst, int ld, hipStream_t st);
// dst = sum_e w[e] * X[e]
void fh_launch_accumulate(const cplx* X, size_t node_stride, const cplx* w, int nodes, int N, int ld, const cplx* extra,
                          cplx* dst, int real_part, hipStream_t st);
// G (ld x ld, column-major, ldg = ld) = X^H Y (bilinear=0) or X^T Y (bilinear=1); f64 MFMA.
// work: at least fh_gram_work_elems(ld) cplx.  skip (here and below): device word; non-zero = the launch does nothing (the
// staged Cholesky-QR queues a fixed number of stages and the device decides how many run).
size_t fh_gram_work_elems(int ld);
void fh_launch_gram(const cplx* X, const cplx* Y, int N, int ld, int bilinear, cplx* work, cplx* G,
                    hipStream_t st, const int* skip = nullptr);
// per-column dots: out[c] = <U[:,c], V[:,c]>; work: nblk*ld cplx
int fh_vec_nblk(int N, int ld);
int fh_kry_nblk(int N, int ld, int nodes);
void fh_launch_dot_cols(const cplx* U, const cplx* V, int N, int ld, cplx* work, cplx* out, hipStream_t st);
// X[:,c] *= s[c]
void fh_launch_scale_cols(cplx* X, const cplx* s, int N, int ld, hipStream_t st);
// X[:, c] /= sqrt(dots[c].x) for c < M, on the device (dots: per-column <x, x> from fh_launch_dot_cols)
void fh_launch_normalize_cols(cplx* X, const cplx* dots, int N, int ld, int M, hipStream_t st);
// Xout = Q * V   (V: ld x ld column-major on device, zero padded)
void fh_launch_small_matmul(const cplx* Q, const cplx* V, int N, int ld, cplx* Xout, hipStream_t st, const int* skip = nullptr);
// dst[:,k] = src[:,perm[k]] for k < count else 0
void fh_launch_gather_cols(const cplx* src, const int* perm, int count, int N, int ld, cplx* dst, hipStream_t st);

// stochastic eigenvalue-count estimate (fh_estimate.hip): Rademacher block X[r, j] = v(row0 + r, col0 + j) (column-major, N x m,
// m <= 65535), and t[2j], t[2j+1] = re, im of sum_i v(i, col0 + j) P[i, j] over the column-major N x m block P; work:
// fh_trace_work_elems.  fh_launch_trace_finish is the second stage on its own: t[j] = sum_{b < nb} partial[j nb + b], in order.
// The entry v(i, j) itself, for a kernel that regenerates it (k_trace_partials, k_spmm_fanin_trace of fh_poly.hip):
__host__ __device__ inline uint64_t fh_mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ inline uint64_t fh_row_key(uint64_t seed, int64_t row) {
    return fh_mix64(seed + 0x9E3779B97F4A7C15ull * (uint64_t)(row + 1));
}
__device__ inline double fh_rademacher(uint64_t row_key, int64_t col) {
    return (fh_mix64(row_key ^ (0xD1B54A32D192ED03ull * (uint64_t)(col + 1))) >> 63) ? -1.0 : 1.0;
}
void fh_launch_rademacher(uint64_t seed, int64_t row0, int64_t nrows, int64_t m, cplx* X, int64_t ldx, hipStream_t st, int64_t col0 = 0);
size_t fh_trace_work_elems(int64_t N, int64_t m);
void fh_launch_trace_dots(const cplx* P, int64_t N, int64_t m, int64_t ldp, uint64_t seed, int real_only, cplx* work, double* t,
                          hipStream_t st, int64_t col0 = 0);
void fh_launch_trace_finish(const cplx* partial, int nb, int64_t m, int real_only, double* t, hipStream_t st);

// column-pivoted modified Gram-Schmidt with re-orthogonalisation, fully on device.
// state: int[4 + ld] = {k (steps done), rank, done, pivot, perm[ld]}; dstate: double[2+ld] = {R11, thr, norm2[ld]}
struct fh_mgs_args {
    cplx* X; int N; int ld; int m;
    int* istate; double* dstate; cplx* coef;   // coef[ld]
    cplx* work;                                // nblk*ld partials
    double rank_tol;
    double ref_scale = 0.0;                    // external R_11 (block of a wider matrix), 0 = own first pivot
    int big_dim = 0;                           // total column count of the wider matrix (eps*max(N,M0) term)
};
void fh_mgs_run(const fh_mgs_args& a, hipStream_t st);

// Rank-revealing Cholesky-QR, one stage's decision on one workgroup (k_pchol_stage; host restatement: fh_cholqr::pivoted_stage).
// istate: int[FH_RR_PERM + ld], dstate: double[2 + ld] = {R11 (< 0: not set), -, |R_kk|[ld]}
enum { FH_RR_RANK = 0, FH_RR_DONE = 1, FH_RR_SKIP = 2, FH_RR_FAIL = 3, FH_RR_NACC = 4, FH_RR_STAGES = 5, FH_RR_PERM = 8 };
void fh_launch_rr_init(int* istate, double* dstate, int ld, hipStream_t st);
// refine = 0: Gram matrix of the working panel -> pivots of this stage; refine = 1: Gram matrix of the accepted columns after
// the first pass -> their second pass.  Rinv: ld x ld, zero padded, permutation (refine = 0) / output column offset (1) folded in.
void fh_launch_pchol_stage(const cplx* G, int m, int ld, int refine, double window, double thr, double ref_scale, int* istate,
                           double* dstate, cplx* Rinv, hipStream_t st);

// dense kernels ---------------------------------------------------------------------------
struct fh_dense;
