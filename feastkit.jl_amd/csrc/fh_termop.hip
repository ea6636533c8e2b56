// fh_termop.hip -- term-operator handles (feasthip_set_term_operator, h->kind == FH_KIND_TERM_OPERATOR): the split form
//     T(z) X = sum_k f_k(z) (A_k X),   k = 0 .. nt-1,   2 <= nt <= 9,
// on the caller's products A_k X.  The handle is a term handle (fh_poly.hip: the feasthip_nep_* entry points, host tables of
// the f_k) that holds no matrix: where a term handle with matrices launches k_spmm_terms or the dense product, the callback
// of fh_operator.hip's ABI forms W_k = A_k X_e (which = k) for ALL nodes of the call into scratch panels of the handle, and ONE
// launch of k_terms_combine -- the sibling of k_op_combine for nt panels -- turns them into what the Krylov drivers, the
// evaluation of the residual-inverse sweep and the candidates' residuals read,
//     Y_e[i, c] = [Bvec_e[i, c] -] sum_{k kept, ascending} F(e, c, k) W_{k,e}[i, c]          W_{k,e} = X_e for an identity term,
// with the fused dots of the other operator kernels (dot modes 0 .. 4 of fh_sparse.hip, same conjugation):
//     1: partial1 = <U, Y>      2: partial1 = <Y, X>, partial2 = <Y, Y>      3: partial2 = <Y, Y>      4: partial1 = X^T Y
// Two table forms.  Node table F[e][k] (the Krylov operator T(z_e)): uniform over the columns, so the nk scalars of a node come
// by scalar loads and stay in scalar registers.  Column table F[k][c] (one node; R[:, j] = T(sigma_j) x_j and the candidates'
// residuals): term-major, the layout poly_upload_cols produces, one value per lane and term, loaded once per node.
// Accumulation order, fixed: acc = 0, then acc += F_k W_k for the kept terms in ascending k, one complex multiply-add per
// term; then Y = Bvec - acc where Bvec is given.  (tests/term_operator_cases.py TermOp.apply restates exactly that.)
// The products land in scratch, never in Y: the panel Y_e of an inactive node is left as it was, although the callback --
// which cannot see the device's activity words -- ran on that node too.
//
// k_terms_combine is a streaming kernel with the geometry of k_op_combine: element e = i LD + c of a panel belongs to thread
// e mod FH_BLOCK of workgroup (e / FH_BLOCK) mod gridDim.x, the grid stride is a multiple of LD, so a thread keeps its column.
// Every access is one 16-byte element per lane; the W_k, Bvec and U are read and Y is written with non-temporal accesses.  The
// kernel is bandwidth-bound with up to nine independent loads per element: the inner loop is instantiated per kept-term count
// NK, so that the NK loads (plus Bvec and U) of an element are issued back to back into registers before the first
// multiply-add waits for any of them; for NK <= 4 two elements are in flight per thread.
// Partial sums as in k_op_combine: ONE row per workgroup and node, partial[(node nblk + blockIdx.x) LD + c], a thread adds its
// rows in ascending order, the FH_BLOCK / LD threads of a column are added through LDS in thread order (fh_column_sum).  No
// atomics: reproducible.  An inactive node is skipped and its partial rows cleared.
// Algorithmic traffic per active node, P = 16 N LD bytes, nt' = the kept non-identity terms: reads nt' P of products; X (P) when
// a kept term is the identity or in modes 2 and 4; Bvec (P) and U (P, mode 1) where given; writes Y (P).  On top of that the
// callbacks write nt' P.  A term whose table entries are zero for every node (or column) of the call is neither produced nor
// read.  scratch: nt' nodes P bytes; when feasthip_set_term_operator's scratch_bytes (default FH_TERMS_SCRATCH_DEFAULT) does
// not hold the nodes of a call, the call runs in node chunks: callbacks on the chunk, one launch per chunk, each chunk's partial
// rows at its nodes' offsets -- the same values as the unchunked call, bit for bit.
#include "fh_common.hpp"
#include "fh_device.hpp"
#include "fh_kernels.hpp"
#include "fh_krylov.hpp"
#include "fh_host.hpp"

#include <algorithm>
#include <cmath>
#include <string>

#define FH_BLOCK 256
#define FH_TERMS_MAX (FH_POLY_MAX_DEGREE + 1)
#define FH_TERMS_SCRATCH_DEFAULT ((size_t)8 << 30)

static_assert(FH_BLOCK % FH_MAX_LD == 0, "a thread of k_terms_combine keeps its column");

struct fh_terms_args {
    const cplx* W[FH_TERMS_MAX]; size_t w_stride[FH_TERMS_MAX];     // the kept terms' panels: scratch products, or X itself (identity)
    int kidx[FH_TERMS_MAX];                                          // their term indices, ascending
    int nk, nt, xk;                                                  // kept terms, terms of the table, first kept identity term (-1: none)
    const cplx* F;
    fh_termop_call c;
    int N;
};

template <int LD, bool COLS, int NK>
__device__ __forceinline__ void terms_combine_body(const fh_terms_args& a, cplx* red) {
    constexpr int NR = NK > 0 ? NK : 1, UNR = NK <= 4 ? 2 : 1;
    const int t = threadIdx.x, c = t % LD;
    const int mode = a.c.dot_mode, nblk = gridDim.x;
    const size_t total = (size_t)a.N * LD, step = (size_t)nblk * FH_BLOCK;
    const bool want_x = (mode == 2 || mode == 4) && a.xk < 0;
    for (int node = 0; node < a.c.nodes; ++node) {
        const size_t pbase = ((size_t)node * nblk + blockIdx.x) * LD;
        if (a.c.node_active && a.c.node_active[node] == 0) {          // (uniform over the workgroup)
            if (mode != 0 && t < LD) {
                if (a.c.partial1) a.c.partial1[pbase + t] = cmake(0, 0);
                if (a.c.partial2) a.c.partial2[pbase + t] = cmake(0, 0);
            }
            continue;
        }
        const cplx* __restrict__ X = a.c.X + (size_t)node * a.c.x_node_stride;
        cplx* __restrict__ Y = a.c.Y + (size_t)node * a.c.y_node_stride;
        const cplx* __restrict__ Bv = a.c.Bvec ? a.c.Bvec + (size_t)node * a.c.b_node_stride : nullptr;
        const cplx* __restrict__ U = a.c.U ? a.c.U + (size_t)node * a.c.u_node_stride : nullptr;
        const cplx* w[NR];
        cplx f[NR];
#pragma unroll
        for (int j = 0; j < NK; ++j) {
            w[j] = a.W[j] + (size_t)node * a.w_stride[j];
            f[j] = COLS ? a.F[(size_t)a.kidx[j] * LD + c] : a.F[(size_t)node * a.nt + a.kidx[j]];      // (node table: uniform address)
        }
        cplx d1 = cmake(0, 0), d2 = cmake(0, 0);
#pragma unroll UNR
        for (size_t e = (size_t)blockIdx.x * FH_BLOCK + t; e < total; e += step) {
            cplx v[NR];
#pragma unroll
            for (int j = 0; j < NK; ++j) v[j] = fh_ld_nt(w[j] + e);
            cplx bv = cmake(0, 0), u = cmake(0, 0), x = cmake(0, 0);
            if (Bv) bv = fh_ld_nt(Bv + e);
            if (mode == 1) u = fh_ld_nt(U + e);
            if (want_x) x = X[e];
            cplx acc = cmake(0, 0);
#pragma unroll
            for (int j = 0; j < NK; ++j) {
                cfma(acc, f[j], v[j]);
                if (j == a.xk) x = v[j];          // an identity term's panel IS X
            }
            if (Bv) acc = csub(bv, acc);
            fh_st_nt(Y + e, acc);
            if (mode == 1) d1 = cadd(d1, cmulc(u, acc));
            else if (mode == 2) { d1 = cadd(d1, cmulc(acc, x)); d2.x += cabs2(acc); }
            else if (mode == 3) d2.x += cabs2(acc);
            else if (mode == 4) d1 = cadd(d1, cmul(x, acc));          // unconjugated p^T (S p), COCG
        }
        if (mode != 0 && mode != 3) fh_column_sum<LD, FH_BLOCK>(red, t, d1, a.c.partial1 + pbase);
        if (mode == 2 || mode == 3) fh_column_sum<LD, FH_BLOCK>(red, t, d2, a.c.partial2 + pbase);
    }
}

template <int LD, bool COLS>
__global__ __launch_bounds__(FH_BLOCK) void k_terms_combine(fh_terms_args a) {
    __shared__ cplx red[FH_BLOCK];
    switch (a.nk) {          // (uniform: one instantiation of the loop per kept-term count)
    case 0: terms_combine_body<LD, COLS, 0>(a, red); break;
    case 1: terms_combine_body<LD, COLS, 1>(a, red); break;
    case 2: terms_combine_body<LD, COLS, 2>(a, red); break;
    case 3: terms_combine_body<LD, COLS, 3>(a, red); break;
    case 4: terms_combine_body<LD, COLS, 4>(a, red); break;
    case 5: terms_combine_body<LD, COLS, 5>(a, red); break;
    case 6: terms_combine_body<LD, COLS, 6>(a, red); break;
    case 7: terms_combine_body<LD, COLS, 7>(a, red); break;
    case 8: terms_combine_body<LD, COLS, 8>(a, red); break;
    default: terms_combine_body<LD, COLS, 9>(a, red); break;
    }
}
static_assert(FH_TERMS_MAX == 9, "k_terms_combine instantiates its loop for 0 .. 9 kept terms");

// one callback: W_e = A_k X_e for `nodes` panels; -1 with h->op.failed set when it reports failure
static int term_callback(feasthip_ctx* h, int k, int nodes, int ld, const cplx* X, size_t x_node_stride, cplx* W) {
    const int N = (int)h->dense.N;
    const size_t panel = (size_t)N * ld;
    const int code = h->op.apply(h->op.user, k, nodes, ld, (int64_t)N, X, (int64_t)(nodes > 1 ? x_node_stride : panel), W, (int64_t)panel,
                                 (void*)h->stream);
    if (code == 0) return 0;
    h->op.failed = 1;
    h->last_error = "operator callback failed (which=" + std::to_string(k) + ", code=" + std::to_string(code) + ")";
    return -1;
}

int fh_apply_term_operator(feasthip_ctx* h, int ld, const fh_termop_call& c) {
    if (h->op.failed) return -1;          // an earlier callback of this entry point failed: nothing more is called or launched
    if (!h->op.apply) { h->last_error = "internal: term-operator handle without a callback"; return -1; }
    const int N = (int)h->dense.N, nt = h->poly.degree + 1;
    const size_t panel = (size_t)N * ld;
    if (c.nodes < 1 || (c.nodes > 1 && (c.x_node_stride < panel || c.y_node_stride < panel)) || (c.cols && c.nodes != 1)) {
        h->last_error = "internal: the term operator takes one panel per node (and one node with a column table)";
        return -1;
    }
    if (c.dot_mode < 0 || c.dot_mode > 4 || ((c.dot_mode == 1) && !c.U) || !c.F) { h->last_error = "internal: dot mode or table of the term combine kernel"; return -1; }
    fh_terms_args a;
    a.c = c; a.N = N; a.nt = nt; a.nk = 0; a.xk = -1; a.F = c.F;
    int slot[FH_TERMS_MAX], nprod = 0;          // scratch slot of a kept term (-1: identity)
    for (int k = 0; k < nt; ++k) {
        if (!((c.terms >> k) & 1u)) continue;
        const bool ident = (h->top.identity_mask >> k) & 1u;
        if (ident && a.xk < 0) a.xk = a.nk;
        slot[a.nk] = ident ? -1 : nprod++;
        a.kidx[a.nk++] = k;
    }
    for (int j = a.nk; j < FH_TERMS_MAX; ++j) { a.W[j] = nullptr; a.w_stride[j] = 0; a.kidx[j] = 0; }
    // node chunks: nprod panels of scratch per node
    const size_t budget = h->top.scratch_bytes ? h->top.scratch_bytes : FH_TERMS_SCRATCH_DEFAULT;
    const size_t per_node = (size_t)nprod * panel * sizeof(cplx);
    const int chunk = nprod == 0 ? c.nodes : (int)std::max<size_t>(1, std::min<size_t>((size_t)c.nodes, budget / per_node));
    cplx* scratch = nullptr;
    if (nprod && fh_buf(h, "top_w", (size_t)nprod * chunk * panel, &scratch)) return -1;
    const int nblk = fh_op_combine_nblk(N, ld);
    for (int e0 = 0; e0 < c.nodes; e0 += chunk) {
        const int nn = std::min(chunk, c.nodes - e0);
        const cplx* Xc = c.X + (size_t)e0 * c.x_node_stride;
        for (int j = 0; j < a.nk; ++j) {
            if (slot[j] < 0) { a.W[j] = Xc; a.w_stride[j] = c.x_node_stride; continue; }
            cplx* Wj = scratch + (size_t)slot[j] * chunk * panel;
            if (term_callback(h, a.kidx[j], nn, ld, Xc, c.x_node_stride, Wj)) return -1;
            a.W[j] = Wj; a.w_stride[j] = panel;
        }
        a.c.nodes = nn;
        a.c.X = Xc;
        a.c.Y = c.Y + (size_t)e0 * c.y_node_stride;
        a.c.Bvec = c.Bvec ? c.Bvec + (size_t)e0 * c.b_node_stride : nullptr;
        a.c.U = c.U ? c.U + (size_t)e0 * c.u_node_stride : nullptr;
        a.c.node_active = c.node_active ? c.node_active + e0 : nullptr;
        a.c.partial1 = c.partial1 ? c.partial1 + (size_t)e0 * nblk * ld : nullptr;
        a.c.partial2 = c.partial2 ? c.partial2 + (size_t)e0 * nblk * ld : nullptr;
        a.F = c.cols ? c.F : c.F + (size_t)e0 * nt;
        fh_prof_begin(h, "terms_combine");
        fh_with_ld(ld, [&](auto L) {
            constexpr int LD = decltype(L)::value;
            if (c.cols) hipLaunchKernelGGL((k_terms_combine<LD, true>), dim3((unsigned)nblk), dim3(FH_BLOCK), 0, h->stream, a);
            else hipLaunchKernelGGL((k_terms_combine<LD, false>), dim3((unsigned)nblk), dim3(FH_BLOCK), 0, h->stream, a);
        });
        fh_prof_end(h);
    }
    return nblk;
}

int fh_term_products(feasthip_ctx* h, int ld, const cplx* X, cplx* W) {
    if (h->op.failed) return -1;
    if (!h->op.apply) { h->last_error = "internal: term-operator handle without a callback"; return -1; }
    const size_t panel = (size_t)h->dense.N * ld;
    for (int k = 0; k <= h->poly.degree; ++k) {
        if ((h->top.identity_mask >> k) & 1u) {
            if (hipMemcpyAsync(W + (size_t)k * panel, X, panel * sizeof(cplx), hipMemcpyDeviceToDevice, h->stream) != hipSuccess) {
                h->last_error = "term operator: copy of the identity term's panel failed";
                return -1;
            }
        } else if (term_callback(h, k, 1, ld, X, panel, W + (size_t)k * panel)) return -1;
    }
    return 0;
}

extern "C" int feasthip_set_term_operator(feasthip_handle h, int64_t N, int nterms, feasthip_apply_fn apply, void* user, int flags,
                                          unsigned identity_mask, int64_t scratch_bytes) {
    const char* what = "feasthip_set_term_operator";
    if (int gate = fh_gate(h)) return gate;
    if (N <= 0 || N > INT32_MAX / FH_MAX_LD) { h->last_error = std::string(what) + ": N out of range"; return FEASTHIP_ERROR_N; }
    if (nterms < 2 || nterms > FH_TERMS_MAX) { h->last_error = std::string(what) + ": nterms must be 2 .. FEASTHIP_POLY_MAX_DEGREE + 1"; return FEASTHIP_ERROR_FPM; }
    const unsigned all = (1u << nterms) - 1u;
    if (identity_mask & ~all) { h->last_error = std::string(what) + ": identity_mask has a bit beyond the last term"; return FEASTHIP_ERROR_FPM; }
    if (!apply && identity_mask != all) { h->last_error = std::string(what) + ": null callback"; return FEASTHIP_ERROR_N; }
    if (flags & ~(FEASTHIP_OP_COMPLEX | FEASTHIP_OP_SYMMETRIC)) { h->last_error = std::string(what) + ": unknown flag (FEASTHIP_OP_COMPLEX and FEASTHIP_OP_SYMMETRIC apply)"; return FEASTHIP_ERROR_FPM; }
    if (scratch_bytes < 0) { h->last_error = std::string(what) + ": scratch_bytes must not be negative (0: the default)"; return FEASTHIP_ERROR_FPM; }
    if (h->comm) {
        h->last_error = std::string(what) + ": an attached communicator is not supported (a term-operator handle sweeps on one rank, under the Krylov solvers FEASTHIP_SOLVER_BICGSTAB, _COCG or _GMRES)";
        return FEASTHIP_ERROR_FPM;
    }
    FH_CHECK(hipSetDevice(h->device));
    FH_CHECK(hipStreamSynchronize(h->stream));
    fh_free_problem(h);
    h->dense.N = N;
    h->dense.is_complex = (flags & FEASTHIP_OP_COMPLEX) ? 1 : 0;
    h->dense.b_identity = 0;
    h->poly.degree = nterms - 1; h->poly.terms = 1; h->poly.sparse = 0;
    for (int k = 0; k < nterms; ++k) h->poly.fro[k] = 0.0;
    h->op.apply = (fh_apply_fn)apply; h->op.user = user;
    h->op.symmetric = (flags & FEASTHIP_OP_SYMMETRIC) ? 1 : 0;
    h->top.identity_mask = identity_mask;
    h->top.scratch_bytes = (size_t)scratch_bytes;
    h->adjoint = 0;
    // the solver settings may date from another problem: what the handle cannot take becomes GMRES (feasthip_set_solver refuses it from now on)
    const bool krylov = h->solver == FEASTHIP_SOLVER_BICGSTAB || h->solver == FEASTHIP_SOLVER_GMRES || (h->solver == FEASTHIP_SOLVER_COCG && h->op.symmetric);
    if (!krylov || h->shifted || h->block || h->factor_precision != 64) { h->solver = FEASTHIP_SOLVER_GMRES; h->shifted = h->block = 0; h->factor_precision = 64; }
    h->node_kinds.clear();
    h->kind = FH_KIND_TERM_OPERATOR;
    return 0;
}

extern "C" int feasthip_set_term_norms(feasthip_handle h, const double* norms) {
    if (!h) return FEASTHIP_ERROR_INTERNAL;
    if (h->kind != FH_KIND_TERM_OPERATOR) { h->last_error = "feasthip_set_term_norms: needs a term-operator handle (feasthip_set_term_operator)"; return FEASTHIP_ERROR_FPM; }
    if (!norms) { h->last_error = "feasthip_set_term_norms: null argument"; return FEASTHIP_ERROR_FPM; }
    for (int k = 0; k <= h->poly.degree; ++k)
        if (!(norms[k] > 0.0) || !std::isfinite(norms[k])) {
            h->last_error = "feasthip_set_term_norms: norm " + std::to_string(k) + " must be positive and finite";
            return FEASTHIP_ERROR_FPM;
        }
    for (int k = 0; k <= h->poly.degree; ++k) h->poly.fro[k] = norms[k];
    h->top.norms_set = 1;
    return 0;
}
