// fh_operator.hip -- operator handles (feasthip_set_operator, h->kind == FH_KIND_OPERATOR): matrix-free FEAST on the caller's products.
//
// The handle holds no matrix.  Where a dense or CSR handle launches its operator kernel, fh_apply_operator (fh_api.hip) comes
// here: the caller's callback forms A X_e and B X_e for ALL nodes of the call in one go each, into scratch panels of the
// handle, and ONE launch of k_op_combine turns them into what the Krylov drivers, the projections and the residuals read,
//     Y_e[i, c] = [Bvec[i, c] -] ( coefB[e][c] BX_e[i, c] + coefA[e][c] AX_e[i, c] )         BX_e = X_e when B = I,
// with the fused dots of the other operator kernels (dot modes 0 .. 4 of fh_sparse.hip, same conjugation):
//     1: partial1 = <U, Y>      2: partial1 = <Y, X>, partial2 = <Y, Y>      3: partial2 = <Y, Y>      4: partial1 = X^T Y
// The products land in scratch, never in Y itself: the panel Y_e of an inactive node is left as it was, as every other
// operator kernel leaves it, although the callback -- which cannot see the device's activity words -- ran on that node too.
//
// k_op_combine is a streaming kernel: element e = i LD + c of a panel belongs to thread e mod FH_BLOCK of workgroup
// (e / FH_BLOCK) mod gridDim.x, the grid stride gridDim.x FH_BLOCK is a multiple of LD, so a thread keeps its column c and its
// two coefficients stay in registers.  Every access is one 16-byte element per lane, a wave reads 1 KiB lines; AX, BX, Bvec
// and U are read and Y is written with non-temporal accesses (they stream past the X panel, which the solver reads again).
// Partial sums as in k_spmm_poly: ONE row per workgroup and node, partial[(node nblk + blockIdx.x) LD + c] with nblk =
// gridDim.x; a thread adds its rows in ascending order, the FH_BLOCK / LD threads of a column are added through LDS in thread
// order.  No atomics: reproducible.  The node loop is outermost; an inactive node is skipped and its partial rows cleared.
// Algorithmic traffic per active node, P = 16 N LD bytes: reads AX (P), BX -- or X when B = I -- (P), Bvec (P) and U (P, mode 1)
// where given, X again (P, modes 2 and 4 with B != I); writes Y (P).  A term whose coefficient the host knows to be zero
// (fh_userop_call::skip) is neither produced nor read.  Against a fused SpMM, which reads its gathered X rows and writes Y,
// the price of the caller's operator is the callback's two panel writes (2 P) plus these two panel reads (2 P) per node.
#include "fh_common.hpp"
#include "fh_device.hpp"
#include "fh_kernels.hpp"
#include "fh_krylov.hpp"
#include "fh_host.hpp"

#include <algorithm>
#include <string>

#define FH_BLOCK 256
#define FH_COMBINE_GRID_MAX 1024

static_assert(FH_BLOCK % FH_MAX_LD == 0, "a thread of k_op_combine keeps its column");

struct fh_combine_args {
    const cplx* AX; const cplx* BX; size_t p_node_stride;      // scratch products (null: the term is left out); BX null and b_is_x: B = I
    fh_userop_call c;
    int N, b_is_x;
};

template <int LD>
__global__ __launch_bounds__(FH_BLOCK) void k_op_combine(fh_combine_args a) {
    __shared__ cplx red[FH_BLOCK];
    const int t = threadIdx.x, c = t % LD;
    const int mode = a.c.dot_mode, nblk = gridDim.x;
    const size_t total = (size_t)a.N * LD, step = (size_t)nblk * FH_BLOCK;
    const bool want_x = a.b_is_x || mode == 2 || mode == 4;
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
        const cplx* __restrict__ AX = a.AX ? a.AX + (size_t)node * a.p_node_stride : nullptr;
        const cplx* __restrict__ BX = a.BX ? a.BX + (size_t)node * a.p_node_stride : nullptr;
        const cplx* __restrict__ Bv = a.c.Bvec ? a.c.Bvec + (size_t)node * a.c.b_node_stride : nullptr;
        const cplx* __restrict__ U = a.c.U ? a.c.U + (size_t)node * a.c.u_node_stride : nullptr;
        const cplx ca = a.c.coefA[(size_t)node * LD + c], cb = a.c.coefB[(size_t)node * LD + c];
        cplx d1 = cmake(0, 0), d2 = cmake(0, 0);
#pragma unroll 2
        for (size_t e = (size_t)blockIdx.x * FH_BLOCK + t; e < total; e += step) {
            cplx x = cmake(0, 0), acc = cmake(0, 0);
            if (want_x) x = X[e];
            if (BX) acc = cmul(cb, fh_ld_nt(BX + e));
            else if (a.b_is_x) acc = cmul(cb, x);
            if (AX) cfma(acc, ca, fh_ld_nt(AX + e));
            if (Bv) acc = csub(fh_ld_nt(Bv + e), acc);
            fh_st_nt(Y + e, acc);
            if (mode == 1) d1 = cadd(d1, cmulc(fh_ld_nt(U + e), acc));
            else if (mode == 2) { d1 = cadd(d1, cmulc(acc, x)); d2.x += cabs2(acc); }
            else if (mode == 3) d2.x += cabs2(acc);
            else if (mode == 4) d1 = cadd(d1, cmul(x, acc));          // unconjugated p^T (S p), COCG
        }
        if (mode != 0 && mode != 3) fh_column_sum<LD, FH_BLOCK>(red, t, d1, a.c.partial1 + pbase);
        if (mode == 2 || mode == 3) fh_column_sum<LD, FH_BLOCK>(red, t, d2, a.c.partial2 + pbase);
    }
}

// one workgroup per FH_BLOCK elements of a panel up to the grid limit; beyond it the grid-stride loop takes further trips
// (N ld > FH_COMBINE_GRID_MAX FH_BLOCK: from N = 4097 at ld = 64, 8193 at 32, 16385 at 16)
int fh_op_combine_nblk(int N, int ld) {
    const size_t total = (size_t)N * ld;
    return (int)std::max<size_t>(1, std::min<size_t>(FH_COMBINE_GRID_MAX, (total + FH_BLOCK - 1) / FH_BLOCK));
}

int fh_apply_user_operator(feasthip_ctx* h, int ld, const fh_userop_call& c) {
    if (h->op.failed) return -1;          // an earlier callback of this entry point failed: nothing more is called or launched
    if (!h->op.apply) { h->last_error = "internal: operator handle without a callback"; return -1; }
    const int N = (int)h->dense.N;
    const size_t panel = (size_t)N * ld;
    const bool bid = h->dense.b_identity != 0;
    const bool needA = !(c.skip & 1), needB = !(c.skip & 2);
    if (c.nodes < 1 || (c.nodes > 1 && (c.x_node_stride < panel || c.y_node_stride < panel))) {
        h->last_error = "internal: the operator callback takes one panel per node";
        return -1;
    }
    if (c.dot_mode < 0 || c.dot_mode > 4 || ((c.dot_mode == 1) && !c.U)) { h->last_error = "internal: dot mode of the operator combine kernel"; return -1; }
    fh_combine_args a;
    a.AX = a.BX = nullptr; a.p_node_stride = panel; a.c = c; a.N = N; a.b_is_x = (bid && needB) ? 1 : 0;
    cplx* scratch[2] = {nullptr, nullptr};
    for (int which = 0; which < 2; ++which) {
        if (which == 0 ? !needA : (!needB || bid)) continue;
        if (fh_buf(h, which == 0 ? "op_ax" : "op_bx", (size_t)c.nodes * panel, &scratch[which])) return -1;
        const int code = h->op.apply(h->op.user, which, c.nodes, ld, (int64_t)N, c.X, (int64_t)(c.nodes > 1 ? c.x_node_stride : panel),
                                     scratch[which], (int64_t)panel, (void*)h->stream);
        if (code != 0) {
            h->op.failed = 1;
            h->last_error = "operator callback failed (which=" + std::to_string(which) + ", code=" + std::to_string(code) + ")";
            return -1;
        }
    }
    a.AX = scratch[0]; a.BX = scratch[1];
    const int nblk = fh_op_combine_nblk(N, ld);
    fh_prof_begin(h, "op_combine");
    FH_LAUNCH_LD(ld, k_op_combine, dim3((unsigned)nblk), dim3(FH_BLOCK), h->stream, a);
    fh_prof_end(h);
    return nblk;
}

extern "C" int feasthip_set_operator(feasthip_handle h, int64_t N, feasthip_apply_fn apply, void* user, int flags) {
    if (int gate = fh_gate(h)) return gate;
    if (N <= 0 || N > INT32_MAX / FH_MAX_LD) { h->last_error = "feasthip_set_operator: N out of range"; return FEASTHIP_ERROR_N; }
    if (!apply) { h->last_error = "feasthip_set_operator: null callback"; return FEASTHIP_ERROR_N; }
    const int known = FEASTHIP_OP_B_IDENTITY | FEASTHIP_OP_COMPLEX | FEASTHIP_OP_SYMMETRIC;
    if (flags & ~known) { h->last_error = "feasthip_set_operator: unknown flag"; return FEASTHIP_ERROR_FPM; }
    if (h->comm) {
        h->last_error = "feasthip_set_operator: an attached communicator is not supported (an operator handle sweeps on one rank, under the Krylov solvers FEASTHIP_SOLVER_BICGSTAB, _COCG or _GMRES)";
        return FEASTHIP_ERROR_FPM;
    }
    FH_CHECK(hipSetDevice(h->device));
    FH_CHECK(hipStreamSynchronize(h->stream));
    fh_free_problem(h);
    h->dense.N = N;
    h->dense.is_complex = (flags & FEASTHIP_OP_COMPLEX) ? 1 : 0;
    h->dense.b_identity = (flags & FEASTHIP_OP_B_IDENTITY) ? 1 : 0;
    h->op.apply = (fh_apply_fn)apply; h->op.user = user;
    h->op.symmetric = (flags & FEASTHIP_OP_SYMMETRIC) ? 1 : 0;
    h->kind = FH_KIND_OPERATOR;
    return 0;
}
