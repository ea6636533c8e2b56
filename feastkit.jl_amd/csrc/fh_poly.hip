// fh_poly.hip -- polynomial eigenproblems P(lambda) x = 0, P(lambda) = A_0 + lambda A_1 + ... + lambda^d A_d, on ONE N x N
// solve per quadrature node (gfx950).  Four flavours share this file:
//   dense coefficients      the batched dense LU of P(z_e)                                  (feasthip_set_polynomial)
//   sparse coefficients     the multifrontal LU of P(z_e), k_spmm_fan for the products      (feasthip_set_polynomial_csr)
//   the projected method    N-row subspaces: k_spmm_horner, the residual-inverse sweep      (either kind of coefficients)
//   Krylov solves on P(z)   BiCGStab / COCG / GMRES on the operator k_spmm_poly             (sparse coefficients)
// A fifth user reads the same storage as a split form: a TERM handle (feasthip_set_terms[_csr], fh_poly::terms) holds the A_k of
// T(lambda) = sum_k f_k(lambda) A_k, the f_k arbitrary scalar functions that only the caller evaluates.  It runs the projected
// method's calls with host tables of the f_k where a polynomial handle forms powers (the feasthip_nep_* entry points; one body
// per call, shared with its feasthip_poly_* sibling), through the table-form kernels k_form_terms, k_mf_assemble_terms
// (fh_dense.hip) and k_spmm_terms; the sum over the terms is fh_term_sum (fh_common.hpp), the sibling of fh_horner.
// A term-OPERATOR handle (feasthip_set_term_operator, h->kind == FH_KIND_TERM_OPERATOR, fh_termop.hip) is a term handle without matrices: the same
// calls under a Krylov solver, with the caller's callback and k_terms_combine where the others launch a product kernel.
// The steps they share exist once: Horner over the coefficients is fh_horner (fh_common.hpp), the batched row gather of the
// three SpMM kernels is POLY_ROW_GATHER, the kernels' coefficient table is fh_poly_coef_ptrs (fh_common.hpp).
//
// Replaces  feast_pep!                 src/dense/feast_dense.jl:715-772  (companion pencil :745-760, feast_gegv! on it :763)
//           feast_gepev!/hepev!/sypev! src/dense/feast_dense.jl:946-979
// The reference builds the dN x dN first companion form
//     A_lin = [ 0 I . . ; . . I . ; ... ; -A_0 ... -A_{d-1} ],   B_lin = diag(I, ..., I, A_d)
// and factors z B_lin - A_lin per node.  The companion matrix is never formed here: for R = [R_0; ...; R_{d-1}] the system
// (z B_lin - A_lin) Y = R is
//     D_p      = sum_{k=0}^{min(d-2, d-1-p)} A_{k+1+p} R_k          p = 0 .. d-1      (node independent)
//     P(z) Y_0 = R_{d-1} + sum_p z^p D_p                                                (one N x N solve)
//     Y_{i+1}  = z Y_i - R_i                                          i = 0 .. d-2
// so a node costs one LU of order N (the batched MFMA LU of fh_dense.hip, its factor cache included) instead of one of
// order dN: d^3 times fewer flops, d^2 times less factor memory.
//
// Panels: a dN x m block is kept as ONE row-major (dN) x ld panel (fh_common.hpp), i.e. the d row-major N x ld panels of
// its blocks one behind the other -- block i of a panel P is P + i N ld -- so the column-major <-> panel kernels, the Gram
// kernel, the small product and the column dots of fh_blockops.hip take it as a tall panel, and the dense product kernel
// takes one block of it.
//
// Sparse coefficients (feasthip_set_polynomial_csr) replace  feast_scsrpev! / feast_hcsrpev! / feast_gcsrpev!
// (src/sparse/feast_sparse.jl), which run on the explicit sparse companion.  The structured solve above touches the matrices in
// two places only, and both have a sparse counterpart: "form P(z_e)" is k_mf_assemble_poly inside the multifrontal LU of the
// sparse direct solver (fh_dense.hip, planned by fh_banded.hip, its per-node factor cache as it stands), and Y +-= A_k X is
// k_spmm_fan below.  Everything else in this file is shared by the two flavours.
#include "fh_common.hpp"
#include "fh_device.hpp"
#include "fh_kernels.hpp"
#include "fh_krylov.hpp"
#include "fh_host.hpp"
#include "fh_dense.hpp"
#include "fh_banded.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

#define FH_BLOCK 256
#define PD FH_POLY_MAX_DEGREE
static_assert(FH_POLY_MAX_DEGREE == FEASTHIP_POLY_MAX_DEGREE, "degree bound of the ABI");

// KERNEL<VT, LD>(a) on the value type of the handle's CSR coefficients and the panel width
#define POLY_LAUNCH_CSR(KERNEL, ld, grid, a)                                                                            \
    fh_with_ld(ld, [&](auto L) {                                                                                         \
        constexpr int LD = decltype(L)::value;                                                                           \
        if (h->csr.is_complex) hipLaunchKernelGGL((KERNEL<cplx, LD>), grid, dim3(FH_BLOCK), 0, h->stream, a);            \
        else hipLaunchKernelGGL((KERNEL<double, LD>), grid, dim3(FH_BLOCK), 0, h->stream, a);                            \
    })

// ---------------------------------------------------------------------------------------
// S_e = P(z_e) for the nf matrices about to be factored, in one pass over the coefficients: a thread owns matrix elements,
// loads their d + 1 coefficient values once (16 B per lane for complex input) and runs Horner per node.  Traffic:
// (d + 1) N^2 sizeof(VT) read, nf N^2 sizeof(T) written (k_form_shifted reads A and B once per node).
// ---------------------------------------------------------------------------------------
template <typename VT, typename T>
__global__ __launch_bounds__(FH_BLOCK) void k_form_poly(fh_poly_ptrs P, int d, T* const* LUs, const cplx* __restrict__ z, int nf,
                                                         size_t total) {
    for (size_t e = (size_t)blockIdx.x * FH_BLOCK + threadIdx.x; e < total; e += (size_t)gridDim.x * FH_BLOCK) {
        cplx a[PD + 1];
#pragma unroll
        for (int k = 0; k <= PD; ++k) a[k] = k <= d ? poly_val(((const VT*)P.c[k])[e]) : cmake(0, 0);
        for (int q = 0; q < nf; ++q) LUs[q][e] = cvt<T>(fh_horner<PD>(d, z[q], [&](int k) { return a[k]; }));
    }
}

// The table form for a term handle: S_q = sum_{k < nt} F[q][k] a_k, F the nf x nt table of fh_poly_term_table.  The same
// streaming pass -- a thread's nt coefficient values loaded once, nf elements written -- with the node's scalars read through
// uniform addresses (the row and term indices are the same in every lane, so they come by scalar loads, not per-lane gathers).
template <typename VT, typename T>
__global__ __launch_bounds__(FH_BLOCK) void k_form_terms(fh_poly_ptrs P, int nt, T* const* LUs, const cplx* __restrict__ F, int nf, size_t total) {
    for (size_t e = (size_t)blockIdx.x * FH_BLOCK + threadIdx.x; e < total; e += (size_t)gridDim.x * FH_BLOCK) {
        cplx a[PD + 1];
#pragma unroll
        for (int k = 0; k <= PD; ++k) a[k] = k < nt ? poly_val(((const VT*)P.c[k])[e]) : cmake(0, 0);
        for (int q = 0; q < nf; ++q) {
            const cplx* __restrict__ f = F + (size_t)q * nt;
            LUs[q][e] = cvt<T>(fh_term_sum<PD>(nt, [&](int k) { return f[k]; }, [&](int k) { return a[k]; }));
        }
    }
}

int fh_poly_term_table(feasthip_ctx* h, const cplx* dz, int nf, const cplx** dF) {
    const int nt = h->poly.degree + 1, ne = (int)h->poly.fnode_z.size();
    if (!h->poly.terms || ne == 0 || h->poly.fnode.size() != (size_t)ne * nt) {
        h->last_error = "term handle: no node values set (feasthip_nep_set_node_values)";
        return FEASTHIP_ERROR_FPM;
    }
    std::vector<cplx> z(nf), rows((size_t)nf * nt);
    FH_CHECK(hipMemcpyAsync(z.data(), dz, nf * sizeof(cplx), hipMemcpyDeviceToHost, h->stream));
    FH_CHECK(hipStreamSynchronize(h->stream));
    for (int q = 0; q < nf; ++q) {
        int e = 0;
        while (e < ne && !(h->poly.fnode_z[e].x == z[q].x && h->poly.fnode_z[e].y == z[q].y)) ++e;
        if (e == ne) { h->last_error = "term handle: a solve at a shift that is no node of the contour the node values were set for"; return FEASTHIP_ERROR_FPM; }
        for (int k = 0; k < nt; ++k) rows[(size_t)q * nt + k] = h->poly.fnode[(size_t)e * nt + k];
    }
    cplx* d;
    int rc = fh_buf(h, "terms_rows", rows.size(), &d);
    if (rc) return rc;
    FH_CHECK(hipMemcpyAsync(d, rows.data(), rows.size() * sizeof(cplx), hipMemcpyHostToDevice, h->stream));
    FH_CHECK(hipStreamSynchronize(h->stream));          // (rows is a local)
    *dF = d;
    return 0;
}

int fh_poly_form(feasthip_ctx* h, void* const* dlus, const cplx* dz, int nf, int prec) {
    const fh_poly_ptrs P = fh_poly_coef_ptrs(h);
    const int d = h->poly.degree;
    const size_t total = (size_t)h->dense.N * (size_t)h->dense.N;
    const dim3 grid((unsigned)std::min<size_t>(2048, (total + FH_BLOCK - 1) / FH_BLOCK)), block(FH_BLOCK);
    if (h->poly.terms) {
        const cplx* dF;
        const int rc = fh_poly_term_table(h, dz, nf, &dF);
        if (rc) return rc;
        fh_prof_begin(h, "terms_form");
        if (h->dense.is_complex) {
            if (prec == 32) hipLaunchKernelGGL((k_form_terms<cplx, cplxf>), grid, block, 0, h->stream, P, d + 1, (cplxf* const*)dlus, dF, nf, total);
            else hipLaunchKernelGGL((k_form_terms<cplx, cplx>), grid, block, 0, h->stream, P, d + 1, (cplx* const*)dlus, dF, nf, total);
        } else {
            if (prec == 32) hipLaunchKernelGGL((k_form_terms<double, cplxf>), grid, block, 0, h->stream, P, d + 1, (cplxf* const*)dlus, dF, nf, total);
            else hipLaunchKernelGGL((k_form_terms<double, cplx>), grid, block, 0, h->stream, P, d + 1, (cplx* const*)dlus, dF, nf, total);
        }
        fh_prof_end(h);
        return 0;
    }
    fh_prof_begin(h, "poly_form");
    if (h->dense.is_complex) {
        if (prec == 32) hipLaunchKernelGGL((k_form_poly<cplx, cplxf>), grid, block, 0, h->stream, P, d, (cplxf* const*)dlus, dz, nf, total);
        else hipLaunchKernelGGL((k_form_poly<cplx, cplx>), grid, block, 0, h->stream, P, d, (cplx* const*)dlus, dz, nf, total);
    } else {
        if (prec == 32) hipLaunchKernelGGL((k_form_poly<double, cplxf>), grid, block, 0, h->stream, P, d, (cplxf* const*)dlus, dz, nf, total);
        else hipLaunchKernelGGL((k_form_poly<double, cplx>), grid, block, 0, h->stream, P, d, (cplx* const*)dlus, dz, nf, total);
    }
    fh_prof_end(h);
    return 0;
}

// ---------------------------------------------------------------------------------------
// Sparse coefficients (feasthip_set_polynomial_csr): fan-out product on the shared pattern.  One input panel X (N x LD,
// row-major) and nout <= FH_FAN_MAX outputs, Y_t = s_t A_{k_t} X (+ the old Y_t when accumulate_t), s_t = +-1.  The structured
// solve and the residual step apply many coefficients to the SAME panel, and the gather of the X rows, not the matrix bytes,
// bounds the SpMM here: so per nonzero the column index and the gathered X row are loaded ONCE and the
// nout coefficient values at that nonzero feed nout accumulators that stay in registers.  A row is owned by one slice of LD
// lanes (lane <-> column: LD = 64 one wave per row, 32 two rows per wave, 16 four), which also reads and writes its Y_t
// elements: no atomics, the summation order is the row's CSR order, the result is reproducible.
// Algorithmic traffic: nnz (4 + nout sizeof(VT)) of matrix, one X row of 16 LD B gathered per nonzero (cache hits for a
// stencil), N LD 16 B per output written and as much read per accumulating output.
// ---------------------------------------------------------------------------------------
// One row of the row-slice SpMM kernels below (k_spmm_fan, k_spmm_horner, k_spmm_poly): LD lanes own the row, lane <-> column
// c.  The nonzeros [k0, k1) go in batches of 4: the gathers of a batch are issued together (a slot past the row end gathers
// the row's last column again and adds nothing), then the statements given last run for each nonzero, K its index and XV its
// gathered X element, in CSR order.  A macro, not a function template taking the term as a callable: through a closure the
// compiler orders the operands of the complex products the other way round and contracts a different half of each into the
// FMA, so the sums would differ in the last bit from what these kernels have always returned.
// POLY_ROW_GATHER_N is the step itself, for np_ <= NP_ panels one behind the other (panel p at X_ + p pstride_) and batches of
// DEPTH_ nonzeros: the column index is loaded once per nonzero and the row of every panel gathered at it, XS[p] the element of
// panel p.  POLY_ROW_GATHER is its one-panel, four-deep form.
#define POLY_ROW_GATHER_N(NP_, DEPTH_, LD_, colidx_, X_, pstride_, np_, k0_, k1_, c_, K, XS, ...)                        \
    for (int kb_ = (k0_); kb_ < (k1_); kb_ += (DEPTH_)) {                                                                \
        cplx xs_[DEPTH_][NP_];                                                                                           \
        _Pragma("unroll") for (int q_ = 0; q_ < (DEPTH_); ++q_) {                                                        \
            const cplx* xp_ = (X_) + ((size_t)(colidx_)[min(kb_ + q_, (k1_) - 1)] * (LD_) + (c_));                       \
            _Pragma("unroll") for (int p_ = 0; p_ < (NP_); ++p_)                                                         \
                if (p_ < (np_)) xs_[q_][p_] = xp_[(size_t)p_ * (pstride_)];                                              \
        }                                                                                                                \
        _Pragma("unroll") for (int q_ = 0; q_ < (DEPTH_); ++q_)                                                          \
            if (kb_ + q_ < (k1_)) { const int K = kb_ + q_; const cplx* XS = xs_[q_]; __VA_ARGS__ }                      \
    }
#define POLY_ROW_GATHER(LD_, colidx_, X_, k0_, k1_, c_, K, XV, ...)                                                     \
    POLY_ROW_GATHER_N(1, 4, LD_, colidx_, X_, 0, 1, k0_, k1_, c_, K, xv_, const cplx& XV = xv_[0]; __VA_ARGS__)

#define FH_FAN_MAX (PD + 1)
struct fh_fan_args {
    const int* rowptr; const int* col;
    const cplx* X;
    int N, nout;
    const void* val[FH_FAN_MAX];      // values of A_{k_t} on the pattern
    cplx* Y[FH_FAN_MAX];
    int flags[FH_FAN_MAX];            // bit 0: accumulate, bit 1: negate
};
struct fh_fan_out { int k; cplx* Y; bool accumulate, negate; };

template <typename VT, int LD>
__global__ __launch_bounds__(FH_BLOCK) void k_spmm_fan(fh_fan_args a) {
    constexpr int ROWS = FH_BLOCK / LD;          // rows of a workgroup
    const int c = threadIdx.x % LD;
    const int i = blockIdx.x * ROWS + threadIdx.x / LD;
    if (i >= a.N) return;
    const int* __restrict__ colidx = a.col;
    const cplx* __restrict__ X = a.X;
    const int k0 = a.rowptr[i], k1 = a.rowptr[i + 1];
    cplx acc[FH_FAN_MAX];
#pragma unroll
    for (int t = 0; t < FH_FAN_MAX; ++t) acc[t] = cmake(0, 0);
    POLY_ROW_GATHER(LD, colidx, X, k0, k1, c, k, x,
        _Pragma("unroll") for (int t = 0; t < FH_FAN_MAX; ++t)
            if (t < a.nout) acc[t] = cadd(acc[t], vmul(((const VT*)a.val[t])[k], x));
    )
    const size_t e = (size_t)i * LD + c;
#pragma unroll
    for (int t = 0; t < FH_FAN_MAX; ++t)
        if (t < a.nout) {
            cplx r = (a.flags[t] & 2) ? cmake(-acc[t].x, -acc[t].y) : acc[t];
            if (a.flags[t] & 1) r = cadd(a.Y[t][e], r);
            a.Y[t][e] = r;
        }
}

// ---------------------------------------------------------------------------------------
// RHS_e = R_last + sum_{p < nd} z_e^p D_p for every node in one pass: the nd + 1 panels are read once, ne panels written
// (stride: what fh_direct_solve_nodes takes as rhs_stride).  D: nd panels of `total` elements one behind the other.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(FH_BLOCK) void k_poly_rhs(const cplx* __restrict__ Rlast, const cplx* __restrict__ D, int nd,
                                                        const cplx* __restrict__ z, int ne, cplx* __restrict__ RHS, size_t stride,
                                                        size_t total) {
    for (size_t e = (size_t)blockIdx.x * FH_BLOCK + threadIdx.x; e < total; e += (size_t)gridDim.x * FH_BLOCK) {
        const cplx r = Rlast[e];
        cplx dv[PD];
#pragma unroll
        for (int p = 0; p < PD; ++p) dv[p] = p < nd ? D[(size_t)p * total + e] : cmake(0, 0);
        // (Horner written out, not fh_horner<PD - 1>(nd - 1, ...): guarded by p <= nd - 1 the compiler keeps eight scalar
        //  compares in the node loop that p < nd lets it hoist, and the kernel ran 5 % longer)
        for (int q = 0; q < ne; ++q) {
            const cplx zz = z[q];
            cplx v = cmake(0, 0);
#pragma unroll
            for (int p = PD - 1; p >= 0; --p)
                if (p < nd) v = cadd(cmul(v, zz), dv[p]);
            RHS[(size_t)q * stride + e] = cadd(r, v);
        }
    }
}

// ---------------------------------------------------------------------------------------
// The sweep's epilogue in one pass over the nodes' Y_0 panels: per panel element d accumulators,
//     y = Y_0e;  acc_0 += w_e y;  y = z_e y - R_i;  acc_{i+1} += w_e y   (i = 0 .. d-2),
// and the d blocks of Q_proj = sum_e w_e Y_e written once.  No dN-row per-node panel exists.  R, OUT: tall panels (block i
// at i * total).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(FH_BLOCK) void k_poly_expand_sum(const cplx* __restrict__ Y, size_t stride, const cplx* __restrict__ R,
                                                               int d, const cplx* __restrict__ z, const cplx* __restrict__ w, int ne,
                                                               cplx* __restrict__ OUT, size_t total) {
    for (size_t e = (size_t)blockIdx.x * FH_BLOCK + threadIdx.x; e < total; e += (size_t)gridDim.x * FH_BLOCK) {
        cplx acc[PD], r[PD - 1];
#pragma unroll
        for (int i = 0; i < PD; ++i) acc[i] = cmake(0, 0);
#pragma unroll
        for (int i = 0; i < PD - 1; ++i) r[i] = i < d - 1 ? R[(size_t)i * total + e] : cmake(0, 0);
        for (int q = 0; q < ne; ++q) {
            const cplx zz = z[q], ww = w[q];
            cplx y = Y[(size_t)q * stride + e];
            cfma(acc[0], ww, y);
#pragma unroll
            for (int i = 0; i < PD - 1; ++i)
                if (i < d - 1) {
                    y = csub(cmul(zz, y), r[i]);
                    cfma(acc[i + 1], ww, y);
                }
        }
#pragma unroll
        for (int i = 0; i < PD; ++i)
            if (i < d) OUT[(size_t)i * total + e] = acc[i];
    }
}

// ---------------------------------------------------------------------------------------
// Residuals of the Ritz pairs, fused with their column norms.  Per column c (lambda = lam[c]) three sums of squares over the
// rows, as partial[block][3][ld]:
//   [0]  || A_lin x - lambda B_lin x ||^2  (use_B = 0: || A_lin x - lambda x ||^2, the reference's measure,
//        src/kernel/feast_kernel.jl:899-906): blocks i < d-1 are x_{i+1} - lambda x_i, the last one -T - lambda (U | x_{d-1})
//        with T = sum_j A_j x_j and U = A_d x_{d-1}
//   [1]  || sum_k lambda^k (A_k x_0) ||^2 = || P(lambda) x_0 ||^2 from the d + 1 product panels PK (Horner)
//   [2]  || x_0 ||^2
// X: tall panel; T, U: N x ld panels; PK: d + 1 panels one behind the other.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(FH_BLOCK) void k_poly_residual(const cplx* __restrict__ X, const cplx* __restrict__ T, const cplx* __restrict__ U,
                                                             const cplx* __restrict__ PK, const cplx* __restrict__ lam, int d, int use_B,
                                                             int ld, size_t total, double* __restrict__ partial) {
    __shared__ double red[3][FH_BLOCK];
    const int t = threadIdx.x;
    const cplx l = lam[t % ld];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (size_t e = (size_t)blockIdx.x * FH_BLOCK + t; e < total; e += (size_t)gridDim.x * FH_BLOCK) {   // (the stride keeps the column)
        cplx xp = X[e];
        s2 += cabs2(xp);
#pragma unroll
        for (int b = 0; b < PD - 1; ++b)
            if (b < d - 1) {
                const cplx xn = X[(size_t)(b + 1) * total + e];
                s0 += cabs2(csub(xn, cmul(l, xp)));
                xp = xn;
            }
        const cplx bx = use_B ? U[e] : xp;
        const cplx tt = T[e];
        s0 += cabs2(cadd(tt, cmul(l, bx)));
        s1 += cabs2(fh_horner<PD>(d, l, [&](int k) { return PK[(size_t)k * total + e]; }));
    }
    red[0][t] = s0; red[1][t] = s1; red[2][t] = s2;
    __syncthreads();
    if (t < ld) {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        for (int j = t; j < FH_BLOCK; j += ld) { a0 += red[0][j]; a1 += red[1][j]; a2 += red[2][j]; }
        double* o = partial + (size_t)blockIdx.x * 3 * ld;
        o[t] = a0; o[ld + t] = a1; o[2 * ld + t] = a2;
    }
}
// out[3][ld] = sum over the blocks' partials, in block order
__global__ __launch_bounds__(FH_BLOCK) void k_poly_residual_fin(const double* __restrict__ partial, int nblk, int n, double* __restrict__ out) {
    for (int i = threadIdx.x; i < n; i += FH_BLOCK) {
        double s = 0.0;
        for (int b = 0; b < nblk; ++b) s += partial[(size_t)b * n + i];
        out[i] = s;
    }
}

// ---------------------------------------------------------------------------------------
// Projected method (feasthip_poly_eval_cols_dev and the calls built on it): R[:, c] = P(lambda_c) X[:, c] on sparse
// coefficients in one pass.  The row-slice layout of k_spmm_fan (lane <-> column, LD lanes own a row, gathers batched four
// deep); per nonzero the column index, the d + 1 coefficient values and the gathered X row are loaded once, the lane forms
// sum_k a_k lambda_c^k by Horner in registers (lambda_c loaded once per row slice) and adds its product with the X element to ONE
// accumulator.  A nout = d + 1 fan-out holds d + 1 accumulators, writes d + 1 panels and needs a pass that combines them.
// No atomics, the row sum runs in CSR order: reproducible.
// Algorithmic traffic: nnz (4 + (d + 1) sizeof(VT)) of matrix, one X row of 16 LD B gathered per nonzero, N LD 16 B written.
// ---------------------------------------------------------------------------------------
struct fh_horner_args {
    const int* rowptr; const int* col;
    const cplx* X; const cplx* lam;   // N x LD panel, LD per-column values
    cplx* Y;
    int N, d;
    fh_poly_ptrs val;
};

template <typename VT, int LD>
__global__ __launch_bounds__(FH_BLOCK) void k_spmm_horner(fh_horner_args a) {
    constexpr int ROWS = FH_BLOCK / LD;
    const int c = threadIdx.x % LD;
    const int i = blockIdx.x * ROWS + threadIdx.x / LD;
    if (i >= a.N) return;
    const int* __restrict__ colidx = a.col;
    const cplx* __restrict__ X = a.X;
    const cplx l = a.lam[c];
    const int k0 = a.rowptr[i], k1 = a.rowptr[i + 1];
    cplx acc = cmake(0, 0);
    POLY_ROW_GATHER(LD, colidx, X, k0, k1, c, k, x,
        cfma(acc, fh_horner<PD>(a.d, l, [&](int j) { return poly_val(((const VT*)a.val.c[j])[k]); }), x);
    )
    a.Y[(size_t)i * LD + c] = acc;
}

// The table form for a term handle (feasthip_nep_eval_cols_dev and the calls built on it): R[:, c] = sum_k F[k][c] A_k X[:, c].
// a.lam is the nt x LD table, term-major, so the lanes of a row slice read consecutive values; a lane loads its nt scalars once
// into registers before the row's nonzeros (at most 9 complex values).  Same layout, same traffic, same order as above.
template <typename VT, int LD>
__global__ __launch_bounds__(FH_BLOCK) void k_spmm_terms(fh_horner_args a) {
    constexpr int ROWS = FH_BLOCK / LD;
    const int c = threadIdx.x % LD;
    const int i = blockIdx.x * ROWS + threadIdx.x / LD;
    if (i >= a.N) return;
    const int* __restrict__ colidx = a.col;
    const cplx* __restrict__ X = a.X;
    const int nt = a.d + 1;
    cplx f[PD + 1];
#pragma unroll
    for (int j = 0; j <= PD; ++j) f[j] = j < nt ? a.lam[(size_t)j * LD + c] : cmake(0, 0);
    const int k0 = a.rowptr[i], k1 = a.rowptr[i + 1];
    cplx acc = cmake(0, 0);
    POLY_ROW_GATHER(LD, colidx, X, k0, k1, c, k, x,
        cfma(acc, fh_term_sum<PD>(nt, [&](int j) { return f[j]; }, [&](int j) { return poly_val(((const VT*)a.val.c[j])[k]); }), x);
    )
    a.Y[(size_t)i * LD + c] = acc;
}

// ---------------------------------------------------------------------------------------
// The residual-inverse sweep's sum in one pass over the ne node-solution panels, nodes in ascending e, one write per element:
//     Q[i, c] = sum_e T[e][c] (X[i, c] - Y_e[i, c]),   T[e][c] = w_e / (z_e - sigma_c)   (host table, ne x ld)
// X == null: the plain sweep Q = sum_e T[e][c] Y_e with T[e][c] = w_e.  (The grid stride is a multiple of ld: a thread keeps its
// column.)  Traffic: ne + 1 panels read, one written.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(FH_BLOCK) void k_poly_resinv_acc(const cplx* __restrict__ X, const cplx* __restrict__ Y, size_t stride,
                                                               const cplx* __restrict__ T, int ne, int ld, cplx* __restrict__ Q, size_t total) {
    const int c = threadIdx.x % ld;
    for (size_t e = (size_t)blockIdx.x * FH_BLOCK + threadIdx.x; e < total; e += (size_t)gridDim.x * FH_BLOCK) {
        const cplx x = X ? X[e] : cmake(0, 0);
        cplx acc = cmake(0, 0);
#pragma unroll 4
        for (int q = 0; q < ne; ++q) {
            const cplx y = Y[(size_t)q * stride + e];
            cfma(acc, T[(size_t)q * ld + c], X ? csub(x, y) : y);
        }
        Q[e] = acc;
    }
}

// ---------------------------------------------------------------------------------------
// Krylov solvers on P(z) (sparse handle; fh_api.hip: fh_apply_operator): the node-batched operator product
//     Y_e = P(z_e) X_e     or     Y_e = Bvec - P(z_e) X_e      e = 0 .. nodes-1
// with the fused dots the batched BiCGStab / COCG / GMRES drivers read (dot modes 0 .. 4 of fh_sparse.hip, same conjugation):
//     1: partial1 = <U, Y>      2: partial1 = <Y, X>, partial2 = <Y, Y>      3: partial2 = <Y, Y>      4: partial1 = X^T Y
// The row-slice layout of k_spmm_fan / k_spmm_horner (LD lanes own a row, lane <-> column, gathers batched four deep); per
// nonzero s = sum_k a_k z_e^k is formed by Horner in registers from the d + 1 value arrays -- P(z_e) is never materialised.
// The node loop is outermost (as in k_spmm), z_e comes from a device table, an inactive node is skipped and its partial rows
// cleared.  Persistent grid of 8 S <= FH_POLYOP_GRID_MAX workgroups, ONE partial row per workgroup and node,
// partial[(node nprow + blockIdx.x) LD + c] with nprow = gridDim.x: a thread adds its rows in ascending order, the FH_BLOCK / LD
// threads of a column are added through LDS in thread order.  No atomics: reproducible.
// Rows to workgroups as in k_spmm: XCD group g = blockIdx.x & 7 owns row slice g of ceil(N / 8) rows and its S workgroups sweep
// it as a moving band of S ROWS consecutive rows, so a gathered X line is wanted by one private L2 only and lives there for the
// stencil's reuse distance.  Y is written and Bvec / U are read with non-temporal accesses: they stream past the X window.
// (Placement affects speed only.)
// Algorithmic traffic per active node: nnz (4 + (d + 1) sizeof(VT)) of matrix, one X row of 16 LD B gathered per nonzero,
// N LD 16 B written, as much read for each of Bvec, U and (modes 2, 4) the row's own X element.
// ---------------------------------------------------------------------------------------
#define FH_POLYOP_GRID_MAX 1024
struct fh_polyop_args {
    const int* rowptr; const int* col;
    fh_poly_ptrs val;
    int N, d, nodes;
    fh_polyop_call c;
    unsigned long long* counters;     // profiling: [0] active node-launches, [1] active column x vector passes (may be null)
};

template <typename VT, int LD>
__global__ __launch_bounds__(FH_BLOCK) void k_spmm_poly(fh_polyop_args a) {
    constexpr int ROWS = FH_BLOCK / LD;
    __shared__ cplx red[FH_BLOCK];
    const int t = threadIdx.x;
    const int c = t % LD, r = t / LD;
    const int* __restrict__ rowptr = a.rowptr;
    const int* __restrict__ colidx = a.col;
    const int nprow = gridDim.x;
    const int mode = a.c.dot_mode;
    const int S = nprow >> 3, grp = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int slice_rows = (a.N + 7) / 8;
    const int row_lo = min(a.N, grp * slice_rows), row_hi = min(a.N, row_lo + slice_rows);
    for (int node = 0; node < a.nodes; ++node) {
        const size_t pbase = ((size_t)node * nprow + blockIdx.x) * LD;
        if (a.c.node_active && a.c.node_active[node] == 0) {          // (uniform over the workgroup)
            if (mode != 0 && t < LD) {
                if (a.c.partial1) a.c.partial1[pbase + t] = cmake(0, 0);
                if (a.c.partial2) a.c.partial2[pbase + t] = cmake(0, 0);
            }
            continue;
        }
        if (a.counters && blockIdx.x == 0 && t == 0) {
            const int cols = a.c.node_active ? a.c.node_active[node] : a.c.m;
            atomicAdd(a.counters + 0, 1ull);
            atomicAdd(a.counters + 1, (unsigned long long)(cols * ((mode == 1 || a.c.Bvec) ? 3 : 2)));
        }
        const cplx* __restrict__ X = a.c.X + (size_t)node * a.c.x_node_stride;
        cplx* __restrict__ Y = a.c.Y + (size_t)node * a.c.y_node_stride;
        const cplx* __restrict__ Bv = a.c.Bvec ? a.c.Bvec + (size_t)node * a.c.b_node_stride : nullptr;
        const cplx* __restrict__ U = a.c.U ? a.c.U + (size_t)node * a.c.u_node_stride : nullptr;
        const cplx z = a.c.znode[(size_t)node * a.c.z_stride];
        cplx d1 = cmake(0, 0), d2 = cmake(0, 0);
        for (int i = row_lo + slot * ROWS + r; i < row_hi; i += S * ROWS) {
            const int k0 = rowptr[i], k1 = rowptr[i + 1];
            cplx acc = cmake(0, 0);
            // per nonzero the d + 1 values are read and P(z_e)[i, j] formed by Horner.  (Written out, not fh_horner: with the
            // helper inlined here the compiler contracts the <Y, Y> dot below the other way round, x x + (y y) for y y + (x x),
            // and the Krylov solves would leave the bits they have had.)
            POLY_ROW_GATHER(LD, colidx, X, k0, k1, c, k, x,
                cplx v = cmake(0, 0);
                _Pragma("unroll") for (int j = PD; j >= 0; --j)
                    if (j <= a.d) v = cadd(cmul(v, z), poly_val(((const VT*)a.val.c[j])[k]));
                cfma(acc, v, x);
            )
            const size_t e = (size_t)i * LD + c;
            if (Bv) acc = csub(fh_ld_nt(Bv + e), acc);
            fh_st_nt(Y + e, acc);
            if (mode == 1) d1 = cadd(d1, cmulc(fh_ld_nt(U + e), acc));
            else if (mode == 2) { d1 = cadd(d1, cmulc(acc, X[e])); d2.x += cabs2(acc); }
            else if (mode == 3) d2.x += cabs2(acc);
            else if (mode == 4) d1 = cadd(d1, cmul(X[e], acc));          // unconjugated p^T (S p), COCG
        }
        if (mode != 0 && mode != 3) fh_column_sum<LD, FH_BLOCK>(red, t, d1, a.c.partial1 + pbase);
        if (mode == 2 || mode == 3) fh_column_sum<LD, FH_BLOCK>(red, t, d2, a.c.partial2 + pbase);
    }
}

// 8 S workgroups: S per row slice, enough for one pass over the slice up to the grid limit
int fh_poly_op_nblk(int N, int ld) {
    const int rows = FH_BLOCK / ld, slice_rows = (N + 7) / 8;
    return 8 * std::max(1, std::min(FH_POLYOP_GRID_MAX / 8, (slice_rows + rows - 1) / rows));
}

int fh_launch_spmm_poly(feasthip_ctx* h, int ld, const fh_polyop_call& c) {
    fh_polyop_args a;
    memset(&a, 0, sizeof(a));
    a.rowptr = h->csr.rowptr; a.col = h->csr.col; a.N = (int)h->csr.N; a.d = h->poly.degree; a.nodes = c.nodes;
    a.val = fh_poly_coef_ptrs(h);
    a.c = c;
    a.counters = h->profiling ? h->d_counters : nullptr;
    const int nprow = fh_poly_op_nblk(a.N, ld);
    fh_prof_begin(h, "spmm_poly");
    POLY_LAUNCH_CSR(k_spmm_poly, ld, dim3((unsigned)nprow), a);
    fh_prof_end(h);
    return nprow;
}

// ---------------------------------------------------------------------------------------
// Count estimate (feasthip_poly_estimate_count): t_c = v_c^T sum_e w_e T'(z_e) T(z_e)^-1 v_c with T'(z_e) = sum_k g_k(z_e) A_k.
// The node sum commutes with the matrices, sum_e w_e T'(z_e) Y_e = sum_k A_k Z_k, so two kernels follow the solves Y_e =
// T(z_e)^-1 V: the fan-out k_node_combine forms the Z_k, the fan-in k_spmm_fanin_trace (CSR coefficients) takes the trace of
// sum_k A_k Z_k against V without writing the product.
//
// k_node_combine: Z_t[i, c] = sum_e G[e][t] Y_e[i, c] for t < nt kept terms, G the ne x nt host table w_e g_k(z_e) of the kept
// terms.  The sibling of k_poly_resinv_acc with a fan-out: a thread owns panel elements, reads every Y_e element once, nodes in
// ascending e, and holds the nt <= 9 sums in registers.  G[e][t] has the same address in every lane, so its loads are scalar
// ones whatever ne is.  No atomics.  Traffic: ne panels read, nt written.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(FH_BLOCK) void k_node_combine(const cplx* __restrict__ Y, size_t stride, const cplx* __restrict__ G, int ne,
                                                            int nt, cplx* __restrict__ Z, size_t total) {
    for (size_t e = (size_t)blockIdx.x * FH_BLOCK + threadIdx.x; e < total; e += (size_t)gridDim.x * FH_BLOCK) {
        cplx acc[PD + 1];
#pragma unroll
        for (int t = 0; t <= PD; ++t) acc[t] = cmake(0, 0);
#pragma unroll 4          // (four node loads in flight per thread, as in k_poly_resinv_acc)
        for (int q = 0; q < ne; ++q) {
            const cplx y = Y[(size_t)q * stride + e];
            const cplx* __restrict__ g = G + (size_t)q * nt;
#pragma unroll
            for (int t = 0; t <= PD; ++t)
                if (t < nt) cfma(acc[t], g[t], y);
        }
#pragma unroll
        for (int t = 0; t <= PD; ++t)
            if (t < nt) Z[(size_t)t * total + e] = acc[t];
    }
}

// k_spmm_fanin_trace: partial sums of t_c = sum_i v(i, col0 + c) sum_t sum_j A_{k_t}[i, j] Z_t[j, c] over nt panels Z_t (one
// behind the other, zstride apart).  The row-slice layout of k_spmm_fan / k_spmm_horner; per nonzero the column index is loaded
// once, then the nt values and the nt gathered rows, into ONE accumulator per lane (gathers batched two deep: 2 nt rows in
// flight).  v is regenerated from (seed, row, column) as in k_trace_partials (fh_estimate.hip); the block V is never read.  A
// workgroup walks its rows in ascending order, its FH_BLOCK / LD threads of a column are added through LDS in thread order, and
// it writes ONE partial row, partial[c nprow + blockIdx.x] with nprow = gridDim.x -- the layout k_trace_finish sums in block
// order.  No atomics: reproducible.
// Algorithmic traffic: nnz (4 + nt sizeof(VT)) of matrix, nt rows of 16 LD B gathered per nonzero, nothing written but the partials.
#define FH_FANIN_GRID_MAX 1024
struct fh_fanin_args {
    const int* rowptr; const int* col;
    const cplx* Z; size_t zstride;
    int N, nt;
    const void* val[FH_FAN_MAX];      // values of the kept A_k on the pattern
    uint64_t seed; int64_t col0;
    cplx* partial;
};

template <typename VT, int LD>
__global__ __launch_bounds__(FH_BLOCK) void k_spmm_fanin_trace(fh_fanin_args a) {
    constexpr int ROWS = FH_BLOCK / LD;
    __shared__ cplx red[FH_BLOCK];
    const int t = threadIdx.x;
    const int c = t % LD;
    const int* __restrict__ colidx = a.col;
    const cplx* __restrict__ Z = a.Z;
    cplx dsum = cmake(0, 0);
    for (int i = blockIdx.x * ROWS + t / LD; i < a.N; i += gridDim.x * ROWS) {
        const int k0 = a.rowptr[i], k1 = a.rowptr[i + 1];
        cplx acc = cmake(0, 0);
        POLY_ROW_GATHER_N(FH_FAN_MAX, 2, LD, colidx, Z, a.zstride, a.nt, k0, k1, c, k, zs,
            _Pragma("unroll") for (int p = 0; p < FH_FAN_MAX; ++p)
                if (p < a.nt) acc = cadd(acc, vmul(((const VT*)a.val[p])[k], zs[p]));
        )
        const double v = fh_rademacher(fh_row_key(a.seed, i), a.col0 + c);
        dsum.x += v * acc.x;
        dsum.y += v * acc.y;
    }
    fh_column_sum<LD, FH_BLOCK>(red, t, dsum, a.partial + blockIdx.x, gridDim.x);
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
// true: the handle's solver is a Krylov method on the operator P(z_e) (CSR coefficients only)
static bool poly_krylov(const feasthip_ctx* h) {
    return h->solver == FEASTHIP_SOLVER_BICGSTAB || h->solver == FEASTHIP_SOLVER_COCG || h->solver == FEASTHIP_SOLVER_GMRES;
}

// What every feasthip_poly_* call needs, linearised or projected: a polynomial handle whose solver the solves with P(z_e)
// cover -- FEASTHIP_SOLVER_LU (the dense LU, or the multifrontal one for CSR coefficients), or for CSR coefficients the plain
// BiCGStab / COCG / GMRES on the operator -- complex128 factors, no adjoint, one rank, the whole contour, and 1 <= m <= maxm.
// what: the entry point's name for the message.  form: which scalar form of the handle the call serves -- POLY_POWERS (the
// default: a polynomial handle only, the call forms powers of lambda), POLY_ANY_FORM (coefficients only) or POLY_TERMS (a term
// handle with its node table set for the current contour).
enum { POLY_POWERS = 0, POLY_ANY_FORM = 1, POLY_TERMS = 2 };
static int poly_check(feasthip_ctx* h, const char* what, int64_t m, int64_t maxm, int form = POLY_POWERS) {
    if (int gate = fh_gate(h)) return gate;
    const char* why = nullptr;
    const bool top = h->kind == FH_KIND_TERM_OPERATOR;
    if (top && (why = fh_termop_solver_why(h, h->shifted ? FEASTHIP_SOLVER_SHIFTED_COCG : h->block ? FEASTHIP_SOLVER_BLOCK_COCG : h->solver, h->factor_precision))) {}
    else if (h->kind == FH_KIND_OPERATOR) why = "an operator handle (feasthip_set_operator) has no polynomial or term form: it takes the pencil entry points under the Krylov solvers FEASTHIP_SOLVER_BICGSTAB, _COCG or _GMRES";
    else if (h->kind != FH_KIND_POLYNOMIAL && !top) why = "needs a polynomial handle (feasthip_set_polynomial); a dense or CSR handle takes the entry points without poly_";
    else if (top && form == POLY_POWERS) why = "forms powers of lambda or linearised columns, which a split form does not have: " FH_TERMOP_TAKES ", through the feasthip_nep_* calls with tables of the f_k";
    else if (h->poly.terms && form == POLY_POWERS)
        why = "forms powers of lambda, which a term handle (feasthip_set_terms) does not have: use feasthip_nep_solve_dev, feasthip_nep_eval_cols_dev, "
              "feasthip_nep_resinv_apply_dev or feasthip_nep_ritz_eval_dev with tables of the f_k";
    else if (!h->poly.terms && form == POLY_TERMS) why = "needs a term handle (feasthip_set_terms / feasthip_set_terms_csr); a polynomial handle takes the feasthip_poly_* calls";
    else if (top) {}          // (its solver was looked at above)
    else if (h->poly.terms && h->solver != FEASTHIP_SOLVER_LU) why = "the solver of a term handle must be FEASTHIP_SOLVER_LU (Krylov solves on T(z) are not provided)";
    else if (h->solver != FEASTHIP_SOLVER_LU && !(poly_krylov(h) && h->poly.sparse && !h->shifted && !h->block))
        why = h->poly.sparse ? "the solver must be FEASTHIP_SOLVER_LU, _BICGSTAB, _COCG or _GMRES" : "the solver of a dense polynomial handle must be FEASTHIP_SOLVER_LU";
    if (why) {}
    else if (h->factor_precision != 64) why = "factor_precision = 32 is not supported (complex128 factors only)";
    else if (h->adjoint) why = "the adjoint switch is not supported";
    else if (h->comm) why = "an attached communicator is not supported (one rank)";
    else if (h->node_count != (int)h->zne.size() || h->node_first != 0) why = "a node range or list is not supported (the whole contour on one rank)";
    else
        for (int e = 0; e < (int)h->node_ids.size(); ++e)
            if (h->node_ids[e] != e) { why = "a node range or list is not supported (the whole contour on one rank)"; break; }
    if (why) { h->last_error = std::string(what) + ": " + why; return FEASTHIP_ERROR_FPM; }
    if (m <= 0 || m > maxm) { h->last_error = std::string(what) + ": block width out of range"; return FEASTHIP_ERROR_M0; }
    if (top) h->op.failed = 0;          // a new entry point: the callback is tried again
    return 0;
}
// the widest subspace of a projected-method call: N on a polynomial, term or term-operator handle
static int64_t poly_rows(const feasthip_ctx* h) { return h && (h->kind == FH_KIND_POLYNOMIAL || h->kind == FH_KIND_TERM_OPERATOR) ? h->dense.N : 1; }
// a feasthip_nep_* call that solves with T(z_e): the node table belongs to the handle's contour
static int nep_check_nodes(feasthip_ctx* h, const char* what) {
    const size_t ne = h->zne.size();
    bool ok = ne > 0 && h->poly.fnode_z.size() == ne && h->poly.fnode.size() == ne * (size_t)(h->poly.degree + 1);
    for (size_t e = 0; ok && e < ne; ++e) ok = h->poly.fnode_z[e].x == h->zne[e].x && h->poly.fnode_z[e].y == h->zne[e].y;
    if (!ok) { h->last_error = std::string(what) + ": no node values for the current contour (feasthip_set_contour, then feasthip_nep_set_node_values)"; return FEASTHIP_ERROR_FPM; }
    return 0;
}

// sum_k |lambda|^k ||A_k||_F, the scale of the backward errors
static double poly_bwd_scale(const feasthip_ctx* h, double la) {
    double scale = 0.0, pw = 1.0;
    for (int k = 0; k <= h->poly.degree; ++k) { scale += pw * h->poly.fro[k]; pw *= la; }
    return scale;
}

// its sibling for a term handle: sum_k |f[k]| ||A_k||_F from one row of a table
static double nep_bwd_scale(const feasthip_ctx* h, const cplx* f) {
    double scale = 0.0;
    for (int k = 0; k <= h->poly.degree; ++k) scale += std::hypot(f[k].x, f[k].y) * h->poly.fro[k];
    return scale;
}
static bool nep_row_finite(const feasthip_ctx* h, const cplx* f) {
    for (int k = 0; k <= h->poly.degree; ++k)
        if (!std::isfinite(f[k].x) || !std::isfinite(f[k].y)) return false;
    return true;
}

// small synchronous host -> device copy into a named workspace
template <typename T> static int poly_upload(feasthip_ctx* h, const char* name, const std::vector<T>& host, T** dev) {
    int rc = fh_buf(h, name, host.size(), dev);
    if (rc) return rc;
    FH_CHECK(hipMemcpyAsync(*dev, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice, h->stream));
    FH_CHECK(hipStreamSynchronize(h->stream));
    return 0;
}

// the unit, minus-unit and zero coefficient vectors the dense product kernel selects with
struct poly_coefs {
    cplx *plus = nullptr, *minus = nullptr, *zero = nullptr;
    int acquire(feasthip_ctx* h) {
        std::vector<cplx> c(3 * FH_MAX_LD, cmake(0, 0));
        for (int i = 0; i < FH_MAX_LD; ++i) { c[i] = cmake(1, 0); c[FH_MAX_LD + i] = cmake(-1, 0); }
        cplx* d;
        const int rc = poly_upload(h, "poly_coefs", c, &d);
        if (rc) return rc;
        plus = d; minus = d + FH_MAX_LD; zero = d + 2 * FH_MAX_LD;
        return 0;
    }
};

// Y = s A_k X (accumulate: Y += s A_k X), s = -1 when negate, on N x ld panels, through the dense product kernel with the
// coefficient pointer in place of dense.A and no B.  (accumulate: the kernel's Y = Bvec - ca A X with Bvec = Y, every element
// read and written by the one lane that owns it.)
static void poly_product(feasthip_ctx* h, const poly_coefs& pc, int ld, int k, const cplx* X, cplx* Y, bool accumulate, bool negate) {
    fh_dense_op_args a;
    memset(&a, 0, sizeof(a));
    a.A = h->poly.coef[k]; a.B = nullptr; a.N = (int)h->dense.N; a.is_complex = h->dense.is_complex; a.nodes = 1;
    a.X = X; a.Y = Y;
    a.coefB = pc.zero;
    if (!accumulate) a.coefA = negate ? pc.minus : pc.plus;
    else { a.coefA = negate ? pc.plus : pc.minus; a.Bvec = Y; }
    fh_prof_begin(h, "dense_op");
    fh_launch_dense_op(a, ld, fh_dense_op_nblk(a.N), h->stream);
    fh_prof_end(h);
}

// Sparse handle: outs[t].Y = +-A_{outs[t].k} X (+ its old value) for nout <= FH_FAN_MAX outputs in one launch of k_spmm_fan
static void poly_fan(feasthip_ctx* h, int ld, const cplx* X, const fh_fan_out* outs, int nout) {
    fh_fan_args a;
    memset(&a, 0, sizeof(a));
    a.rowptr = h->csr.rowptr; a.col = h->csr.col; a.X = X; a.N = (int)h->csr.N; a.nout = nout;
    const fh_poly_ptrs P = fh_poly_coef_ptrs(h);
    for (int t = 0; t < nout; ++t) {
        a.val[t] = P.c[outs[t].k]; a.Y[t] = outs[t].Y;
        a.flags[t] = (outs[t].accumulate ? 1 : 0) | (outs[t].negate ? 2 : 0);
    }
    fh_prof_begin(h, "poly_spmm");
    POLY_LAUNCH_CSR(k_spmm_fan, ld, dim3((unsigned)((a.N + FH_BLOCK / ld - 1) / (FH_BLOCK / ld))), a);
    fh_prof_end(h);
}

// Y = s A_k X (accumulate: Y += s A_k X) on either flavour of handle
static void poly_apply(feasthip_ctx* h, const poly_coefs& pc, int ld, int k, const cplx* X, cplx* Y, bool accumulate, bool negate) {
    if (h->poly.sparse) { const fh_fan_out o{k, Y, accumulate, negate}; poly_fan(h, ld, X, &o, 1); }
    else poly_product(h, pc, ld, k, X, Y, accumulate, negate);
}

// The products of the residual step on a sparse handle, T = sum_{k<d} A_k x_k, U = A_d x_{d-1} (use_B) and PK_k = A_k x_0, in d
// launches instead of 2 d + 2: x_0 fans to A_0 .. A_d (the PK panels; T starts as a copy of PK_0 = A_0 x_0), one launch adds
// A_j x_j to T for each x_j in between, x_{d-1} fans to A_{d-1} (into T) and A_d (U).  X: tall panel.
static int poly_residual_fan(feasthip_ctx* h, int ld, bool use_B, const cplx* X, cplx* T, cplx* U, cplx* PK) {
    const int d = h->poly.degree;
    const size_t panel = (size_t)h->dense.N * ld;
    fh_fan_out outs[FH_FAN_MAX];
    for (int k = 0; k <= d; ++k) outs[k] = fh_fan_out{k, PK + (size_t)k * panel, false, false};
    poly_fan(h, ld, X, outs, d + 1);
    FH_CHECK(hipMemcpyAsync(T, PK, panel * sizeof(cplx), hipMemcpyDeviceToDevice, h->stream));
    if (d == 1) {
        if (use_B) FH_CHECK(hipMemcpyAsync(U, PK + panel, panel * sizeof(cplx), hipMemcpyDeviceToDevice, h->stream));
        return 0;
    }
    for (int k = 1; k <= d - 2; ++k) { outs[0] = fh_fan_out{k, T, true, false}; poly_fan(h, ld, X + (size_t)k * panel, outs, 1); }
    outs[0] = fh_fan_out{d - 1, T, true, false};
    outs[1] = fh_fan_out{d, U, false, false};
    poly_fan(h, ld, X + (size_t)(d - 1) * panel, outs, use_B ? 2 : 1);
    return 0;
}

// W = A_lin X (which 0) or B_lin X (which 1) on tall panels: block shifts, -sum_j A_j X_j and A_d X_{d-1}
static int poly_lin_product(feasthip_ctx* h, const poly_coefs& pc, int which, int ld, const cplx* X, cplx* W) {
    const int d = h->poly.degree;
    const size_t panel = (size_t)h->dense.N * ld;
    cplx* last = W + (size_t)(d - 1) * panel;
    if (d > 1) FH_CHECK(hipMemcpyAsync(W, which == 0 ? X + panel : X, (size_t)(d - 1) * panel * sizeof(cplx), hipMemcpyDeviceToDevice, h->stream));
    if (which == 0) for (int j = 0; j < d; ++j) poly_apply(h, pc, ld, j, X + (size_t)j * panel, last, j > 0, true);
    else poly_apply(h, pc, ld, d, X + (size_t)(d - 1) * panel, last, false, false);
    return 0;
}

// The two setters' shared steps.  poly_set_check: the handle, N <= Nmax and the degree (what: the setter's name for the
// message).  poly_set_begin: the handle's problem replaced by an empty polynomial of this size.  poly_sumsq: the sum of squares
// of n doubles, for ||A_k||_F of the backward error (ingest arithmetic, once per problem).  poly_set_commit: the handle is a
// polynomial one.
static int poly_set_check(feasthip_ctx* h, const char* what, int64_t N, int64_t Nmax, int degree, bool terms = false) {
    if (int gate = fh_gate(h)) return gate;
    if (N <= 0 || N > Nmax) { h->last_error = std::string(what) + ": N out of range"; return FEASTHIP_ERROR_N; }
    if (degree < 1 || degree > FEASTHIP_POLY_MAX_DEGREE) {
        h->last_error = std::string(what) + (terms ? ": nterms must be 2 .. FEASTHIP_POLY_MAX_DEGREE + 1" : ": degree must be 1 .. FEASTHIP_POLY_MAX_DEGREE");
        return FEASTHIP_ERROR_FPM;
    }
    return 0;
}
static int poly_set_begin(feasthip_ctx* h, int64_t N, int degree, int is_complex) {
    FH_CHECK(hipSetDevice(h->device));
    FH_CHECK(hipStreamSynchronize(h->stream));
    fh_free_problem(h);
    h->dense.N = N; h->dense.is_complex = is_complex ? 1 : 0; h->dense.b_identity = 0;
    h->poly.degree = degree;
    return 0;
}
static double poly_sumsq(const double* v, size_t n) {
    double s = 0.0;
    for (size_t i = 0; i < n; ++i) s += v[i] * v[i];
    return s;
}
static int poly_set_commit(feasthip_ctx* h, bool terms = false) {
    h->adjoint = 0;
    h->kind = FH_KIND_POLYNOMIAL;
    h->poly.terms = terms ? 1 : 0;
    if (terms) { h->solver = FEASTHIP_SOLVER_LU; h->shifted = h->block = 0; h->factor_precision = 64; }
    return 0;
}

// (both setters: `what` the entry point's name; terms: the matrices are the A_k of a split form, feasthip_set_terms[_csr])
static int poly_set_dense(feasthip_ctx* h, const std::string& what, bool terms, int64_t N, int degree, int is_complex, const void* const* coeffs,
                          const int64_t* ld) {
    int rc = poly_set_check(h, what.c_str(), N, 65536, degree, terms);
    if (rc) return rc;
    if (!coeffs || !ld) { h->last_error = what + ": null argument"; return FEASTHIP_ERROR_N; }
    for (int k = 0; k <= degree; ++k)
        if (!coeffs[k] || ld[k] < N) { h->last_error = what + ": bad coefficient pointer or leading dimension"; return FEASTHIP_ERROR_N; }
    if ((rc = poly_set_begin(h, N, degree, is_complex))) return rc;
    const size_t es = is_complex ? sizeof(cplx) : sizeof(double), per = is_complex ? 2 : 1;
    for (int k = 0; k <= degree; ++k) {
        FH_CHECK(hipMalloc(&h->poly.coef[k], (size_t)N * N * es));
        FH_CHECK(hipMemcpy2D(h->poly.coef[k], (size_t)N * es, coeffs[k], (size_t)ld[k] * es, (size_t)N * es, (size_t)N, hipMemcpyHostToDevice));
        double s = 0.0;          // column by column
        for (int64_t j = 0; j < N; ++j) s += poly_sumsq((const double*)coeffs[k] + (size_t)j * ld[k] * per, (size_t)N * per);
        h->poly.fro[k] = std::sqrt(s);
    }
    return poly_set_commit(h, terms);
}
extern "C" int feasthip_set_polynomial(feasthip_handle h, int64_t N, int degree, int is_complex, const void* const* coeffs,
                                       const int64_t* ld) {
    return poly_set_dense(h, "feasthip_set_polynomial", false, N, degree, is_complex, coeffs, ld);
}
extern "C" int feasthip_set_terms(feasthip_handle h, int64_t N, int nterms, int is_complex, const void* const* mats, const int64_t* ld) {
    return poly_set_dense(h, "feasthip_set_terms", true, N, nterms - 1, is_complex, mats, ld);
}

// Sparse coefficients on one CSR pattern (0-based, columns strictly increasing inside a row, so no duplicates): the multifrontal
// LU of P(z_e) (fh_banded.hip plans it, k_mf_assemble_poly forms the fronts) in place of the dense one, k_spmm_fan in place of
// the dense product.  The pattern is kept in the caller's order (no renumbering: the multifrontal plan brings its own).
static int poly_set_csr(feasthip_ctx* h, const std::string& what, bool terms, int64_t N, int degree, int is_complex, const int64_t* rowptr,
                        const int64_t* col, const void* const* vals) {
    int rc = poly_set_check(h, what.c_str(), N, INT32_MAX / FH_MAX_LD / FEASTHIP_POLY_MAX_DEGREE, degree, terms);
    if (rc) return rc;
    if (!rowptr || !vals) { h->last_error = what + ": null argument"; return FEASTHIP_ERROR_N; }
    if (rowptr[0] != 0) { h->last_error = what + ": rowptr[0] must be 0"; return FEASTHIP_ERROR_N; }
    for (int64_t i = 0; i < N; ++i)
        if (rowptr[i + 1] < rowptr[i]) { h->last_error = what + ": row pointers not monotone at row " + std::to_string(i); return FEASTHIP_ERROR_N; }
    const int64_t nnz = rowptr[N];
    if (nnz > INT32_MAX) { h->last_error = what + ": more than 2^31 - 1 nonzeros"; return FEASTHIP_ERROR_N; }
    if (nnz > 0 && !col) { h->last_error = what + ": null column array"; return FEASTHIP_ERROR_N; }
    for (int k = 0; k <= degree; ++k)
        if (nnz > 0 && !vals[k]) { h->last_error = what + ": null value array of coefficient " + std::to_string(k); return FEASTHIP_ERROR_N; }
    std::vector<int> rp((size_t)N + 1), cl((size_t)nnz);
    for (int64_t i = 0; i < N; ++i) {
        rp[i] = (int)rowptr[i];
        for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
            if (col[k] < 0 || col[k] >= N) { h->last_error = what + ": column index out of range in row " + std::to_string(i); return FEASTHIP_ERROR_N; }
            if (k > rowptr[i] && col[k] <= col[k - 1]) { h->last_error = what + ": columns of row " + std::to_string(i) + " are not strictly increasing"; return FEASTHIP_ERROR_N; }
            cl[k] = (int)col[k];
        }
    }
    rp[N] = (int)nnz;
    if ((rc = poly_set_begin(h, N, degree, is_complex))) return rc;
    const size_t es = is_complex ? sizeof(cplx) : sizeof(double);
    h->poly.sparse = 1;
    fh_csr& c = h->csr;
    c.N = N; c.nnz = nnz; c.is_complex = is_complex ? 1 : 0; c.b_identity = 0;
    FH_CHECK(hipMalloc((void**)&c.rowptr, ((size_t)N + 1) * sizeof(int)));
    FH_CHECK(hipMalloc((void**)&c.col, std::max<size_t>(1, (size_t)nnz) * sizeof(int)));
    FH_CHECK(hipMemcpy(c.rowptr, rp.data(), ((size_t)N + 1) * sizeof(int), hipMemcpyHostToDevice));
    if (nnz) FH_CHECK(hipMemcpy(c.col, cl.data(), (size_t)nnz * sizeof(int), hipMemcpyHostToDevice));
    for (int k = 0; k <= degree; ++k) {
        FH_CHECK(hipMalloc(&h->poly.coef[k], std::max<size_t>(1, (size_t)nnz) * es));
        if (nnz) FH_CHECK(hipMemcpy(h->poly.coef[k], vals[k], (size_t)nnz * es, hipMemcpyHostToDevice));
        h->poly.fro[k] = std::sqrt(poly_sumsq((const double*)vals[k], (size_t)nnz * (is_complex ? 2 : 1)));      // (the explicit zeros add nothing)
    }
    h->host_rowptr.swap(rp); h->host_col.swap(cl);
    return poly_set_commit(h, terms);
}
extern "C" int feasthip_set_polynomial_csr(feasthip_handle h, int64_t N, int degree, int is_complex, const int64_t* rowptr,
                                           const int64_t* col, const void* const* vals) {
    return poly_set_csr(h, "feasthip_set_polynomial_csr", false, N, degree, is_complex, rowptr, col, vals);
}
extern "C" int feasthip_set_terms_csr(feasthip_handle h, int64_t N, int nterms, int is_complex, const int64_t* rowptr, const int64_t* col,
                                      const void* const* vals) {
    return poly_set_csr(h, "feasthip_set_terms_csr", true, N, nterms - 1, is_complex, rowptr, col, vals);
}

// The node table of a term handle: F[e * nterms + k] = f_k(z_e) for the contour set last.  Factors cached for other values are dropped.
extern "C" int feasthip_nep_set_node_values(feasthip_handle h, int ne, const void* F_host) {
    int rc = poly_check(h, "feasthip_nep_set_node_values", 1, 1, POLY_TERMS);
    if (rc) return rc;
    const int nt = h->poly.degree + 1;
    if (!F_host || ne != (int)h->zne.size() || ne <= 0) {
        h->last_error = "feasthip_nep_set_node_values: ne must be the node count of the contour set before (feasthip_set_contour), F not null";
        return FEASTHIP_ERROR_FPM;
    }
    const cplx* F = (const cplx*)F_host;
    for (int i = 0; i < ne * nt; ++i)
        if (!std::isfinite(F[i].x) || !std::isfinite(F[i].y)) {
            h->last_error = "feasthip_nep_set_node_values: f_" + std::to_string(i % nt) + " is not finite at contour node " + std::to_string(i / nt);
            return FEASTHIP_ERROR_FPM;
        }
    bool same = h->poly.fnode.size() == (size_t)ne * nt && h->poly.fnode_z.size() == (size_t)ne;
    for (int i = 0; same && i < ne * nt; ++i) same = h->poly.fnode[i].x == F[i].x && h->poly.fnode[i].y == F[i].y;
    for (int e = 0; same && e < ne; ++e) same = h->poly.fnode_z[e].x == h->zne[e].x && h->poly.fnode_z[e].y == h->zne[e].y;
    if (same) return 0;
    if ((rc = feasthip_release_factors(h))) return rc;          // the cache matches by z_e alone
    h->poly.fnode.assign(F, F + (size_t)ne * nt);
    h->poly.fnode_z = h->zne;
    return 0;
}

// Krylov solves P(z_e) Y_e = RHS for the nodes z (one right-hand-side panel shared by all of them), from a zero start, under the
// handle's rtol / atol / maxit / restart, through the batched drivers of fh_api.hip on the operator k_spmm_poly.  status[e] = 5
// for a node with a column that did not pass the stop test.  The counts go into `it`.
struct poly_iters {
    int64_t sum = 0, op_calls = 0;
    double max_rel_res = 0.0;
    std::vector<int> node, col;       // per node: most steps of a column; [node][m]
};
static int poly_krylov_nodes(feasthip_ctx* h, int ld, int m, const std::vector<cplx>& z, const cplx* RHS, size_t panel, cplx* Y,
                             std::vector<int>& status, poly_iters& it) {
    const int ne = (int)z.size();
    FH_CHECK(hipMemsetAsync(Y, 0, (size_t)ne * panel * sizeof(cplx), h->stream));
    fh_solve_result sr;
    const int rc = h->solver == FEASTHIP_SOLVER_GMRES ? fh_gmres(h, ld, m, ne, z, RHS, Y, panel, sr)
                                                      : fh_krylov(h, h->solver == FEASTHIP_SOLVER_COCG ? 1 : 0, 64, ld, m, ne, z, RHS, Y, panel, sr, fh_krylov_opts());
    if (rc) return rc;
    status = sr.status;
    it.sum += sr.iters_sum; it.op_calls += sr.op_calls; it.max_rel_res = std::max(it.max_rel_res, sr.max_rel_res);
    it.node = sr.node_iters; it.col = sr.col_iters;
    return 0;
}

// Y = P(z)^-1 Rhs under the handle's solver: the Krylov solves above, else the dense LU of P(z), for sparse coefficients the
// multifrontal one through the factor cache of the sparse direct solver (same slots, same matching by z)
static int poly_solve_single(feasthip_ctx* h, int ld, int m, cplx z, const cplx* Rhs, cplx* Y, int* status, int64_t* nfact, poly_iters& it) {
    if (poly_krylov(h)) {
        std::vector<int> st;
        const int rc = poly_krylov_nodes(h, ld, m, std::vector<cplx>(1, z), Rhs, (size_t)h->dense.N * ld, Y, st, it);
        if (!rc) *status = st[0];
        return rc;
    }
    return fh_direct_solve_single(h, h->poly.sparse != 0, ld, m, z, Rhs, Y, status, nfact);
}
// The same for every contour node, Y_e = P(z_e)^-1 RHS_e (rhs_stride: `panel` for one right-hand side panel per node, 0 for
// one panel shared by all nodes -- the only form the Krylov drivers take)
static int poly_solve_nodes(feasthip_ctx* h, int ld, int m, int ne, const cplx* RHS, size_t rhs_stride, size_t panel, cplx* Y, std::vector<int>& status, int64_t* nfact, poly_iters& it) {
    if (poly_krylov(h)) {
        if (rhs_stride != 0) { h->last_error = "internal: a Krylov solver takes one right-hand-side panel shared by the nodes"; return FEASTHIP_ERROR_INTERNAL; }
        return poly_krylov_nodes(h, ld, m, h->zne, RHS, panel, Y, status, it);
    }
    return fh_direct_solve_nodes(h, h->poly.sparse != 0, ld, m, ne, h->zne, RHS, rhs_stride, Y, panel, status, nfact);
}

// The Krylov counts of a call that ran `ne` nodes on m64 columns in 64-column panels: the statistics, and what
// feasthip_last_node_iterations / feasthip_last_column_iterations report ([node][m64]; a node's count is its slowest column's)
struct poly_iter_record {
    int ne; int64_t m64;
    poly_iters tot;
    std::vector<int> node, col;
    poly_iter_record(int ne_, int64_t m64_) : ne(ne_), m64(m64_), node(ne_, 0), col((size_t)ne_ * m64_, 0) {}
    void panel(const poly_iters& it, int64_t c0, int m) {
        for (int e = 0; e < ne && e < (int)it.node.size(); ++e) {
            node[e] = std::max(node[e], it.node[e]);
            for (int c = 0; c < m; ++c) col[(size_t)e * m64 + c0 + c] = it.col[(size_t)e * m + c];
        }
    }
    void publish(feasthip_ctx* h, const poly_iters& it, feasthip_stats* stats) {
        h->last_node_iters = node; h->last_col_iters = col; h->last_col_m = (int)m64;
        if (stats) { stats->krylov_iterations = it.sum; stats->spmm_calls = it.op_calls; stats->max_rel_residual = it.max_rel_res; }
    }
};

// Y = P(z)^-1 R, N x m column-major; the factor is cached in the slot of the contour node z equals, else in one extra slot
static int poly_solve_body(feasthip_ctx* h, const std::string& what, double z_re, double z_im, int64_t m64, const void* dR, void* dY,
                           feasthip_stats* stats) {
    int rc;
    if (!dR || !dY) { h->last_error = what + ": null argument"; return FEASTHIP_ERROR_INTERNAL; }
    FH_CHECK(hipSetDevice(h->device));
    const double t0 = fh_now_s();
    const int N = (int)h->dense.N;
    if (stats) memset(stats, 0, sizeof(*stats));
    int worst = 0;
    poly_iters it;
    poly_iter_record rec(1, m64);
    for (int64_t c0 = 0; c0 < m64; c0 += FH_MAX_LD) {
        const int m = (int)std::min<int64_t>(FH_MAX_LD, m64 - c0), ld = fh_pick_ld(m);
        const size_t panel = (size_t)N * ld;
        cplx *Rhs, *Y;
        if ((rc = fh_buf(h, "ps_rhs", panel, &Rhs))) return rc;
        if ((rc = fh_buf(h, "ps_Y", panel, &Y))) return rc;
        fh_launch_to_panel((const cplx*)dR + (size_t)c0 * N, N, N, m, Rhs, ld, h->stream);
        int status = 0;
        int64_t nfact = 0;
        if ((rc = poly_solve_single(h, ld, m, cmake(z_re, z_im), Rhs, Y, &status, &nfact, it))) return rc;
        if (poly_krylov(h)) rec.panel(it, c0, m);
        fh_launch_from_panel(Y, ld, N, m, (cplx*)dY + (size_t)c0 * N, N, h->stream);
        if (stats) stats->factorizations += nfact;
        worst = std::max(worst, status);
    }
    if ((rc = fh_finish(h))) return rc;
    if (poly_krylov(h)) rec.publish(h, it, stats);
    if (stats) stats->seconds_total = fh_now_s() - t0;
    return worst;
}
extern "C" int feasthip_poly_solve_dev(feasthip_handle h, double z_re, double z_im, int64_t m64, const void* dR, void* dY,
                                       feasthip_stats* stats) {
    const int rc = poly_check(h, "feasthip_poly_solve_dev", m64, 1 << 20);       // right-hand sides, not a subspace: any count
    return rc ? rc : poly_solve_body(h, "feasthip_poly_solve_dev", z_re, z_im, m64, dR, dY, stats);
}
// Term handle: Y = T(z_e)^-1 R for the contour node `node`, N x m column-major, on the cached factor of that node
extern "C" int feasthip_nep_solve_dev(feasthip_handle h, int node, int64_t m64, const void* dR, void* dY, feasthip_stats* stats) {
    int rc = poly_check(h, "feasthip_nep_solve_dev", m64, 1 << 20, POLY_TERMS);
    if (rc || (rc = nep_check_nodes(h, "feasthip_nep_solve_dev"))) return rc;
    if (node < 0 || node >= (int)h->zne.size()) { h->last_error = "feasthip_nep_solve_dev: node index outside the contour"; return FEASTHIP_ERROR_FPM; }
    return poly_solve_body(h, "feasthip_nep_solve_dev", h->zne[node].x, h->zne[node].y, m64, dR, dY, stats);
}

// Qproj = sum_e weight_scale w_e (z_e B_lin - A_lin)^-1 (B_lin Q) on dN x m column-major blocks
extern "C" int feasthip_poly_contour_apply_dev(feasthip_handle h, int64_t m64, const void* dQ, void* dQproj, int* node_status,
                                               feasthip_stats* stats) {
    int rc = poly_check(h, "feasthip_poly_contour_apply_dev", m64, h && h->kind == FH_KIND_POLYNOMIAL ? h->dense.N * h->poly.degree : 1);
    if (rc) return rc;
    if (!dQ || !dQproj) { h->last_error = "feasthip_poly_contour_apply_dev: null argument"; return FEASTHIP_ERROR_INTERNAL; }
    if (h->zne.empty()) { h->last_error = "feasthip_poly_contour_apply_dev: no contour set (feasthip_set_contour)"; return FEASTHIP_ERROR_FPM; }
    if (h->real_projection) { h->last_error = "feasthip_poly_contour_apply_dev: the real projection does not apply to a polynomial sweep"; return FEASTHIP_ERROR_FPM; }
    if (poly_krylov(h)) {
        h->last_error = "feasthip_poly_contour_apply_dev: the linearised sweep has one right-hand side per node, which the Krylov solvers do not take; "
                        "under a Krylov solver use the projected method (feasthip_poly_resinv_apply_dev), or FEASTHIP_SOLVER_LU";
        return FEASTHIP_ERROR_FPM;
    }
    FH_CHECK(hipSetDevice(h->device));
    const double t0 = fh_now_s();
    const int N = (int)h->dense.N, d = h->poly.degree, ne = (int)h->zne.size();
    const int64_t dN = (int64_t)d * N;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (node_status) for (int e = 0; e < ne; ++e) node_status[e] = 0;
    poly_coefs pc;
    if ((rc = pc.acquire(h))) return rc;
    std::vector<cplx> zw(2 * (size_t)ne);
    for (int e = 0; e < ne; ++e) { zw[e] = h->zne[e]; zw[ne + e] = cscale(h->wne[e], h->weight_scale); }
    cplx* dzw;
    if ((rc = poly_upload(h, "pc_zw", zw, &dzw))) return rc;
    const int nd = d == 1 ? 0 : d;          // D panels the right-hand side reads (degree 1: none, the pencil's own sweep)
    for (int64_t c0 = 0; c0 < m64; c0 += FH_MAX_LD) {
        const int m = (int)std::min<int64_t>(FH_MAX_LD, m64 - c0), ld = fh_pick_ld(m);
        const size_t panel = (size_t)N * ld;
        cplx *Qs, *Rs, *D, *RHS, *Y, *OUT;
        if ((rc = fh_buf(h, "pc_Q", (size_t)d * panel, &Qs))) return rc;
        if ((rc = fh_buf(h, "pc_R", (size_t)d * panel, &Rs))) return rc;
        if ((rc = fh_buf(h, "pc_D", (size_t)std::max(1, nd) * panel, &D))) return rc;
        if ((rc = fh_buf(h, "pc_rhs", (size_t)ne * panel, &RHS))) return rc;
        if ((rc = fh_buf(h, "pc_Y", (size_t)ne * panel, &Y))) return rc;
        if ((rc = fh_buf(h, "pc_out", (size_t)d * panel, &OUT))) return rc;
        fh_launch_to_panel((const cplx*)dQ + (size_t)c0 * dN, dN, (int)dN, m, Qs, ld, h->stream);
        if ((rc = poly_lin_product(h, pc, 1, ld, Qs, Rs))) return rc;              // R = B_lin Q
        // D_p = sum_k A_{k+1+p} R_k: d (d + 1) / 2 - 1 products per sweep, whatever the node count.  Sparse: one launch per R_k
        // fanning over p (d - 1 launches; with R_{d-1} above, d per sweep), each D_p still summed in ascending k.
        if (h->poly.sparse) {
            for (int k = 0; k <= d - 2; ++k) {
                fh_fan_out outs[FH_FAN_MAX];
                int nout = 0;
                for (int p = 0; p <= d - 1 - k; ++p) outs[nout++] = fh_fan_out{k + 1 + p, D + (size_t)p * panel, k > 0, false};
                poly_fan(h, ld, Rs + (size_t)k * panel, outs, nout);
            }
        } else {
            for (int p = 0; p < nd; ++p)
                for (int k = 0; k <= std::min(d - 2, d - 1 - p); ++k)
                    poly_product(h, pc, ld, k + 1 + p, Rs + (size_t)k * panel, D + (size_t)p * panel, k > 0, false);
        }
        const dim3 grid(fh_vec_nblk(N, ld)), block(FH_BLOCK);
        fh_prof_begin(h, "poly_rhs");
        hipLaunchKernelGGL(k_poly_rhs, grid, block, 0, h->stream, Rs + (size_t)(d - 1) * panel, D, nd, dzw, ne, RHS, panel, panel);
        fh_prof_end(h);
        std::vector<int> status;
        int64_t nfact = 0;
        poly_iters none;
        if ((rc = poly_solve_nodes(h, ld, m, ne, RHS, panel, panel, Y, status, &nfact, none))) return rc;
        fh_prof_begin(h, "poly_expand");
        hipLaunchKernelGGL(k_poly_expand_sum, grid, block, 0, h->stream, Y, panel, Rs, d, dzw, dzw + ne, ne, OUT, panel);
        fh_prof_end(h);
        fh_launch_from_panel(OUT, ld, (int)dN, m, (cplx*)dQproj + (size_t)c0 * dN, dN, h->stream);
        if (stats) stats->factorizations += nfact;
        if (node_status) for (int e = 0; e < ne; ++e) node_status[e] = std::max(node_status[e], status[e]);
    }
    if ((rc = fh_finish(h))) return rc;
    if (stats) stats->seconds_total = fh_now_s() - t0;
    return 0;
}

// The operator of the Krylov solvers as a product of its own (which 2, 3, 4 of feasthip_poly_matmul_dev): CSR coefficients, a
// contour of ne nodes, m <= 64; X and Y hold ne blocks of N x m (column-major) one behind the other.
//   2: Y_e = P(z_e) X_e      3: Y_e = B - P(z_e) X_e, B = block 0 of Y on entry      4: Y_e = B_e - P(z_e) X_e, B_e = block e of Y on entry
static int poly_node_products(feasthip_ctx* h, int which, int64_t m64, const cplx* dX, cplx* dY) {
    const char* why = nullptr;
    if (!h->poly.sparse) why = "the node products (which 2, 3, 4) need CSR coefficients (feasthip_set_polynomial_csr)";
    else if (h->zne.empty()) why = "the node products (which 2, 3, 4) need a contour (feasthip_set_contour)";
    if (why) { h->last_error = std::string("feasthip_poly_matmul_dev: ") + why; return FEASTHIP_ERROR_FPM; }
    if (m64 > FH_MAX_LD) { h->last_error = "feasthip_poly_matmul_dev: the node products take at most 64 columns"; return FEASTHIP_ERROR_M0; }
    FH_CHECK(hipSetDevice(h->device));
    const int N = (int)h->dense.N, ne = (int)h->zne.size(), m = (int)m64, ld = fh_pick_ld(m);
    const size_t panel = (size_t)N * ld, blockN = (size_t)N * m;
    const int nb = which == 4 ? ne : which == 3 ? 1 : 0;
    int rc;
    cplx *Xs, *Ys, *Bs, *dz;
    if ((rc = fh_buf(h, "pn_X", (size_t)ne * panel, &Xs))) return rc;
    if ((rc = fh_buf(h, "pn_Y", (size_t)ne * panel, &Ys))) return rc;
    if ((rc = fh_buf(h, "pn_B", (size_t)std::max(1, nb) * panel, &Bs))) return rc;
    if ((rc = poly_upload(h, "pn_z", h->zne, &dz))) return rc;
    for (int e = 0; e < ne; ++e) fh_launch_to_panel(dX + (size_t)e * blockN, N, N, m, Xs + (size_t)e * panel, ld, h->stream);
    for (int e = 0; e < nb; ++e) fh_launch_to_panel(dY + (size_t)e * blockN, N, N, m, Bs + (size_t)e * panel, ld, h->stream);
    fh_polyop_call c;
    memset(&c, 0, sizeof(c));
    c.X = Xs; c.x_node_stride = panel; c.Y = Ys; c.y_node_stride = panel; c.znode = dz; c.z_stride = 1;
    c.Bvec = nb ? Bs : nullptr; c.b_node_stride = which == 4 ? panel : 0;
    c.nodes = ne; c.m = m;
    fh_launch_spmm_poly(h, ld, c);
    for (int e = 0; e < ne; ++e) fh_launch_from_panel(Ys + (size_t)e * panel, ld, N, m, dY + (size_t)e * blockN, N, h->stream);
    return fh_finish(h);
}

// Y = A_lin X (which 0) or B_lin X (which 1), dN x m column-major; which 2, 3, 4: poly_node_products
extern "C" int feasthip_poly_matmul_dev(feasthip_handle h, int which, int64_t m64, const void* dX, void* dY) {
    int rc = poly_check(h, "feasthip_poly_matmul_dev", m64, h && h->kind == FH_KIND_POLYNOMIAL ? h->dense.N * h->poly.degree : 1);
    if (rc) return rc;
    if (!dX || !dY || which < 0 || which > 4) { h->last_error = "feasthip_poly_matmul_dev: bad argument"; return FEASTHIP_ERROR_INTERNAL; }
    if (which >= 2) return poly_node_products(h, which, m64, (const cplx*)dX, (cplx*)dY);
    FH_CHECK(hipSetDevice(h->device));
    const int N = (int)h->dense.N, d = h->poly.degree;
    const int64_t dN = (int64_t)d * N;
    poly_coefs pc;
    if ((rc = pc.acquire(h))) return rc;
    for (int64_t c0 = 0; c0 < m64; c0 += FH_MAX_LD) {
        const int m = (int)std::min<int64_t>(FH_MAX_LD, m64 - c0), ld = fh_pick_ld(m);
        const size_t tall = (size_t)dN * ld;
        cplx *Xs, *Ws;
        if ((rc = fh_buf(h, "pm_X", tall, &Xs))) return rc;
        if ((rc = fh_buf(h, "pm_W", tall, &Ws))) return rc;
        fh_launch_to_panel((const cplx*)dX + (size_t)c0 * dN, dN, (int)dN, m, Xs, ld, h->stream);
        if ((rc = poly_lin_product(h, pc, which, ld, Xs, Ws))) return rc;
        fh_launch_from_panel(Ws, ld, (int)dN, m, (cplx*)dY + (size_t)c0 * dN, dN, h->stream);
    }
    return fh_finish(h);
}

// The blocked Gram projection of both methods: out[w] = Q^H W_w, w < nops (raw products, r x r column-major on the host), Q:
// rows x r column-major on the device, by 64-column panels.  Per block column j, form(ld, Qj, W) writes the nops product panels
// W + w rows ld of the staged panel Q_j; then per block (i, j) one Gram launch over the rows per product, ONE download and the
// scatter into the host blocks.  buf: the entry point's workspace names for Q_i, Q_j, the products and the Gram blocks.
template <typename F>
static int poly_project_blocks(feasthip_ctx* h, const char* const (&buf)[4], int64_t rows, int r, int nops, const cplx* dQ,
                               cplx* const* out, F&& form) {
    const int ld = r > FH_MAX_LD ? FH_MAX_LD : fh_pick_ld(r), npan = (r + ld - 1) / ld;
    const size_t tall = (size_t)rows * ld, g2 = (size_t)ld * ld;
    int rc;
    cplx *Qi, *Qj, *W, *G, *gw;
    if ((rc = fh_buf(h, buf[0], tall, &Qi))) return rc;
    if ((rc = fh_buf(h, buf[1], tall, &Qj))) return rc;
    if ((rc = fh_buf(h, buf[2], nops * tall, &W))) return rc;
    if ((rc = fh_buf(h, buf[3], nops * g2, &G))) return rc;
    if ((rc = fh_buf(h, "gram_work", fh_gram_work_elems(ld), &gw))) return rc;
    std::vector<cplx> Gh(nops * g2);
    for (int j = 0; j < npan; ++j) {
        const int mj = std::min(ld, r - j * ld);
        fh_launch_to_panel(dQ + (size_t)j * ld * rows, rows, (int)rows, mj, Qj, ld, h->stream);
        if ((rc = form(ld, Qj, W))) return rc;
        for (int i = 0; i < npan; ++i) {
            const int mi = std::min(ld, r - i * ld);
            const cplx* Ql = Qj;
            if (i != j) { fh_launch_to_panel(dQ + (size_t)i * ld * rows, rows, (int)rows, mi, Qi, ld, h->stream); Ql = Qi; }
            for (int w = 0; w < nops; ++w) {
                fh_prof_begin(h, "gram");
                fh_launch_gram(Ql, W + w * tall, (int)rows, ld, 0, gw, G + w * g2, h->stream);
                fh_prof_end(h);
            }
            FH_CHECK(hipMemcpyAsync(Gh.data(), G, Gh.size() * sizeof(cplx), hipMemcpyDeviceToHost, h->stream));
            FH_CHECK(hipStreamSynchronize(h->stream));
            for (int w = 0; w < nops; ++w)
                for (int c2 = 0; c2 < mj; ++c2)
                    for (int c1 = 0; c1 < mi; ++c1)
                        out[w][(size_t)(j * ld + c2) * r + i * ld + c1] = Gh[w * g2 + (size_t)c2 * ld + c1];
        }
    }
    fh_prof_collect(h);          // (every block ended on a synchronisation)
    FH_CHECK(hipGetLastError());
    return 0;
}

// Aq = Q^H A_lin Q, Sq = Q^H B_lin Q (raw products, r x r column-major on the host) by 64-column panels: block (i, j) is
// Q_i^H (op Q_j), one linearised product per block column and operator, one Gram launch over the dN rows per block
extern "C" int feasthip_poly_project_dev(feasthip_handle h, int64_t r64, const void* dQ, void* Aq_host, void* Sq_host) {
    int rc = poly_check(h, "feasthip_poly_project_dev", r64, h && h->kind == FH_KIND_POLYNOMIAL ? h->dense.N * h->poly.degree : 1);
    if (rc) return rc;
    if (!dQ || !Aq_host || !Sq_host) { h->last_error = "feasthip_poly_project_dev: null argument"; return FEASTHIP_ERROR_INTERNAL; }
    FH_CHECK(hipSetDevice(h->device));
    const int64_t dN = h->dense.N * h->poly.degree;
    poly_coefs pc;
    if ((rc = pc.acquire(h))) return rc;
    cplx* const out[2] = {(cplx*)Aq_host, (cplx*)Sq_host};
    return poly_project_blocks(h, {"pp_Qi", "pp_Qj", "pp_W", "pp_G"}, dN, (int)r64, 2, (const cplx*)dQ, out, [&](int ld, const cplx* Qj, cplx* W) {
        for (int which = 0; which < 2; ++which)
            if (const int e = poly_lin_product(h, pc, which, ld, Qj, W + (size_t)which * dN * ld)) return e;
        return 0;
    });
}

// The Ritz back-transform of both methods, block column j of X = Q V on `rows`-row panels: ws.X = sum_i Q_i V_ij (Q: rows x r
// column-major on the device, V: r x nc column-major on the host, V_ij uploaded as a zero-padded ld x ld block into the
// workspace ws.vname), its first nnorm columns scaled to unit length, its mj columns written to block column j of dX.
struct poly_ritz_ws { const char* vname; cplx *Q, *X, *T, *part, *dots; };
static int poly_ritz_vectors(feasthip_ctx* h, const poly_coefs& pc, const poly_ritz_ws& ws, int64_t rows, int r, int64_t nc, int ld,
                             int64_t j, const cplx* dQ, const cplx* Vh, int mj, int nnorm, cplx* dX) {
    std::vector<cplx> Vp;
    for (int i = 0; i < (r + ld - 1) / ld; ++i) {
        fh_pad_block(Vh, r, nc, ld, i, j, nullptr, Vp);
        cplx* dV;
        const int rc = poly_upload(h, ws.vname, Vp, &dV);
        if (rc) return rc;
        fh_launch_to_panel(dQ + (size_t)i * ld * rows, rows, (int)rows, std::min(ld, r - i * ld), ws.Q, ld, h->stream);
        fh_prof_begin(h, "ritz");
        if (i == 0) fh_launch_small_matmul(ws.Q, dV, (int)rows, ld, ws.X, h->stream);
        else {
            fh_launch_small_matmul(ws.Q, dV, (int)rows, ld, ws.T, h->stream);
            fh_launch_axpy_cols(ws.X, ws.T, pc.minus, (int)rows, ld, h->stream);          // X += T
        }
        fh_prof_end(h);
    }
    if (nnorm > 0) {
        fh_launch_dot_cols(ws.X, ws.X, (int)rows, ld, ws.part, ws.dots, h->stream);
        fh_launch_normalize_cols(ws.X, ws.dots, (int)rows, ld, nnorm, h->stream);
    }
    fh_launch_from_panel(ws.X, ld, (int)rows, mj, dX + (size_t)j * ld * rows, rows, h->stream);
    return 0;
}

// X = Q V (dN x r), the first M columns scaled to unit length (normalize), and for j < M
//   res[j]            = || A_lin x_j - lambda_j B_lin x_j || / max(|lambda_j|, 1)   (use_B = 0: without B_lin)
//   backward_error[j] = || P(lambda_j) x_j^(0) || / (sum_k |lambda_j|^k ||A_k||_F  ||x_j^(0)||),  x^(0) = the first block
extern "C" int feasthip_poly_ritz_residual_dev(feasthip_handle h, int64_t r64, const void* dQ, const void* V_host, const void* lambda,
                                               int64_t M, int normalize, int use_B, void* dX, double* res, double* backward_error) {
    int rc = poly_check(h, "feasthip_poly_ritz_residual_dev", r64, h && h->kind == FH_KIND_POLYNOMIAL ? h->dense.N * h->poly.degree : 1);
    if (rc) return rc;
    if (!dQ || !V_host || !lambda || !dX || dQ == dX) { h->last_error = "feasthip_poly_ritz_residual_dev: null argument, or X aliases Q"; return FEASTHIP_ERROR_INTERNAL; }
    if (M < 0 || M > r64) { h->last_error = "feasthip_poly_ritz_residual_dev: M out of range"; return FEASTHIP_ERROR_M0; }
    FH_CHECK(hipSetDevice(h->device));
    const int N = (int)h->dense.N, d = h->poly.degree, r = (int)r64;
    const int64_t dN = (int64_t)d * N;
    const int ld = r > FH_MAX_LD ? FH_MAX_LD : fh_pick_ld(r), npan = (r + ld - 1) / ld;
    const size_t panel = (size_t)N * ld, tall = (size_t)dN * ld;
    const int nblk = fh_vec_nblk(N, ld);
    poly_coefs pc;
    if ((rc = pc.acquire(h))) return rc;
    cplx *Qp, *Xp, *Tp, *Tl, *U, *PK, *part, *ddots;
    double *rpart, *rsum;
    if ((rc = fh_buf(h, "pr_Q", tall, &Qp))) return rc;
    if ((rc = fh_buf(h, "pr_X", tall, &Xp))) return rc;
    if ((rc = fh_buf(h, "pr_T", tall, &Tp))) return rc;
    if ((rc = fh_buf(h, "pr_Tl", panel, &Tl))) return rc;
    if ((rc = fh_buf(h, "pr_U", panel, &U))) return rc;
    if ((rc = fh_buf(h, "pr_PK", (size_t)(d + 1) * panel, &PK))) return rc;
    if ((rc = fh_buf(h, "pr_part", (size_t)fh_vec_nblk((int)dN, ld) * ld, &part))) return rc;
    if ((rc = fh_buf(h, "pr_dots", (size_t)ld, &ddots))) return rc;
    if ((rc = fh_buf(h, "pr_rpart", (size_t)nblk * 3 * ld, &rpart))) return rc;
    if ((rc = fh_buf(h, "pr_rsum", (size_t)3 * ld, &rsum))) return rc;
    const poly_ritz_ws ws{"pr_V", Qp, Xp, Tp, part, ddots};
    const cplx* lamh = (const cplx*)lambda;
    std::vector<cplx> lamp(ld);
    std::vector<double> sums(3 * (size_t)ld);
    for (int j = 0; j < npan; ++j) {
        const int mj = std::min(ld, r - j * ld), Mj = std::max(0, std::min(mj, (int)M - j * ld));
        if ((rc = poly_ritz_vectors(h, pc, ws, dN, r, r, ld, j, (const cplx*)dQ, (const cplx*)V_host, mj, normalize ? Mj : 0, (cplx*)dX))) return rc;
        if (Mj > 0 && (res || backward_error)) {
            if (h->poly.sparse) {
                if ((rc = poly_residual_fan(h, ld, use_B != 0, Xp, Tl, U, PK))) return rc;
            } else {
                for (int k = 0; k < d; ++k) poly_product(h, pc, ld, k, Xp + (size_t)k * panel, Tl, k > 0, false);     // T = sum_k A_k x_k
                if (use_B) poly_product(h, pc, ld, d, Xp + (size_t)(d - 1) * panel, U, false, false);               // U = A_d x_{d-1}
                for (int k = 0; k <= d; ++k) poly_product(h, pc, ld, k, Xp, PK + (size_t)k * panel, false, false);  // A_k x_0
            }
            std::fill(lamp.begin(), lamp.end(), cmake(0, 0));
            for (int c = 0; c < mj; ++c) lamp[c] = lamh[j * ld + c];
            cplx* dlam;
            if ((rc = poly_upload(h, "pr_lam", lamp, &dlam))) return rc;
            fh_prof_begin(h, "poly_residual");
            hipLaunchKernelGGL(k_poly_residual, dim3(nblk), dim3(FH_BLOCK), 0, h->stream, Xp, Tl, U, PK, dlam, d, use_B ? 1 : 0, ld, panel, rpart);
            hipLaunchKernelGGL(k_poly_residual_fin, dim3(1), dim3(FH_BLOCK), 0, h->stream, rpart, nblk, 3 * ld, rsum);
            fh_prof_end(h);
            FH_CHECK(hipMemcpyAsync(sums.data(), rsum, sums.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            FH_CHECK(hipStreamSynchronize(h->stream));
            for (int c = 0; c < Mj; ++c) {
                const double la = std::hypot(lamp[c].x, lamp[c].y);
                if (res) res[j * ld + c] = std::sqrt(sums[c]) / std::max(la, 1.0);
                if (backward_error) {
                    const double den = poly_bwd_scale(h, la) * std::sqrt(sums[2 * ld + c]);
                    backward_error[j * ld + c] = den > 0.0 ? std::sqrt(sums[ld + c]) / den : 0.0;
                }
            }
        }
    }
    return fh_finish(h);
}

// ---------------------------------------------------------------------------------------
// Projected method (method = "projected" of feast_polynomial): the subspace lives in the N-dimensional space, so every call
// below works on N x m panels and a node's solve has m right-hand sides, not m d.
// ---------------------------------------------------------------------------------------

// R[:, c] = P(lam_c) X[:, c] on one N x ld panel; dlam: ld device values.  Sparse: k_spmm_horner.  Dense: R = sum_k A_k (X diag
// lam^k) through the dense product on the column-scaled copy W of X (scaled once more per degree).  X is left as it is.
static int poly_eval_panel(feasthip_ctx* h, const poly_coefs& pc, int ld, const cplx* dlam, const cplx* X, cplx* W, cplx* R) {
    const int N = (int)h->dense.N, d = h->poly.degree;
    if (h->kind == FH_KIND_TERM_OPERATOR) {          // the callback flavour: one callback per kept term on the panel, then k_terms_combine on the column table
        fh_termop_call a;
        memset(&a, 0, sizeof(a));
        a.X = X; a.Y = R; a.F = dlam; a.cols = 1; a.terms = h->top.col_terms; a.nodes = 1;
        return fh_apply_term_operator(h, ld, a) < 0 ? (int)FEASTHIP_ERROR_INTERNAL : 0;
    }
    if (h->poly.sparse) {
        fh_horner_args a;
        memset(&a, 0, sizeof(a));
        a.rowptr = h->csr.rowptr; a.col = h->csr.col; a.X = X; a.lam = dlam; a.Y = R; a.N = N; a.d = d;
        a.val = fh_poly_coef_ptrs(h);
        const dim3 grid((unsigned)((N + FH_BLOCK / ld - 1) / (FH_BLOCK / ld)));
        fh_prof_begin(h, h->poly.terms ? "terms_spmm" : "poly_horner");
        if (h->poly.terms) POLY_LAUNCH_CSR(k_spmm_terms, ld, grid, a);
        else POLY_LAUNCH_CSR(k_spmm_horner, ld, grid, a);
        fh_prof_end(h);
        return 0;
    }
    if (h->poly.terms) {          // R = sum_k A_k (X diag F[k]): the copy of X scaled by row k of the table, per term
        for (int k = 0; k <= d; ++k) {
            FH_CHECK(hipMemcpyAsync(W, X, (size_t)N * ld * sizeof(cplx), hipMemcpyDeviceToDevice, h->stream));
            fh_prof_begin(h, "terms_scale");
            fh_launch_scale_cols(W, dlam + (size_t)k * ld, N, ld, h->stream);
            fh_prof_end(h);
            poly_product(h, pc, ld, k, W, R, k > 0, false);
        }
        return 0;
    }
    FH_CHECK(hipMemcpyAsync(W, X, (size_t)N * ld * sizeof(cplx), hipMemcpyDeviceToDevice, h->stream));
    for (int k = 0; k <= d; ++k) {
        poly_product(h, pc, ld, k, W, R, k > 0, false);
        if (k < d) {
            fh_prof_begin(h, "poly_horner");
            fh_launch_scale_cols(W, dlam, N, ld, h->stream);
            fh_prof_end(h);
        }
    }
    return 0;
}

// ld device values: v[c0 .. c0 + m) of the host array, zero padded; a non-finite entry is replaced by `instead`.  (Term handle:
// v is the caller's m x (degree + 1) table of the f_k per column, uploaded term-major for poly_eval_panel.)
static int poly_upload_cols(feasthip_ctx* h, const char* name, const cplx* v, int64_t c0, int m, int ld, cplx instead, cplx** dev) {
    std::vector<cplx> p(ld, cmake(0, 0));
    if (h->poly.terms) {          // v: rows of degree + 1 values per column -> the term-major table; a non-finite row becomes zero
        const int nt = h->poly.degree + 1;
        p.assign((size_t)nt * ld, cmake(0, 0));
        for (int c = 0; c < m; ++c)
            if (nep_row_finite(h, v + (size_t)(c0 + c) * nt))
                for (int k = 0; k < nt; ++k) p[(size_t)k * ld + c] = v[(size_t)(c0 + c) * nt + k];
        h->top.col_terms = 0;          // (term operator: the terms with a non-zero entry are the ones its callbacks produce)
        for (int k = 0; k < nt; ++k)
            for (int c = 0; c < m; ++c)
                if (p[(size_t)k * ld + c].x != 0.0 || p[(size_t)k * ld + c].y != 0.0) { h->top.col_terms |= 1u << k; break; }
        return poly_upload(h, name, p, dev);
    }
    for (int c = 0; c < m; ++c) {
        const cplx x = v[c0 + c];
        p[c] = std::isfinite(x.x) && std::isfinite(x.y) ? x : instead;
    }
    return poly_upload(h, name, p, dev);
}

// R[:, j] = P(lambda_j) X[:, j], N x m column-major, lambda: m complex values on the host
static int poly_eval_cols_body(feasthip_ctx* h, const std::string& what, int64_t m64, const void* lambda, const void* dX, void* dR) {
    int rc;
    if (!lambda || !dX || !dR) { h->last_error = what + ": null argument"; return FEASTHIP_ERROR_INTERNAL; }
    FH_CHECK(hipSetDevice(h->device));
    const int N = (int)h->dense.N;
    poly_coefs pc;
    if ((rc = pc.acquire(h))) return rc;
    for (int64_t c0 = 0; c0 < m64; c0 += FH_MAX_LD) {
        const int m = (int)std::min<int64_t>(FH_MAX_LD, m64 - c0), ld = fh_pick_ld(m);
        const size_t panel = (size_t)N * ld;
        cplx *Xs, *W, *R, *dlam;
        if ((rc = fh_buf(h, "pe_X", panel, &Xs))) return rc;
        if ((rc = fh_buf(h, "pe_W", panel, &W))) return rc;
        if ((rc = fh_buf(h, "pe_R", panel, &R))) return rc;
        if ((rc = poly_upload_cols(h, "pe_lam", (const cplx*)lambda, c0, m, ld, cmake(0, 0), &dlam))) return rc;
        fh_launch_to_panel((const cplx*)dX + (size_t)c0 * N, N, N, m, Xs, ld, h->stream);
        if ((rc = poly_eval_panel(h, pc, ld, dlam, Xs, W, R))) return rc;
        fh_launch_from_panel(R, ld, N, m, (cplx*)dR + (size_t)c0 * N, N, h->stream);
    }
    return fh_finish(h);
}
extern "C" int feasthip_poly_eval_cols_dev(feasthip_handle h, int64_t m64, const void* lambda, const void* dX, void* dR) {
    const int rc = poly_check(h, "feasthip_poly_eval_cols_dev", m64, 1 << 20);
    return rc ? rc : poly_eval_cols_body(h, "feasthip_poly_eval_cols_dev", m64, lambda, dX, dR);
}
// Term handle: R[:, j] = sum_k F[j][k] A_k X[:, j], N x m column-major, F: m x nterms on the host
extern "C" int feasthip_nep_eval_cols_dev(feasthip_handle h, int64_t m64, const void* F_host, const void* dX, void* dR) {
    const int rc = poly_check(h, "feasthip_nep_eval_cols_dev", m64, 1 << 20, POLY_TERMS);
    return rc ? rc : poly_eval_cols_body(h, "feasthip_nep_eval_cols_dev", m64, F_host, dX, dR);
}

// The contour step of the projected method on an N x m block.
//   sigma == null:  Q = sum_e w_e P(z_e)^-1 X                                                  (plain sweep)
//   else         :  R[:, j] = P(sigma_j) x_j,  Y_e = P(z_e)^-1 R,  Q[:, j] = sum_e w_e (x_j - Y_e[:, j]) / (z_e - sigma_j)
// One right-hand side panel is shared by all nodes; the factors come from the per-node cache as in the linearised sweep.
// (ftab: a term handle's m x nterms table f_k(sigma_j), which takes the place of the powers of sigma_j)
static int poly_resinv_body(feasthip_ctx* h, const std::string& what, int64_t m64, const void* sigma, const void* ftab, const void* dX, void* dQ,
                            int* node_status, feasthip_stats* stats) {
    int rc;
    if (!dX || !dQ) { h->last_error = what + ": null argument"; return FEASTHIP_ERROR_INTERNAL; }
    if (h->zne.empty()) { h->last_error = what + ": no contour set (feasthip_set_contour)"; return FEASTHIP_ERROR_FPM; }
    if (h->real_projection) { h->last_error = what + ": the real projection does not apply to a polynomial sweep"; return FEASTHIP_ERROR_FPM; }
    const int N = (int)h->dense.N, ne = (int)h->zne.size();
    const cplx* sg = (const cplx*)sigma;
    if (sg)
        for (int64_t j = 0; j < m64; ++j) {
            if (!std::isfinite(sg[j].x) || !std::isfinite(sg[j].y)) { h->last_error = what + ": shift " + std::to_string(j) + " is not finite"; return FEASTHIP_ERROR_FPM; }
            for (int e = 0; e < ne; ++e) {
                const cplx z = h->zne[e];
                const double dist = std::hypot(z.x - sg[j].x, z.y - sg[j].y), scale = std::max(std::hypot(z.x, z.y), std::hypot(sg[j].x, sg[j].y));
                if (dist <= 4.0 * 2.220446049250313e-16 * scale || dist == 0.0) {
                    h->last_error = what + ": shift " + std::to_string(j) + " coincides with contour node " + std::to_string(e);
                    return FEASTHIP_ERROR_FPM;
                }
            }
        }
    FH_CHECK(hipSetDevice(h->device));
    const double t0 = fh_now_s();
    if (stats) memset(stats, 0, sizeof(*stats));
    if (node_status) for (int e = 0; e < ne; ++e) node_status[e] = 0;
    poly_coefs pc;
    if ((rc = pc.acquire(h))) return rc;
    poly_iters it;
    poly_iter_record rec(ne, m64);
    for (int64_t c0 = 0; c0 < m64; c0 += FH_MAX_LD) {
        const int m = (int)std::min<int64_t>(FH_MAX_LD, m64 - c0), ld = fh_pick_ld(m);
        const size_t panel = (size_t)N * ld;
        cplx *Xs, *W, *R, *Y, *Q, *dlam = nullptr, *dT;
        if ((rc = fh_buf(h, "ri_X", panel, &Xs))) return rc;
        if ((rc = fh_buf(h, "ri_W", panel, &W))) return rc;
        if ((rc = fh_buf(h, "ri_R", panel, &R))) return rc;
        if ((rc = fh_buf(h, "ri_Y", (size_t)ne * panel, &Y))) return rc;
        if ((rc = fh_buf(h, "ri_Q", panel, &Q))) return rc;
        // T[e][c] = w_e / (z_e - sigma_c), or w_e for the plain sweep; the padding columns are zero
        std::vector<cplx> T((size_t)ne * ld, cmake(0, 0));
        for (int e = 0; e < ne; ++e) {
            const cplx w = cscale(h->wne[e], h->weight_scale);
            for (int c = 0; c < m; ++c) T[(size_t)e * ld + c] = sg ? cdiv(w, csub(h->zne[e], sg[c0 + c])) : w;
        }
        if ((rc = poly_upload(h, "ri_T", T, &dT))) return rc;
        fh_launch_to_panel((const cplx*)dX + (size_t)c0 * N, N, N, m, Xs, ld, h->stream);
        const cplx* rhs = Xs;
        if (sg) {
            if ((rc = poly_upload_cols(h, "ri_lam", ftab ? (const cplx*)ftab : sg, c0, m, ld, cmake(0, 0), &dlam))) return rc;
            if ((rc = poly_eval_panel(h, pc, ld, dlam, Xs, W, R))) return rc;
            rhs = R;
        }
        std::vector<int> status;
        int64_t nfact = 0;
        if ((rc = poly_solve_nodes(h, ld, m, ne, rhs, 0, panel, Y, status, &nfact, it))) return rc;
        if (poly_krylov(h)) rec.panel(it, c0, m);
        fh_prof_begin(h, "poly_resinv");
        hipLaunchKernelGGL(k_poly_resinv_acc, dim3(fh_vec_nblk(N, ld)), dim3(FH_BLOCK), 0, h->stream, sg ? Xs : (const cplx*)nullptr, Y, panel, dT, ne, ld, Q, panel);
        fh_prof_end(h);
        fh_launch_from_panel(Q, ld, N, m, (cplx*)dQ + (size_t)c0 * N, N, h->stream);
        if (stats) stats->factorizations += nfact;
        if (node_status) for (int e = 0; e < ne; ++e) node_status[e] = std::max(node_status[e], status[e]);
    }
    if ((rc = fh_finish(h))) return rc;
    if (poly_krylov(h)) rec.publish(h, it, stats);
    if (stats) stats->seconds_total = fh_now_s() - t0;
    return 0;
}
extern "C" int feasthip_poly_resinv_apply_dev(feasthip_handle h, int64_t m64, const void* sigma, const void* dX, void* dQ,
                                              int* node_status, feasthip_stats* stats) {
    const int rc = poly_check(h, "feasthip_poly_resinv_apply_dev", m64, 1 << 20);
    return rc ? rc : poly_resinv_body(h, "feasthip_poly_resinv_apply_dev", m64, sigma, nullptr, dX, dQ, node_status, stats);
}
// Term handle: the same contour step with T in place of P.  sigma and F_sigma (m x nterms on the host, F_sigma[j][k] =
// f_k(sigma_j)) both null: the plain sweep; both given: the residual-inverse sweep.
extern "C" int feasthip_nep_resinv_apply_dev(feasthip_handle h, int64_t m64, const void* sigma, const void* F_sigma, const void* dX, void* dQ,
                                             int* node_status, feasthip_stats* stats) {
    int rc = poly_check(h, "feasthip_nep_resinv_apply_dev", m64, 1 << 20, POLY_TERMS);
    if (rc || (rc = nep_check_nodes(h, "feasthip_nep_resinv_apply_dev"))) return rc;
    if ((sigma == nullptr) != (F_sigma == nullptr)) { h->last_error = "feasthip_nep_resinv_apply_dev: sigma and F_sigma go together (both null: the plain sweep)"; return FEASTHIP_ERROR_FPM; }
    if (F_sigma)
        for (int64_t j = 0; j < m64; ++j)
            if (!nep_row_finite(h, (const cplx*)F_sigma + j * (h->poly.degree + 1))) {
                h->last_error = "feasthip_nep_resinv_apply_dev: the table row of shift " + std::to_string(j) + " is not finite";
                return FEASTHIP_ERROR_FPM;
            }
    return poly_resinv_body(h, "feasthip_nep_resinv_apply_dev", m64, sigma, F_sigma, dX, dQ, node_status, stats);
}

// Count estimate of a polynomial or term handle: samples t_c = v_c^T [sum_e w_e T'(z_e) T(z_e)^-1 v_c], c < m, for the Rademacher
// block V of `seed` (the (seed, i, j) rule of fh_estimate.hip).  G_host: ne x (degree + 1), G[e][k] = w_e g_k(z_e) with T'(z) =
// sum_k g_k(z) A_k; a term whose column of G is zero at every node is dropped (A_0 of a polynomial, a constant f_k).  Per
// 64-column panel: Y_e = T(z_e)^-1 V on one shared right-hand-side panel (poly_solve_nodes: any solver of the handle, the factor
// cache as in the sweeps), Z_t = sum_e G[e][k_t] Y_e (k_node_combine), then the trace of sum_t A_{k_t} Z_t against V --
// k_spmm_fanin_trace and k_trace_finish on CSR coefficients, the dense product accumulated into one panel and the pencil
// estimate's k_trace_partials / k_trace_finish on dense ones.  dV (may be null): receives V, N x m column-major.
extern "C" int feasthip_poly_estimate_count(feasthip_handle h, int64_t m64, uint64_t seed, const void* G_host, double* samples, void* dV,
                                            int* node_status, feasthip_stats* stats) {
    const char* what = "feasthip_poly_estimate_count";
    if (h && h->kind == FH_KIND_TERM_OPERATOR && !h->poisoned) { h->last_error = std::string(what) + ": the count estimate is not provided for operators: " FH_TERMOP_TAKES ", with an integer subspace size"; return FEASTHIP_ERROR_FPM; }
    int rc = poly_check(h, what, m64, h && h->kind == FH_KIND_POLYNOMIAL ? std::min<int64_t>(h->dense.N, 65535) : 1, POLY_ANY_FORM);
    if (rc) return rc;
    if (h->poly.terms && (rc = nep_check_nodes(h, what))) return rc;
    if (!G_host || !samples) { h->last_error = std::string(what) + ": null argument"; return FEASTHIP_ERROR_INTERNAL; }
    if (h->zne.empty()) { h->last_error = std::string(what) + ": no contour set (feasthip_set_contour)"; return FEASTHIP_ERROR_FPM; }
    if (h->real_projection) { h->last_error = std::string(what) + ": the real projection does not apply to a polynomial sweep"; return FEASTHIP_ERROR_FPM; }
    const int N = (int)h->dense.N, ne = (int)h->zne.size(), nt = h->poly.degree + 1;
    const cplx* Gh = (const cplx*)G_host;
    for (int i = 0; i < ne * nt; ++i)
        if (!std::isfinite(Gh[i].x) || !std::isfinite(Gh[i].y)) {
            h->last_error = std::string(what) + ": G is not finite at contour node " + std::to_string(i / nt) + ", term " + std::to_string(i % nt);
            return FEASTHIP_ERROR_FPM;
        }
    int kept[PD + 1], ntk = 0;
    for (int k = 0; k < nt; ++k) {
        bool zero = true;
        for (int e = 0; zero && e < ne; ++e) zero = Gh[(size_t)e * nt + k].x == 0.0 && Gh[(size_t)e * nt + k].y == 0.0;
        if (!zero) kept[ntk++] = k;
    }
    std::vector<cplx> Gk((size_t)ne * std::max(1, ntk));
    for (int e = 0; e < ne; ++e)
        for (int t = 0; t < ntk; ++t) Gk[(size_t)e * ntk + t] = Gh[(size_t)e * nt + kept[t]];
    FH_CHECK(hipSetDevice(h->device));
    const double t0 = fh_now_s();
    if (stats) memset(stats, 0, sizeof(*stats));
    if (node_status) for (int e = 0; e < ne; ++e) node_status[e] = 0;
    poly_coefs pc;
    if ((rc = pc.acquire(h))) return rc;
    cplx* dG;
    double* dT;
    if ((rc = poly_upload(h, "ec_G", Gk, &dG))) return rc;
    if ((rc = fh_buf(h, "ec_t", (size_t)m64 * 2, &dT))) return rc;
    FH_CHECK(hipMemsetAsync(dT, 0, (size_t)m64 * 2 * sizeof(double), h->stream));
    const fh_poly_ptrs P = fh_poly_coef_ptrs(h);
    poly_iters it;
    poly_iter_record rec(ne, m64);
    for (int64_t c0 = 0; c0 < m64; c0 += FH_MAX_LD) {
        const int m = (int)std::min<int64_t>(FH_MAX_LD, m64 - c0), ld = fh_pick_ld(m);
        const size_t panel = (size_t)N * ld;
        cplx *Vc, *Vs, *Y, *Z;
        if (dV) Vc = (cplx*)dV + (size_t)c0 * N;
        else if ((rc = fh_buf(h, "ec_Vc", (size_t)N * m, &Vc))) return rc;
        if ((rc = fh_buf(h, "ec_V", panel, &Vs))) return rc;
        fh_launch_rademacher(seed, 0, N, m, Vc, N, h->stream, c0);
        fh_launch_to_panel(Vc, N, N, m, Vs, ld, h->stream);
        if (ntk == 0) continue;          // T' = 0 on the whole contour: every sample is zero
        if ((rc = fh_buf(h, "ec_Y", (size_t)ne * panel, &Y))) return rc;
        if ((rc = fh_buf(h, "ec_Z", (size_t)ntk * panel, &Z))) return rc;
        std::vector<int> status;
        int64_t nfact = 0;
        if ((rc = poly_solve_nodes(h, ld, m, ne, Vs, 0, panel, Y, status, &nfact, it))) return rc;
        if (poly_krylov(h)) rec.panel(it, c0, m);
        fh_prof_begin(h, "node_combine");
        hipLaunchKernelGGL(k_node_combine, dim3(fh_vec_nblk(N, ld)), dim3(FH_BLOCK), 0, h->stream, Y, panel, dG, ne, ntk, Z, panel);
        fh_prof_end(h);
        if (h->poly.sparse) {
            fh_fanin_args a;
            memset(&a, 0, sizeof(a));
            a.rowptr = h->csr.rowptr; a.col = h->csr.col; a.Z = Z; a.zstride = panel; a.N = N; a.nt = ntk;
            for (int t = 0; t < ntk; ++t) a.val[t] = P.c[kept[t]];
            a.seed = seed; a.col0 = c0;
            const int rows = FH_BLOCK / ld, nprow = std::max(1, std::min(FH_FANIN_GRID_MAX, (N + rows - 1) / rows));
            if ((rc = fh_buf(h, "ec_part", (size_t)nprow * ld, &a.partial))) return rc;
            fh_prof_begin(h, "fanin_trace");
            POLY_LAUNCH_CSR(k_spmm_fanin_trace, ld, dim3((unsigned)nprow), a);
            fh_prof_end(h);
            fh_launch_trace_finish(a.partial, nprow, m, 0, dT + 2 * c0, h->stream);
        } else {
            cplx *W, *Pc, *work;
            if ((rc = fh_buf(h, "ec_W", panel, &W))) return rc;
            if ((rc = fh_buf(h, "ec_P", (size_t)N * m, &Pc))) return rc;
            if ((rc = fh_buf(h, "ec_work", fh_trace_work_elems(N, m), &work))) return rc;
            for (int t = 0; t < ntk; ++t) poly_product(h, pc, ld, kept[t], Z + (size_t)t * panel, W, t > 0, false);
            fh_launch_from_panel(W, ld, N, m, Pc, N, h->stream);
            fh_launch_trace_dots(Pc, N, m, N, seed, 0, work, dT + 2 * c0, h->stream, c0);
        }
        if (stats) stats->factorizations += nfact;
        if (node_status) for (int e = 0; e < ne; ++e) node_status[e] = std::max(node_status[e], status[e]);
    }
    FH_CHECK(hipMemcpyAsync(samples, dT, (size_t)m64 * 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if ((rc = fh_finish(h))) return rc;
    if (poly_krylov(h)) rec.publish(h, it, stats);
    if (stats) stats->seconds_total = fh_now_s() - t0;
    return 0;
}

// Ahat_k = Q^H A_k Q, k = 0 .. d: d + 1 r x r column-major matrices one behind the other on the host.  Per 64-column panel Q_j
// the products W_k = A_k Q_j (sparse: one fan-out launch), then one Gram launch per block (i, j) and coefficient.
extern "C" int feasthip_poly_project_reduced_dev(feasthip_handle h, int64_t r64, const void* dQ, void* Ahat_host) {
    int rc = poly_check(h, "feasthip_poly_project_reduced_dev", r64, poly_rows(h), POLY_ANY_FORM);
    if (rc) return rc;
    if (!dQ || !Ahat_host) { h->last_error = "feasthip_poly_project_reduced_dev: null argument"; return FEASTHIP_ERROR_INTERNAL; }
    FH_CHECK(hipSetDevice(h->device));
    const int N = (int)h->dense.N, d = h->poly.degree;
    poly_coefs pc;
    if ((rc = pc.acquire(h))) return rc;
    cplx* out[PD + 1];
    for (int k = 0; k <= d; ++k) out[k] = (cplx*)Ahat_host + (size_t)k * r64 * r64;
    return poly_project_blocks(h, {"pq_Qi", "pq_Qj", "pq_W", "pq_G"}, N, (int)r64, d + 1, (const cplx*)dQ, out, [&](int ld, const cplx* Qj, cplx* W) {
        const size_t panel = (size_t)N * ld;
        if (h->kind == FH_KIND_TERM_OPERATOR) return fh_term_products(h, ld, Qj, W) < 0 ? (int)FEASTHIP_ERROR_INTERNAL : 0;          // the callback flavour
        fh_fan_out outs[FH_FAN_MAX];
        for (int k = 0; k <= d; ++k) outs[k] = fh_fan_out{k, W + (size_t)k * panel, false, false};
        if (h->poly.sparse) poly_fan(h, ld, Qj, outs, d + 1);
        else for (int k = 0; k <= d; ++k) poly_product(h, pc, ld, k, Qj, outs[k].Y, false, false);
        return 0;
    });
}

// X = Q Y (N x ncand; Q: N x r, Y: r x ncand column-major on the host), every column scaled to unit length, and
//   backward_error[i] = || P(theta_i) x_i || / sum_k |theta_i|^k ||A_k||_F
// (+inf for a non-finite theta_i and for a column of zero length).  backward_error may be null.
// (term handle: theta is the ncand x nterms table f_k(theta_i) instead)
static int poly_ritz_eval_body(feasthip_ctx* h, const std::string& what, int64_t r64, const void* dQ, int64_t ncand, const void* Y_host,
                               const void* theta, void* dX, double* backward_error) {
    int rc;
    if (!dQ || !Y_host || !dX || dQ == dX || (backward_error && !theta)) { h->last_error = what + ": null argument, or X aliases Q"; return FEASTHIP_ERROR_INTERNAL; }
    if (ncand < 1 || ncand > (1 << 20)) { h->last_error = what + ": candidate count out of range"; return FEASTHIP_ERROR_M0; }
    FH_CHECK(hipSetDevice(h->device));
    const int N = (int)h->dense.N, r = (int)r64;
    const int ld = (r > FH_MAX_LD || ncand > FH_MAX_LD) ? FH_MAX_LD : fh_pick_ld(std::max<int64_t>(r, ncand));
    const int npc = (int)((ncand + ld - 1) / ld);
    const size_t panel = (size_t)N * ld;
    poly_coefs pc;
    if ((rc = pc.acquire(h))) return rc;
    cplx *Qp, *Xp, *Tp, *W, *R, *part, *ddots;
    if ((rc = fh_buf(h, "pv_Q", panel, &Qp))) return rc;
    if ((rc = fh_buf(h, "pv_X", panel, &Xp))) return rc;
    if ((rc = fh_buf(h, "pv_T", panel, &Tp))) return rc;
    if ((rc = fh_buf(h, "pv_W", panel, &W))) return rc;
    if ((rc = fh_buf(h, "pv_R", panel, &R))) return rc;
    if ((rc = fh_buf(h, "pv_part", (size_t)fh_vec_nblk(N, ld) * ld, &part))) return rc;
    if ((rc = fh_buf(h, "pv_dots", (size_t)2 * ld, &ddots))) return rc;
    const poly_ritz_ws ws{"pv_V", Qp, Xp, Tp, part, ddots};
    const cplx* th = (const cplx*)theta;
    std::vector<cplx> dots(2 * (size_t)ld);
    for (int j = 0; j < npc; ++j) {
        const int mj = (int)std::min<int64_t>(ld, ncand - (int64_t)j * ld);
        if ((rc = poly_ritz_vectors(h, pc, ws, N, r, ncand, ld, j, (const cplx*)dQ, (const cplx*)Y_host, mj, mj, (cplx*)dX))) return rc;
        if (!backward_error) continue;
        cplx* dlam;
        if ((rc = poly_upload_cols(h, "pv_lam", th, (int64_t)j * ld, mj, ld, cmake(0, 0), &dlam))) return rc;
        if ((rc = poly_eval_panel(h, pc, ld, dlam, Xp, W, R))) return rc;
        fh_launch_dot_cols(R, R, N, ld, part, ddots + ld, h->stream);
        FH_CHECK(hipMemcpyAsync(dots.data(), ddots, dots.size() * sizeof(cplx), hipMemcpyDeviceToHost, h->stream));
        FH_CHECK(hipStreamSynchronize(h->stream));
        for (int c = 0; c < mj; ++c) {
            const cplx* t = th + ((int64_t)j * ld + c) * (h->poly.terms ? h->poly.degree + 1 : 1);
            double be = INFINITY;
            if ((h->poly.terms ? nep_row_finite(h, t) : std::isfinite(t->x) && std::isfinite(t->y)) && dots[c].x > 0.0) {
                const double scale = h->poly.terms ? nep_bwd_scale(h, t) : poly_bwd_scale(h, std::hypot(t->x, t->y));
                be = scale > 0.0 ? std::sqrt(dots[ld + c].x) / scale : 0.0;
                if (!std::isfinite(be)) be = INFINITY;
            }
            backward_error[(int64_t)j * ld + c] = be;
        }
    }
    return fh_finish(h);
}
extern "C" int feasthip_poly_ritz_eval_dev(feasthip_handle h, int64_t r64, const void* dQ, int64_t ncand, const void* Y_host,
                                           const void* theta, void* dX, double* backward_error) {
    const int rc = poly_check(h, "feasthip_poly_ritz_eval_dev", r64, h && h->kind == FH_KIND_POLYNOMIAL ? h->dense.N : 1);
    return rc ? rc : poly_ritz_eval_body(h, "feasthip_poly_ritz_eval_dev", r64, dQ, ncand, Y_host, theta, dX, backward_error);
}
// Term handle: X = Q Y with unit columns and backward_error[i] = || sum_k F_theta[i][k] A_k x_i || / sum_k |F_theta[i][k]| ||A_k||_F
// (F_theta: ncand x nterms on the host; +inf for a non-finite row and for a column of zero length)
extern "C" int feasthip_nep_ritz_eval_dev(feasthip_handle h, int64_t r64, const void* dQ, int64_t ncand, const void* Y_host,
                                          const void* F_theta, void* dX, double* backward_error) {
    const int rc = poly_check(h, "feasthip_nep_ritz_eval_dev", r64, poly_rows(h), POLY_TERMS);
    if (!rc && h->kind == FH_KIND_TERM_OPERATOR && !h->top.norms_set) {
        h->last_error = "feasthip_nep_ritz_eval_dev: a term-operator handle has no matrices to take ||A_k||_F from: set the norms of the backward error with feasthip_set_term_norms";
        return FEASTHIP_ERROR_FPM;
    }
    return rc ? rc : poly_ritz_eval_body(h, "feasthip_nep_ritz_eval_dev", r64, dQ, ncand, Y_host, F_theta, dX, backward_error);
}
