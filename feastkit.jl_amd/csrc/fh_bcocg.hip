// fh_bcocg.hip -- kernels of the block COCG sweep (FEASTHIP_SOLVER_BLOCK_COCG; driver: fh_block_cocg in fh_api.hip).
//
// Per contour node e the live columns of the panel (unmasked, c < m, non-zero start residual; n of them) share ONE block
// Krylov space of S = z_e B - A.  Block COCG with residual orthonormalisation (Dubrulle's BCGrQ, the bilinear form x^T y
// wherever CG has an inner product):
//     R = Q C (Q^H Q = I, n columns; C is n x ld: column c of C belongs to ORIGINAL column c, zero for a column not live),
//     W = S P ; G = P^T W ; alpha = G^-1 T ; X += P (alpha C) ; Qh = Q - W alpha ; Qh = Q zeta (Cholesky of Qh^H Qh) ;
//     C <- zeta C ; T' = Q^T Q = zeta^-T (Qh^T Qh) zeta^-1 ; beta = T^-1 (Qh^T Qh) zeta^-1 (= T^-1 zeta^T T') ;
//     P <- Q + P beta ; T <- T'.        ||R e_c|| = ||C e_c||_2: the stop test reads no panel.
// Launches of one step:  SpMM | k_bcocg_gram (P^T W) | k_bcocg_small<1> | k_bcocg_update<1> | k_bcocg_gram (Qh^H Qh and
// Qh^T Qh from the same four accumulators) | k_bcocg_small<2> | k_bcocg_update<2>.
// Every kernel looks at the node's stop word first (0 running, 1 converged, 2 breakdown) and does nothing for a node that
// has left the iteration: the host queues steps without knowing which run.  Small matrices are LD x LD, ROW-major, zero
// padded, one set per node.  No atomics on data: the Gram partials are summed in slot order.
#include "fh_common.hpp"
#include "fh_kernels.hpp"
#include "fh_device.hpp"
#include <algorithm>

typedef double bc_v4d __attribute__((ext_vector_type(4)));

#define FH_BC_GRAM_BLOCKS 32       // workgroups per node of the Gram product
#define FH_BC_SMALL_THREADS 1024
#define FH_BC_PIVOT_TOL 1e-13      // LU pivot of G or T against the largest entry of the matrix
#define FH_BC_CHOL_TOL 1e-10       // pivot of the equilibrated Cholesky (unit diagonal): the rank test of the residual block

// ---------------------------------------------------------------------------------------------------------------------
// Gram products of two panels per node, both forms at once: H = X^H Y and B = X^T Y (k_gram_mfma's operand layout and
// accumulation order; partial tiles per (node, workgroup, row subset), summed by k_bcocg_gram_reduce in slot order).
// ---------------------------------------------------------------------------------------------------------------------
template <int LD>
__global__ __launch_bounds__(256) void k_bcocg_gram(const cplx* __restrict__ X, size_t xs, const cplx* __restrict__ Y, size_t ys,
                                                    int N, cplx* __restrict__ partial, const int* __restrict__ stop) {
    const int node = blockIdx.y;
    if (stop && stop[node]) return;
    constexpr int NS = LD / 16, SUB = 4 / NS;
    X += (size_t)node * xs; Y += (size_t)node * ys;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int stripe = wave % NS, sub = wave / NS;
    const int lc = lane & 15, lk = lane >> 4;
    const int rows_per_block = ((N + gridDim.x - 1) / gridDim.x + 3) & ~3;
    const int row_begin = blockIdx.x * rows_per_block;
    const int row_end = min(N, row_begin + rows_per_block);
    bc_v4d rr[NS], ii[NS], ri[NS], ir[NS];
#pragma unroll
    for (int t = 0; t < NS; ++t) { rr[t] = (bc_v4d){0, 0, 0, 0}; ii[t] = rr[t]; ri[t] = rr[t]; ir[t] = rr[t]; }
    constexpr int UG = 4;
    for (int i0 = row_begin + sub * 4; i0 < row_end; i0 += 4 * SUB * UG) {
        cplx x[UG], y[UG][NS];
#pragma unroll
        for (int u = 0; u < UG; ++u) {
            const int i = i0 + u * 4 * SUB + lk;
            const bool in = i < row_end;
            x[u] = in ? X[(size_t)i * LD + stripe * 16 + lc] : cmake(0, 0);
#pragma unroll
            for (int t = 0; t < NS; ++t) y[u][t] = in ? Y[(size_t)i * LD + t * 16 + lc] : cmake(0, 0);
        }
#pragma unroll
        for (int u = 0; u < UG; ++u) {
#pragma unroll
            for (int t = 0; t < NS; ++t) {
                rr[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[u].x, y[u][t].x, rr[t], 0, 0, 0);
                ii[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[u].y, y[u][t].y, ii[t], 0, 0, 0);
                ri[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[u].x, y[u][t].y, ri[t], 0, 0, 0);
                ir[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[u].y, y[u][t].x, ir[t], 0, 0, 0);
            }
        }
    }
    // slot (node, workgroup, subset): [c1][c2] row-major, two cplx per entry: (rr, ii), (ri, ir)
    cplx* p = partial + (((size_t)node * gridDim.x + blockIdx.x) * SUB + sub) * (size_t)LD * LD * 2;
#pragma unroll
    for (int t = 0; t < NS; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c1 = stripe * 16 + lk + 4 * r, c2 = t * 16 + lc;
            const size_t o = ((size_t)c1 * LD + c2) * 2;
            p[o] = cmake(rr[t][r], ii[t][r]);
            p[o + 1] = cmake(ri[t][r], ir[t][r]);
        }
    }
}

template <int LD>
__global__ __launch_bounds__(256) void k_bcocg_gram_reduce(const cplx* __restrict__ partial, int nslots, cplx* __restrict__ outH,
                                                           cplx* __restrict__ outT, const int* __restrict__ stop) {
    const int node = blockIdx.y;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= LD * LD || (stop && stop[node])) return;
    const cplx* base = partial + (size_t)node * nslots * LD * LD * 2 + (size_t)e * 2;
    double rr = 0, ii = 0, ri = 0, ir = 0;
    int s = 0;
    for (; s + 8 <= nslots; s += 8) {          // eight slots' loads in flight, added in slot order
        cplx a[8], b[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) { const cplx* p = base + (size_t)(s + q) * LD * LD * 2; a[q] = p[0]; b[q] = p[1]; }
#pragma unroll
        for (int q = 0; q < 8; ++q) { rr += a[q].x; ii += a[q].y; ri += b[q].x; ir += b[q].y; }
    }
    for (; s < nslots; ++s) {
        const cplx* p = base + (size_t)s * LD * LD * 2;
        rr += p[0].x; ii += p[0].y; ri += p[1].x; ir += p[1].y;
    }
    if (outH) outH[(size_t)node * LD * LD + e] = cmake(rr + ii, ri - ir);
    if (outT) outT[(size_t)node * LD * LD + e] = cmake(rr - ii, ri + ir);
}

size_t fh_bcocg_gram_work_elems(int ld, int nodes) {
    const int sub = 4 / (ld / 16);
    return (size_t)nodes * FH_BC_GRAM_BLOCKS * sub * ld * ld * 2;
}

template <int LD>
static void bcocg_gram_launch(const cplx* X, size_t xs, const cplx* Y, size_t ys, int N, int nodes, cplx* work, cplx* outH,
                              cplx* outT, const int* stop, hipStream_t st) {
    constexpr int sub = 4 / (LD / 16), nslots = FH_BC_GRAM_BLOCKS * sub;
    hipLaunchKernelGGL((k_bcocg_gram<LD>), dim3(FH_BC_GRAM_BLOCKS, nodes), dim3(256), 0, st, X, xs, Y, ys, N, work, stop);
    hipLaunchKernelGGL((k_bcocg_gram_reduce<LD>), dim3((LD * LD + 255) / 256, nodes), dim3(256), 0, st, work, nslots, outH, outT, stop);
}
void fh_launch_bcocg_gram(const cplx* X, size_t xs, const cplx* Y, size_t ys, int N, int ld, int nodes, cplx* work, cplx* outH,
                          cplx* outT, const int* stop, hipStream_t st) {
    fh_with_ld(ld, [&](auto L) { bcocg_gram_launch<decltype(L)::value>(X, xs, Y, ys, N, nodes, work, outH, outT, stop, st); });
}

// ---------------------------------------------------------------------------------------------------------------------
// k_bcocg_small: the n x n algebra of one node on one workgroup; the two working matrices (LD x LD complex128 each: 128 KiB
// at LD = 64) live in LDS, everything else in the node's global slots.
// ---------------------------------------------------------------------------------------------------------------------
// out (global, LD x LD row-major, zero outside ni x nj) = op(A) B with A, B in LDS (stride LD); op = transpose when ta
template <int LD>
__device__ inline void bc_mm(cplx* __restrict__ out, const cplx* A, bool ta, const cplx* B, int ni, int nk, int nj, cplx scale) {
    for (int e = threadIdx.x; e < LD * LD; e += blockDim.x) {
        const int i = e / LD, j = e % LD;
        cplx acc = cmake(0, 0);
        if (i < ni && j < nj) {
            for (int k = 0; k < nk; ++k) cfma(acc, ta ? A[k * LD + i] : A[i * LD + k], B[k * LD + j]);
            acc = cmul(scale, acc);
        }
        out[e] = acc;
    }
}
// LDS (LD x LD) <- global (LD x LD)
template <int LD>
__device__ inline void bc_load(cplx* dst, const cplx* __restrict__ src) {
    for (int e = threadIdx.x; e < LD * LD; e += blockDim.x) dst[e] = src[e];
}

// Solves A Y = B in place (A, B in LDS, n x n and n x nb): LU with partial pivoting (ties: the lowest row), B <- Y.
// *bad (LDS word) is set when a pivot is below FH_BC_PIVOT_TOL times the largest entry of A, or not finite.
template <int LD>
__device__ __forceinline__ void bc_lu_solve(cplx* A, cplx* B, int n, int nb, int* bad, int* piv_row, double* amax_s, double* red) {
    const int t = threadIdx.x;
    if (t == 0) *amax_s = 0.0;
    __syncthreads();
    if (t < n) {                       // row maxima, then one thread takes the largest
        double mx = 0.0;
        for (int j = 0; j < n; ++j) mx = fmax(mx, cabs2(A[t * LD + j]));
        red[t] = mx;
    }
    __syncthreads();
    if (t == 0) {
        double mx = 0.0;
        for (int i = 0; i < n; ++i) mx = fmax(mx, red[i]);
        *amax_s = sqrt(mx);
    }
    __syncthreads();
    const double amax = *amax_s;
    for (int k = 0; k < n; ++k) {
        if (t == 0) {                  // the largest entry of column k from row k down; ties: the lowest row
            double v = -1.0;
            int idx = k;
            for (int i = k; i < n; ++i) { const double vi = cabs2(A[i * LD + k]); if (vi > v) { v = vi; idx = i; } }
            *piv_row = idx;
            if (!(sqrt(v) >= FH_BC_PIVOT_TOL * amax) || !(v > 0.0) || !isfinite(v)) *bad = 1;
        }
        __syncthreads();
        if (*bad) return;              // uniform: every thread reads the same word after the barrier
        const int p = *piv_row;
        if (p != k) {
            for (int j = t; j < n; j += blockDim.x) { const cplx a = A[k * LD + j]; A[k * LD + j] = A[p * LD + j]; A[p * LD + j] = a; }
            for (int j = t; j < nb; j += blockDim.x) { const cplx a = B[k * LD + j]; B[k * LD + j] = B[p * LD + j]; B[p * LD + j] = a; }
        }
        __syncthreads();
        const cplx piv = A[k * LD + k];
        const int w = (n - k - 1) + nb;          // columns k+1 .. n-1 of A, then all of B
        for (int e = t; e < (n - k - 1) * w; e += blockDim.x) {
            const int i = k + 1 + e / w, jj = e % w;
            const cplx l = cdiv(A[i * LD + k], piv);
            if (jj < n - k - 1) { const int j = k + 1 + jj; A[i * LD + j] = csub(A[i * LD + j], cmul(l, A[k * LD + j])); }
            else { const int j = jj - (n - k - 1); B[i * LD + j] = csub(B[i * LD + j], cmul(l, B[k * LD + j])); }
        }
        __syncthreads();
    }
    // back substitution with the upper triangle
    for (int k = n - 1; k >= 0; --k) {
        const cplx piv = A[k * LD + k];
        for (int j = t; j < nb; j += blockDim.x) B[k * LD + j] = cdiv(B[k * LD + j], piv);
        __syncthreads();
        for (int e = t; e < k * nb; e += blockDim.x) {
            const int i = e / nb, j = e % nb;
            B[i * LD + j] = csub(B[i * LD + j], cmul(A[i * LD + k], B[k * LD + j]));
        }
        __syncthreads();
    }
}

// Equilibrated Cholesky of the Hermitian n x n matrix in A (LDS): H' = D^-1 H D^-1 = L L^H, d = sqrt(diag H) in dsc (scaled by
// the caller already when pre != 0).  On success A holds zeta = L^H D (upper triangular, zeros below) and B its inverse.
template <int LD>
__device__ __forceinline__ void bc_chol_zeta(cplx* A, cplx* B, int n, double* dsc, int* bad) {
    const int t = threadIdx.x;
    if (t < n) {
        const double g = A[t * LD + t].x;
        const double d = (g > 0.0 && isfinite(g)) ? sqrt(g) : 0.0;
        dsc[t] = d;
        if (!(d > 0.0)) *bad = 1;
    }
    __syncthreads();
    if (*bad) return;
    for (int e = t; e < n * n; e += blockDim.x) {
        const int i = e / n, j = e % n;
        const cplx v = A[i * LD + j];
        if (!fh_finite(v)) *bad = 1;
        const double s = 1.0 / (dsc[i] * dsc[j]);
        A[i * LD + j] = cmake(v.x * s, v.y * s);
    }
    __syncthreads();
    if (*bad) return;
    for (int k = 0; k < n; ++k) {
        const double pv = A[k * LD + k].x;
        if (!(pv > FH_BC_CHOL_TOL) || !isfinite(pv)) { if (t == 0) *bad = 1; }
        __syncthreads();
        if (*bad) return;
        const double r = sqrt(pv), ir = 1.0 / r;
        for (int i = k + 1 + t; i < n; i += blockDim.x) { const cplx v = A[i * LD + k]; A[i * LD + k] = cmake(v.x * ir, v.y * ir); }
        __syncthreads();
        if (t == 0) A[k * LD + k] = cmake(r, 0.0);
        const int w = n - k - 1;
        for (int e = t; e < w * w; e += blockDim.x) {
            const int i = k + 1 + e / w, j = k + 1 + e % w;
            if (j <= i) A[i * LD + j] = csub(A[i * LD + j], cmul(A[i * LD + k], cconj(A[j * LD + k])));
        }
        __syncthreads();
    }
    // zeta[k][j] = conj(L[j][k]) d[j] (j >= k): transposed in place through registers
    constexpr int NH = (LD * LD + FH_BC_SMALL_THREADS - 1) / FH_BC_SMALL_THREADS;
    cplx hold[NH];
#pragma unroll
    for (int q = 0; q < NH; ++q) {
        const int e = t + q * FH_BC_SMALL_THREADS, k = e / LD, j = e % LD;
        hold[q] = (e < LD * LD && k < n && j < n && j >= k) ? cscale(cconj(A[j * LD + k]), dsc[j]) : cmake(0, 0);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NH; ++q) {
        const int e = t + q * FH_BC_SMALL_THREADS;
        if (e < LD * LD) {
            A[e] = hold[q];
            B[e] = (e / LD == e % LD && e / LD < n) ? cmake(1, 0) : cmake(0, 0);
        }
    }
    __syncthreads();
    // B = zeta^-1: back substitution on the identity
    for (int k = n - 1; k >= 0; --k) {
        const double ir = 1.0 / A[k * LD + k].x;         // the diagonal of zeta is real
        for (int j = t; j < n; j += blockDim.x) B[k * LD + j] = cscale(B[k * LD + j], ir);
        __syncthreads();
        for (int e = t; e < k * n; e += blockDim.x) {
            const int i = e / n, j = e % n;
            B[i * LD + j] = csub(B[i * LD + j], cmul(A[i * LD + k], B[k * LD + j]));
        }
        __syncthreads();
    }
}

__device__ inline void bc_leave(int* stop, int* node_active, int node, int word) {
    if (threadIdx.x == 0) { stop[node] = word; node_active[node] = 0; }
}

// PHASE 0: start (live columns, zeta_0, C, the compaction matrix Zi = E^T D_f zeta_0^-1, T); 1: alpha, w_e alpha C;
// 2: zeta, T', beta, C <- zeta C, norms, stop word
template <int LD, int PHASE>
__global__ __launch_bounds__(FH_BC_SMALL_THREADS) void k_bcocg_small(fh_bcocg_args a) {
    extern __shared__ cplx bc_sm[];
    cplx* Am = bc_sm;
    cplx* Bm = bc_sm + LD * LD;
    __shared__ double dsc[LD];
    __shared__ int live_s[LD];
    __shared__ int bad, piv_row, nl_s;
    __shared__ double amax_s;
    const int node = blockIdx.x, t = threadIdx.x;
    const size_t mo = (size_t)node * LD * LD, co = (size_t)node * LD;
    if (PHASE != 0 && a.stop[node]) return;
    if (t == 0) bad = 0;
    __syncthreads();
    if (PHASE == 0) {
        if (t < LD) {
            const cplx f = a.fscale[co + t];
            const double g = a.SH[t * LD + t].x;
            const double d = sqrt(cabs2(f)) * ((g > 0.0) ? sqrt(g) : (g == 0.0 ? 0.0 : g));
            const double tg = a.rtol * d + a.atol;
            const bool on = t < a.m && (!a.col_mask || a.col_mask[t]) && isfinite(d) && d > tg;
            a.r0norm[co + t] = t < a.m ? d : 0.0; a.rnorm[co + t] = t < a.m ? d : 0.0; a.target[co + t] = tg;
            a.active[co + t] = on ? 1 : 0; a.iters[co + t] = 0;
            a.status[co + t] = (t < a.m && !isfinite(d)) ? 8 : 0;
            live_s[t] = on ? 1 : 0;
        }
        __syncthreads();
        if (t == 0) {
            int n = 0;
            for (int c = 0; c < LD; ++c) if (live_s[c]) live_s[n++] = c;       // (n <= c: in place)
            nl_s = n;
            a.nlive[node] = n; a.steps[node] = 0; a.passes[node] = 0;
        }
        __syncthreads();
        const int n = nl_s;
        if (t < LD) a.live[co + t] = t < n ? live_s[t] : -1;
        if (n == 0) { a.node_active[node] = 0; bc_leave(a.stop, a.node_active, node, 1); return; }
        // H of the scaled, compacted start residual R0 = src D_f E^T
        for (int e = t; e < LD * LD; e += blockDim.x) {
            const int i = e / LD, j = e % LD;
            Am[e] = (i < n && j < n) ? cmul(cmulc(a.fscale[co + live_s[i]], a.SH[live_s[i] * LD + live_s[j]]), a.fscale[co + live_s[j]]) : cmake(0, 0);
        }
        __syncthreads();
        bc_chol_zeta<LD>(Am, Bm, n, dsc, &bad);
        __syncthreads();
        if (bad) { bc_leave(a.stop, a.node_active, node, 2); return; }
        // C[j][live[k]] = zeta0[j][k]
        for (int e = t; e < LD * LD; e += blockDim.x) a.Cs[mo + e] = cmake(0, 0);
        __syncthreads();
        for (int e = t; e < n * n; e += blockDim.x) a.Cs[mo + (e / n) * LD + live_s[e % n]] = Am[(e / n) * LD + e % n];
        // Zi[live[i]][k] = f_live[i] zeta0^-1[i][k]
        for (int e = t; e < LD * LD; e += blockDim.x) a.Zi[mo + e] = cmake(0, 0);
        __syncthreads();
        for (int e = t; e < n * n; e += blockDim.x) {
            const int i = e / n, k = e % n;
            a.Zi[mo + live_s[i] * LD + k] = cmul(a.fscale[co + live_s[i]], Bm[i * LD + k]);
        }
        __syncthreads();
        // T = Zi^T (src^T src) Zi
        bc_load<LD>(Am, a.ST);
        bc_load<LD>(Bm, a.Zi + mo);
        __syncthreads();
        bc_mm<LD>(a.U + mo, Am, false, Bm, LD, LD, n, cmake(1, 0));
        __syncthreads();
        bc_load<LD>(Am, a.U + mo);
        __syncthreads();
        bc_mm<LD>(a.T + mo, Bm, true, Am, n, LD, n, cmake(1, 0));
        if (t == 0) a.node_active[node] = 1;
        return;
    }
    const int n = a.nlive[node];
    if (PHASE == 1) {
        if (t == 0) a.passes[node] += 1;
        bc_load<LD>(Am, a.GA + mo);
        bc_load<LD>(Bm, a.T + mo);
        __syncthreads();
        for (int e = t; e < n * n; e += blockDim.x) if (!fh_finite(Am[(e / n) * LD + e % n]) || !fh_finite(Bm[(e / n) * LD + e % n])) bad = 1;
        __syncthreads();
        if (!bad) bc_lu_solve<LD>(Am, Bm, n, n, &bad, &piv_row, &amax_s, dsc);
        __syncthreads();
        if (bad) { bc_leave(a.stop, a.node_active, node, 2); return; }
        for (int e = t; e < LD * LD; e += blockDim.x) a.Al[mo + e] = (e / LD < n && e % LD < n) ? Bm[e] : cmake(0, 0);
        bc_load<LD>(Am, a.Cs + mo);
        __syncthreads();
        bc_mm<LD>(a.M1 + mo, Bm, false, Am, n, n, LD, a.wnode[node]);
        if (t == 0) a.steps[node] += 1;
        return;
    }
    // PHASE 2
    bc_load<LD>(Am, a.GH + mo);
    __syncthreads();
    bc_chol_zeta<LD>(Am, Bm, n, dsc, &bad);
    __syncthreads();
    if (bad) { bc_leave(a.stop, a.node_active, node, 2); return; }
    for (int e = t; e < LD * LD; e += blockDim.x) { a.Ze[mo + e] = Am[e]; a.Zi[mo + e] = Bm[e]; }
    __syncthreads();
    bc_load<LD>(Am, a.GT + mo);
    __syncthreads();
    bc_mm<LD>(a.U + mo, Am, false, Bm, n, n, n, cmake(1, 0));              // U = (Qh^T Qh) zeta^-1
    __syncthreads();
    bc_load<LD>(Am, a.U + mo);
    __syncthreads();
    bc_mm<LD>(a.Tn + mo, Bm, true, Am, n, n, n, cmake(1, 0));              // T' = zeta^-T U
    __syncthreads();
    bc_load<LD>(Bm, a.U + mo);                                             // beta = T^-1 U
    bc_load<LD>(Am, a.T + mo);
    __syncthreads();
    for (int e = t; e < n * n; e += blockDim.x) if (!fh_finite(Am[(e / n) * LD + e % n]) || !fh_finite(Bm[(e / n) * LD + e % n])) bad = 1;
    __syncthreads();
    if (!bad) bc_lu_solve<LD>(Am, Bm, n, n, &bad, &piv_row, &amax_s, dsc);
    __syncthreads();
    if (bad) { bc_leave(a.stop, a.node_active, node, 2); return; }
    for (int e = t; e < LD * LD; e += blockDim.x) {
        a.Be[mo + e] = (e / LD < n && e % LD < n) ? Bm[e] : cmake(0, 0);
        a.T[mo + e] = a.Tn[mo + e];
    }
    __syncthreads();
    bc_load<LD>(Am, a.Ze + mo);                                            // C <- zeta C
    bc_load<LD>(Bm, a.Cs + mo);
    __syncthreads();
    bc_mm<LD>(a.Cs + mo, Am, false, Bm, n, n, LD, cmake(1, 0));
    __syncthreads();
    if (t < LD) {
        double s = 0.0;
        for (int j = 0; j < n; ++j) s += cabs2(a.Cs[mo + j * LD + t]);
        const double rn = sqrt(s);
        const bool lv = a.active[co + t] != 0 || a.iters[co + t] > 0;      // a live column of this node
        live_s[t] = 0;
        if (lv) {
            a.rnorm[co + t] = rn;
            a.iters[co + t] = a.steps[node];
            const bool on = !(rn <= a.target[co + t]);
            a.active[co + t] = on ? 1 : 0;
            if (!isfinite(rn)) { a.status[co + t] = 8; bad = 1; }
            live_s[t] = on ? 1 : 0;
        }
    }
    __syncthreads();
    if (bad) { bc_leave(a.stop, a.node_active, node, 2); return; }
    if (t == 0) {
        int on = 0;
        for (int c = 0; c < LD; ++c) on += live_s[c];
        if (on == 0) { a.stop[node] = 1; a.node_active[node] = 0; }
    }
}

template <int LD, int PHASE>
static void bcocg_small_launch(const fh_bcocg_args& a, hipStream_t st) {
    const size_t dyn = 2 * (size_t)LD * LD * sizeof(cplx);
    static bool raised = false;
    if (!raised) {
        (void)hipFuncSetAttribute((const void*)k_bcocg_small<LD, PHASE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
        raised = true;
    }
    hipLaunchKernelGGL((k_bcocg_small<LD, PHASE>), dim3(a.nodes), dim3(FH_BC_SMALL_THREADS), dyn, st, a);
}
template <int LD>
static void bcocg_small_ld(const fh_bcocg_args& a, int phase, hipStream_t st) {
    if (phase == 0) bcocg_small_launch<LD, 0>(a, st);
    else if (phase == 1) bcocg_small_launch<LD, 1>(a, st);
    else bcocg_small_launch<LD, 2>(a, st);
}
void fh_launch_bcocg_small(const fh_bcocg_args& a, int ld, int phase, hipStream_t st) {
    fh_with_ld(ld, [&](auto L) { bcocg_small_ld<decltype(L)::value>(a, phase, st); });
}

// ---------------------------------------------------------------------------------------------------------------------
// k_bcocg_update: panel times small matrix on v_mfma_f64_16x16x4 (k_small_matmul_mfma's operand layout).  A workgroup owns
// chunks of 64 rows and walks the nodes in order, so the shared accumulator gets the nodes' contributions in a fixed order:
//   PHASE 0  Q_e = src Zi_e ; P_e = Q_e                                   (start: src is the shared start residual)
//   PHASE 1  ACC += sum_e P_e M1_e ; Q_e <- Q_e - W_e alpha_e              (M1 = w_e alpha C; Q_e then holds Qh)
//   PHASE 2  Q_e <- Q_e Zi_e ; P_e <- Q_e + P_e beta_e
//   PHASE 3  W_e = Q_e C_e       (nodes that broke down: the residual panel the per-column sweep finishes from)
// ---------------------------------------------------------------------------------------------------------------------
template <int LD, int PHASE>
__global__ __launch_bounds__(256) void k_bcocg_update(fh_bcocg_args a) {
    constexpr int NS = LD / 16, SUB = 4 / NS, RB = 16 * SUB, KS = LD / 4, STEPS = 64 / RB;
    constexpr bool TWO = PHASE == 1 || PHASE == 2;
    __shared__ cplx As[RB][LD + 1];
    __shared__ cplx Bs[TWO ? RB : 1][LD + 1];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int lr = lane & 15, lk = lane >> 4;
    const int ct = wave % NS, sb = wave / NS;
    const int N = a.N;
    const int want = PHASE == 3 ? 2 : 0;
    for (int row0 = blockIdx.x * 64; row0 < N; row0 += gridDim.x * 64) {
        bc_v4d xr[STEPS], xi[STEPS];
#pragma unroll
        for (int s = 0; s < STEPS; ++s) { xr[s] = (bc_v4d){0, 0, 0, 0}; xi[s] = xr[s]; }
        bool any = false;
        for (int e = 0; e < a.nodes; ++e) {
            if (a.stop[e] != want) continue;
            if (PHASE == 3 && a.steps[e] == 0 && a.passes[e] == 0) continue;      // broke down at the start: no Q panel exists
            any = true;
            const size_t mo = (size_t)e * LD * LD;
            const cplx* V1 = PHASE == 1 ? a.M1 + mo : PHASE == 3 ? a.Cs + mo : a.Zi + mo;
            const cplx* V2 = PHASE == 1 ? a.Al + mo : a.Be + mo;
            const cplx* PA = PHASE == 0 ? a.src : PHASE == 1 ? a.P + e * a.node_stride : a.Q + e * a.node_stride;
            const cplx* PB = PHASE == 1 ? a.W + e * a.node_stride : a.P + e * a.node_stride;
            cplx* Qe = a.Q + e * a.node_stride;
            cplx* Pe = a.P + e * a.node_stride;
            cplx* We = a.W + e * a.node_stride;
            cplx v1[KS], v2[TWO ? KS : 1];
#pragma unroll
            for (int kk = 0; kk < KS; ++kk) {
                v1[kk] = V1[(size_t)(4 * kk + lk) * LD + 16 * ct + lr];
                if (TWO) v2[kk] = V2[(size_t)(4 * kk + lk) * LD + 16 * ct + lr];
            }
#pragma unroll
            for (int s = 0; s < STEPS; ++s) {
                const int r0 = row0 + s * RB;
                for (int q = t; q < RB * LD; q += 256) {
                    const int r = q / LD, c = q % LD;
                    const bool in = r0 + r < N;
                    As[r][c] = in ? PA[(size_t)(r0 + r) * LD + c] : cmake(0, 0);
                    if (TWO) Bs[r][c] = in ? PB[(size_t)(r0 + r) * LD + c] : cmake(0, 0);
                }
                __syncthreads();
                bc_v4d re1 = {0, 0, 0, 0}, im1 = {0, 0, 0, 0}, re2 = {0, 0, 0, 0}, im2 = {0, 0, 0, 0};
#pragma unroll
                for (int kk = 0; kk < KS; ++kk) {
                    const cplx x = As[16 * sb + lr][4 * kk + lk];
                    re1 = __builtin_amdgcn_mfma_f64_16x16x4f64(x.x, v1[kk].x, re1, 0, 0, 0);
                    re1 = __builtin_amdgcn_mfma_f64_16x16x4f64(-x.y, v1[kk].y, re1, 0, 0, 0);
                    im1 = __builtin_amdgcn_mfma_f64_16x16x4f64(x.x, v1[kk].y, im1, 0, 0, 0);
                    im1 = __builtin_amdgcn_mfma_f64_16x16x4f64(x.y, v1[kk].x, im1, 0, 0, 0);
                    if (TWO) {
                        const cplx y = Bs[16 * sb + lr][4 * kk + lk];
                        re2 = __builtin_amdgcn_mfma_f64_16x16x4f64(y.x, v2[kk].x, re2, 0, 0, 0);
                        re2 = __builtin_amdgcn_mfma_f64_16x16x4f64(-y.y, v2[kk].y, re2, 0, 0, 0);
                        im2 = __builtin_amdgcn_mfma_f64_16x16x4f64(y.x, v2[kk].y, im2, 0, 0, 0);
                        im2 = __builtin_amdgcn_mfma_f64_16x16x4f64(y.y, v2[kk].x, im2, 0, 0, 0);
                    }
                }
                if (PHASE == 1) { xr[s] += re1; xi[s] += im1; }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = r0 + 16 * sb + lk + 4 * r;
                    if (i >= N) continue;
                    const size_t o = (size_t)i * LD + 16 * ct + lr;
                    if (PHASE == 0) { const cplx q = cmake(re1[r], im1[r]); Qe[o] = q; Pe[o] = q; }
                    if (PHASE == 1) { const cplx q = Qe[o]; Qe[o] = cmake(q.x - re2[r], q.y - im2[r]); }
                    if (PHASE == 2) { Qe[o] = cmake(re1[r], im1[r]); Pe[o] = cmake(re1[r] + re2[r], im1[r] + im2[r]); }
                    if (PHASE == 3) We[o] = cmake(re1[r], im1[r]);
                }
                __syncthreads();
            }
        }
        if (PHASE == 1 && any) {
#pragma unroll
            for (int s = 0; s < STEPS; ++s) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = row0 + s * RB + 16 * sb + lk + 4 * r;
                    if (i >= N) continue;
                    const size_t o = (size_t)i * LD + 16 * ct + lr;
                    const cplx v = a.sum_acc[o];
                    a.sum_acc[o] = cmake(v.x + xr[s][r], v.y + xi[s][r]);
                }
            }
        }
    }
}

template <int LD>
static void bcocg_update_ld(const fh_bcocg_args& a, int phase, hipStream_t st) {
    const int nb = std::min((a.N + 63) / 64, 2048);
    if (phase == 0) hipLaunchKernelGGL((k_bcocg_update<LD, 0>), dim3(nb), dim3(256), 0, st, a);
    else if (phase == 1) hipLaunchKernelGGL((k_bcocg_update<LD, 1>), dim3(nb), dim3(256), 0, st, a);
    else if (phase == 2) hipLaunchKernelGGL((k_bcocg_update<LD, 2>), dim3(nb), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_bcocg_update<LD, 3>), dim3(nb), dim3(256), 0, st, a);
}
void fh_launch_bcocg_update(const fh_bcocg_args& a, int ld, int phase, hipStream_t st) {
    fh_with_ld(ld, [&](auto L) { bcocg_update_ld<decltype(L)::value>(a, phase, st); });
}
