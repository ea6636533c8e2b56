// fh_estimate.hip -- stochastic estimate of the eigenvalue count inside the search contour (fpm[14] = 2).
//
// Hutchinson's estimator on the contour filter: for a Rademacher block V (entries +-1) the sweep gives Q_proj = rho V,
// and t_j = v_j^T Q_proj[:, j] is an unbiased sample of tr rho = sum_i f(lambda_i).  Two kernels:
//   k_rademacher_fill  writes the N x m block column-major (the source block of feasthip_contour_apply_dev);
//   k_trace_partials / k_trace_finish  t_j for all m columns in one pass over Q_proj, regenerating v_ij from the hash
//                      instead of reading a stored block; fixed-order two-stage reduction (per-workgroup partials, one
//                      finishing workgroup, no atomics), so the samples are bitwise reproducible from run to run.
// Each entry v_ij is a pure function of (seed, caller's row i, column j): the block does not depend on the grid, the node
// range, the rank or a row renumbering of the matrix, and a numpy restatement reproduces it bit for bit:
//     k   = mix64(seed + 0x9E3779B97F4A7C15 * (i + 1))
//     b   = mix64(k ^ (0xD1B54A32D192ED03 * (j + 1)))          (all arithmetic mod 2^64)
//     v_ij = +1 when the top bit of b is clear, else -1
// with mix64 the splitmix64 finaliser (fh_mix64 / fh_row_key / fh_rademacher, fh_kernels.hpp).
// col0: the block's first column is column col0 of the caller's block (a 64-column panel of a wider block).
#include "fh_common.hpp"
#include "fh_kernels.hpp"

#include <algorithm>

#define FH_EST_BLOCK 256
#define FH_EST_GRID 2048          // memory-bound stream kernels: 256 CUs x 8 blocks, grid-stride beyond

// blocks along the rows of one column: enough to keep FH_EST_GRID blocks over all columns, at least 4 rows per thread
static int fh_est_row_blocks(int64_t nrows, int64_t m) {
    const int64_t want = (nrows + 4 * FH_EST_BLOCK - 1) / (4 * FH_EST_BLOCK);
    const int64_t cap = std::max<int64_t>(1, FH_EST_GRID / std::max<int64_t>(m, 1));
    return (int)std::max<int64_t>(1, std::min(want, cap));
}

// X[r, j] (column-major, leading dimension ldx) = v(row0 + r, j) for r < nrows, j < m.  grid = (row blocks, m)
__global__ __launch_bounds__(FH_EST_BLOCK) void k_rademacher_fill(uint64_t seed, int64_t row0, int64_t nrows, cplx* __restrict__ X,
                                                                  int64_t ldx, int64_t col0) {
    const int64_t j = blockIdx.y;
    cplx* col = X + j * ldx;
    for (int64_t r = (int64_t)blockIdx.x * FH_EST_BLOCK + threadIdx.x; r < nrows; r += (int64_t)gridDim.x * FH_EST_BLOCK)
        col[r] = cmake(fh_rademacher(fh_row_key(seed, row0 + r), col0 + j), 0.0);
}

void fh_launch_rademacher(uint64_t seed, int64_t row0, int64_t nrows, int64_t m, cplx* X, int64_t ldx, hipStream_t st, int64_t col0) {
    if (nrows <= 0 || m <= 0) return;
    hipLaunchKernelGGL(k_rademacher_fill, dim3(fh_est_row_blocks(nrows, m), (unsigned)m), dim3(FH_EST_BLOCK), 0, st,
                       seed, row0, nrows, X, ldx, col0);
}

// stage 1: partial[j * gridDim.x + b] = sum over block b's rows of v(i, j) * P[i, j].  Every block owns a contiguous row
// range of one column; one 16-byte load per lane, wave sums by shuffles, the four waves summed in wave order.
__global__ __launch_bounds__(FH_EST_BLOCK) void k_trace_partials(const cplx* __restrict__ P, int64_t N, int64_t ldp, uint64_t seed,
                                                                 cplx* __restrict__ partial, int64_t col0) {
    const int64_t j = blockIdx.y;
    const int64_t per = (N + gridDim.x - 1) / gridDim.x;
    const int64_t r0 = (int64_t)blockIdx.x * per, r1 = std::min(N, r0 + per);
    const cplx* col = P + j * ldp;
    double sx = 0.0, sy = 0.0;
    for (int64_t r = r0 + threadIdx.x; r < r1; r += FH_EST_BLOCK) {
        const cplx p = col[r];
        const double v = fh_rademacher(fh_row_key(seed, r), col0 + j);
        sx += v * p.x;
        sy += v * p.y;
    }
    for (int off = 32; off > 0; off >>= 1) {
        sx += __shfl_down(sx, off, 64);
        sy += __shfl_down(sy, off, 64);
    }
    __shared__ double wx[FH_EST_BLOCK / 64], wy[FH_EST_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { wx[wave] = sx; wy[wave] = sy; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double tx = 0.0, ty = 0.0;
        for (int w = 0; w < FH_EST_BLOCK / 64; ++w) { tx += wx[w]; ty += wy[w]; }
        partial[j * gridDim.x + blockIdx.x] = cmake(tx, ty);
    }
}

// stage 2 (one workgroup): t[j] = sum_b partial[j * nb + b] in block order; real_only: the imaginary parts are dropped
// (real-projection sweep: Q_proj is real)
__global__ __launch_bounds__(FH_EST_BLOCK) void k_trace_finish(const cplx* __restrict__ partial, int nb, int64_t m, int real_only,
                                                               double* __restrict__ t) {
    for (int64_t j = threadIdx.x; j < m; j += FH_EST_BLOCK) {
        double tx = 0.0, ty = 0.0;
        for (int b = 0; b < nb; ++b) {
            const cplx p = partial[j * nb + b];
            tx += p.x;
            ty += p.y;
        }
        t[2 * j] = tx;
        t[2 * j + 1] = real_only ? 0.0 : ty;
    }
}

size_t fh_trace_work_elems(int64_t N, int64_t m) { return (size_t)fh_est_row_blocks(N, m) * (size_t)m; }

void fh_launch_trace_finish(const cplx* partial, int nb, int64_t m, int real_only, double* t, hipStream_t st) {
    if (nb <= 0 || m <= 0) return;
    hipLaunchKernelGGL(k_trace_finish, dim3(1), dim3(FH_EST_BLOCK), 0, st, partial, nb, m, real_only, t);
}

void fh_launch_trace_dots(const cplx* P, int64_t N, int64_t m, int64_t ldp, uint64_t seed, int real_only, cplx* work, double* t,
                          hipStream_t st, int64_t col0) {
    if (N <= 0 || m <= 0) return;
    const int nb = fh_est_row_blocks(N, m);
    hipLaunchKernelGGL(k_trace_partials, dim3(nb, (unsigned)m), dim3(FH_EST_BLOCK), 0, st, P, N, ldp, seed, work, col0);
    fh_launch_trace_finish(work, nb, m, real_only, t, st);
}
