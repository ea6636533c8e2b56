// fh_device.hpp -- device helpers that more than one .hip unit uses.
#pragma once
#include "fh_common.hpp"

__device__ __forceinline__ bool fh_finite(cplx a) { return isfinite(a.x) && isfinite(a.y); }

// one complex128 element past the caches: panels that a kernel streams once (fh_poly.hip: k_spmm_poly, fh_operator.hip)
__device__ __forceinline__ cplx fh_ld_nt(const cplx* p) { return cmake(__builtin_nontemporal_load(&p->x), __builtin_nontemporal_load(&p->y)); }
__device__ __forceinline__ void fh_st_nt(cplx* p, cplx v) { __builtin_nontemporal_store(v.x, &p->x); __builtin_nontemporal_store(v.y, &p->y); }

// out[c] = the sum over the NT / LD threads t = c + k LD of a workgroup of NT threads of their dsum, added through LDS in
// ascending k (every thread of the workgroup calls it; red: NT elements; ostride: elements between the columns of out)
template <int LD, int NT> __device__ __forceinline__ void fh_column_sum(cplx* red, int t, cplx dsum, cplx* out, size_t ostride = 1) {
    red[t] = dsum;
    __syncthreads();
    if (t < LD) {
        cplx s = red[t];
#pragma unroll
        for (int k = 1; k < NT / LD; ++k) s = cadd(s, red[t + k * LD]);
        out[t * ostride] = s;
    }
    __syncthreads();
}
