// batched banded LU for narrow-band CSR input (fh_banded.hip)
#pragma once
#include <cstdint>
#include <vector>

#include "fh_common.hpp"

int fh_banded_solve_nodes(feasthip_ctx* h, int ld, int m, int nodes, const std::vector<cplx>& z, const cplx* RHS, size_t rhs_stride, cplx* Y,
                          size_t stride, std::vector<int>& status, int64_t* nfact);
int fh_banded_solve_subset(feasthip_ctx* h, int ld, int m, const std::vector<cplx>& z, const cplx* RHS, cplx* Y, size_t stride,
                           std::vector<int>& status, int64_t* nfact);
int fh_banded_plan_bytes(feasthip_ctx* h, int nodes, int64_t* factor_bytes, int64_t* transient_bytes);
int fh_banded_solve_single(feasthip_ctx* h, int ld, int m, cplx z, const cplx* RHS, cplx* Y, int* status, int64_t* nfact);
// Shift preconditioner (feasthip_set_preconditioner): factors of z B - A for the distinct shifts in `pivots`, through the same
// cache, matched by shift as for fh_banded_solve_subset.  slots[p]: the slot of pivot p, status[p]: 0 or FEASTHIP_ERROR_LAPACK;
// *fell_back: the multifrontal plan rejected a pivot and the band plan took over; *slot_bytes: one factor's device memory.
int fh_banded_precond_factor(feasthip_ctx* h, const std::vector<cplx>& pivots, std::vector<int>& slots, std::vector<int>& status,
                             int64_t* nfact, int* fell_back, int64_t* slot_bytes);
// Y_q = M^-1 RHS_q with the factors in slots[q] (a slot may be named more than once), q < slots.size()
int fh_banded_precond_solve(feasthip_ctx* h, int ld, int m, const std::vector<int>& slots, const cplx* RHS, size_t rhs_stride, cplx* Y,
                            size_t stride);
void fh_banded_free(feasthip_ctx* h);
int fh_banded_plan(feasthip_ctx* h, int* kl, int* ku, int64_t* bytes_per_node, int* blocked);
int fh_banded_plan_flops(feasthip_ctx* h, double* flops);
// adjoint switch on a CSR handle: 0 when the direct plan (made here if need be) is the multifrontal one, else FEASTHIP_ERROR_FPM
int fh_banded_adjoint_ready(feasthip_ctx* h);
