// batched banded LU for narrow-band CSR input (fh_banded.hip)
#pragma once
#include <cstdint>
#include <vector>

#include "fh_common.hpp"

// the sparse direct solver's operations for the sequences of fh_direct.hip
const fh_direct_ops& fh_banded_direct_ops();
int fh_banded_plan_bytes(feasthip_ctx* h, int nodes, int64_t* factor_bytes, int64_t* transient_bytes);
// Shift preconditioner (feasthip_set_preconditioner): factors of z B - A for the distinct shifts in `pivots`, through the same
// cache, matched by shift as for fh_direct_solve_subset.  slots[p]: the slot of pivot p, status[p]: 0 or FEASTHIP_ERROR_LAPACK;
// *fell_back: the multifrontal plan rejected a pivot and the band plan took over; *slot_bytes: one factor's device memory.
int fh_banded_precond_factor(feasthip_ctx* h, const std::vector<cplx>& pivots, std::vector<int>& slots, std::vector<int>& status,
                             int64_t* nfact, int* fell_back, int64_t* slot_bytes);
void fh_banded_free(feasthip_ctx* h);
int fh_banded_plan(feasthip_ctx* h, int* kl, int* ku, int64_t* bytes_per_node, int* blocked);
int fh_banded_plan_flops(feasthip_ctx* h, double* flops);
// adjoint switch on a CSR handle: 0 when the direct plan (made here if need be) is the multifrontal one, else FEASTHIP_ERROR_FPM
int fh_banded_adjoint_ready(feasthip_ctx* h);
