// fh_host.hpp -- the host helpers that more than one .hip unit of libfeasthip.so uses: the steps an entry point opens and
// closes with, the problem checks, the pinned ring and the operator application (fh_api.hip), and the part of the
// orthonormalisation (fh_ortho.hip) that the resident loop (fh_ritz.hip) calls.  What one unit alone uses stays static there.
// With it come the public header and the standard headers that the host code of every unit uses.
#pragma once
#include "fh_common.hpp"
#include "../../include/feasthip.h"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

// ---- the steps of an entry point --------------------------------------------------------
// non-zero: no handle, or one that an earlier device failure poisoned -- the entry point returns it at once
inline int fh_gate(feasthip_ctx* h) {
    if (!h) return FEASTHIP_ERROR_INTERNAL;
    if (h->poisoned) { h->last_error = "handle poisoned by an earlier device failure: destroy it"; return FEASTHIP_ERROR_INTERNAL; }
    return 0;
}
// the end of an entry point: everything queued has run, the profile is read, a launch failure is reported
inline int fh_finish(feasthip_ctx* h) {
    FH_CHECK(hipStreamSynchronize(h->stream));
    fh_prof_collect(h);
    FH_CHECK(hipGetLastError());       // launch-configuration errors do not surface through the stream sync
    return 0;
}
inline double fh_now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// ---- the problem of a handle (fh_api.hip; the adjoint CSR set and the solver refusals: fh_problem.hip) ----
// row permutation of the panels (block order of a renumbered sparse matrix), or null
inline const int* fh_perm(feasthip_ctx* h) { return h->kind == FH_KIND_CSR ? h->csr.perm : nullptr; }
inline int64_t fh_N(feasthip_ctx* h) { return h->kind == FH_KIND_CSR ? h->csr.N : h->dense.N; }
inline bool fh_b_identity(feasthip_ctx* h) { return h->kind == FH_KIND_CSR ? h->csr.b_identity != 0 : h->dense.b_identity != 0; }
// wide = 1: the entry point also takes m > FH_MAX_LD (processed in 64-column panels)
int fh_check_problem(feasthip_ctx* h, int64_t m, int wide = 0);
// Adjoint switch (feasthip_set_adjoint).  unsupported != null: the entry point has no adjoint form at all
int fh_check_adjoint(feasthip_ctx* h, const char* what, const char* unsupported = nullptr);
// What an operator handle (FH_KIND_OPERATOR, feasthip_set_operator) cannot take; every message names the solvers it does take
extern const char* const fh_operator_why_adjoint;
const char* fh_operator_solver_why(const feasthip_ctx* h, int kind, int factor_precision);
// the conjugate-transposed CSR set of the problem (h->csr_adj), built on first use and freed with the problem
int fh_adjoint_csr_ensure(feasthip_ctx* h);
void fh_free_adjoint_csr(feasthip_ctx* h);

// ---- small copies through the pinned ring, and the staging of a host-pointer entry point (fh_api.hip) ----
int fh_upload_small(feasthip_ctx* h, void* dst, const void* src, size_t bytes);
int fh_upload_coefs(feasthip_ctx* h, const char* name, const std::vector<cplx>& host, cplx** dev);
int fh_download_small(feasthip_ctx* h, const void* src, size_t bytes, const void** slot, std::vector<char>& fallback);
int fh_stage_in(feasthip_ctx* h, const char* name, const void* host, size_t bytes, void** dev);

// ---- operator application on panels (sparse or dense):  Y = (cb*B + ca*A) X  per column (fh_api.hip) ----
struct fh_op_call {
    const void* X = nullptr; size_t x_stride = 0;
    void* Y = nullptr; size_t y_stride = 0;
    const cplx* coefA = nullptr; const cplx* coefB = nullptr;   // device [nodes][ld]
    const void* Bvec = nullptr; size_t b_stride = 0;
    const void* U = nullptr; size_t u_stride = 0;
    int dot_mode = 0; cplx* partial1 = nullptr; cplx* partial2 = nullptr;
    const int* node_active = nullptr;
    int nodes = 1;
    int m = FH_MAX_LD;     // active columns (measurement only)
    int uniform_coef = 0;  // coefA/coefB identical across columns
    int prec = 64;         // panel precision of X/Y/Bvec/U
    const cplx* colscale = nullptr;   // row kernel only (fh_spmm_args::colscale): X is a shared panel times per-node column factors
    int skip = 0;          // host hint (operator handle): bit 0 -- coefA is zero everywhere, bit 1 -- coefB is: that callback is not made
};
// returns number of blocks used in x (needed to size / read partials), -1 with last_error set when the operator failed
int fh_apply_operator(feasthip_ctx* h, int ld, const fh_op_call& c);
// an upper bound of what fh_apply_operator returns: it sizes the partial-sum buffers
int fh_op_nblk(feasthip_ctx* h, int ld);

// ---- orthonormalisation (fh_ortho.hip) and the resident panels (fh_ritz.hip) ----
void fh_ortho_note(feasthip_ctx* h, int used, int stages, int fell_back, int rank, const int* perm, const double* rdiag);
void fh_ortho_note_reset(feasthip_ctx* h);
int fh_ortho_panel(feasthip_ctx* h, int m, int ld, cplx* X, cplx* Out, double rank_tol, double ref_scale, int big_dim, int* rank, cplx** res);
int fh_rs_panels(feasthip_ctx* h, cplx** P, cplx** X, cplx** R);
