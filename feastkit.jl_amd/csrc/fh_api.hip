// fh_api.hip -- the sweep side of the C ABI of libfeasthip.so (include/feasthip.h): the operator application, the batched
// Krylov drivers and their launch geometry, the contour sweep, the count estimate, and the products and shifted solves of the
// RCI seams.  Host-side orchestration of the gfx950 kernels; no arithmetic on the host except M0 x M0 bookkeeping.  The handle
// itself: fh_handle.hip; the problem: fh_problem.hip; orthonormalisation: fh_ortho.hip; Rayleigh-Ritz: fh_ritz.hip.
#include "fh_host.hpp"
#include "fh_kernels.hpp"
#include "fh_krylov.hpp"
#include "fh_dense.hpp"
#include "fh_banded.hpp"
#include "fh_comm.hpp"
#include "fh_policy.hpp"       // fh_column_failed
#include "fh_precond.hpp"      // nearest_pivot
#include "fh_knobs.hpp"

#include <thread>

// ---------------------------------------------------------------------------------------
// operator application on panels (sparse or dense):  Y = (cb*B + ca*A) X  per column
// ---------------------------------------------------------------------------------------

// full-width panels over a real matrix go through the row-per-wave kernel (FH_SPMM_ROW=0: the 4-rows-per-wave gather kernel)
static bool fh_row_kernel_ok(feasthip_ctx* h, int ld) {
    return h->kind == FH_KIND_CSR && ld == 64 && !h->csr.is_complex && h->csr.rp8 && fh_knob::spmm_row();
}

// The operands that every argument block of an operator has under the same names (fh_spmm_args, fh_polyop_call, fh_userop_call,
// fh_termop_call, fh_dense_op_args), from the call; the panels take the block's own pointer types.
template <class Args> static void fh_op_operands(Args& a, const fh_op_call& c) {
    a.X = (decltype(a.X))c.X; a.x_node_stride = c.x_stride; a.Y = (decltype(a.Y))c.Y; a.y_node_stride = c.y_stride;
    a.Bvec = (decltype(a.Bvec))c.Bvec; a.b_node_stride = c.b_stride; a.U = (decltype(a.U))c.U; a.u_node_stride = c.u_stride;
    a.dot_mode = c.dot_mode; a.partial1 = c.partial1; a.partial2 = c.partial2; a.node_active = c.node_active;
}

// returns number of blocks used in x (needed to size / read partials)
int fh_apply_operator(feasthip_ctx* h, int ld, const fh_op_call& c) {
    if (h->kind == FH_KIND_CSR && h->adjoint) {
        // the conjugate-transposed set through the gather kernel (plain products only, as for the dense adjoint operator)
        if (c.dot_mode != 0 || c.colscale) { h->last_error = "internal: adjoint operator with fused dots"; return -1; }
        if (fh_adjoint_csr_ensure(h)) return -1;
        fh_spmm_args a;
        a.rowptr = h->csr_adj.rowptr; a.col = h->csr_adj.col; a.aval = h->csr_adj.aval; a.bval = h->csr_adj.bval;
        a.N = (int)h->csr.N; a.nodes = c.nodes;
        fh_op_operands(a, c);
        a.coefA = c.coefA; a.coefB = c.coefB; a.partial1 = nullptr; a.partial2 = nullptr;      // (dot_mode is 0: no partial sums)
        a.nblk_rows = 0; a.blk_start = nullptr; a.ext_ptr = nullptr; a.ext_idx = nullptr; a.lcol = nullptr;
        a.counters = h->profiling ? h->d_counters : nullptr; a.m = c.m; a.uniform_coef = c.uniform_coef; a.prec = c.prec;
        fh_prof_begin(h, "spmm_adjoint");
        fh_launch_spmm(a, ld, h->csr.is_complex != 0, h->csr.b_identity != 0, fh_spmm_grid(a.N, ld), h->stream);
        fh_prof_end(h);
        return fh_spmm_partials(a.N, ld);
    }
    if (h->kind == FH_KIND_CSR) {
        fh_spmm_args a;
        a.rowptr = h->csr.rowptr; a.col = h->csr.col; a.aval = h->csr.aval; a.bval = h->csr.bval;
        a.N = (int)h->csr.N; a.nodes = c.nodes;
        fh_op_operands(a, c);
        a.coefA = c.coefA; a.coefB = c.coefB;
        a.counters = h->profiling ? h->d_counters : nullptr; a.m = c.m; a.uniform_coef = c.uniform_coef; a.prec = c.prec;
        // (the LDS-window kernel keeps its active-node list in a 64-entry LDS array: wider node batches -- trapezoid
        //  contours put no bound on fpm[2] -- take the gather kernel, which has no such limit)
        const bool lds_kernel = h->csr.lcol && c.prec == 64 && fh_knob::lds_spmm() && c.nodes <= 64 && c.dot_mode != 6;   // (fused-COCG dots: gather kernel only)
        a.nblk_rows = h->csr.nblk; a.blk_start = h->csr.blk_start; a.ext_ptr = h->csr.ext_ptr; a.ext_idx = h->csr.ext_idx;
        a.lcol = lds_kernel ? h->csr.lcol : nullptr;
        // full-width panels over a real matrix: the row-per-wave kernel (FH_SPMM_ROW=0: the 4-rows-per-wave gather kernel)
        a.use_row_kernel = (fh_row_kernel_ok(h, ld) && !lds_kernel) ? 1 : 0;
        a.colscale = c.colscale;
        if (c.colscale && (lds_kernel || c.prec != 64 || h->csr.is_complex)) { h->last_error = "internal: column-scaled operand needs a gather kernel over a real matrix on complex128 panels"; return -1; }
        a.rp8 = h->csr.rp8; a.col8 = h->csr.col8; a.a8 = h->csr.a8; a.b8 = h->csr.b8;
        fh_prof_begin(h, "spmm");
        fh_launch_spmm(a, ld, h->csr.is_complex != 0, h->csr.b_identity != 0, fh_spmm_grid(a.N, ld), h->stream);
        fh_prof_end(h);
        if (a.use_row_kernel) return fh_spmm_row_grid(a.N);
        if (lds_kernel) return (8 / (ld / 16)) * fh_spmm_lds_slots(a.nblk_rows, ld);
        return fh_spmm_partials(a.N, ld);     // partial-sum rows per node
    }
    if (h->kind == FH_KIND_POLYNOMIAL) {
        // sparse polynomial handle: S_e = P(z_e), z_e = coefB[node][0] of the shifted-operator coefficients (coefA is not read);
        // complex128 panels, the plain product and dot modes 1 .. 4
        if (!h->poly.sparse || h->adjoint || c.prec != 64 || c.colscale || c.dot_mode == 6 || !c.coefB) {
            h->last_error = "internal: the polynomial operator takes a CSR polynomial handle, complex128 panels and dot modes 0 .. 4";
            return -1;
        }
        fh_polyop_call a;
        fh_op_operands(a, c);
        a.znode = c.coefB; a.z_stride = ld;
        a.nodes = c.nodes; a.m = c.m;
        return fh_launch_spmm_poly(h, ld, a);
    }
    if (h->kind == FH_KIND_OPERATOR) {
        // operator handle: the caller's products, then one launch of k_op_combine (fh_operator.hip); complex128 panels, the
        // plain product and dot modes 1 .. 4.  -1 also when a callback failed (h->op.failed): the caller returns at once
        if (h->adjoint || c.prec != 64 || c.colscale || c.dot_mode == 6 || !c.coefA || !c.coefB) {
            h->last_error = "internal: the operator handle takes forward products on complex128 panels and dot modes 0 .. 4";
            return -1;
        }
        fh_userop_call a;
        fh_op_operands(a, c);
        a.coefA = c.coefA; a.coefB = c.coefB;
        a.nodes = c.nodes; a.skip = c.skip;
        return fh_apply_user_operator(h, ld, a);
    }
    if (h->kind == FH_KIND_TERM_OPERATOR) {
        // term-operator handle: S_e = T(z_e) = sum_k f_k(z_e) A_k on the caller's products (fh_termop.hip); z_e = coefB[node][0] is
        // the key into the node table, as on the polynomial branch, and comes from the host record of the upload; complex128
        // panels, the plain product and dot modes 1 .. 4.  -1 also when a callback failed (h->op.failed)
        if (h->adjoint || c.prec != 64 || c.colscale || c.dot_mode == 6 || !c.coefB || c.coefB != h->top.shift_dev || c.nodes > (int)h->top.shift_z.size()) {
            h->last_error = "internal: the term operator takes forward products at uploaded node shifts, complex128 panels and dot modes 0 .. 4";
            return -1;
        }
        const int nt = h->poly.degree + 1, ne = (int)h->poly.fnode_z.size();
        std::vector<cplx> rows((size_t)c.nodes * nt);
        unsigned terms = 0;
        for (int q = 0; q < c.nodes; ++q) {
            const cplx z = h->top.shift_z[q];
            int e = 0;
            while (e < ne && !(h->poly.fnode_z[e].x == z.x && h->poly.fnode_z[e].y == z.y)) ++e;
            if (e == ne || h->poly.fnode.size() != (size_t)ne * nt) { h->last_error = "term operator: a solve at a shift that is no node of the contour the node values were set for (feasthip_nep_set_node_values)"; return -1; }
            for (int k = 0; k < nt; ++k) {
                const cplx f = h->poly.fnode[(size_t)e * nt + k];
                rows[(size_t)q * nt + k] = f;
                if (f.x != 0.0 || f.y != 0.0) terms |= 1u << k;
            }
        }
        cplx* dF;
        if (fh_upload_coefs(h, "top_F", rows, &dF)) return -1;
        fh_termop_call a;
        fh_op_operands(a, c);
        a.F = dF; a.cols = 0; a.terms = terms;
        a.nodes = c.nodes;
        return fh_apply_term_operator(h, ld, a);
    }
    fh_dense_op_args a;
    a.A = h->dense.A; a.B = h->dense.B; a.N = (int)h->dense.N; a.is_complex = h->dense.is_complex;
    // dense operator: complex128 panels only (fh_krylov forces prec 64 for dense matrices)
    a.nodes = c.nodes; a.coefA = c.coefA; a.coefB = c.coefB;
    fh_op_operands(a, c);
    int nblk = fh_dense_op_nblk(a.N);
    if (h->adjoint) {
        // the entry points that honour the switch use plain products only (fh_check_adjoint keeps the Krylov solvers out)
        if (c.dot_mode != 0) { h->last_error = "internal: adjoint operator with fused dots"; return -1; }
        fh_prof_begin(h, "dense_op_adjoint");
        fh_launch_dense_op_adjoint(a, ld, h->stream);
        fh_prof_end(h);
        return nblk;
    }
    fh_prof_begin(h, "dense_op");
    fh_launch_dense_op(a, ld, nblk, h->stream);
    fh_prof_end(h);
    return nblk;
}

int fh_op_nblk(feasthip_ctx* h, int ld) {
    // (an upper bound is enough here: it sizes the partial-sum buffers; the row count used by the finalize kernels is what
    //  fh_apply_operator returns for the kernel it actually launched)
    if (h->kind == FH_KIND_CSR) return std::max(std::max(fh_spmm_partials((int)h->csr.N, ld), ld == 64 ? fh_spmm_row_grid((int)h->csr.N) : 0),
                                      h->csr.lcol ? (8 / (ld / 16)) * fh_spmm_lds_slots(h->csr.nblk, ld) : 0);
    if (h->kind == FH_KIND_POLYNOMIAL && h->poly.sparse) return fh_poly_op_nblk((int)h->dense.N, ld);
    if (fh_callback_products(h)) return fh_op_combine_nblk((int)h->dense.N, ld);
    return fh_dense_op_nblk((int)h->dense.N);
}

// wide = 1: the entry point also takes m > FH_MAX_LD (processed in 64-column panels)
int fh_check_problem(feasthip_ctx* h, int64_t m, int wide) {
    if (int gate = fh_gate(h)) return gate;
    if (h->kind == FH_KIND_NONE) { h->last_error = "no matrix set (feasthip_set_dense / feasthip_set_csr)"; return FEASTHIP_ERROR_N; }
    if (h->kind == FH_KIND_POLYNOMIAL) {     // every entry point that comes through here works on a pencil; the polynomial has its own (fh_poly.hip)
        h->last_error = "this entry point does not take a polynomial handle (feasthip_set_polynomial): use feasthip_poly_solve_dev, "
                        "feasthip_poly_contour_apply_dev, feasthip_poly_matmul_dev, feasthip_poly_project_dev or feasthip_poly_ritz_residual_dev";
        return FEASTHIP_ERROR_FPM;
    }
    if (h->kind == FH_KIND_TERM_OPERATOR) {
        h->last_error = "this entry point works on a pencil: " FH_TERMOP_TAKES ", through feasthip_nep_set_node_values, feasthip_nep_solve_dev, "
                        "feasthip_nep_eval_cols_dev, feasthip_nep_resinv_apply_dev, feasthip_nep_ritz_eval_dev, feasthip_poly_project_reduced_dev and feasthip_poly_orthonormalize_dev";
        return FEASTHIP_ERROR_FPM;
    }
    if (h->kind == FH_KIND_OPERATOR) {
        h->op.failed = 0;          // a new entry point: the callback is tried again
        if (h->comm) { h->last_error = "an operator handle (feasthip_set_operator) does not take an attached communicator: it sweeps on one rank, under the Krylov solvers FEASTHIP_SOLVER_BICGSTAB, _COCG or _GMRES"; return FEASTHIP_ERROR_FPM; }
    }
    if (m <= 0 || (!wide && m > FH_MAX_LD) || m > fh_N(h)) {
        h->last_error = wide ? "block width m must satisfy 1 <= m <= N" : "block width m must satisfy 1 <= m <= min(N, 64)";
        return FEASTHIP_ERROR_M0;
    }
    return 0;
}

// Adjoint switch (feasthip_set_adjoint).  unsupported != null: the entry point has no adjoint form at all.  Otherwise the
// handle must be what the adjoint kernels cover: fp64 factors, no real projection, one rank, and either a dense problem under
// the dense LU or a CSR problem under the sparse direct solver with the multifrontal plan or the blocked band LU (the plan is
// made here if need be; fh_banded_adjoint_ready).
int fh_check_adjoint(feasthip_ctx* h, const char* what, const char* unsupported) {
    if (!h || !h->adjoint) return 0;
    const char* why = unsupported;
    if (!why && h->kind == FH_KIND_OPERATOR) why = fh_operator_why_adjoint;
    if (!why && h->kind == FH_KIND_CSR && h->solver == FEASTHIP_SOLVER_LU) why = "a CSR problem has no dense LU; its adjoint substitution needs FEASTHIP_SOLVER_BANDED (multifrontal plan or blocked band LU)";
    if (!why && h->kind == FH_KIND_CSR && h->solver != FEASTHIP_SOLVER_BANDED) why = "the solver of a CSR problem must be the sparse direct one (FEASTHIP_SOLVER_BANDED): there is no Krylov solver on the conjugate transpose";
    if (!why && h->kind != FH_KIND_CSR && h->solver != FEASTHIP_SOLVER_LU) why = "the solver must be the dense LU (FEASTHIP_SOLVER_LU)";
    if (!why && h->factor_precision == 32) why = "factor_precision = 32 is not supported (complex128 factors only)";
    if (!why && h->real_projection) why = "the real projection does not apply to an adjoint sweep";
    if (!why && h->comm) why = "an attached communicator is not supported";
    if (!why && h->kind == FH_KIND_CSR)
        for (int k : h->node_kinds) if (k != 0) { why = "per-node solver kinds (feasthip_set_node_solver) are not supported"; break; }
    std::string plan_why;
    if (!why && h->kind == FH_KIND_CSR && !h->poisoned) {
        if (hipSetDevice(h->device) != hipSuccess) { h->last_error = "hipSetDevice"; return FEASTHIP_ERROR_INTERNAL; }
        if (fh_banded_adjoint_ready(h)) { plan_why = h->last_error; why = plan_why.c_str(); }
        // the conjugate-transposed CSR set, built here at the first adjoint call so that a failed build is an error of the call
        else if (int rc = fh_adjoint_csr_ensure(h)) return rc;
    }
    if (!why) return 0;
    h->last_error = std::string(what) + " with the adjoint switch on (feasthip_set_adjoint): " + why;
    return FEASTHIP_ERROR_FPM;
}

// Operator handle: the solver settings may date from another problem (feasthip_set_solver refuses them only while the operator
// is set), so the entry points that solve look again
static int fh_check_operator_solve(feasthip_ctx* h, const char* what) {
    if (h->kind != FH_KIND_OPERATOR) return 0;
    const char* why = fh_operator_solver_why(h, h->solver, h->factor_precision);
    if (!why)
        for (int k : h->node_kinds) if (k != 0) { why = "an operator handle (feasthip_set_operator) has no matrix for a direct node (feasthip_set_node_solver); every node takes the Krylov solvers FEASTHIP_SOLVER_BICGSTAB, _COCG or _GMRES"; break; }
    if (!why) return 0;
    h->last_error = std::string(what) + ": " + why;
    return FEASTHIP_ERROR_FPM;
}

// Reserves a 64-byte aligned slot of `bytes` in the pinned ring, or *slot = null when there is no ring or the copy is too large
// for it.  Copies through the ring are queued without a synchronisation each (a FEAST loop makes about twenty); the ring
// wraps behind a stream synchronisation, so a slot is never rewritten under a copy that is still queued.
static int fh_pin_reserve(feasthip_ctx* h, size_t bytes, char** slot) {
    *slot = nullptr;
    if (!h->pin || bytes > h->pin_cap / 4) return 0;
    const size_t need = (bytes + 63) & ~(size_t)63;
    if (h->pin_off + need > h->pin_cap) { FH_CHECK(hipStreamSynchronize(h->stream)); h->pin_off = 0; }
    *slot = h->pin + h->pin_off;
    h->pin_off += need;
    return 0;
}

// Small host -> device copy through the pinned ring (queued: the source may go out of scope at once; falls back to a
// synchronous copy)
int fh_upload_small(feasthip_ctx* h, void* dst, const void* src, size_t bytes) {
    char* pin;
    int rc = fh_pin_reserve(h, bytes, &pin);
    if (rc) return rc;
    if (pin) {
        memcpy(pin, src, bytes);
        FH_CHECK(hipMemcpyAsync(dst, pin, bytes, hipMemcpyHostToDevice, h->stream));
        return 0;
    }
    FH_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream));
    FH_CHECK(hipStreamSynchronize(h->stream));
    return 0;
}

// upload per-column coefficient arrays [nodes][ld]
int fh_upload_coefs(feasthip_ctx* h, const char* name, const std::vector<cplx>& host, cplx** dev) {
    const int rc = fh_buf(h, name, host.size(), dev);
    return rc ? rc : fh_upload_small(h, *dev, host.data(), host.size() * sizeof(cplx));
}

// shifted-operator coefficients S_e = z_e B - A as [nodes][ld] arrays: coefA = -1, coefB = z_e in every column of node e
static int fh_upload_shift_coefs(feasthip_ctx* h, const char* nameA, const char* nameB, const cplx* z, int nodes, int ld,
                                 cplx** dca, cplx** dcb) {
    std::vector<cplx> ca((size_t)nodes * ld, cmake(-1, 0)), cb((size_t)nodes * ld);
    for (int e = 0; e < nodes; ++e)
        for (int c = 0; c < ld; ++c) cb[(size_t)e * ld + c] = z[e];
    int rc = fh_upload_coefs(h, nameA, ca, dca);
    if (!rc) rc = fh_upload_coefs(h, nameB, cb, dcb);
    if (!rc && h->kind == FH_KIND_TERM_OPERATOR) { h->top.shift_dev = *dcb; h->top.shift_z.assign(z, z + nodes); }      // the key into the node table
    return rc;
}

// the column mask of the running sweep, padded with ones to ld, in "kry_colmask"; *mask = null when no mask is live
static int fh_upload_col_mask(feasthip_ctx* h, int ld, const int** mask) {
    *mask = nullptr;
    if (!h->mask_live || h->col_mask.empty()) return 0;
    std::vector<int> mk(ld, 1);
    for (int c = 0; c < ld && c < (int)h->col_mask.size(); ++c) mk[c] = h->col_mask[c];
    int* dmk;
    const int rc = fh_buf(h, "kry_colmask", ld, &dmk);
    if (rc) return rc;
    FH_CHECK(hipMemcpyAsync(dmk, mk.data(), ld * sizeof(int), hipMemcpyHostToDevice, h->stream));
    FH_CHECK(hipStreamSynchronize(h->stream));
    *mask = dmk;
    return 0;
}

// start factors of a shared start, [nodes][ld]: f[e][c] = 1 / (z_e - lambda_c); 1 without Ritz values and in the padding
static std::vector<cplx> fh_start_factors(const std::vector<cplx>& z, int nodes, int m, int ld, const double* lambda_host) {
    std::vector<cplx> fs((size_t)nodes * ld, cmake(1, 0));
    if (lambda_host)
        for (int e = 0; e < nodes; ++e)
            for (int c = 0; c < m; ++c) fs[(size_t)e * ld + c] = cdiv(cmake(1, 0), cmake(z[e].x - lambda_host[c], z[e].y));
    return fs;
}

// the Ritz values of a warm start, padded with zeros to ld, in "ca_lam"; *dlam = null without a warm start
static int fh_upload_ritz_lambda(feasthip_ctx* h, const double* ritz_lambda, int m, int ld, double** dlam) {
    *dlam = nullptr;
    if (!ritz_lambda) return 0;
    std::vector<double> lam(ld, 0.0);
    for (int c = 0; c < m; ++c) lam[c] = ritz_lambda[c];
    double* dl;
    const int rc = fh_buf(h, "ca_lam", ld, &dl);
    if (rc) return rc;
    FH_CHECK(hipMemcpy(dl, lam.data(), ld * sizeof(double), hipMemcpyHostToDevice));
    *dlam = dl;
    return 0;
}

// Small device -> host copy: lands in the pinned ring (one DMA, no pageable staging), *slot points at it; valid after the
// caller's next stream synchronisation and until the ring wraps
int fh_download_small(feasthip_ctx* h, const void* src, size_t bytes, const void** slot, std::vector<char>& fallback) {
    char* pin;
    int rc = fh_pin_reserve(h, bytes, &pin);
    if (rc) return rc;
    if (!pin) {
        fallback.resize(bytes);
        pin = fallback.data();
    }
    FH_CHECK(hipMemcpyAsync(pin, src, bytes, hipMemcpyDeviceToHost, h->stream));
    *slot = pin;
    return 0;
}

// ---------------------------------------------------------------------------------------
// batched Krylov solves on panels:  (z_e B - A) X_e = RHS  for e in [0, nodes)
//   method 0: BiCGStab (general), method 1: COCG (complex-symmetric S only)
//   prec 64 : everything in complex128; X holds the initial guess on entry.
//   prec 32 : mixed precision.  The fp64 residual r0 = RHS - S X0 of the initial guess is
//             normalised per column and narrowed to complex64; the correction S d = r0/||r0||
//             is solved in complex64 from a zero guess (all panels 8 B/element, reductions still
//             fp64) and added back, X = X0 + ||r0|| d.  The FEAST refinement loop only needs a
//             relative reduction of r0 (inexact solves), so single precision is ample; the
//             warm start, the residual and the Rayleigh-Ritz step stay fp64.
// ---------------------------------------------------------------------------------------
// (fh_solve_result: fh_krylov.hpp)

// A call is about to return an error while its kernels may still be queued or running on h->stream (progress
// deadline, faulted queue).  Give the stream a bounded chance to drain; if it does not, the handle is POISONED: the
// workspaces those kernels use must not be reused or freed, so every later call fails fast until destroy (which then
// skips the stream synchronisation and leaks the buffers to the process -- the host must exit non-zero or continue in
// a fresh process; see include/feasthip.h).
static void fh_poison_unless_drained(feasthip_ctx* h, double grace_s) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t q = hipStreamQuery(h->stream);
        if (q == hipSuccess) return;                        // drained: the handle stays usable
        if (q != hipErrorNotReady) break;                   // the queue itself reports a fault
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > grace_s) break;
        std::this_thread::sleep_for(std::chrono::milliseconds(5));
    }
    h->poisoned = 1;
    h->last_error += " [handle poisoned: device work may still be in flight; destroy the handle and exit the process]";
}

// Throttle of the Krylov drivers' queueing loops: after chunk `tag` has been queued (with its publish kernel), wait -- by
// polling the host-mapped progress word -- until the device is at most three chunks behind; *all_done when a published
// count of active columns is zero.
static int fh_iter_throttle(feasthip_ctx* h, unsigned tag, std::chrono::steady_clock::time_point t_loop0, int N, int nodes,
                            bool* all_done) {
    unsigned st = 0, sc = 0;
    for (unsigned spins = 1;; ++spins) {
        const unsigned long long w = *h->h_progress;
        st = (unsigned)(w >> 32); sc = (unsigned)(w & 0xffffffffull);
        if (st >= 1 && sc == 0) { *all_done = true; break; }
        if (tag < 3 || st + 3 > tag) break;      // at most three chunks queued ahead of the device
        std::this_thread::sleep_for(std::chrono::microseconds(100));   // poll, do not burn the core
        if ((spins & 2047u) == 0) {              // every ~0.2 s: a faulted queue never publishes; do not wait for it
            const hipError_t q = hipStreamQuery(h->stream);
            if (q != hipSuccess && q != hipErrorNotReady) {
                h->last_error = std::string("device queue failed while iterating: ") + hipGetErrorString(q);
                h->poisoned = 1;
                return FEASTHIP_ERROR_INTERNAL;
            }
            // a wedged kernel keeps answering "not ready": overall deadline, generous against the slowest
            // measured iteration (2 ms with 16 nodes x 64 columns at N = 50 000), scaled by the problem size
            const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_loop0).count();
            const double budget = 30.0 + 0.05 * (double)h->maxit * (1.0 + (double)N * nodes / 8.0e5);
            if (waited > budget) {
                h->last_error = "device did not make progress on the Krylov iterations within the deadline (" + std::to_string((int)budget) + " s)";
                fh_poison_unless_drained(h, 2.0);
                return FEASTHIP_ERROR_INTERNAL;
            }
        }
    }
    return 0;
}

// partial-sum rows that one launch of the fused vector kernels leaves (half = 1: the 8 B/element geometry)
static int fh_fused_vec_rows(int N, int ld, int half) {
    int blk, seg, per;
    fh_fused_vec_geometry(N, ld, half, &blk, &seg, &per);
    return blk * seg;
}

// The queueing loop of the Krylov sweeps.  It never blocks in the HIP runtime: chunks of `check_every` steps are queued back
// to back (body(it) queues step `it`), each chunk followed by a tiny kernel that publishes (chunk tag, sum of live[0 .. nlive))
// to a host-mapped word.  The host polls that word, stays at most three chunks ahead of the device and stops queueing once a
// published count is zero.  (A hipStreamSynchronize per chunk idled the GPU for milliseconds each time: 1.1 s -> 0.7 s per
// cfg-3 solve.)  N and nodes scale the deadline.  Returns the number of steps queued; *rc != 0: a step or the throttle failed.
template <class Body>
static int fh_queue_chunks(feasthip_ctx* h, const int* live, int nlive, int N, int nodes, Body body, int* rc) {
    const int check_every = fh_knob::check_every();
    *h->h_progress = 0ull;
    int it = *rc = 0;
    unsigned tag = 0;
    bool all_done = false;
    const auto t_loop0 = std::chrono::steady_clock::now();
    while (it < h->maxit && !all_done) {
        const int chunk = std::min(check_every, h->maxit - it);
        for (int k = 0; k < chunk; ++k)
            if ((*rc = body(it + k))) return it + k;
        it += chunk;
        ++tag;
        fh_launch_publish_progress(live, nlive, h->d_progress, tag, h->stream);
        if ((*rc = fh_iter_throttle(h, tag, t_loop0, N, nodes, &all_done))) return it;
    }
    return it;
}

// Per-column bookkeeping of `nodes` nodes ([nodes][ld] device arrays; d_target: FH_FAIL_TARGET only; the rules: fh_policy.hpp, fh_column_failed), folded into res: the
// iterations per column and per node, the worst relative residual and the status of node node0 + e (the caller sizes
// res.status).
static int fh_collect_columns(feasthip_ctx* h, const int* d_iters, const int* d_status, const int* d_active, const double* d_rnorm,
                              const double* d_r0norm, const double* d_target, int nodes, int m, int ld, int node0,
                              fh_fail_rule rule, fh_solve_result& res) {
    const size_t nl = (size_t)nodes * ld;
    std::vector<int> iters(nl), status(nl), active(nl);
    std::vector<double> rnorm(nl), r0(nl), target(d_target ? nl : 0);
    FH_CHECK(hipMemcpy(iters.data(), d_iters, nl * sizeof(int), hipMemcpyDeviceToHost));
    FH_CHECK(hipMemcpy(status.data(), d_status, nl * sizeof(int), hipMemcpyDeviceToHost));
    FH_CHECK(hipMemcpy(active.data(), d_active, nl * sizeof(int), hipMemcpyDeviceToHost));
    FH_CHECK(hipMemcpy(rnorm.data(), d_rnorm, nl * sizeof(double), hipMemcpyDeviceToHost));
    FH_CHECK(hipMemcpy(r0.data(), d_r0norm, nl * sizeof(double), hipMemcpyDeviceToHost));
    if (d_target) FH_CHECK(hipMemcpy(target.data(), d_target, nl * sizeof(double), hipMemcpyDeviceToHost));
    for (int e = 0; e < nodes; ++e) {
        int mx = 0, st = 0;
        for (int c = 0; c < m; ++c) {
            const size_t i = (size_t)e * ld + c;
            mx = std::max(mx, iters[i]);
            res.col_iters.push_back(iters[i]);
            if (fh_column_failed(rule, active[i], status[i], rnorm[i], r0[i], d_target ? target[i] : 0.0, h->atol, h->rtol)) st = FEASTHIP_ERROR_NO_CONVERGENCE;
            if (r0[i] > 0) res.max_rel_res = std::max(res.max_rel_res, rnorm[i] / r0[i]);
        }
        res.iters_sum += mx; res.node_iters.push_back(mx); res.max_iters = std::max(res.max_iters, mx);
        res.status[node0 + e] = st;
    }
    return 0;
}

// (fh_krylov_opts, the optional parts of a fh_krylov call: fh_krylov.hpp)

namespace {      // (internal linkage for the member functions, as the static helpers have)
// What the phases of fh_krylov share: the shape of the call, the work panels and the argument blocks of the kernels
struct fh_krylov_work {
    feasthip_ctx* h;
    fh_solve_result& res;
    int method, prec, ld, m, nodes, N;
    size_t panel;
    bool fused = false, lazy = false;
    void *R, *Rh, *P, *V, *S, *T, *D = nullptr, *RHS32 = nullptr, *Xk = nullptr;    // Xk: the panel the recurrences update, X or D
    fh_krylov_scalars s;
    double *r0_64, *inv_r0;                  // fp64 initial-residual norms and their inverses (mixed precision)
    cplx *part1, *part2, *sp[2] = {nullptr, nullptr};
    int nblk_vec, fv_rows = 0, fv1_rows = 0; // partial rows of the vector kernels; fv1: the lazy start's first fused launch
    cplx *sum_acc = nullptr, *dfs = nullptr; // dfs, lazy_src: start factors and shared source of a lazy start
    const cplx* lazy_src = nullptr;
    fh_op_call oc;                           // the argument blocks of the operator, finalize and vector kernels
    fh_fin_args fa;
    fh_vec_args va;
    fh_fused_fin_args ff;                    // (fused iteration; s, rho, rr and tickets are filled once)
    int alloc(const std::vector<cplx>& z, const std::vector<cplx>* wnode);
    int start(const std::vector<cplx>& z, const cplx* RHS, cplx* X, const fh_krylov_opts& opt);
    int bicgstab_step(), cocg_step();          // non-zero: the operator failed (an operator handle's callback), nothing more was queued
    void cocg_fused_step(int it);
};

// allocate: the work panels R, Rhat, P, V, S, T (+ D and RHS32 for the mixed-precision correction), the per-column scalars
// and the partial sums come from the handle's buffer cache; the shift coefficients, the node weights and the column mask go
// up; the argument blocks of the operator, finalize and vector kernels are filled.
int fh_krylov_work::alloc(const std::vector<cplx>& z, const std::vector<cplx>* wnode) {
    const size_t esz = prec == 32 ? sizeof(cplxf) : sizeof(cplx);
    int rc;
    char* base;                                  // complex128 or complex64 panels: sized in bytes
    const int nvec = 6 + (prec == 32 ? 2 : 0);
    if ((rc = fh_buf(h, "kry_vecs", (size_t)nvec * nodes * panel * esz, &base))) return rc;
    auto vec = [&](int i) { return (void*)(base + (size_t)i * nodes * panel * esz); };
    R = vec(0); Rh = vec(1); P = vec(2); V = vec(3); S = vec(4); T = vec(5);
    if (prec == 32) { D = vec(6); RHS32 = vec(7); }
    // operator handle: the callback sees whole panels, and the vector kernels never write the padding columns of S and T
    if (fh_callback_products(h)) FH_CHECK(hipMemsetAsync(base, 0, (size_t)nvec * nodes * panel * esz, h->stream));
    const size_t nl = (size_t)nodes * ld;
    if ((rc = fh_buf(h, "kry_scal_c", 4 * nl, &s.rho))) return rc;
    s.alpha = s.rho + nl; s.omega = s.alpha + nl; s.beta = s.omega + nl;
    if ((rc = fh_buf(h, "kry_scal_d", 5 * nl, &s.r0norm))) return rc;
    s.target = s.r0norm + nl; s.rnorm = s.target + nl;
    r0_64 = s.rnorm + nl; inv_r0 = r0_64 + nl;
    if ((rc = fh_buf(h, "kry_scal_i", 4 * nl + 2 * nodes + 4, &s.active))) return rc;
    s.iters = s.active + nl; s.status = s.iters + nl; s.node_active = s.status + nl;
    // Fused COCG iteration (fh_sparse.hip): SpMM with five dots -> one finalize -> one vector kernel.  CSR operator through
    // the gather kernel only; FH_COCG_FUSED=0 selects the five-launch form for comparison.
    fused = method == 1 && h->kind == FH_KIND_CSR && fh_knob::cocg_fused();
    if (sum_acc || fused) {
        s.accum = s.node_active + nodes + 4; s.node_accum = s.accum + nl;
        FH_CHECK(hipMemsetAsync(s.accum, 0, (nl + nodes) * sizeof(int), h->stream));
    }
    cplx* d_wnode = nullptr;
    if (sum_acc && (rc = fh_upload_coefs(h, "kry_wnode", *wnode, &d_wnode))) return rc;
    const int nblk_op = fh_op_nblk(h, ld);
    nblk_vec = fh_kry_nblk(N, ld, nodes);
    if (fused) { fv_rows = fh_fused_vec_rows(N, ld, prec == 32); fv1_rows = fh_fused_vec_rows(N, ld, 1); }
    const int nblk_max = std::max(std::max(std::max(nblk_op, nblk_vec), fv_rows), fv1_rows);
    if ((rc = fh_buf(h, "kry_partials", 2 * (size_t)nodes * nblk_max * ld, &part1))) return rc;
    part2 = part1 + (size_t)nodes * nblk_max * ld;
    if (fused) {
        const size_t one = (size_t)nodes * nblk_op * ld;
        if ((rc = fh_buf(h, "kry_partials_op", 2 * one, &sp[0]))) return rc;
        sp[1] = sp[0] + one;
        if ((rc = fh_buf(h, "kry_tickets", (size_t)nodes, &ff.tickets))) return rc;
        ff.s = s; ff.rho = part1; ff.rr = part2;
        FH_CHECK(hipMemsetAsync(ff.tickets, 0, (size_t)nodes * sizeof(unsigned long long), h->stream));
    }
    cplx *dca, *dcb;
    if ((rc = fh_upload_shift_coefs(h, "kry_coefA", "kry_coefB", z.data(), nodes, ld, &dca, &dcb))) return rc;
    oc.m = m; oc.uniform_coef = 1; oc.coefA = dca; oc.coefB = dcb; oc.nodes = nodes;
    oc.partial1 = part1; oc.partial2 = part2;
    fa.s = s; fa.partial1 = part1; fa.partial2 = part2; fa.m = m; fa.rtol = h->rtol; fa.atol = h->atol;
    fa.atol_scale = nullptr; fa.mode = method;
    if ((rc = fh_upload_col_mask(h, ld, &fa.col_mask))) return rc;
    memset(&va, 0, sizeof(va));
    va.N = N; va.node_stride = panel; va.R = R; va.Rhat = Rh; va.P = P; va.V = V; va.S = S; va.T = T;
    va.s = s; va.partial1 = part1; va.partial2 = part2; va.prec = prec;
    va.counters = h->profiling ? h->d_counters : nullptr;
    va.sum_acc = sum_acc; va.wnode = d_wnode; va.sum_scale = (sum_acc && prec == 32) ? r0_64 : nullptr; va.nodes = nodes;
    return 0;
}

// start: R, P (BiCGStab: Rhat too), rho and the norms of the stop test.  fp64: R = RHS - S X in one operator product, then
// P = R.  Mixed precision: that residual in fp64, normalised per column and narrowed to complex64; the recurrences then update
// the correction D from zero instead of X.  Shared start (sum mode, fp64): R = P = f_e,c * shared_src; lazy (fused iteration
// over a real CSR operator): not even those are written -- the first operator product reads the source itself and the first
// vector kernel writes them (fh_sparse.hip: k_cocg_init_lazy).
int fh_krylov_work::start(const std::vector<cplx>& z, const cplx* RHS, cplx* X, const fh_krylov_opts& opt) {
    const size_t nl = (size_t)nodes * ld;
    int rc;
    Xk = X;
    const bool shared_start = opt.shared_src && sum_acc && method == 1 && prec == 64;
    cplx* R64 = (cplx*)R;                        // mixed precision: the fp64 residual goes to a panel set of its own
    if (!shared_start && prec == 32 && (rc = fh_buf(h, "kry_r64", (size_t)nodes * panel, &R64))) return rc;
    if (!shared_start) {
        // R = RHS - S X0, ||R||^2
        oc.prec = 64; oc.X = X; oc.x_stride = panel; oc.Y = R64; oc.y_stride = panel; oc.Bvec = RHS; oc.b_stride = 0;
        oc.dot_mode = 3; oc.node_active = nullptr;
        fa.nblk = fh_apply_operator(h, ld, oc);
        if (fa.nblk < 0) return FEASTHIP_ERROR_INTERNAL;
        res.op_calls += 1;
    }
    if (!shared_start && prec == 32) {
        fh_fin_args f0 = fa;                       // only to obtain ||r0|| per column
        f0.rtol = 0.0; f0.atol = 0.0; f0.mode = 0;
        fh_launch_fin_init(f0, ld, nodes, h->stream);
        FH_CHECK(hipMemcpyAsync(r0_64, s.r0norm, nl * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
        // narrow: RHS32 = R64 / ||r0||, D = 0, R = RHS32
        fh_launch_narrow_scaled(R64, panel, (cplxf*)RHS32, panel, r0_64, N, ld, nblk_vec, nodes, h->stream);
        FH_CHECK(hipMemsetAsync(D, 0, (size_t)nodes * panel * sizeof(cplxf), h->stream));
        FH_CHECK(hipMemcpyAsync(R, RHS32, (size_t)nodes * panel * sizeof(cplxf), hipMemcpyDeviceToDevice, h->stream));
        Xk = D;
        // norms of the (unit) scaled residual for the stop test; atol is rescaled by 1/||r0||
        std::vector<double> hr0(nl), hinv(nl);
        FH_CHECK(hipMemcpyAsync(hr0.data(), r0_64, nl * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        FH_CHECK(hipStreamSynchronize(h->stream));
        for (size_t i = 0; i < nl; ++i) hinv[i] = hr0[i] > 0 ? 1.0 / hr0[i] : 0.0;
        FH_CHECK(hipMemcpyAsync(inv_r0, hinv.data(), nl * sizeof(double), hipMemcpyHostToDevice, h->stream));
        FH_CHECK(hipStreamSynchronize(h->stream));
        fa.atol_scale = inv_r0;
    }
    va.X = Xk;
    // FH_NO_LAZY_START=1: materialise R and P of a shared start as before.  Read per call (the tests flip it).
    lazy = shared_start && fused && h->kind == FH_KIND_CSR && !h->csr.is_complex && !fh_knob::no_lazy_start() &&
           (!opt.shared_lambda || opt.shared_lambda_host) && !fh_knob::lds_spmm();
    if (lazy) {
        if ((rc = fh_upload_coefs(h, "kry_fscale", fh_start_factors(z, nodes, m, ld, opt.shared_lambda_host), &dfs))) return rc;
        lazy_src = opt.shared_src;
        fh_vec_args vs = va;
        vs.Q = opt.shared_src; vs.first_scale = dfs;
        fh_launch_cocg_init_lazy(vs, ld, nblk_vec, nodes, h->stream);
    } else if (shared_start) {
        fh_vec_args vs = va;
        vs.Q = opt.shared_src; vs.lambda = opt.shared_lambda; vs.znode = opt.dznode;
        fh_launch_cocg_init_shared(vs, ld, nblk_vec, nodes, h->stream);
    } else if (method == 1 || prec == 32) {
        // COCG: P = R, rho = r^T r, ||r||.  BiCGStab needs it for ||R||^2 of the narrowed residual only.
        fh_launch_cocg_init(va, ld, nblk_vec, nodes, h->stream);
    }
    if (method == 1 || prec == 32) fa.nblk = nblk_vec;     // else: the partial rows of the residual product
    fh_launch_fin_init(fa, ld, nodes, h->stream);
    if (method == 0) fh_launch_copy_r(va, ld, nblk_vec, nodes, h->stream);            // Rhat = R ; P = R
    oc.prec = prec; oc.Bvec = nullptr; oc.b_stride = 0; oc.x_stride = panel; oc.y_stride = panel;
    return 0;
}

// One BiCGStab step: two operator products, each with its finalize and vector update, then rho and the new direction
int fh_krylov_work::bicgstab_step() {
    // V = S P, sigma = <Rhat, V>
    oc.X = P; oc.Y = V; oc.U = Rh; oc.u_stride = panel; oc.dot_mode = 1; oc.node_active = s.node_active;
    fa.nblk = fh_apply_operator(h, ld, oc);
    if (fa.nblk < 0) return FEASTHIP_ERROR_INTERNAL;
    fh_prof_begin(h, "dot_finalize"); fh_launch_fin_alpha(fa, ld, nodes, h->stream); fh_prof_end(h);
    fh_prof_begin(h, "bicg_s"); fh_launch_s_update(va, ld, nblk_vec, nodes, h->stream); fh_prof_end(h);
    // T = S S, <T,S>, <T,T>
    oc.X = S; oc.Y = T; oc.U = nullptr; oc.dot_mode = 2;
    fa.nblk = fh_apply_operator(h, ld, oc);
    if (fa.nblk < 0) return FEASTHIP_ERROR_INTERNAL;
    fh_prof_begin(h, "dot_finalize"); fh_launch_fin_omega(fa, ld, nodes, h->stream); fh_prof_end(h);
    fh_prof_begin(h, "bicg_xr"); fh_launch_xr_update(va, ld, nblk_vec, nodes, h->stream); fh_prof_end(h);
    fa.nblk = nblk_vec;
    fh_prof_begin(h, "dot_finalize"); fh_launch_fin_rho(fa, ld, nodes, h->stream); fh_prof_end(h);
    fh_prof_begin(h, "bicg_p"); fh_launch_p_update(va, ld, nblk_vec, nodes, h->stream); fh_prof_end(h);
    res.op_calls += 2;
    return 0;
}

// One COCG step in five launches: Q = S P with sigma = p^T S p, finalize, x / r update, finalize of rho, new direction
int fh_krylov_work::cocg_step() {
    oc.X = P; oc.Y = V; oc.U = nullptr; oc.dot_mode = 4; oc.node_active = s.node_active;     // Q is stored in V
    fa.nblk = fh_apply_operator(h, ld, oc);
    if (fa.nblk < 0) return FEASTHIP_ERROR_INTERNAL;
    fh_prof_begin(h, "dot_finalize"); fh_launch_fin_alpha(fa, ld, nodes, h->stream); fh_prof_end(h);
    fh_prof_begin(h, "cocg_xr"); fh_launch_cocg_update(va, ld, nblk_vec, nodes, h->stream); fh_prof_end(h);
    fa.nblk = nblk_vec;
    fh_prof_begin(h, "dot_finalize"); fh_launch_fin_rho(fa, ld, nodes, h->stream); fh_prof_end(h);
    fh_prof_begin(h, "cocg_p");
    if (sum_acc) fh_launch_cocg_p_sum(va, ld, nodes, h->stream);
    else fh_launch_cocg_p(va, ld, nblk_vec, nodes, h->stream);
    fh_prof_end(h);
    res.op_calls += 1;
    return 0;
}

// Step `it` of the fused COCG iteration (fh_sparse.hip): Q = S P (stored in V) with sigma = p^T q and kappa = q^T q, one
// finalize, one vector kernel.  Step 0 of a lazy start reads the shared source times the start factors instead of P.
void fh_krylov_work::cocg_fused_step(int it) {
    const bool first_lazy = lazy && it == 0;
    oc.X = first_lazy ? (const void*)lazy_src : P; oc.x_stride = first_lazy ? 0 : panel; oc.colscale = first_lazy ? dfs : nullptr;
    oc.Y = V; oc.U = nullptr; oc.dot_mode = 6; oc.node_active = s.node_active;
    oc.partial1 = sp[0]; oc.partial2 = sp[1];
    va.first_src = first_lazy ? lazy_src : nullptr; va.first_scale = first_lazy ? dfs : nullptr;
    ff.sig = sp[0]; ff.kap = sp[1]; ff.final_check = 0;
    ff.predict_stop = (h->rtol >= 1e-3 && h->atol == 0.0) ? 1 : 0;
    ff.nblk_op = fh_apply_operator(h, ld, oc);
    // first step: the init kernel's partial rows; second (lazy start): the half-geometry launch's
    ff.nblk_vec = it == 0 ? fa.nblk : ((lazy && it == 1) ? fv1_rows : fv_rows);
    fh_prof_begin(h, "dot_finalize"); fh_launch_fused_fin(ff, ld, nodes, h->stream); fh_prof_end(h);
    fh_prof_begin(h, "cocg_vec"); fh_launch_fused_vec(va, ld, h->stream); fh_prof_end(h);
    res.op_calls += 1;
}

}  // namespace

// Batched BiCGStab (method 0) or COCG (method 1) on `nodes` panels, in five phases: allocate, start, iterate, finish, collect.
int fh_krylov(feasthip_ctx* h, int method, int prec, int ld, int m, int nodes, const std::vector<cplx>& z,
              const cplx* RHS, cplx* X, size_t stride, fh_solve_result& res, const fh_krylov_opts& opt) {
    if (h->kind != FH_KIND_CSR) prec = 64;          // the dense operator kernel takes complex128 panels only
    fh_krylov_work k{h, res};
    k.method = method; k.prec = prec; k.ld = ld; k.m = m; k.nodes = nodes; k.N = (int)fh_N(h); k.panel = (size_t)k.N * ld;
    k.sum_acc = (method == 1 && opt.wnode) ? opt.sum_acc : nullptr;
    if (stride != k.panel) { h->last_error = "internal: solution stride mismatch"; return FEASTHIP_ERROR_INTERNAL; }
    int rc;
    if ((rc = k.alloc(z, opt.wnode))) return rc;
    if ((rc = k.start(z, RHS, X, opt))) return rc;
    // iterate: the steps go to the stream in chunks; the published count is the number of nodes with a live column
    const auto t_loop0 = std::chrono::steady_clock::now();
    const int it = fh_queue_chunks(h, k.s.node_active, nodes, k.N, nodes, [&](int i) {
        if (k.fused) { k.cocg_fused_step(i); return 0; }
        return method == 0 ? k.bicgstab_step() : k.cocg_step();
    }, &rc);
    if (rc) return rc;
    // finish: the fused iteration's last stop test (true norms from the last vector kernel's partials: no SpMM follows it),
    // the one synchronisation of the solve, and X = X0 + ||r0|| D for a mixed-precision solve outside sum mode
    if (k.fused && it > 0) {
        fh_fused_fin_args& ff = k.ff;
        ff.sig = ff.kap = nullptr; ff.nblk_op = 0; ff.final_check = 1; ff.predict_stop = 0;
        ff.nblk_vec = (k.lazy && it == 1) ? k.fv1_rows : k.fv_rows;
        fh_launch_fused_fin(ff, ld, nodes, h->stream);
    }
    FH_CHECK(hipStreamSynchronize(h->stream));
    if (fh_knob::debug_timing())
        fprintf(stderr, "[fh_krylov] nodes=%d its queued=%d loop wall %.3f ms\n", nodes, it,
                1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t_loop0).count());
    if (prec == 32 && !k.sum_acc)
        fh_launch_widen_axpy(X, k.panel, (const cplxf*)k.Xk, k.panel, k.r0_64, k.N, ld, k.nblk_vec, nodes, h->stream);
    // collect: the per-column counts, norms and flags come back and fold into res
    res.status.assign(nodes, 0);
    return fh_collect_columns(h, k.s.iters, k.s.status, k.s.active, k.s.rnorm, k.s.r0norm, nullptr, nodes, m, ld, 0,
                              FH_FAIL_STOP_TEST, res);
}

// ---------------------------------------------------------------------------------------
// Shifted COCG sweep in sum mode (fh_sparse.hip, "shifted COCG"): CSR operator with real values, B = I, complex128 panels,
// shared start r_e^0 = f_e,c * shared_src with f = 1 / (z_e - lambda_c) (lambda_host given) or 1.  One operator product per
// iteration, on the direction panel of the seed (the node with the smallest |Im z_e|, ties to the lowest index); the other
// nodes follow by scalar recurrences and one direction panel each.  Work panels: r, q, `nodes` directions (+ the caller's
// accumulator).  res as fh_krylov fills it: per (node, column) the steps in which that pair still advanced.
// ---------------------------------------------------------------------------------------
static int fh_shifted_cocg(feasthip_ctx* h, int ld, int m, int nodes, const std::vector<cplx>& z, fh_solve_result& res,
                           cplx* sum_acc, const std::vector<cplx>& wnode, const cplx* shared_src, const double* lambda_host,
                           int* seed_out, int* seed_iters_out) {
    const int N = (int)fh_N(h);
    const size_t panel = (size_t)N * ld;
    const size_t nl = (size_t)nodes * ld;
    const int ntiles = ld / 16;
    int rc;
    int seed = 0;
    for (int e = 1; e < nodes; ++e)
        if (fabs(z[e].y) < fabs(z[seed].y)) seed = e;
    fh_shift_args a;
    memset(&a, 0, sizeof(a));
    a.N = N; a.nodes = nodes; a.seed = seed; a.m = m; a.node_stride = panel;
    if ((rc = fh_buf(h, "shc_vecs", (size_t)(2 + nodes) * panel, &a.R))) return rc;
    a.Qv = a.R + panel; a.P = a.Qv + panel;
    a.sum_acc = sum_acc; a.src = shared_src;
    if ((rc = fh_buf(h, "shc_scal_c", 5 * nl + 2 * (size_t)ld, &a.pi))) return rc;
    a.pi_old = a.pi + nl; a.coef = a.pi_old + nl; a.ipi = a.coef + nl; a.beta_e = a.ipi + nl;
    a.alpha = a.beta_e + nl; a.beta = a.alpha + ld;
    if ((rc = fh_buf(h, "shc_scal_d", 3 * nl, &a.r0norm))) return rc;
    a.target = a.r0norm + nl; a.rnorm = a.target + nl;
    const size_t nint = 4 * nl + (size_t)ld + (size_t)ntiles * nodes + ntiles + 2;
    if ((rc = fh_buf(h, "shc_scal_i", nint, &a.active))) return rc;
    a.accum = a.active + nl; a.iters = a.accum + nl; a.status = a.iters + nl;
    a.col_step = a.status + nl; a.node_step = a.col_step + ld;
    a.tile_alive = a.node_step + (size_t)ntiles * nodes; a.alive_total = a.tile_alive + ntiles; a.passes = a.alive_total + 1;
    FH_CHECK(hipMemsetAsync(a.active, 0, nint * sizeof(int), h->stream));
    // start factors, shifts against the seed, weights, the seed's operator coefficients
    std::vector<cplx> sg(nodes);
    for (int e = 0; e < nodes; ++e) sg[e] = csub(z[e], z[seed]);
    cplx *dfs, *dsg, *dw, *dca, *dcb;
    if ((rc = fh_upload_coefs(h, "shc_fscale", fh_start_factors(z, nodes, m, ld, lambda_host), &dfs))) return rc;
    if ((rc = fh_upload_coefs(h, "shc_sigma", sg, &dsg))) return rc;
    if ((rc = fh_upload_coefs(h, "shc_wnode", wnode, &dw))) return rc;
    if ((rc = fh_upload_shift_coefs(h, "shc_coefA", "shc_coefB", &z[seed], 1, ld, &dca, &dcb))) return rc;
    a.fscale = dfs; a.sigma = dsg; a.wnode = dw;
    a.rtol = h->rtol; a.atol = h->atol;
    if ((rc = fh_upload_col_mask(h, ld, &a.col_mask))) return rc;
    const int nblk_op = fh_op_nblk(h, ld);
    const int nrow_max = std::max(256, fh_fused_vec_rows(N, ld, 1));
    if ((rc = fh_buf(h, "shc_partials", 2 * (size_t)(nrow_max + nblk_op) * ld, &a.rho_part))) return rc;
    a.rr_part = a.rho_part + (size_t)nrow_max * ld;
    cplx* sp0 = a.rr_part + (size_t)nrow_max * ld;
    cplx* sp1 = sp0 + (size_t)nblk_op * ld;
    a.sig = sp0; a.kap = sp1;

    a.nblk_vec = fh_launch_shift_init(a, ld, h->stream);
    fh_op_call oc;
    oc.m = m; oc.uniform_coef = 1; oc.coefA = dca; oc.coefB = dcb; oc.nodes = 1; oc.prec = 64;
    oc.X = a.P + (size_t)seed * panel; oc.x_stride = panel; oc.Y = a.Qv; oc.y_stride = panel;
    oc.dot_mode = 6; oc.node_active = a.alive_total; oc.partial1 = sp0; oc.partial2 = sp1;
    // iterate: the published count is the number of column tiles with a live column
    const int it = fh_queue_chunks(h, a.tile_alive, ntiles, N, nodes, [&](int i) {
        a.nblk_op = fh_apply_operator(h, ld, oc);
        if (a.nblk_op < 0) return (int)FEASTHIP_ERROR_INTERNAL;
        a.phase = i == 0 ? 0 : 1;
        fh_prof_begin(h, "dot_finalize"); fh_launch_shift_fin(a, ld, h->stream); fh_prof_end(h);
        fh_prof_begin(h, "shift_vec"); a.nblk_vec = fh_launch_shift_vec(a, ld, h->stream); fh_prof_end(h);
        return 0;
    }, &rc);
    if (rc) return rc;
    if (it > 0) {
        a.phase = 2;                     // the stop test of the last step, on the true norm the last vector kernel left
        fh_launch_shift_fin(a, ld, h->stream);
    }
    FH_CHECK(hipStreamSynchronize(h->stream));
    res.status.assign(nodes, 0);
    if ((rc = fh_collect_columns(h, a.iters, a.status, a.active, a.rnorm, a.r0norm, nullptr, nodes, m, ld, 0, FH_FAIL_STOP_TEST, res)))
        return rc;
    *seed_out = seed;
    FH_CHECK(hipMemcpy(seed_iters_out, a.passes, sizeof(int), hipMemcpyDeviceToHost));
    res.op_calls = *seed_iters_out;        // the products that ran (those queued behind the last live column return at once)
    return 0;
}

// ---------------------------------------------------------------------------------------
// Block COCG sweep in sum mode (fh_bcocg.hip): CSR operator with real values (B given or B = I), complex128 panels, shared
// start r_e^0 = f_e,c * shared_src as the shifted sweep has it.  Per node the live columns share one block Krylov space; the
// nodes advance in lock-step and each leaves on its own (converged / breakdown), decided on the device.  A node that broke
// down is finished by the per-column sweep (fh_krylov, one node, sum mode) from the residual it stopped with: that panel is
// its shared source, the accumulator the same.  res as fh_krylov fills it: a live column reports its node's block steps
// (plus the per-column steps of a fallback).  *steps_max: most block steps of a node; *passes: operator node-passes that ran.
// ---------------------------------------------------------------------------------------
static int fh_block_cocg(feasthip_ctx* h, int ld, int m, int nodes, const std::vector<cplx>& z, fh_solve_result& res,
                         cplx* sum_acc, const std::vector<cplx>& wnode, const cplx* shared_src, const double* lambda_host,
                         const double* dlam, const cplx* dz, cplx* Xdummy, int* steps_max, int* breakdowns, int* passes) {
    const int N = (int)fh_N(h);
    const size_t panel = (size_t)N * ld, nl = (size_t)nodes * ld, mat = (size_t)ld * ld;
    int rc;
    fh_bcocg_args a;
    memset(&a, 0, sizeof(a));
    a.N = N; a.nodes = nodes; a.m = m; a.node_stride = panel; a.sum_acc = sum_acc; a.src = shared_src;
    a.rtol = h->rtol; a.atol = h->atol;
    if ((rc = fh_buf(h, "bcg_vecs", 3 * (size_t)nodes * panel, &a.Q))) return rc;
    a.P = a.Q + (size_t)nodes * panel; a.W = a.P + (size_t)nodes * panel;
    cplx* sm;
    if ((rc = fh_buf(h, "bcg_small", (2 + 12 * (size_t)nodes) * mat, &sm))) return rc;
    auto slot = [&](int i) { return sm + 2 * mat + (size_t)i * nodes * mat; };
    a.SH = sm; a.ST = sm + mat;
    a.GA = slot(0); a.GH = slot(1); a.GT = slot(2); a.T = slot(3); a.Tn = slot(4); a.U = slot(5); a.Ze = slot(6); a.Zi = slot(7);
    a.Cs = slot(8); a.Al = slot(9); a.M1 = slot(10); a.Be = slot(11);
    FH_CHECK(hipMemsetAsync(sm, 0, (2 + 12 * (size_t)nodes) * mat * sizeof(cplx), h->stream));
    if ((rc = fh_buf(h, "bcg_scal_d", 3 * nl, &a.r0norm))) return rc;
    a.target = a.r0norm + nl; a.rnorm = a.target + nl;
    const size_t nint = 4 * nl + 5 * (size_t)nodes;
    if ((rc = fh_buf(h, "bcg_scal_i", nint, &a.active))) return rc;
    a.iters = a.active + nl; a.status = a.iters + nl; a.live = a.status + nl;
    a.node_active = a.live + nl; a.stop = a.node_active + nodes; a.steps = a.stop + nodes; a.passes = a.steps + nodes;
    a.nlive = a.passes + nodes;
    FH_CHECK(hipMemsetAsync(a.active, 0, nint * sizeof(int), h->stream));
    cplx* gw;
    if ((rc = fh_buf(h, "bcg_gram", fh_bcocg_gram_work_elems(ld, nodes), &gw))) return rc;
    cplx *dfs, *dw, *dca, *dcb;
    if ((rc = fh_upload_coefs(h, "bcg_fscale", fh_start_factors(z, nodes, m, ld, lambda_host), &dfs))) return rc;
    if ((rc = fh_upload_coefs(h, "bcg_wnode", wnode, &dw))) return rc;
    if ((rc = fh_upload_shift_coefs(h, "bcg_coefA", "bcg_coefB", z.data(), nodes, ld, &dca, &dcb))) return rc;
    a.fscale = dfs; a.wnode = dw;
    if ((rc = fh_upload_col_mask(h, ld, &a.col_mask))) return rc;

    // start: the two Gram matrices of the shared source serve every node; Q_e = P_e = src Zi_e
    fh_prof_begin(h, "bcocg_gram"); fh_launch_bcocg_gram(shared_src, 0, shared_src, 0, N, ld, 1, gw, a.SH, a.ST, nullptr, h->stream); fh_prof_end(h);
    fh_prof_begin(h, "bcocg_small"); fh_launch_bcocg_small(a, ld, 0, h->stream); fh_prof_end(h);
    fh_prof_begin(h, "bcocg_update"); fh_launch_bcocg_update(a, ld, 0, h->stream); fh_prof_end(h);
    fh_op_call oc;
    oc.m = m; oc.uniform_coef = 1; oc.coefA = dca; oc.coefB = dcb; oc.nodes = nodes; oc.prec = 64;
    oc.X = a.P; oc.x_stride = panel; oc.Y = a.W; oc.y_stride = panel; oc.dot_mode = 0; oc.node_active = a.node_active;
    // iterate: the published count is the number of nodes still running
    fh_queue_chunks(h, a.node_active, nodes, N, nodes, [&](int) {
        if (fh_apply_operator(h, ld, oc) < 0) return (int)FEASTHIP_ERROR_INTERNAL;
        fh_prof_begin(h, "bcocg_gram"); fh_launch_bcocg_gram(a.P, panel, a.W, panel, N, ld, nodes, gw, nullptr, a.GA, a.stop, h->stream); fh_prof_end(h);
        fh_prof_begin(h, "bcocg_small"); fh_launch_bcocg_small(a, ld, 1, h->stream); fh_prof_end(h);
        fh_prof_begin(h, "bcocg_update"); fh_launch_bcocg_update(a, ld, 1, h->stream); fh_prof_end(h);
        fh_prof_begin(h, "bcocg_gram"); fh_launch_bcocg_gram(a.Q, panel, a.Q, panel, N, ld, nodes, gw, a.GH, a.GT, a.stop, h->stream); fh_prof_end(h);
        fh_prof_begin(h, "bcocg_small"); fh_launch_bcocg_small(a, ld, 2, h->stream); fh_prof_end(h);
        fh_prof_begin(h, "bcocg_update"); fh_launch_bcocg_update(a, ld, 2, h->stream); fh_prof_end(h);
        return 0;
    }, &rc);
    if (rc) return rc;
    FH_CHECK(hipStreamSynchronize(h->stream));
    res.status.assign(nodes, 0);
    if ((rc = fh_collect_columns(h, a.iters, a.status, a.active, a.rnorm, a.r0norm, nullptr, nodes, m, ld, 0, FH_FAIL_STOP_TEST, res)))
        return rc;
    std::vector<int> word(3 * (size_t)nodes);          // stop, steps, passes (adjacent on the device)
    FH_CHECK(hipMemcpy(word.data(), a.stop, word.size() * sizeof(int), hipMemcpyDeviceToHost));
    const int *stop = word.data(), *steps = stop + nodes, *ran = steps + nodes;
    *steps_max = *breakdowns = *passes = 0;
    int launches = 0;
    for (int e = 0; e < nodes; ++e) {
        *steps_max = std::max(*steps_max, steps[e]); *passes += ran[e]; launches = std::max(launches, ran[e]);
        if (stop[e] == 2) *breakdowns += 1;
    }
    res.op_calls = launches;
    if (!*breakdowns) return 0;
    // fallback: W_e = Q_e C_e is what is left of the right-hand side of a node that broke down; the per-column sweep adds its
    // solution of S_e D = W_e to the accumulator.  A node that broke down before its first step starts from the source itself.
    fh_prof_begin(h, "bcocg_update"); fh_launch_bcocg_update(a, ld, 3, h->stream); fh_prof_end(h);
    for (int e = 0; e < nodes; ++e) {
        if (stop[e] != 2) continue;
        const bool at_start = steps[e] == 0 && ran[e] == 0;
        fh_krylov_opts opt;
        const std::vector<cplx> ze(1, z[e]), we(1, wnode[e]);
        opt.sum_acc = sum_acc; opt.wnode = &we;
        opt.shared_src = at_start ? shared_src : a.W + (size_t)e * panel;
        if (at_start) { opt.shared_lambda = dlam; opt.shared_lambda_host = lambda_host; opt.dznode = dz + e; }
        fh_solve_result re;
        if ((rc = fh_krylov(h, 1, 64, ld, m, 1, ze, shared_src, Xdummy, panel, re, opt))) return rc;
        res.status[e] = re.status[0];
        res.iters_sum += re.node_iters[0]; res.node_iters[e] += re.node_iters[0];
        res.max_iters = std::max(res.max_iters, res.node_iters[e]);
        for (int c = 0; c < m; ++c) res.col_iters[(size_t)e * m + c] += re.col_iters[c];
        res.max_rel_res = std::max(res.max_rel_res, re.max_rel_res);
        res.op_calls += re.op_calls; *passes += (int)re.op_calls;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------
// restarted GMRES(m) on panels -- the reference's iterative solver
// (solve_shifted_iterative!, src/sparse/feast_sparse.jl:164-203; Krylov.jl gmres with
// restart=true, memory=m, zero initial guess unless X holds one, stop ||r|| <= atol + rtol ||r0||).
// Device resident (fh_gmres.hip): all columns of all local nodes advance in lock-step; basis panels, Hessenberg
// columns, Givens rotations and the per-column stop test live on the device.  The host only queues kernels: it
// looks at the device's published progress word without blocking to stop queueing once every column has converged
// inside a cycle, and reads the true-residual check once per restart cycle.
// maxit caps the lock-steps that RAN, and spmm_calls counts them: the host may have queued up to six steps behind the last
// live column of a cycle (they return at once), so the device leaves the cycle's largest kdim in the second host-mapped word
// and the host adds it after the synchronisation of the next cycle start.  (Counting queued steps made the budget left for a
// column that the restart's true residual reactivates, and spmm_calls, depend on host/device timing.)
// ---------------------------------------------------------------------------------------
// Preconditioned (pc != null, feasthip_set_preconditioner; a CSR problem): the same cycles in the variable u = M x, which lives
// in X; the operator is I + c_e B M^-1 -- one substitution on the pivot factors of the batch's nodes into the T panels, then
// k_precond_op -- at every cycle start and every step.  u0 = M x0 is one product of the plain operator with the pivot's
// coefficients (skipped for a zero guess, whose first cycle start needs no substitution either); after the last cycle
// x = M^-1 u goes back into X and one more plain product forms the true residual b - S_e x, whose norm is the one reported.
int fh_gmres(feasthip_ctx* h, int ld, int m, int nodes_all, const std::vector<cplx>& z, const cplx* RHS, cplx* X,
             size_t stride, fh_solve_result& res, fh_gmres_precond* pc) {
    const int N = (int)fh_N(h);
    const size_t panel = (size_t)N * ld;
    const int mr = std::max(h->restart, 2);
    int rc;
    cplx *V, *W, *part, *npart;
    res.status.assign(nodes_all, 0);
    // node batches: the basis costs (mr + 2) panels per node, and one more for T = M^-1 v under the preconditioner
    const size_t per_node = (size_t)(mr + 2 + (pc ? 1 : 0)) * panel * sizeof(cplx);
    cplx* T = nullptr;
    // budget: at most 48 GiB and at most half of what the device has free right now (plus what this handle already
    // holds for the basis) -- several ranks may share one card (shm rehearsal layout), and parts with less HBM exist
    size_t budget = (size_t)48 << 30;
    {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            auto held = h->bufs.find("gm_V");
            const size_t avail = free_b / 2 + (held != h->bufs.end() ? held->second.second : 0);
            budget = std::min(budget, std::max(avail, per_node));
        }
    }
    budget = fh_knob::gmres_budget_bytes(budget);
    int nbatch = (int)std::max<size_t>(1, std::min<size_t>((size_t)nodes_all, budget / std::max<size_t>(per_node, 1)));
    // an allocation failure halves the batch before it becomes an error
    for (;;) {
        if (fh_buf(h, "gm_V", (size_t)nbatch * (mr + 1) * panel, &V) == 0 && fh_buf(h, "gm_W", (size_t)nbatch * panel, &W) == 0 &&
            (!pc || fh_buf(h, "gm_T", (size_t)nbatch * panel, &T) == 0)) break;
        if (nbatch == 1) return FEASTHIP_ERROR_MEMORY;
        hipGetLastError();                                   // clear the sticky out-of-memory status
        nbatch = (nbatch + 1) / 2;
    }
    const int nblk_vec = fh_kry_nblk(N, ld, nbatch);
    const int nblk_op = fh_op_nblk(h, ld);
    for (int e0 = 0; e0 < nodes_all; e0 += nbatch) {
        const int nodes = std::min(nbatch, nodes_all - e0);
        const size_t nl = (size_t)nodes * ld;
        if ((rc = fh_buf(h, "gm_V", (size_t)nodes * (mr + 1) * panel, &V))) return rc;
        if ((rc = fh_buf(h, "gm_W", (size_t)nodes * panel, &W))) return rc;
        if ((rc = fh_buf(h, "gm_part", fh_gm_partial_elems(mr, nblk_vec, nodes, ld), &part))) return rc;
        if ((rc = fh_buf(h, "gm_npart", (size_t)nodes * std::max(nblk_vec, nblk_op) * ld, &npart))) return rc;
        const size_t hsz = nl * (size_t)(mr + 1) * mr;
        cplx* sc;
        double* sd;
        int* si;
        if ((rc = fh_buf(h, "gm_small_c", hsz + nl * (mr + 1) * 2 + nl * mr * 3, &sc))) return rc;
        if ((rc = fh_buf(h, "gm_small_d", nl * 4, &sd))) return rc;
        if ((rc = fh_buf(h, "gm_small_i", nl * 4 + nodes, &si))) return rc;
        fh_gmres_args ga;
        ga.N = N; ga.mr = mr; ga.panel = panel; ga.V = V; ga.v_node_stride = (size_t)(mr + 1) * panel; ga.W = W;
        ga.partial = part; ga.npartial = npart;
        ga.H = sc; ga.hcur = ga.H + hsz; ga.g = ga.hcur + nl * (mr + 1); ga.cs = ga.g + nl * (mr + 1); ga.sn = ga.cs + nl * mr;
        ga.y = ga.sn + nl * mr;
        ga.inv = sd; ga.r0norm = sd + nl; ga.target = sd + 2 * nl; ga.rnorm = sd + 3 * nl;
        ga.active = si; ga.iters = si + nl; ga.status = si + 2 * nl; ga.kdim = si + 3 * nl; ga.node_active = si + 4 * nl;
        FH_CHECK(hipMemsetAsync(sc, 0, hsz * sizeof(cplx), h->stream));
        if (fh_callback_products(h)) {     // operator handle: the callback sees whole basis panels, padding columns included
            FH_CHECK(hipMemsetAsync(V, 0, (size_t)nodes * (mr + 1) * panel * sizeof(cplx), h->stream));
            FH_CHECK(hipMemsetAsync(W, 0, (size_t)nodes * panel * sizeof(cplx), h->stream));
        }

        cplx *dca, *dcb;
        if ((rc = fh_upload_shift_coefs(h, "gm_coefA", "gm_coefB", z.data() + e0, nodes, ld, &dca, &dcb))) return rc;
        cplx* Xb = X + (size_t)e0 * stride;
        fh_op_call oc;
        oc.m = m; oc.uniform_coef = 1; oc.coefA = dca; oc.coefB = dcb; oc.nodes = nodes; oc.prec = 64;
        oc.partial2 = npart;
        // preconditioned batch: the slots of its nodes' pivots, c_e = z_e - z_p, and u0 = M x0 in place of the guess
        std::vector<int> pslots;
        fh_precond_args pa;
        memset(&pa, 0, sizeof(pa));
        // (pc->sweeps counts the substitutions of the cycle starts, of the lock-steps that RAN and the final one: like
        //  spmm_calls it does not depend on how far ahead of the device the host queued)
        auto substitute = [&](const cplx* src, size_t src_stride, cplx* dst, size_t dst_stride) -> int {
            return fh_direct_solve_slots(h, true, ld, m, pslots, src, src_stride, dst, dst_stride);
        };
        auto copy_panels = [&](const cplx* src, size_t src_stride, cplx* dst, size_t dst_stride) -> hipError_t {
            hipError_t err = hipSuccess;
            for (int e = 0; e < nodes && err == hipSuccess; ++e)
                err = hipMemcpyAsync(dst + (size_t)e * dst_stride, src + (size_t)e * src_stride, panel * sizeof(cplx), hipMemcpyDeviceToDevice, h->stream);
            return err;
        };
        if (pc) {
            if ((rc = fh_buf(h, "gm_T", (size_t)nodes * panel, &T))) return rc;
            pslots.assign(pc->slot.begin() + e0, pc->slot.begin() + e0 + nodes);
            std::vector<cplx> ce(nodes);
            for (int e = 0; e < nodes; ++e) ce[e] = csub(z[e0 + e], pc->zp[e0 + e]);
            cplx* dce;
            if ((rc = fh_upload_coefs(h, "gm_cnode", ce, &dce))) return rc;
            pa.rowptr = h->csr.rowptr; pa.col = h->csr.col; pa.bval = h->csr.bval; pa.N = N; pa.nodes = nodes; pa.m = m;
            pa.T = T; pa.t_node_stride = panel; pa.Y = W; pa.y_node_stride = panel; pa.cnode = dce;
            if (!pc->zero_guess) {
                cplx *dpa, *dpb;
                if ((rc = fh_upload_shift_coefs(h, "gm_pcoefA", "gm_pcoefB", pc->zp.data() + e0, nodes, ld, &dpa, &dpb))) return rc;
                fh_op_call uc = oc;
                uc.coefA = dpa; uc.coefB = dpb; uc.X = Xb; uc.x_stride = stride; uc.Y = W; uc.y_stride = panel; uc.partial2 = nullptr;
                if (fh_apply_operator(h, ld, uc) < 0) return FEASTHIP_ERROR_INTERNAL;
                res.op_calls += 1;
                FH_CHECK(copy_panels(W, panel, Xb, stride));
            }
        }

        int total_it = 0, first = 1;                             // total_it: the lock-steps that ran
        unsigned tag = 0;
        h->h_progress[0] = 0ull; h->h_progress[1] = 0ull;
        auto seen = [&](unsigned& st, unsigned& cnt) { unsigned long long w = *h->h_progress; st = (unsigned)(w >> 32); cnt = (unsigned)(w & 0xffffffffull); };
        while (true) {
            // true residual r = b - S x (into W), ||r|| per column, activity from the stop test
            oc.X = Xb; oc.x_stride = stride; oc.Y = W; oc.y_stride = panel; oc.Bvec = RHS; oc.b_stride = 0; oc.dot_mode = 3; oc.node_active = nullptr;
            int nb_norm;
            if (pc) {
                // r = b - u - c B M^-1 u; the zero guess of the first cycle has T = 0 without a substitution
                if (first && pc->zero_guess) FH_CHECK(hipMemsetAsync(T, 0, (size_t)nodes * panel * sizeof(cplx), h->stream));
                else if ((rc = substitute(Xb, stride, T, panel))) return rc;
                else pc->sweeps += 1;
                pa.V = Xb; pa.v_node_stride = stride; pa.Bvec = RHS; pa.partial2 = npart; pa.node_active = nullptr;
                fh_prof_begin(h, "precond_op_start");      // (a class of its own: every node of the batch is live here)
                fh_launch_precond_op(pa, ld, h->csr.is_complex != 0, h->csr.b_identity != 0, h->stream);
                fh_prof_end(h);
                nb_norm = fh_spmm_partials(N, ld);
            } else {
                nb_norm = fh_apply_operator(h, ld, oc);
            }
            if (nb_norm < 0) return FEASTHIP_ERROR_INTERNAL;
            res.op_calls += 1;
            fh_launch_gm_start(ga, ld, nb_norm, nodes, first, h->rtol, h->atol, m, h->stream);
            first = 0;
            ++tag;
            fh_launch_publish_progress(ga.node_active, nodes, h->d_progress, tag, h->stream);
            FH_CHECK(hipStreamSynchronize(h->stream));           // the one host round trip per restart cycle
            const int ran = (int)h->h_progress[1];               // of the cycle just finished (0 before the first)
            total_it += ran; res.op_calls += ran;
            unsigned st = 0, cnt = 0;
            seen(st, cnt);
            if (cnt == 0 || total_it >= h->maxit) break;
            fh_launch_gm_scale_store(ga, ld, W, panel, 0, nblk_vec, nodes, h->stream);           // v_0 = r / beta
            int ksteps = 0;
            const unsigned tag0 = tag;
            for (int k = 0; k < mr && total_it + k < h->maxit; ++k) {
                oc.X = V + (size_t)k * panel; oc.x_stride = ga.v_node_stride; oc.Y = W; oc.y_stride = panel; oc.Bvec = nullptr;
                oc.dot_mode = 0; oc.node_active = ga.node_active; oc.partial2 = nullptr;
                int nb_w = 0;
                if (pc) {                                                                      // w = v_k + c B M^-1 v_k
                    if ((rc = substitute(V + (size_t)k * panel, ga.v_node_stride, T, panel))) return rc;
                    pa.V = V + (size_t)k * panel; pa.v_node_stride = ga.v_node_stride; pa.Bvec = nullptr; pa.partial2 = nullptr;
                    pa.node_active = ga.node_active;
                    fh_prof_begin(h, "precond_op");
                    fh_launch_precond_op(pa, ld, h->csr.is_complex != 0, h->csr.b_identity != 0, h->stream);
                    fh_prof_end(h);
                } else {
                    nb_w = fh_apply_operator(h, ld, oc);                                       // w = S v_k
                }
                oc.partial2 = npart;
                if (nb_w < 0) return FEASTHIP_ERROR_INTERNAL;
                fh_prof_begin(h, "gmres_ortho");
                fh_launch_gm_orthogonalize(ga, ld, k, nblk_vec, nodes, h->stream);             // CGS2 against v_0..v_k
                fh_launch_gm_givens(ga, ld, k, nblk_vec, nodes, h->stream);
                fh_launch_gm_scale_store(ga, ld, W, panel, k + 1, nblk_vec, nodes, h->stream); // v_{k+1} = w / h_{k+1,k}
                fh_prof_end(h);
                ++tag;
                fh_launch_publish_progress(ga.node_active, nodes, h->d_progress, tag, h->stream);
                ++ksteps;
                // non-blocking look at the device's progress: stop queueing steps once every column has converged
                seen(st, cnt);
                if (st > tag0 && cnt == 0) break;
                if (tag - st > 6) {                       // stay at most six steps ahead of the device
                    for (unsigned spins = 1; tag - st > 6; ++spins) {
                        std::this_thread::sleep_for(std::chrono::microseconds(100));
                        seen(st, cnt);
                        if ((spins & 2047u) == 0) {
                            const hipError_t q = hipStreamQuery(h->stream);
                            if (q != hipSuccess && q != hipErrorNotReady) {
                                h->last_error = std::string("device queue failed inside a GMRES cycle: ") + hipGetErrorString(q);
                                return FEASTHIP_ERROR_INTERNAL;
                            }
                        }
                    }
                    if (st > tag0 && cnt == 0) break;
                }
            }
            fh_launch_gm_finish_cycle(ga, ld, Xb, stride, ksteps, nblk_vec, nodes, h->d_progress + 1, h->stream);   // x += V y
        }
        const double worst_before = res.max_rel_res;
        if ((rc = fh_collect_columns(h, ga.iters, ga.status, ga.active, ga.rnorm, ga.r0norm, ga.target, nodes, m, ld, e0, FH_FAIL_TARGET, res)))
            return rc;
        if (pc) {
            // x = M^-1 u, then the true residual b - S_e x: its norm replaces the estimate in what the call reports (the
            // statuses stay those of the last cycle start, which the step counts and the reference are pinned to)
            if ((rc = substitute(Xb, stride, T, panel))) return rc;
            pc->sweeps += 1 + total_it;
            FH_CHECK(copy_panels(T, panel, Xb, stride));
            oc.X = Xb; oc.x_stride = stride; oc.Y = W; oc.y_stride = panel; oc.Bvec = RHS; oc.b_stride = 0; oc.dot_mode = 0;
            oc.node_active = nullptr; oc.partial2 = nullptr;
            if (fh_apply_operator(h, ld, oc) < 0) return FEASTHIP_ERROR_INTERNAL;
            res.op_calls += 1;
            cplx *dwork, *ddots;
            if ((rc = fh_buf(h, "gm_tn_work", (size_t)fh_vec_nblk(N, ld) * ld, &dwork))) return rc;
            if ((rc = fh_buf(h, "gm_tn_dots", nl, &ddots))) return rc;
            for (int e = 0; e < nodes; ++e)
                fh_launch_dot_cols(W + (size_t)e * panel, W + (size_t)e * panel, N, ld, dwork, ddots + (size_t)e * ld, h->stream);
            std::vector<cplx> dots(nl);
            std::vector<double> r0(nl);
            FH_CHECK(hipMemcpyAsync(dots.data(), ddots, nl * sizeof(cplx), hipMemcpyDeviceToHost, h->stream));
            FH_CHECK(hipMemcpyAsync(r0.data(), ga.r0norm, nl * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            FH_CHECK(hipStreamSynchronize(h->stream));
            res.max_rel_res = worst_before;
            for (int e = 0; e < nodes; ++e)
                for (int c = 0; c < m; ++c)
                    if (r0[(size_t)e * ld + c] > 0) res.max_rel_res = std::max(res.max_rel_res, std::sqrt(dots[(size_t)e * ld + c].x) / r0[(size_t)e * ld + c]);
        }
    }
    return 0;
}

// What a set preconditioner (feasthip_set_preconditioner) cannot go with; checked by every entry point that honours it
static int fh_check_precond(feasthip_ctx* h, const char* what) {
    if (h->pc_pivots.empty() || h->kind == FH_KIND_NONE) return 0;
    const char* why = nullptr;
    if (h->kind != FH_KIND_CSR) why = "it needs a CSR problem (feasthip_set_csr): a dense, operator, term or polynomial handle has no sparse factors for the pivots";
    else if (h->solver != FEASTHIP_SOLVER_GMRES) why = "the solver must be FEASTHIP_SOLVER_GMRES (BiCGStab, COCG and the direct solvers do not take it)";
    else if (h->factor_precision != 64) why = "factor_precision = 32 is not supported: the identity form I + c B M^-1 needs exact (complex128) pivot factors";
    else if (h->adjoint) why = "the adjoint switch (feasthip_set_adjoint) is not supported";
    else if (fh_comm_nranks(h) > 1) why = "a communicator with more than one rank is not supported";
    else if (h->pc_node_pivot.size() != h->zne.size()) why = "it was set for a contour with another node count";
    else
        for (int k : h->node_kinds) if (k != 0) { why = "a node-solver setting with a direct node (feasthip_set_node_solver) is not supported"; break; }
    if (!why) return 0;
    h->last_error = std::string(what) + " with a preconditioner set (feasthip_set_preconditioner): " + why;
    return FEASTHIP_ERROR_FPM;
}

// GMRES over nodes that each name a pivot (pivot[i]: index into h->pc_pivots, -1: unpreconditioned).  The pivots the nodes name
// are factored through the band / multifrontal cache; then maximal runs of nodes of one kind -- preconditioned, plain, or
// without factors (pivot not factorable: status 8, a zero panel) -- go to fh_gmres one after the other.  With every node
// preconditioned, the usual case, that is one call and one lock-step count.  Adds to h->pc_last.
static int fh_gmres_preconditioned(feasthip_ctx* h, int ld, int m, const std::vector<cplx>& z, const std::vector<int>& pivot, bool zero_guess,
                                   const cplx* RHS, cplx* X, size_t stride, int64_t* nfact, fh_solve_result& sr) {
    const int nodes = (int)z.size();
    const size_t panel = (size_t)fh_N(h) * ld;
    int rc;
    std::vector<int> used, where(h->pc_pivots.size(), -1);           // distinct pivots of these nodes, pivot -> position in `used`
    for (int i = 0; i < nodes; ++i)
        if (pivot[i] >= 0 && where[pivot[i]] < 0) { where[pivot[i]] = (int)used.size(); used.push_back(pivot[i]); }
    std::vector<cplx> zp(used.size());
    for (size_t p = 0; p < used.size(); ++p) zp[p] = h->pc_pivots[used[p]];
    std::vector<int> slots, pstatus;
    int64_t nf = 0, slot_bytes = 0;
    int fell_back = 0;
    h->pc_last.panels += 1;
    if (!used.empty()) {
        if ((rc = fh_banded_precond_factor(h, zp, slots, pstatus, &nf, &fell_back, &slot_bytes))) return rc;
        h->pc_last.used += 1;
    }
    if (nfact) *nfact += nf;
    h->pc_last.pivots = std::max(h->pc_last.pivots, (int)used.size());
    h->pc_last.factorizations += nf; h->pc_last.fell_back |= fell_back;
    h->pc_last.factor_bytes = std::max<int64_t>(h->pc_last.factor_bytes, (int64_t)used.size() * slot_bytes);
    std::vector<int> kind(nodes, 0);                                 // 0 plain, 1 preconditioned, 2 no factors
    for (int i = 0; i < nodes; ++i)
        if (pivot[i] >= 0) kind[i] = pstatus[where[pivot[i]]] == 0 ? 1 : 2;
    sr.status.assign(nodes, 0);
    for (int i0 = 0; i0 < nodes;) {
        int i1 = i0 + 1;
        while (i1 < nodes && kind[i1] == kind[i0]) ++i1;
        const int cnt = i1 - i0;
        if (kind[i0] == 2) {
            FH_CHECK(hipMemsetAsync(X + (size_t)i0 * stride, 0, ((size_t)(cnt - 1) * stride + panel) * sizeof(cplx), h->stream));
            for (int i = i0; i < i1; ++i) { sr.status[i] = FEASTHIP_ERROR_LAPACK; sr.node_iters.push_back(0); sr.col_iters.insert(sr.col_iters.end(), m, 0); }
        } else {
            const std::vector<cplx> zr(z.begin() + i0, z.begin() + i1);
            fh_solve_result part;
            fh_gmres_precond pc;
            if (kind[i0] == 1) {
                pc.zero_guess = zero_guess;
                for (int i = i0; i < i1; ++i) { pc.slot.push_back(slots[where[pivot[i]]]); pc.zp.push_back(h->pc_pivots[pivot[i]]); }
            }
            if ((rc = fh_gmres(h, ld, m, cnt, zr, RHS, X + (size_t)i0 * stride, stride, part, kind[i0] == 1 ? &pc : nullptr))) return rc;
            h->pc_last.sweeps += pc.sweeps;
            std::copy(part.status.begin(), part.status.end(), sr.status.begin() + i0);
            sr.node_iters.insert(sr.node_iters.end(), part.node_iters.begin(), part.node_iters.end());
            sr.col_iters.insert(sr.col_iters.end(), part.col_iters.begin(), part.col_iters.end());
            sr.iters_sum += part.iters_sum; sr.op_calls += part.op_calls;
            sr.max_iters = std::max(sr.max_iters, part.max_iters); sr.max_rel_res = std::max(sr.max_rel_res, part.max_rel_res);
        }
        i0 = i1;
    }
    return 0;
}

static bool fh_is_complex_input(feasthip_ctx* h) { return h->kind == FH_KIND_CSR ? h->csr.is_complex != 0 : h->dense.is_complex != 0; }

// ---------------------------------------------------------------------------------------
// contour sweep
// ---------------------------------------------------------------------------------------
// Mixed-precision dense solves (factor_precision = 32): complex64 LU factors, fp64 iterative refinement
//     Y <- Y + LU32^-1 (RHS - (z_e B - A) Y)
// until the relative residual of every column is below max(rtol, 1e-14) (rtol of feasthip_set_solver; a
// value >= 1 means no refinement at all: plain complex64 solves for the early, inexact FEAST loops), or
// stops improving; at most 8 steps.
// The residual is the fp64 dense operator kernel, so the result has fp64 accuracy as long as
// cond(z_e B - A) * eps32 < 1.  `single`: one shift through fh_direct_solve_single (nodes == 1).
static int fh_dense_lu_refined(feasthip_ctx* h, int ld, int m, int nodes, const std::vector<cplx>& z, const cplx* Rhs, cplx* Y,
                               size_t panel, std::vector<int>& status, int64_t* nfact, bool single, double* worst_out, bool banded) {
    const int N = (int)fh_N(h);
    int rc;
    // banded: the same loop over the complex64 band factors of the sparse direct solver (residual = fp64 SpMM)
    auto solve = [&](const cplx* rhs, size_t rhs_stride, cplx* out, int64_t* nf) -> int {
        if (single) return fh_direct_solve_single(h, banded, ld, m, z[0], rhs, out, &status[0], nf);
        return fh_direct_solve_nodes(h, banded, ld, m, nodes, z, rhs, rhs_stride, out, panel, status, nf);
    };
    if ((rc = solve(Rhs, 0, Y, nfact))) return rc;
    const double tol = std::max(h->rtol, 1e-14);
    if (tol >= 1.0) { if (worst_out) *worst_out = 0.0; return 0; }
    cplx *R, *D, *part, *ddots;
    if ((rc = fh_buf(h, "lr_R", (size_t)nodes * panel, &R))) return rc;
    if ((rc = fh_buf(h, "lr_D", (size_t)nodes * panel, &D))) return rc;
    if ((rc = fh_buf(h, "lr_part", (size_t)fh_vec_nblk(N, ld) * ld, &part))) return rc;
    if ((rc = fh_buf(h, "lr_dots", (size_t)(nodes + 1) * ld, &ddots))) return rc;
    const std::vector<cplx> mone(ld, cmake(-1, 0));
    cplx *dca, *dcb, *dmone;
    if ((rc = fh_upload_shift_coefs(h, "lr_coefA", "lr_coefB", z.data(), nodes, ld, &dca, &dcb))) return rc;
    if ((rc = fh_upload_coefs(h, "lr_mone", mone, &dmone))) return rc;
    std::vector<cplx> dots((size_t)(nodes + 1) * ld);
    fh_launch_dot_cols(Rhs, Rhs, N, ld, part, ddots + (size_t)nodes * ld, h->stream);
    double prev = 1e300, worst = 0.0;
    for (int it = 0; it < 8; ++it) {
        fh_op_call oc;
        oc.m = m; oc.uniform_coef = 1; oc.prec = 64;
        oc.X = Y; oc.x_stride = panel; oc.Y = R; oc.y_stride = panel; oc.coefA = dca; oc.coefB = dcb;
        oc.Bvec = Rhs; oc.nodes = nodes;
        fh_apply_operator(h, ld, oc);                               // R = RHS - S Y
        for (int e = 0; e < nodes; ++e)
            fh_launch_dot_cols(R + (size_t)e * panel, R + (size_t)e * panel, N, ld, part, ddots + (size_t)e * ld, h->stream);
        FH_CHECK(hipMemcpyAsync(dots.data(), ddots, dots.size() * sizeof(cplx), hipMemcpyDeviceToHost, h->stream));
        FH_CHECK(hipStreamSynchronize(h->stream));
        worst = 0.0;
        for (int e = 0; e < nodes; ++e) {
            if (status[e]) continue;                                 // singular factor: reported, not refined
            for (int c = 0; c < m; ++c) {
                const double b2 = dots[(size_t)nodes * ld + c].x, r2 = dots[(size_t)e * ld + c].x;
                if (b2 > 0.0) worst = std::max(worst, std::sqrt(r2 / b2));
            }
        }
        if (!(worst > tol) || !(worst < 0.5 * prev) || !std::isfinite(worst)) break;
        prev = worst;
        if ((rc = solve(R, panel, D, nullptr))) return rc;          // D = LU32^-1 R
        for (int e = 0; e < nodes; ++e)
            fh_launch_axpy_cols(Y + (size_t)e * panel, D + (size_t)e * panel, dmone, N, ld, h->stream);   // Y += D
    }
    if (worst_out) *worst_out = worst;
    return 0;
}

// Moment matrices of a sweep that is wider than one panel (variant B with M0 > 64): the panel call below holds the
// solution block Y_e of ITS columns only, so it adds the block column  w_e Q_all^H Y_e  (all rows, its columns) to the
// host accumulators; the caller uploads them once every panel is done.
struct fh_moment_ctx {
    const cplx* dQ_all = nullptr;       // N x m_all column-major device pointer (the whole subspace)
    int m_all = 0, col0 = 0;            // total width, first column of the current panel
    std::vector<cplx>* aq = nullptr;    // m_all x m_all column-major host accumulators
    std::vector<cplx>* sq = nullptr;
};

// Panels handed in / left behind in the kernels' own row-major layout (resident refinement loop): Qp replaces the import of a
// column-major dQ, eigres is A q - lambda B q for the Ritz values passed as ritz_lambda (the shared start residual: saves its
// product), out receives Q_proj as a panel (the export to a column-major dQproj is skipped when that pointer is null).
struct fh_panel_io {
    const cplx* Qp = nullptr;
    const cplx* eigres = nullptr;
    cplx* out = nullptr;
};

// Local nodes in sweep order: the Krylov nodes, then the *nd direct ones (feasthip_set_node_solver), each ascending.  With at
// least one direct node the handle must be able to mix the two families: a CSR problem, COCG or BiCGStab on fp64 panels.
// A handle whose own solver is the sparse direct one takes every node there anyway, so the kinds change nothing.
static int fh_split_nodes(feasthip_ctx* h, std::vector<int>& order, int* nd) {
    const int nodes = h->node_count;
    order.clear();
    std::vector<int> direct;
    const bool mixed = h->node_kinds.size() == h->zne.size() && h->solver != FEASTHIP_SOLVER_BANDED;
    for (int e = 0; e < nodes; ++e) {
        if (mixed && h->node_kinds[h->node_ids[e]] == FEASTHIP_SOLVER_BANDED) direct.push_back(e);
        else order.push_back(e);
    }
    *nd = (int)direct.size();
    order.insert(order.end(), direct.begin(), direct.end());
    if (!*nd) return 0;
    const char* why = nullptr;
    if (h->kind != FH_KIND_CSR) why = "a dense problem has no sparse direct solver";
    else if (h->solver != FEASTHIP_SOLVER_COCG && h->solver != FEASTHIP_SOLVER_BICGSTAB) why = "the handle's solver must be COCG or BICGSTAB (GMRES sweeps do not mix)";
    else if (h->factor_precision != 64) why = "factor_precision = 32 is not supported";
    else if (*nd > FH_NODE_FINISH_MAX) why = "more than 64 direct nodes on one rank";
    if (why) { h->last_error = std::string("per-node solver (feasthip_set_node_solver) with direct nodes: ") + why; return FEASTHIP_ERROR_FPM; }
    return 0;
}

// What the solver branches of one panel sweep share.  The panels of Y, and z / w with them, are ordered Krylov nodes first,
// then the direct ones, both in ascending node order (order[i] = local node of panel i).
struct fh_panel_sweep {
    int m, ld, N, nodes, nk, nd;
    size_t panel;
    cplx *Qp, *Rhs, *Y;
    std::vector<int> order;
    std::vector<cplx> z, w;
    const double* ritz_lambda; const fh_panel_io* io;
    cplx* sum_acc = nullptr;
    bool sum_shared = false;          // sum mode started from one shared residual panel: no per-node solution panels exist
};

// Dense LU or sparse direct solves of every node (the two differ in the solver called only); factor_precision 32 refines
// complex64 factors.  Y_e = S_e^-1 Rhs, sr.status per node, sr.max_rel_res the worst refined residual.
static int fh_panel_direct(feasthip_ctx* h, const fh_panel_sweep& g, int64_t* nfact, fh_solve_result& sr) {
    const bool banded = h->solver == FEASTHIP_SOLVER_BANDED;
    if (!banded && h->kind != FH_KIND_DENSE) { h->last_error = "solver LU requires a dense matrix (sparse direct factorisation is not provided; use BICGSTAB)"; return FEASTHIP_ERROR_FPM; }
    sr.status.assign(g.nodes, 0);
    if (h->factor_precision == 32)
        return fh_dense_lu_refined(h, g.ld, g.m, g.nodes, g.z, g.Rhs, g.Y, g.panel, sr.status, nfact, false, &sr.max_rel_res, banded);
    return fh_direct_solve_nodes(h, banded, g.ld, g.m, g.nodes, g.z, g.Rhs, 0, g.Y, g.panel, sr.status, nfact);
}

// Shared start (sum mode, fp64 panels): the warm start Y0_e = q_c/(z_e - lambda_c) has the residual
// (A q_c - lambda_c B q_c)/(z_e - lambda_c) -- ONE eigen-residual panel serves every node -- and its weighted
// sum over the nodes is q_c * sum_e w_e/(z_e - lambda_c): neither the warm-start panels nor their residual
// products are ever formed.  Zero guess: the residual is RHS for every node.  *src: that one panel.
static int fh_shared_start_source(feasthip_ctx* h, const fh_panel_sweep& g, const cplx** src) {
    if (!g.ritz_lambda) { *src = g.Rhs; return 0; }
    if (g.io && g.io->eigres) { *src = g.io->eigres; return 0; }      // left behind by the Ritz step of the previous loop
    std::vector<cplx> ca(g.ld, cmake(1, 0)), cb(g.ld, cmake(0, 0));
    for (int c = 0; c < g.m; ++c) cb[c] = cmake(-g.ritz_lambda[c], 0);
    cplx *dca, *dcb, *eigres;
    int rc;
    if ((rc = fh_upload_coefs(h, "ca_rcoefA", ca, &dca))) return rc;
    if ((rc = fh_upload_coefs(h, "ca_rcoefB", cb, &dcb))) return rc;
    if ((rc = fh_buf(h, "ca_eigres", g.panel, &eigres))) return rc;
    fh_op_call oc;
    oc.m = g.m;
    oc.X = g.Qp; oc.Y = eigres; oc.coefA = dca; oc.coefB = dcb;
    if (fh_apply_operator(h, g.ld, oc) < 0) return FEASTHIP_ERROR_INTERNAL;      // A q - lambda B q (B = I handled by the operator kernel)
    *src = eigres;
    return 0;
}

// COCG / BiCGStab: the direct nodes' solves into their own panels, the initial guess (or the shared start of sum mode), the
// shifted or the per-node sweep over the Krylov nodes.  sr comes back in local node order.
static int fh_panel_krylov(feasthip_ctx* h, fh_panel_sweep& g, bool want_moments, int64_t* nfact, fh_solve_result& sr) {
    const int m = g.m, ld = g.ld, nodes = g.nodes, nk = g.nk, nd = g.nd;
    const size_t panel = g.panel;
    int rc;
    if (h->solver == FEASTHIP_SOLVER_COCG && fh_is_complex_input(h)) {
        h->last_error = "solver COCG needs a complex-SYMMETRIC shifted matrix: real-symmetric A and B only";
        return FEASTHIP_ERROR_FPM;
    }
    const std::vector<cplx> zk(g.z.begin(), g.z.begin() + nk), wk(g.w.begin(), g.w.begin() + nk), zd(g.z.begin() + nk, g.z.end());
    // direct nodes first, on the same stream: sparse direct solves of the shared right-hand side into their own panels
    // (no warm start, no column mask, as the LU path); the factors live in the band / multifrontal cache, matched by z
    std::vector<int> status_d;
    if (nd && (rc = fh_direct_solve_subset(h, true, ld, m, zd, g.Rhs, g.Y + (size_t)nk * panel, panel, status_d, nfact))) return rc;
    fh_krylov_opts opt;
    cplx* dz = nullptr; double* dlam = nullptr;
    if (nk && (rc = fh_upload_coefs(h, "ca_z", zk, &dz))) return rc;
    if ((rc = fh_upload_ritz_lambda(h, g.ritz_lambda, m, ld, &dlam))) return rc;
    // sum mode: only Q_proj is wanted (no moments), so the per-node solutions are never formed
    if (h->solver == FEASTHIP_SOLVER_COCG && !want_moments && h->sum_mode) {
        if ((rc = fh_buf(h, "ca_acc", panel, &g.sum_acc))) return rc;
        FH_CHECK(hipMemsetAsync(g.sum_acc, 0, panel * sizeof(cplx), h->stream));
    }
    g.sum_shared = g.sum_acc && h->factor_precision == 64 && !fh_knob::no_shared_start();
    if (g.sum_shared) {
        if ((rc = fh_shared_start_source(h, g, &opt.shared_src))) return rc;
    } else if (nk) {
        fh_vec_args va;
        memset(&va, 0, sizeof(va));
        va.N = g.N; va.node_stride = panel; va.X = g.Y; va.Q = g.Qp; va.lambda = dlam; va.znode = dz;
        fh_launch_init_guess(va, ld, fh_vec_nblk(g.N, ld), nk, h->stream);
    }
    // Shifted COCG (feasthip_set_solver kind SHIFTED_COCG): a CSR operator with real values and B = I, fp64 panels, sum mode
    // from a shared start, no direct nodes.  Anything else is the per-node sweep.
    const bool shifted = h->shifted && g.sum_shared && opt.shared_src && nk && !nd && h->kind == FH_KIND_CSR && h->csr.b_identity &&
                         !h->csr.is_complex;
    h->shift_panels += 1;
    // Block COCG (kind BLOCK_COCG): a CSR operator with real values (any real symmetric B), fp64 panels, sum mode from a
    // shared start, no direct nodes.  Anything else is the per-node sweep.
    const bool block = h->block && g.sum_shared && opt.shared_src && nk && !nd && h->kind == FH_KIND_CSR && !h->csr.is_complex;
    h->block_panels += 1;
    if (block) {
        int smax = 0, brk = 0, ran = 0;
        if ((rc = fh_block_cocg(h, ld, m, nk, zk, sr, g.sum_acc, wk, opt.shared_src, g.ritz_lambda, dlam, dz, g.Y, &smax, &brk, &ran))) return rc;
        h->block_used += 1; h->block_steps_max = std::max(h->block_steps_max, smax); h->block_breakdowns += brk; h->block_passes += ran;
    } else if (shifted) {
        int seed = 0, seed_its = 0;
        if ((rc = fh_shifted_cocg(h, ld, m, nk, zk, sr, g.sum_acc, wk, opt.shared_src, g.ritz_lambda, &seed, &seed_its))) return rc;
        h->shift_used += 1; h->shift_seed = h->node_ids[g.order[seed]]; h->shift_seed_iters += seed_its;
    } else if (nk) {
        opt.sum_acc = g.sum_acc; opt.wnode = &wk; opt.shared_lambda = dlam; opt.dznode = dz; opt.shared_lambda_host = g.ritz_lambda;
        rc = fh_krylov(h, h->solver == FEASTHIP_SOLVER_COCG ? 1 : 0, h->factor_precision, ld, m, nk, zk, g.Rhs, g.Y, panel, sr, opt);
        if (rc) return rc;
    }
    if (!nd) return 0;
    // back to local node order; a direct node reports 0 iterations
    std::vector<int> status(nodes, 0), node_iters(nodes, 0), col_iters((size_t)nodes * m, 0);
    for (int i = 0; i < nk; ++i) {
        const int e = g.order[i];
        status[e] = sr.status[i];
        node_iters[e] = sr.node_iters[i];
        std::copy_n(sr.col_iters.begin() + (size_t)i * m, m, col_iters.begin() + (size_t)e * m);
    }
    for (int d = 0; d < nd; ++d) status[g.order[nk + d]] = status_d[d];
    sr.status = status; sr.node_iters = node_iters; sr.col_iters = col_iters;
    return 0;
}

// GMRES: zero initial guess like Krylov.jl (or the Ritz warm start when given), then the restarted cycles over every node
static int fh_panel_gmres(feasthip_ctx* h, const fh_panel_sweep& g, int64_t* nfact, fh_solve_result& sr) {
    int rc;
    cplx* dz; double* dlam;
    if ((rc = fh_upload_coefs(h, "ca_z", g.z, &dz))) return rc;
    if ((rc = fh_upload_ritz_lambda(h, g.ritz_lambda, g.m, g.ld, &dlam))) return rc;
    fh_vec_args va;
    memset(&va, 0, sizeof(va));
    va.N = g.N; va.node_stride = g.panel; va.X = g.Y; va.Q = g.Qp; va.lambda = dlam; va.znode = dz; va.prec = 64;
    fh_launch_init_guess(va, g.ld, fh_vec_nblk(g.N, g.ld), g.nodes, h->stream);
    if (h->pc_pivots.empty()) return fh_gmres(h, g.ld, g.m, g.nodes, g.z, g.Rhs, g.Y, g.panel, sr);
    std::vector<int> pivot(g.nodes);
    for (int i = 0; i < g.nodes; ++i) pivot[i] = h->pc_node_pivot[h->node_ids[g.order[i]]];
    return fh_gmres_preconditioned(h, g.ld, g.m, g.z, pivot, g.ritz_lambda == nullptr, g.Rhs, g.Y, g.panel, nfact, sr);
}

// What an iterative sweep leaves in the handle (feasthip_last_node_iterations / _column_iterations) and in the stats
static void fh_store_sweep_result(feasthip_ctx* h, const fh_solve_result& sr, int m, feasthip_stats* stats) {
    h->last_node_iters = sr.node_iters; h->last_col_iters = sr.col_iters; h->last_col_m = m;
    if (stats) { stats->krylov_iterations = sr.iters_sum; stats->spmm_calls = sr.op_calls; stats->max_rel_residual = sr.max_rel_res; }
}

// Moments (variant B): zAq += w_e Q^H Y_e ; zSq += w_e z_e Q^H Y_e, one Gram product per node (and per row block of a wide
// sweep, whose block columns go to mom's host accumulators); the sums of a one-panel sweep are uploaded to dzAq / dzSq.
static int fh_panel_moments(feasthip_ctx* h, const fh_panel_sweep& g, cplx* dzAq, cplx* dzSq, const fh_moment_ctx* mom) {
    const int m = g.m, ld = g.ld, N = g.N;
    int rc;
    cplx *gw, *G;
    if ((rc = fh_buf(h, "gram_work", fh_gram_work_elems(ld), &gw))) return rc;
    if ((rc = fh_buf(h, "gram_G", (size_t)ld * ld, &G))) return rc;
    const int m_all = mom ? mom->m_all : m, col0 = mom ? mom->col0 : 0;
    std::vector<cplx> Gh((size_t)ld * ld), aq_local, sq_local;
    if (!mom) { aq_local.assign((size_t)m * m, cmake(0, 0)); sq_local.assign((size_t)m * m, cmake(0, 0)); }
    std::vector<cplx>& aq = mom ? *mom->aq : aq_local;
    std::vector<cplx>& sq = mom ? *mom->sq : sq_local;
    cplx* Qrow = g.Qp;                     // row block of Q in panel layout (the panel's own columns when not wide)
    if (mom && (rc = fh_buf(h, "ca_Qrow", g.panel, &Qrow))) return rc;
    for (int r0 = 0; r0 < m_all; r0 += ld) {
        const int mr_ = std::min(ld, m_all - r0);
        if (mom) fh_launch_to_panel(mom->dQ_all + (size_t)r0 * N, N, N, mr_, Qrow, ld, h->stream, fh_perm(h));
        for (int e = 0; e < g.nodes; ++e) {
            fh_prof_begin(h, "gram");
            fh_launch_gram(Qrow, g.Y + (size_t)e * g.panel, N, ld, 0, gw, G, h->stream);
            fh_prof_end(h);
            FH_CHECK(hipMemcpyAsync(Gh.data(), G, Gh.size() * sizeof(cplx), hipMemcpyDeviceToHost, h->stream));
            FH_CHECK(hipStreamSynchronize(h->stream));
            cplx wz = cmul(g.w[e], g.z[e]);
            for (int c2 = 0; c2 < m; ++c2)
                for (int c1 = 0; c1 < mr_; ++c1) {
                    cplx gv = Gh[(size_t)c2 * ld + c1];
                    cfma(aq[(size_t)(col0 + c2) * m_all + r0 + c1], g.w[e], gv);
                    cfma(sq[(size_t)(col0 + c2) * m_all + r0 + c1], wz, gv);
                }
        }
        if (!mom) break;
    }
    if (!mom) {
        if (h->real_projection) for (size_t i = 0; i < aq.size(); ++i) { aq[i].y = 0.0; sq[i].y = 0.0; }
        if (dzAq) FH_CHECK(hipMemcpyAsync(dzAq, aq.data(), aq.size() * sizeof(cplx), hipMemcpyHostToDevice, h->stream));
        if (dzSq) FH_CHECK(hipMemcpyAsync(dzSq, sq.data(), sq.size() * sizeof(cplx), hipMemcpyHostToDevice, h->stream));
    }
    return 0;
}

// One panel (m <= 64) of the sweep, in phases: import Q, rhs = B Q, split the nodes, solve, sum the weighted solutions
// into Q_proj, moments, one synchronisation.
static int fh_contour_apply_panel(feasthip_ctx* h, int64_t m64, const cplx* dQ, const double* ritz_lambda,
                                  cplx* dQproj, cplx* dzAq, cplx* dzSq, int* node_status, feasthip_stats* stats,
                                  const fh_moment_ctx* mom = nullptr, const fh_panel_io* io = nullptr) {
    int rc = fh_check_problem(h, m64);
    if (rc) return rc;
    if ((rc = fh_check_operator_solve(h, "contour_apply"))) return rc;
    if (h->zne.empty()) { h->last_error = "no contour set"; return FEASTHIP_ERROR_FPM; }
    auto t0 = std::chrono::steady_clock::now();
    FH_CHECK(hipSetDevice(h->device));
    fh_panel_sweep g;
    const int m = g.m = (int)m64, ld = g.ld = fh_pick_ld(m), N = g.N = (int)fh_N(h);
    const int nodes = g.nodes = h->node_count;
    const size_t panel = g.panel = (size_t)N * ld;
    g.ritz_lambda = ritz_lambda; g.io = io;
    if (io && io->Qp) {
        g.Qp = const_cast<cplx*>(io->Qp);        // read only below (the right-hand side when B = I)
    } else {
        if ((rc = fh_buf(h, "ca_Qp", panel, &g.Qp))) return rc;
        fh_launch_to_panel(dQ, N, N, m, g.Qp, ld, h->stream, fh_perm(h));
    }
    cplx* Outp = io ? io->out : nullptr;
    if (!Outp) {
        if ((rc = fh_buf(h, "ca_out", panel, &Outp))) return rc;
    }
    if (stats) memset(stats, 0, sizeof(*stats));
    if (nodes == 0) {
        if (io && io->out) FH_CHECK(hipMemsetAsync(io->out, 0, panel * sizeof(cplx), h->stream));
        if (dQproj) FH_CHECK(hipMemsetAsync(dQproj, 0, (size_t)N * m * sizeof(cplx), h->stream));
        if (dzAq) FH_CHECK(hipMemsetAsync(dzAq, 0, (size_t)m * m * sizeof(cplx), h->stream));
        if (dzSq) FH_CHECK(hipMemsetAsync(dzSq, 0, (size_t)m * m * sizeof(cplx), h->stream));
        FH_CHECK(hipStreamSynchronize(h->stream));
        return 0;
    }
    // rhs = B Q  (hoisted out of the node loop; the reference recomputes it per node,
    // src/dense/feast_dense.jl:184 -- it is loop invariant); B^H Q under the adjoint switch (fh_apply_operator)
    g.Rhs = g.Qp;
    if (!fh_b_identity(h)) {
        if ((rc = fh_buf(h, "ca_rhs", panel, &g.Rhs))) return rc;
        std::vector<cplx> ca(ld, cmake(0, 0)), cb(ld, cmake(1, 0));
        cplx *dca, *dcb;
        if ((rc = fh_upload_coefs(h, "ca_coefA", ca, &dca))) return rc;
        if ((rc = fh_upload_coefs(h, "ca_coefB", cb, &dcb))) return rc;
        fh_op_call oc;
        oc.m = m;
        oc.X = g.Qp; oc.Y = g.Rhs; oc.coefA = dca; oc.coefB = dcb; oc.skip = 1;
        if (fh_apply_operator(h, ld, oc) < 0) return FEASTHIP_ERROR_INTERNAL;
    }
    // Per-node solver (feasthip_set_node_solver): the local nodes split into a Krylov set and a direct set; with no direct
    // node the order is the identity and nothing below differs from the one-solver sweep.
    if ((rc = fh_split_nodes(h, g.order, &g.nd))) return rc;
    const int nd = g.nd, nk = g.nk = nodes - nd;
    std::vector<cplx>& z = g.z;
    std::vector<cplx>& w = g.w;
    z.resize(nodes); w.resize(nodes);
    for (int i = 0; i < nodes; ++i) {
        z[i] = h->zne[h->node_ids[g.order[i]]];
        w[i] = cscale(h->wne[h->node_ids[g.order[i]]], h->weight_scale);
        if (h->adjoint) w[i].y = -w[i].y;         // adjoint sweep: Q_proj = sum_e conj(w_e) S_e^-H B^H Q
    }
    if ((rc = fh_buf(h, "ca_Y", (size_t)nodes * panel, &g.Y))) return rc;
    cplx* Y = g.Y;

    // destroyed on every return path (the solver branches below return early on errors)
    struct ev_guard { hipEvent_t a = nullptr, b = nullptr; ~ev_guard() { if (a) hipEventDestroy(a); if (b) hipEventDestroy(b); } } evg;
    FH_CHECK(hipEventCreate(&evg.a)); FH_CHECK(hipEventCreate(&evg.b));
    const hipEvent_t ev0 = evg.a, ev1 = evg.b;
    FH_CHECK(hipEventRecord(ev0, h->stream));
    // solve: Y_e = (z_e B - A)^-1 rhs for every local node (sum mode: their weighted sum only, in g.sum_acc)
    const bool direct = h->solver == FEASTHIP_SOLVER_LU || h->solver == FEASTHIP_SOLVER_BANDED;
    int64_t nfact = 0;
    fh_solve_result sr;
    if (direct) rc = fh_panel_direct(h, g, &nfact, sr);
    else if (h->solver == FEASTHIP_SOLVER_BICGSTAB || h->solver == FEASTHIP_SOLVER_COCG) rc = fh_panel_krylov(h, g, dzAq || dzSq || mom, &nfact, sr);
    else rc = fh_panel_gmres(h, g, &nfact, sr);
    if (rc) return rc;
    if (!direct) fh_store_sweep_result(h, sr, m, stats);
    else if (stats) stats->max_rel_residual = sr.max_rel_res;
    if (stats) stats->factorizations = nfact;
    FH_CHECK(hipEventRecord(ev1, h->stream));

    // Q_proj = sum_e (scale*w_e) Y_e
    cplx* dw;
    if ((rc = fh_upload_coefs(h, "ca_w", w, &dw))) return rc;
    cplx* dwd = nullptr;
    if (g.sum_shared && nd) {
        const std::vector<cplx> wd(w.begin() + nk, w.end());
        if ((rc = fh_upload_coefs(h, "ca_wd", wd, &dwd))) return rc;
    }
    fh_prof_begin(h, dwd ? "node_finish" : "accumulate");
    if (g.sum_shared) {
        cplx* drho = nullptr;
        if (ritz_lambda) {
            // the closed-form sum of the warm starts runs over the Krylov nodes only
            std::vector<cplx> rho(ld, cmake(0, 0));
            for (int c = 0; c < m; ++c)
                for (int e = 0; e < nk; ++e) rho[c] = cadd(rho[c], cdiv(w[e], cmake(z[e].x - ritz_lambda[c], z[e].y)));
            if ((rc = fh_upload_coefs(h, "ca_rho", rho, &drho))) return rc;
        }
        if (dwd) fh_launch_node_finish(g.Qp, drho, g.sum_acc, Y + (size_t)nk * panel, panel, dwd, nd, Outp, N, ld, h->real_projection, h->stream);
        else fh_launch_sum_finish(g.Qp, drho, g.sum_acc, Outp, N, ld, h->real_projection, h->stream);
    } else {
        fh_launch_accumulate(Y, panel, dw, nodes, N, ld, g.sum_acc, Outp, h->real_projection, h->stream);
    }
    fh_prof_end(h);
    if (dQproj) fh_launch_from_panel(Outp, ld, N, m, dQproj, N, h->stream, fh_perm(h));
    if ((dzAq || dzSq || mom) && (rc = fh_panel_moments(h, g, dzAq, dzSq, mom))) return rc;
    FH_CHECK(hipStreamSynchronize(h->stream));
    if (node_status) for (int e = 0; e < nodes; ++e) node_status[e] = sr.status[e];
    if (stats) {
        float ms = 0.f;
        hipEventElapsedTime(&ms, ev0, ev1);
        stats->seconds_solve = ms * 1e-3;
        stats->seconds_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    fh_prof_collect(h);
    FH_CHECK(hipGetLastError());       // launch-configuration errors do not surface through the stream sync
    return 0;
}

// While it lives, the handle's column mask is its slice [c0, c1) (columns past the mask's end count as set); the
// destructor puts the whole mask back, on every return path.
struct fh_mask_slice {
    feasthip_ctx* h;
    const std::vector<int> whole;
    fh_mask_slice(feasthip_ctx* h_, int64_t c0, int64_t c1) : h(h_), whole(h_->col_mask) {
        if (whole.empty()) return;
        h->col_mask.clear();
        for (int64_t c = c0; c < c1; ++c) h->col_mask.push_back(c < (int64_t)whole.size() ? whole[c] : 1);
    }
    ~fh_mask_slice() { h->col_mask = whole; }
};

// m > 64: the columns of Q are independent right-hand sides, so the sweep runs panel by panel
// (64 columns each); LU factors are shared by the panels through the per-node cache.
static int fh_contour_apply_local(feasthip_ctx* h, int64_t m64, const cplx* dQ, const double* ritz_lambda,
                                  cplx* dQproj, cplx* dzAq, cplx* dzSq, int* node_status, feasthip_stats* stats) {
    if (m64 <= FH_MAX_LD) return fh_contour_apply_panel(h, m64, dQ, ritz_lambda, dQproj, dzAq, dzSq, node_status, stats);
    int rc = fh_check_problem(h, m64, 1);
    if (rc) return rc;
    const int m = (int)m64, N = (int)fh_N(h), nodes = h->node_count;
    // moment matrices of a wide sweep: block columns gathered on the host, uploaded after the last panel
    std::vector<cplx> aq_all, sq_all;
    fh_moment_ctx mom;
    const bool want_mom = dzAq || dzSq;
    if (want_mom) {
        aq_all.assign((size_t)m * m, cmake(0, 0)); sq_all.assign((size_t)m * m, cmake(0, 0));
        mom.dQ_all = dQ; mom.m_all = m; mom.aq = &aq_all; mom.sq = &sq_all;
    }
    if (stats) memset(stats, 0, sizeof(*stats));
    std::vector<int> ns(std::max(nodes, 1), 0), node_it(nodes, 0), col_it((size_t)nodes * m, 0);
    if (node_status) for (int e = 0; e < nodes; ++e) node_status[e] = 0;
    for (int c0 = 0; c0 < m; c0 += FH_MAX_LD) {
        const int mc = std::min(FH_MAX_LD, m - c0);
        feasthip_stats st;
        h->last_node_iters.clear(); h->last_col_iters.clear();
        mom.col0 = c0;
        {
            fh_mask_slice slice(h, c0, c0 + mc);
            rc = fh_contour_apply_panel(h, mc, dQ + (size_t)c0 * N, ritz_lambda ? ritz_lambda + c0 : nullptr,
                                        dQproj + (size_t)c0 * N, nullptr, nullptr, ns.data(), &st, want_mom ? &mom : nullptr);
        }
        if (rc) return rc;
        for (int e = 0; e < nodes; ++e) {
            if (node_status) node_status[e] = std::max(node_status[e], ns[e]);
            if (e < (int)h->last_node_iters.size()) node_it[e] = std::max(node_it[e], h->last_node_iters[e]);
            for (int c = 0; c < mc; ++c)
                if ((size_t)e * mc + c < h->last_col_iters.size()) col_it[(size_t)e * m + c0 + c] = h->last_col_iters[(size_t)e * mc + c];
        }
        if (stats) {
            stats->seconds_total += st.seconds_total; stats->seconds_solve += st.seconds_solve;
            stats->krylov_iterations += st.krylov_iterations; stats->spmm_calls += st.spmm_calls;
            stats->factorizations += st.factorizations;
            stats->max_rel_residual = std::max(stats->max_rel_residual, st.max_rel_residual);
        }
    }
    h->last_node_iters = node_it; h->last_col_iters = col_it; h->last_col_m = m;
    if (want_mom) {
        if (h->real_projection) for (size_t i = 0; i < aq_all.size(); ++i) { aq_all[i].y = 0.0; sq_all[i].y = 0.0; }
        if (dzAq) FH_CHECK(hipMemcpy(dzAq, aq_all.data(), aq_all.size() * sizeof(cplx), hipMemcpyHostToDevice));
        if (dzSq) FH_CHECK(hipMemcpy(dzSq, sq_all.data(), sq_all.size() * sizeof(cplx), hipMemcpyHostToDevice));
    }
    return 0;
}

// The sweep as the caller sees it: this rank's nodes x this rank's column block (feasthip_set_column_block),
// then -- when a communicator is attached -- ONE packed all-reduce
//     [ Q_proj (N*m reals for a real-projection sweep, else 2*N*m) | zAq | zSq | per-node failure flags ]
// on the handle's stream: the image of MPI.Allreduce in src/parallel/feast_mpi.jl:117-119, 856-858 and of the
// master sum src/parallel/feast_parallel.jl:497-503.  With a communicator node_status is GLOBAL (ne entries,
// indexed by contour node), without one it is per local node as before.
// Resident form (rs != null; m <= 64, no moments): the subspace comes in as the panel rs->Q (with, optionally, its
// eigen-residual panel rs->eigres), the summed Q_proj is left in the panel rs->P (N x rs->ld); column blocks are cut out of
// / packed into the panels by fh_launch_panel_cols / fh_launch_pack_cols, and the reduce carries N x ld values.
struct fh_resident_sweep {
    const cplx* Q; const cplx* eigres; cplx* P; int ld;
};

// While a sweep runs, the handle's column mask (feasthip_set_column_mask) is live.  The mask is one-shot: it applies to this
// sweep only and never leaks into later calls (shifted_solve / RCI jobs on the same handle), whatever the outcome of the sweep.
struct fh_mask_live {
    feasthip_ctx* h;
    explicit fh_mask_live(feasthip_ctx* h_) : h(h_) { h->mask_live = 1; }
    ~fh_mask_live() { h->mask_live = 0; h->col_mask.clear(); }
};

static int fh_contour_apply_impl(feasthip_ctx* h, int64_t m64, const cplx* dQ, const double* ritz_lambda,
                                 cplx* dQproj, cplx* dzAq, cplx* dzSq, int* node_status, feasthip_stats* stats,
                                 const fh_resident_sweep* rs = nullptr) {
    fh_mask_live live(h);
    h->shift_panels = h->shift_used = h->shift_seed_iters = 0; h->shift_seed = -1;      // feasthip_last_shifted_sweep
    h->block_panels = h->block_used = h->block_steps_max = h->block_breakdowns = h->block_passes = 0;   // feasthip_last_block_sweep
    h->pc_last = {};                                                                                    // feasthip_last_precond_sweep
    if (int prc = fh_check_precond(h, "contour_apply")) return prc;
    const int nr = fh_comm_nranks(h);
    int64_t c0 = 0, c1 = m64;
    if (h->col_block_hi >= 0) { c0 = std::min(h->col_block_lo, m64); c1 = std::min(std::max(h->col_block_hi, c0), m64); }
    const bool full = (c0 == 0 && c1 == m64);
    if (nr == 1 && full) {
        if (rs) {
            fh_panel_io io; io.Qp = rs->Q; io.eigres = rs->eigres; io.out = rs->P;
            return fh_contour_apply_panel(h, m64, nullptr, ritz_lambda, nullptr, nullptr, nullptr, node_status, stats, nullptr, &io);
        }
        return fh_contour_apply_local(h, m64, dQ, ritz_lambda, dQproj, dzAq, dzSq, node_status, stats);
    }
    // The shape of the packed reduce depends only on what every rank was called with (N, m, ne, the moment pointers, the
    // projection mode).  An argument error is therefore the same on every rank and may return at once; anything that
    // can fail on ONE rank only (allocations, the sweep, copies) is recorded in local_rc and the rank still joins the
    // reduce with a zeroed payload and its failure flag set -- its peers are waiting in the collective, and RCCL has no
    // timeout.
    int rc = fh_check_problem(h, m64, rs ? 0 : 1);
    if (rc) return rc;
    if (!full && (dzAq || dzSq)) { h->last_error = "contour_apply: moment matrices need the full column block"; return FEASTHIP_ERROR_M0; }
    const int N = (int)fh_N(h), m = (int)m64, nodes = h->node_count, ne = (int)h->zne.size();
    std::vector<int> ns(std::max(nodes, 1), 0);
    if (stats) memset(stats, 0, sizeof(*stats));
    int local_rc = 0;
    auto soft = [&](hipError_t e, const char* what) {
        if (e != hipSuccess && !local_rc) {
            h->last_error = std::string(what) + ": " + hipGetErrorString(e);
            local_rc = (e == hipErrorOutOfMemory) ? FEASTHIP_ERROR_MEMORY : FEASTHIP_ERROR_INTERNAL;
        }
    };
    soft(hipSetDevice(h->device), "hipSetDevice");
    // the reduce buffer comes first: without it this rank cannot join the collective at all
    const size_t nq = (size_t)N * (rs ? rs->ld : m) * (h->real_projection ? 1 : 2);
    const size_t nm = (size_t)m * m * 2;
    const size_t total = nq + (dzAq ? nm : 0) + (dzSq ? nm : 0) + 3 * (size_t)ne + 1;
    double* pack = nullptr;
    if (nr > 1) {
        if ((rc = fh_buf(h, "comm_pack", total, &pack))) {
            // nothing to reduce into: tell the peers through the transport's own failure path where there is one
            // (shm: the failed flag releases their barriers), then give up -- the caller must treat this as fatal
            fh_comm_mark_failed(h);
            return rc;
        }
    }
    if (!local_rc && !full && !rs) soft(hipMemsetAsync(dQproj, 0, (size_t)N * m * sizeof(cplx), h->stream), "hipMemsetAsync(Q_proj)");
    cplx* rs_out = nullptr;                       // resident form: this rank's block of Q_proj, an N x rs_ldw panel
    int rs_ldw = 0;
    if (!local_rc && c1 <= c0) {
        soft(hipStreamSynchronize(h->stream), "hipStreamSynchronize");
    } else if (!local_rc && rs) {
        const int w = (int)(c1 - c0);
        rs_ldw = fh_pick_ld(w);
        fh_panel_io io;
        cplx* sub = nullptr;
        int brc = fh_buf(h, "rs_Osub", (size_t)N * rs_ldw, &rs_out);
        if (!brc && full) { io.Qp = rs->Q; io.eigres = rs->eigres; }
        if (!brc && !full) {
            // this rank's columns of the subspace (and of its eigen-residual) as panels of their own
            if (!(brc = fh_buf(h, "rs_Qsub", (size_t)N * rs_ldw, &sub))) {
                fh_launch_panel_cols(rs->Q, rs->ld, (int)c0, w, N, sub, rs_ldw, h->stream);
                io.Qp = sub;
            }
            if (!brc && rs->eigres && !(brc = fh_buf(h, "rs_Esub", (size_t)N * rs_ldw, &sub))) {
                fh_launch_panel_cols(rs->eigres, rs->ld, (int)c0, w, N, sub, rs_ldw, h->stream);
                io.eigres = sub;
            }
        }
        if (brc) local_rc = brc;
        else {
            io.out = rs_out;
            fh_mask_slice slice(h, c0, c1);
            local_rc = fh_contour_apply_panel(h, w, nullptr, ritz_lambda ? ritz_lambda + c0 : nullptr, nullptr, nullptr, nullptr,
                                              ns.data(), stats, nullptr, &io);
        }
    } else if (!local_rc) {
        fh_mask_slice slice(h, c0, c1);
        local_rc = fh_contour_apply_local(h, c1 - c0, dQ + (size_t)c0 * N, ritz_lambda ? ritz_lambda + c0 : nullptr,
                                          dQproj + (size_t)c0 * N, dzAq, dzSq, ns.data(), stats);
    }
    if (nr == 1) {
        if (local_rc) return local_rc;
        if (rs) {                                 // one rank, a column block: the other columns of Q_proj are zero
            FH_CHECK(hipMemsetAsync(rs->P, 0, (size_t)N * rs->ld * sizeof(cplx), h->stream));
            if (rs_out) {
                if ((rc = fh_buf(h, "comm_pack", nq, &pack))) return rc;
                fh_launch_pack_cols(rs_out, rs_ldw, (int)c0, (int)(c1 - c0), N, pack, rs->ld, h->real_projection, h->stream);
                if (h->real_projection) fh_launch_unpack_real(pack, rs->P, nq, h->stream);
                else FH_CHECK(hipMemcpyAsync(rs->P, pack, nq * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
            }
            FH_CHECK(hipStreamSynchronize(h->stream));
        }
        if (node_status) for (int e = 0; e < nodes; ++e) node_status[e] = ns[e];
        return 0;
    }
    size_t off = nq;
    if (!local_rc) {
        if (rs && rs_out) fh_launch_pack_cols(rs_out, rs_ldw, (int)c0, (int)(c1 - c0), N, pack, rs->ld, h->real_projection, h->stream);
        else if (rs) soft(hipMemsetAsync(pack, 0, nq * sizeof(double), h->stream), "pack Q_proj (no columns)");
        else if (h->real_projection) fh_launch_pack_real(dQproj, pack, nq, h->stream);
        else soft(hipMemcpyAsync(pack, dQproj, nq * sizeof(double), hipMemcpyDeviceToDevice, h->stream), "pack Q_proj");
        if (dzAq) { soft(hipMemcpyAsync(pack + off, dzAq, nm * sizeof(double), hipMemcpyDeviceToDevice, h->stream), "pack zAq"); off += nm; }
        if (dzSq) { soft(hipMemcpyAsync(pack + off, dzSq, nm * sizeof(double), hipMemcpyDeviceToDevice, h->stream), "pack zSq"); off += nm; }
    } else {
        off += (dzAq ? nm : 0) + (dzSq ? nm : 0);
    }
    // tail of the packed buffer: [no-convergence flags | singular flags | Krylov iterations per contour node | rank failed]
    std::vector<double> flags(3 * (size_t)ne + 1, 0.0);
    for (int e = 0; e < nodes && !local_rc; ++e) {
        const int g = h->node_ids[e];
        if (ns[e] == FEASTHIP_ERROR_LAPACK) flags[ne + g] = 1.0;
        else if (ns[e] != 0) flags[g] = 1.0;
        if (c1 > c0 && e < (int)h->last_node_iters.size()) flags[2 * (size_t)ne + g] = (double)h->last_node_iters[e];
    }
    hipError_t e_flags = hipSuccess;
    if (local_rc) {
        // our own payload may be garbage: contribute zeros so that the peers' sums stay finite
        e_flags = hipMemsetAsync(pack, 0, off * sizeof(double), h->stream);
    }
    flags[3 * (size_t)ne] = local_rc ? 1.0 : 0.0;
    if (e_flags == hipSuccess) e_flags = hipMemcpyAsync(pack + off, flags.data(), flags.size() * sizeof(double), hipMemcpyHostToDevice, h->stream);
    if (e_flags != hipSuccess) {
        // the stream itself refuses work: the flag cannot be shipped.  Still enter the collective (whatever the buffer
        // holds) so that the peers return; this rank reports the error
        soft(e_flags, "pack flags");
    }
    fh_prof_begin(h, "allreduce");
    rc = fh_comm_allreduce_sum(h, pack, total);
    fh_prof_end(h);
    if (rc) return local_rc ? local_rc : rc;
    if (local_rc) {
        hipStreamSynchronize(h->stream);          // best effort: leave no work of ours queued behind the error
        return local_rc;
    }
    cplx* const qdst = rs ? rs->P : dQproj;
    if (h->real_projection) fh_launch_unpack_real(pack, qdst, nq, h->stream);
    else FH_CHECK(hipMemcpyAsync(qdst, pack, nq * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    off = nq;
    if (dzAq) { FH_CHECK(hipMemcpyAsync(dzAq, pack + off, nm * sizeof(double), hipMemcpyDeviceToDevice, h->stream)); off += nm; }
    if (dzSq) { FH_CHECK(hipMemcpyAsync(dzSq, pack + off, nm * sizeof(double), hipMemcpyDeviceToDevice, h->stream)); off += nm; }
    FH_CHECK(hipMemcpyAsync(flags.data(), pack + off, flags.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    FH_CHECK(hipStreamSynchronize(h->stream));
    if (node_status)
        for (int g = 0; g < ne; ++g)
            node_status[g] = flags[ne + g] > 0.0 ? (int)FEASTHIP_ERROR_LAPACK : (flags[g] > 0.0 ? (int)FEASTHIP_ERROR_NO_CONVERGENCE : 0);
    h->global_node_iters.assign(ne, 0);
    for (int g = 0; g < ne; ++g) h->global_node_iters[g] = (int)(flags[2 * (size_t)ne + g] + 0.5);
    if (flags[3 * (size_t)ne] > 0.0) { h->last_error = "contour_apply: the sweep failed on another rank"; return FEASTHIP_ERROR_INTERNAL; }
    return 0;
}

extern "C" int feasthip_set_column_block(feasthip_handle h, int64_t first, int64_t count) {
    if (!h) return FEASTHIP_ERROR_INTERNAL;
    if (count < 0) { h->col_block_lo = 0; h->col_block_hi = -1; return 0; }
    if (first < 0) { h->last_error = "set_column_block: first must be >= 0"; return FEASTHIP_ERROR_M0; }
    h->col_block_lo = first; h->col_block_hi = first + count;
    return 0;
}

extern "C" int feasthip_contour_apply_dev(feasthip_handle h, int64_t m, const void* dQ, const double* ritz_lambda_host,
                                          void* dQproj, void* dzAq, void* dzSq, int* node_status, feasthip_stats* stats) {
    if (!h) return FEASTHIP_ERROR_INTERNAL;
    if (!dQ || !dQproj) { h->last_error = "contour_apply: null Q/Qproj"; return FEASTHIP_ERROR_INTERNAL; }
    if (int arc = fh_check_adjoint(h, "contour_apply", (dzAq || dzSq) ? "the moment matrices zAq / zSq must be NULL" : nullptr)) return arc;
    return fh_contour_apply_impl(h, m, (const cplx*)dQ, ritz_lambda_host, (cplx*)dQproj, (cplx*)dzAq, (cplx*)dzSq, node_status, stats);
}

// host-pointer wrapper helpers
int fh_stage_in(feasthip_ctx* h, const char* name, const void* host, size_t bytes, void** dev) {
    int rc = fh_get_buf(h, name, bytes, dev);
    if (rc) return rc;
    FH_CHECK(hipMemcpyAsync(*dev, host, bytes, hipMemcpyHostToDevice, h->stream));
    return 0;
}

extern "C" int feasthip_contour_apply(feasthip_handle h, int64_t m, const void* Q, const double* ritz_lambda,
                                      void* Qproj, void* zAq, void* zSq, int* node_status, feasthip_stats* stats) {
    int rc = fh_check_problem(h, m, 1);
    if (rc) return rc;
    if (!Q || !Qproj) { h->last_error = "contour_apply: null Q/Qproj"; return FEASTHIP_ERROR_INTERNAL; }
    if ((rc = fh_check_adjoint(h, "contour_apply", (zAq || zSq) ? "the moment matrices zAq / zSq must be NULL" : nullptr))) return rc;
    FH_CHECK(hipSetDevice(h->device));
    const size_t nb = (size_t)fh_N(h) * m * sizeof(cplx), mb = (size_t)m * m * sizeof(cplx);
    void *dQ, *dP, *dA = nullptr, *dS = nullptr;
    if ((rc = fh_stage_in(h, "host_Q", Q, nb, &dQ))) return rc;
    if ((rc = fh_get_buf(h, "host_Qproj", nb, &dP))) return rc;
    if (zAq && (rc = fh_get_buf(h, "host_zAq", mb, &dA))) return rc;
    if (zSq && (rc = fh_get_buf(h, "host_zSq", mb, &dS))) return rc;
    if ((rc = fh_contour_apply_impl(h, m, (const cplx*)dQ, ritz_lambda, (cplx*)dP, (cplx*)dA, (cplx*)dS, node_status, stats))) return rc;
    FH_CHECK(hipMemcpy(Qproj, dP, nb, hipMemcpyDeviceToHost));
    if (zAq) FH_CHECK(hipMemcpy(zAq, dA, mb, hipMemcpyDeviceToHost));
    if (zSq) FH_CHECK(hipMemcpy(zSq, dS, mb, hipMemcpyDeviceToHost));
    return 0;
}

// ---------------------------------------------------------------------------------------
// stochastic eigenvalue-count estimate (fpm[14] = 2): kernels in fh_estimate.hip
// ---------------------------------------------------------------------------------------
static int fh_check_estimate(feasthip_ctx* h, int64_t m) {
    int rc = fh_check_problem(h, m, 1);
    if (rc) return rc;
    if (m > 65535) { h->last_error = "estimate: at most 65535 columns"; return FEASTHIP_ERROR_M0; }
    return 0;
}

extern "C" int feasthip_random_block_dev(feasthip_handle h, int64_t m, uint64_t seed, void* dX) {
    int rc = fh_check_estimate(h, m);
    if (rc) return rc;
    if (!dX) { h->last_error = "random_block: null X"; return FEASTHIP_ERROR_INTERNAL; }
    FH_CHECK(hipSetDevice(h->device));
    const int64_t N = fh_N(h);
    fh_launch_rademacher(seed, 0, N, m, (cplx*)dX, N, h->stream);
    FH_CHECK(hipGetLastError());
    FH_CHECK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int feasthip_estimate_count(feasthip_handle h, int64_t m, uint64_t seed, double* samples, int* node_status,
                                       feasthip_stats* stats) {
    int rc = fh_check_estimate(h, m);
    if (rc) return rc;
    if ((rc = fh_check_adjoint(h, "estimate_count", "the estimate has no adjoint form"))) return rc;
    if (!samples) { h->last_error = "estimate_count: null samples"; return FEASTHIP_ERROR_INTERNAL; }
    const double t0 = fh_now_s();
    FH_CHECK(hipSetDevice(h->device));
    const int64_t N = fh_N(h);
    cplx *dV, *dP, *dW;
    double* dT;
    if ((rc = fh_buf(h, "est_V", (size_t)N * m, &dV))) return rc;
    if ((rc = fh_buf(h, "est_P", (size_t)N * m, &dP))) return rc;
    if ((rc = fh_buf(h, "est_work", fh_trace_work_elems(N, m), &dW))) return rc;
    if ((rc = fh_buf(h, "est_t", (size_t)m * 2, &dT))) return rc;
    fh_launch_rademacher(seed, 0, N, m, dV, N, h->stream);
    FH_CHECK(hipGetLastError());
    // the sweep of feasthip_contour_apply_dev from a zero start: Q_proj = rho V, summed over the ranks of a communicator
    if ((rc = fh_contour_apply_impl(h, m, dV, nullptr, dP, nullptr, nullptr, node_status, stats))) return rc;
    fh_launch_trace_dots(dP, N, m, N, seed, h->real_projection, dW, dT, h->stream);
    FH_CHECK(hipGetLastError());
    FH_CHECK(hipMemcpyAsync(samples, dT, (size_t)m * 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    FH_CHECK(hipStreamSynchronize(h->stream));
    if (stats) stats->seconds_total = fh_now_s() - t0;
    return 0;
}

// The sweep of the resident refinement loop (fh_ritz.hip, "Resident refinement loop"): Q and Q_proj stay panels
extern "C" int feasthip_contour_apply_resident(feasthip_handle h, int64_t m64, const void* dQ, const double* ritz_lambda_host,
                                               int* node_status, feasthip_stats* stats) {
    int rc = fh_check_problem(h, m64);
    if (rc) return rc;
    if ((rc = fh_check_adjoint(h, "contour_apply_resident", "the resident loop has no adjoint form"))) return rc;
    if (h->zne.empty()) { h->last_error = "no contour set"; return FEASTHIP_ERROR_FPM; }
    FH_CHECK(hipSetDevice(h->device));
    const int m = (int)m64, ld = fh_pick_ld(m), N = (int)fh_N(h);
    cplx *P, *X, *R;
    if ((rc = fh_rs_panels(h, &P, &X, &R))) return rc;
    fh_resident_sweep rs;
    rs.P = P; rs.ld = ld; rs.eigres = nullptr;
    if (dQ) {
        cplx* Q0;
        if ((rc = fh_buf(h, "rs_Q0", (size_t)N * FH_MAX_LD, &Q0))) return rc;
        fh_launch_to_panel((const cplx*)dQ, N, N, m, Q0, ld, h->stream, fh_perm(h));
        rs.Q = Q0;
    } else {
        if (h->rs_X != X || h->rs_X_m != m || h->rs_X_ld != ld) {
            h->last_error = "contour_apply_resident: no resident Ritz vectors of this width (pass Q, or run rr_ritz_resident first)";
            return FEASTHIP_ERROR_M0;
        }
        rs.Q = X;
        if (ritz_lambda_host && h->rs_R == R && (int)h->rs_R_lambda.size() >= m) {
            bool same = true;
            for (int c = 0; c < m && same; ++c) same = h->rs_R_lambda[c].y == 0.0 && h->rs_R_lambda[c].x == ritz_lambda_host[c];
            if (same) rs.eigres = R;
        }
    }
    h->rs_P = nullptr; h->rs_basis = nullptr; h->rs_T.clear(); h->rs_rank = 0;
    if ((rc = fh_contour_apply_impl(h, m64, nullptr, ritz_lambda_host, nullptr, nullptr, nullptr, node_status, stats, &rs))) return rc;
    h->rs_P = P; h->rs_m = m; h->rs_ld = ld;
    return 0;
}

// ---------------------------------------------------------------------------------------
// RCI seams: Y = A X / B X (jobs 30/40), Y = (zB - A)^{-1} X (jobs 10+11, linear_solver)
// ---------------------------------------------------------------------------------------
extern "C" int feasthip_matmul_dev(feasthip_handle h, int which, int64_t m64, const void* dX, void* dY) {
    if (m64 > FH_MAX_LD) {          // independent columns: 64 at a time
        int rc0 = fh_check_problem(h, m64, 1);
        if (rc0) return rc0;
        const size_t N0 = (size_t)fh_N(h);
        for (int64_t c0 = 0; c0 < m64; c0 += FH_MAX_LD) {
            const int64_t mc = std::min<int64_t>(FH_MAX_LD, m64 - c0);
            rc0 = feasthip_matmul_dev(h, which, mc, (const cplx*)dX + c0 * N0, (cplx*)dY + c0 * N0);
            if (rc0) return rc0;
        }
        return 0;
    }

    int rc = fh_check_problem(h, m64);
    if (rc) return rc;
    if (!dX || !dY || (which != 0 && which != 1)) { h->last_error = "matmul: bad argument"; return FEASTHIP_ERROR_INTERNAL; }
    if ((rc = fh_check_adjoint(h, "matmul"))) return rc;
    FH_CHECK(hipSetDevice(h->device));
    const int m = (int)m64, ld = fh_pick_ld(m), N = (int)fh_N(h);
    const size_t panel = (size_t)N * ld;
    cplx *Xp, *Yp;
    if ((rc = fh_buf(h, "mm_X", panel, &Xp))) return rc;
    if ((rc = fh_buf(h, "mm_Y", panel, &Yp))) return rc;
    fh_launch_to_panel((const cplx*)dX, N, N, m, Xp, ld, h->stream, fh_perm(h));
    std::vector<cplx> ca(ld, cmake(which == 0 ? 1 : 0, 0)), cb(ld, cmake(which == 1 ? 1 : 0, 0));
    cplx *dca, *dcb;
    if ((rc = fh_upload_coefs(h, "mm_coefA", ca, &dca))) return rc;
    if ((rc = fh_upload_coefs(h, "mm_coefB", cb, &dcb))) return rc;
    fh_op_call oc;
    oc.m = m;
    oc.X = Xp; oc.Y = Yp; oc.coefA = dca; oc.coefB = dcb; oc.skip = which == 0 ? 2 : 1;
    if (fh_apply_operator(h, ld, oc) < 0) return FEASTHIP_ERROR_INTERNAL;
    fh_launch_from_panel(Yp, ld, N, m, (cplx*)dY, N, h->stream, fh_perm(h));
    return fh_finish(h);
}

extern "C" int feasthip_matmul(feasthip_handle h, int which, int64_t m, const void* X, void* Y) {
    int rc = fh_check_problem(h, m, 1);
    if (rc) return rc;
    if (!X || !Y) { h->last_error = "matmul: null argument"; return FEASTHIP_ERROR_INTERNAL; }
    if ((rc = fh_check_adjoint(h, "matmul"))) return rc;
    FH_CHECK(hipSetDevice(h->device));
    const size_t nb = (size_t)fh_N(h) * m * sizeof(cplx);
    void *dX, *dY;
    if ((rc = fh_stage_in(h, "host_Q", X, nb, &dX))) return rc;
    if ((rc = fh_get_buf(h, "host_X", nb, &dY))) return rc;
    rc = feasthip_matmul_dev(h, which, m, dX, dY);
    if (rc) return rc;
    FH_CHECK(hipMemcpy(Y, dY, nb, hipMemcpyDeviceToHost));
    return 0;
}

static int fh_shifted_solve_panel(feasthip_ctx* h, double z_re, double z_im, int64_t m64, const void* dX, void* dY, feasthip_stats* stats);

extern "C" int feasthip_shifted_solve_dev(feasthip_handle h, double z_re, double z_im, int64_t m64, const void* dX,
                                          void* dY, feasthip_stats* stats) {
    if (h) h->pc_last = {};         // feasthip_last_precond_sweep: the panels of this call add to one report
    if (m64 > FH_MAX_LD) {          // independent right-hand sides: 64 at a time (LU factor cached between panels)
        int rc0 = fh_check_problem(h, m64, 1);
        if (rc0) return rc0;
        const size_t N0 = (size_t)fh_N(h);
        feasthip_stats tot;
        memset(&tot, 0, sizeof(tot));
        int worst = 0;
        for (int64_t c0 = 0; c0 < m64; c0 += FH_MAX_LD) {
            const int64_t mc = std::min<int64_t>(FH_MAX_LD, m64 - c0);
            feasthip_stats st;
            rc0 = fh_shifted_solve_panel(h, z_re, z_im, mc, (const cplx*)dX + c0 * N0, (cplx*)dY + c0 * N0, &st);
            if (rc0 != 0 && rc0 != FEASTHIP_ERROR_NO_CONVERGENCE && rc0 != FEASTHIP_ERROR_LAPACK) return rc0;
            worst = std::max(worst, rc0);
            tot.krylov_iterations += st.krylov_iterations; tot.spmm_calls += st.spmm_calls; tot.factorizations += st.factorizations;
            tot.max_rel_residual = std::max(tot.max_rel_residual, st.max_rel_residual);
        }
        if (stats) *stats = tot;
        return worst;
    }
    return fh_shifted_solve_panel(h, z_re, z_im, m64, dX, dY, stats);
}

// one panel (m <= 64) of feasthip_shifted_solve_dev
static int fh_shifted_solve_panel(feasthip_ctx* h, double z_re, double z_im, int64_t m64, const void* dX, void* dY, feasthip_stats* stats) {
    int rc = fh_check_problem(h, m64);
    if (rc) return rc;
    if (!dX || !dY) { h->last_error = "shifted_solve: null argument"; return FEASTHIP_ERROR_INTERNAL; }
    if ((rc = fh_check_operator_solve(h, "shifted_solve"))) return rc;
    if ((rc = fh_check_adjoint(h, "shifted_solve"))) return rc;
    if ((rc = fh_check_precond(h, "shifted_solve"))) return rc;
    FH_CHECK(hipSetDevice(h->device));
    const int m = (int)m64, ld = fh_pick_ld(m), N = (int)fh_N(h);
    const size_t panel = (size_t)N * ld;
    cplx *Rhs, *Y;
    if ((rc = fh_buf(h, "ss_rhs", panel, &Rhs))) return rc;
    if ((rc = fh_buf(h, "ss_Y", panel, &Y))) return rc;
    if (stats) memset(stats, 0, sizeof(*stats));
    fh_launch_to_panel((const cplx*)dX, N, N, m, Rhs, ld, h->stream, fh_perm(h));
    std::vector<cplx> z(1, cmake(z_re, z_im));
    std::vector<int> status(1, 0);
    if (h->solver == FEASTHIP_SOLVER_LU || h->solver == FEASTHIP_SOLVER_BANDED) {
        const bool banded = h->solver == FEASTHIP_SOLVER_BANDED;
        if (!banded && h->kind != FH_KIND_DENSE) { h->last_error = "solver LU requires a dense matrix"; return FEASTHIP_ERROR_FPM; }
        int64_t nfact = 0;          // (the factors are cached per quadrature node when z is one, else in one extra slot)
        double worst = 0.0;
        if (h->factor_precision == 32) rc = fh_dense_lu_refined(h, ld, m, 1, z, Rhs, Y, panel, status, &nfact, true, &worst, banded);
        else rc = fh_direct_solve_single(h, banded, ld, m, z[0], Rhs, Y, &status[0], &nfact);
        if (rc) return rc;
        if (stats) { stats->factorizations = nfact; stats->max_rel_residual = worst; }
    } else {
        if (h->solver == FEASTHIP_SOLVER_COCG && fh_is_complex_input(h)) {
            h->last_error = "solver COCG needs real-symmetric A and B";
            return FEASTHIP_ERROR_FPM;
        }
        FH_CHECK(hipMemsetAsync(Y, 0, panel * sizeof(cplx), h->stream));
        fh_solve_result sr;
        const int method = h->solver == FEASTHIP_SOLVER_COCG ? 1 : h->solver == FEASTHIP_SOLVER_BICGSTAB ? 0 : -1;      // -1: GMRES
        int64_t nfact = 0;
        if (method >= 0) rc = fh_krylov(h, method, h->factor_precision, ld, m, 1, z, Rhs, Y, panel, sr, fh_krylov_opts());
        else if (!h->pc_pivots.empty()) {             // a single shift takes the nearest pivot
            const std::vector<int> pivot(1, fh_precond::nearest_pivot(z_re, z_im, &h->pc_pivots[0].x, (int)h->pc_pivots.size()));
            rc = fh_gmres_preconditioned(h, ld, m, z, pivot, true, Rhs, Y, panel, &nfact, sr);
        } else rc = fh_gmres(h, ld, m, 1, z, Rhs, Y, panel, sr);
        if (rc) return rc;
        status = sr.status;
        if (stats) { stats->krylov_iterations = sr.iters_sum; stats->spmm_calls = sr.op_calls; stats->max_rel_residual = sr.max_rel_res; stats->factorizations = nfact; }
    }
    fh_launch_from_panel(Y, ld, N, m, (cplx*)dY, N, h->stream, fh_perm(h));
    FH_CHECK(hipStreamSynchronize(h->stream));
    fh_prof_collect(h);
    return status[0];
}

extern "C" int feasthip_shifted_solve(feasthip_handle h, double z_re, double z_im, int64_t m, const void* X, void* Y,
                                      feasthip_stats* stats) {
    int rc = fh_check_problem(h, m, 1);
    if (rc) return rc;
    if (!X || !Y) { h->last_error = "shifted_solve: null argument"; return FEASTHIP_ERROR_INTERNAL; }
    if ((rc = fh_check_adjoint(h, "shifted_solve"))) return rc;
    FH_CHECK(hipSetDevice(h->device));
    const size_t nb = (size_t)fh_N(h) * m * sizeof(cplx);
    void *dX, *dY;
    if ((rc = fh_stage_in(h, "host_Q", X, nb, &dX))) return rc;
    if ((rc = fh_get_buf(h, "host_X", nb, &dY))) return rc;
    rc = feasthip_shifted_solve_dev(h, z_re, z_im, m, dX, dY, stats);
    if (rc != 0 && rc != FEASTHIP_ERROR_NO_CONVERGENCE) return rc;
    FH_CHECK(hipMemcpy(Y, dY, nb, hipMemcpyDeviceToHost));
    return rc;
}
