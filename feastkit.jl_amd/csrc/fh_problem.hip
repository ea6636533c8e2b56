// fh_problem.hip -- what a handle works on: CSR and dense ingest, the adjoint CSR set, contour, node and solver settings,
// the plan queries.
#include "fh_host.hpp"
#include "fh_dense.hpp"
#include "fh_banded.hpp"
#include "fh_knobs.hpp"

// ---------------------------------------------------------------------------------------
// problem definition
// ---------------------------------------------------------------------------------------
static inline cplx fh_ing_zero(cplx) { return cmake(0, 0); }
static inline cplx fh_ing_add(cplx a, cplx b) { return cadd(a, b); }
static inline cplx fh_ing_conj(cplx a) { return cmake(a.x, -a.y); }
#define FH_INGEST_STORAGE_CSR FEASTHIP_STORAGE_CSR
#include "fh_ingest.hpp"       // host side of the ingest (pure C++; also compiled under ASan/UBSan by tests/host_ingest_harness.cpp)

template <typename VT>
static int set_csr_typed(feasthip_ctx* h, int64_t N, int index_base, int storage, int64_t nnzA, const int64_t* ptrA,
                         const int64_t* idxA, const VT* valA, int64_t nnzB, const int64_t* ptrB, const int64_t* idxB,
                         const VT* valB) {
    // Row-block renumbering (fh_ingest.hpp: recursive bisection into 128-row blocks).  ON by default for wide patterns since
    // round 3: the row-per-wave SpMM is bound by the traffic that misses L2 (1-KB rows: the two far stencil planes of the
    // caller's order do not fit 4 MiB), and compact blocks keep a slice's gathers local -- cfg 3: 37 -> 30 us per node and
    // launch, 163 -> 159 ms per solve.  (k_spmm, with its 256-B tiles, never cared: round 2.)  FH_REORDER=0 keeps the caller's
    // order, FH_REORDER=2 renumbers whenever there are at least two blocks (test rigs push small problems through it).  The
    // LDS-window kernel the renumbering was built for stays opt-in (FH_LDS_SPMM=1): 57 vs 33 us per node on cfg 3.
    fh_prepared<VT> P;
    std::string err;
    const int prc = fh_prepare_csr<VT>(N, index_base, storage, nnzA, ptrA, idxA, valA, nnzB, ptrB, idxB, valB, fh_knob::reorder(),
                                       FH_SPMM_R, FH_SPMM_EXT, sizeof(VT) == sizeof(double), P, err);
    if (prc) { h->last_error = "feasthip_set_csr: " + err; return prc == 3 ? FEASTHIP_ERROR_MEMORY : FEASTHIP_ERROR_N; }
    const bool hasB = ptrB != nullptr;
    fh_free_problem(h);
    h->csr_kl = P.kl; h->csr_ku = P.ku;
    h->host_rowptr = P.rowptr; h->host_col = P.col;
    const std::vector<int>& rowptr = P.rowptr;
    const std::vector<int>& col = P.col;
    fh_csr& d = h->csr;
    d.N = N; d.nnz = (int64_t)col.size(); d.is_complex = sizeof(VT) == sizeof(cplx); d.b_identity = hasB ? 0 : 1;
    FH_CHECK(hipMalloc((void**)&d.rowptr, (N + 1) * sizeof(int)));
    FH_CHECK(hipMalloc((void**)&d.col, std::max<size_t>(1, col.size()) * sizeof(int)));
    FH_CHECK(hipMalloc(&d.aval, std::max<size_t>(1, col.size()) * sizeof(VT)));
    FH_CHECK(hipMemcpy(d.rowptr, rowptr.data(), (N + 1) * sizeof(int), hipMemcpyHostToDevice));
    FH_CHECK(hipMemcpy(d.col, col.data(), col.size() * sizeof(int), hipMemcpyHostToDevice));
    FH_CHECK(hipMemcpy(d.aval, P.av.data(), col.size() * sizeof(VT), hipMemcpyHostToDevice));
    if (hasB) {
        FH_CHECK(hipMalloc(&d.bval, std::max<size_t>(1, col.size()) * sizeof(VT)));
        FH_CHECK(hipMemcpy(d.bval, P.bv.data(), col.size() * sizeof(VT), hipMemcpyHostToDevice));
    }
    if (!P.rp8.empty()) {
        FH_CHECK(hipMalloc((void**)&d.rp8, (N + 1) * sizeof(int)));
        FH_CHECK(hipMalloc((void**)&d.col8, P.col8.size() * sizeof(int)));
        FH_CHECK(hipMalloc((void**)&d.a8, P.a8.size() * sizeof(double)));
        FH_CHECK(hipMemcpy(d.rp8, P.rp8.data(), (N + 1) * sizeof(int), hipMemcpyHostToDevice));
        FH_CHECK(hipMemcpy(d.col8, P.col8.data(), P.col8.size() * sizeof(int), hipMemcpyHostToDevice));
        FH_CHECK(hipMemcpy(d.a8, P.a8.data(), P.a8.size() * sizeof(double), hipMemcpyHostToDevice));
        if (hasB) {
            FH_CHECK(hipMalloc((void**)&d.b8, P.b8.size() * sizeof(double)));
            FH_CHECK(hipMemcpy(d.b8, P.b8.data(), P.b8.size() * sizeof(double), hipMemcpyHostToDevice));
        }
    }
    if (!P.perm.empty()) {
        const int nb = (int)P.blk_start.size() - 1;
        FH_CHECK(hipMalloc((void**)&d.perm, N * sizeof(int)));
        FH_CHECK(hipMemcpy(d.perm, P.perm.data(), N * sizeof(int), hipMemcpyHostToDevice));
        d.nblk = nb;
        FH_CHECK(hipMalloc((void**)&d.blk_start, (nb + 1) * sizeof(int)));
        FH_CHECK(hipMalloc((void**)&d.ext_ptr, (nb + 1) * sizeof(int)));
        FH_CHECK(hipMalloc((void**)&d.ext_idx, std::max<size_t>(1, P.ext_idx.size()) * sizeof(int)));
        FH_CHECK(hipMalloc((void**)&d.lcol, std::max<size_t>(1, P.lcol.size()) * sizeof(unsigned short)));
        FH_CHECK(hipMemcpy(d.blk_start, P.blk_start.data(), (nb + 1) * sizeof(int), hipMemcpyHostToDevice));
        FH_CHECK(hipMemcpy(d.ext_ptr, P.ext_ptr.data(), (nb + 1) * sizeof(int), hipMemcpyHostToDevice));
        FH_CHECK(hipMemcpy(d.ext_idx, P.ext_idx.data(), P.ext_idx.size() * sizeof(int), hipMemcpyHostToDevice));
        FH_CHECK(hipMemcpy(d.lcol, P.lcol.data(), P.lcol.size() * sizeof(unsigned short), hipMemcpyHostToDevice));
        if (fh_knob::debug_timing())
            fprintf(stderr, "[feasthip] renumbered into %d row blocks, %.1f outside rows per block on average\n", nb, nb ? (double)P.ext_idx.size() / nb : 0.0);
    }
    h->kind = FH_KIND_CSR;
    return 0;
}

// The adjoint CSR set of the problem (h->csr_adj), built on first use: the host keeps only the pattern, so the values come back
// from the device once; the transpose is fh_adjoint_csr (fh_ingest.hpp).  Only what k_spmm reads is made: no chunk-of-8 rows,
// no LDS-window data.
template <typename VT>
static int fh_adjoint_csr_build(feasthip_ctx* h) {
    const fh_csr& d = h->csr;
    const int64_t N = d.N;
    const size_t nnz = (size_t)d.nnz;
    if ((int64_t)h->host_rowptr.size() != N + 1 || h->host_col.size() != nnz) { h->last_error = "adjoint CSR set: no host pattern"; return FEASTHIP_ERROR_INTERNAL; }
    std::vector<VT> av(nnz), bv(d.b_identity ? 0 : nnz);
    FH_CHECK(hipStreamSynchronize(h->stream));
    if (nnz) FH_CHECK(hipMemcpy(av.data(), d.aval, nnz * sizeof(VT), hipMemcpyDeviceToHost));
    if (nnz && !d.b_identity) FH_CHECK(hipMemcpy(bv.data(), d.bval, nnz * sizeof(VT), hipMemcpyDeviceToHost));
    std::vector<int> rp, cl;
    std::vector<VT> avt, bvt;
    fh_adjoint_csr<VT>(N, h->host_rowptr, h->host_col, av.data(), d.b_identity ? nullptr : bv.data(), rp, cl, avt, bvt);
    fh_free_adjoint_csr(h);
    fh_csr& t = h->csr_adj;
    FH_CHECK(hipMalloc((void**)&t.rowptr, (N + 1) * sizeof(int)));
    FH_CHECK(hipMalloc((void**)&t.col, std::max<size_t>(1, nnz) * sizeof(int)));
    FH_CHECK(hipMalloc(&t.aval, std::max<size_t>(1, nnz) * sizeof(VT)));
    FH_CHECK(hipMemcpy(t.rowptr, rp.data(), (N + 1) * sizeof(int), hipMemcpyHostToDevice));
    if (nnz) FH_CHECK(hipMemcpy(t.col, cl.data(), nnz * sizeof(int), hipMemcpyHostToDevice));
    if (nnz) FH_CHECK(hipMemcpy(t.aval, avt.data(), nnz * sizeof(VT), hipMemcpyHostToDevice));
    if (!d.b_identity) {
        FH_CHECK(hipMalloc(&t.bval, std::max<size_t>(1, nnz) * sizeof(VT)));
        if (nnz) FH_CHECK(hipMemcpy(t.bval, bvt.data(), nnz * sizeof(VT), hipMemcpyHostToDevice));
    }
    t.N = N; t.nnz = d.nnz; t.is_complex = d.is_complex; t.b_identity = d.b_identity;
    return 0;
}
int fh_adjoint_csr_ensure(feasthip_ctx* h) {
    if (h->csr_adj.rowptr && h->csr_adj.N == h->csr.N) return 0;
    const int rc = h->csr.is_complex ? fh_adjoint_csr_build<cplx>(h) : fh_adjoint_csr_build<double>(h);
    if (rc) fh_free_adjoint_csr(h);
    return rc;
}

extern "C" int feasthip_set_csr(feasthip_handle h, int64_t N, int is_complex, int index_base, int storage,
                                int64_t nnzA, const int64_t* ptrA, const int64_t* idxA, const void* valA,
                                int64_t nnzB, const int64_t* ptrB, const int64_t* idxB, const void* valB) {
    if (!h) return FEASTHIP_ERROR_INTERNAL;
    if (N <= 0 || N > INT32_MAX / FH_MAX_LD) { h->last_error = "feasthip_set_csr: N out of range"; return FEASTHIP_ERROR_N; }
    if (!ptrA || (nnzA > 0 && (!idxA || !valA))) { h->last_error = "feasthip_set_csr: null A"; return FEASTHIP_ERROR_N; }
    if (index_base != 0 && index_base != 1) { h->last_error = "feasthip_set_csr: index_base must be 0 or 1"; return FEASTHIP_ERROR_FPM; }
    if (storage != FEASTHIP_STORAGE_CSR && storage != FEASTHIP_STORAGE_CSC) { h->last_error = "feasthip_set_csr: bad storage"; return FEASTHIP_ERROR_FPM; }
    FH_CHECK(hipSetDevice(h->device));
    FH_CHECK(hipStreamSynchronize(h->stream));
    if (is_complex)
        return set_csr_typed<cplx>(h, N, index_base, storage, nnzA, ptrA, idxA, (const cplx*)valA, nnzB, ptrB, idxB, (const cplx*)valB);
    return set_csr_typed<double>(h, N, index_base, storage, nnzA, ptrA, idxA, (const double*)valA, nnzB, ptrB, idxB, (const double*)valB);
}

extern "C" int feasthip_release_factors(feasthip_handle h) {
    if (int gate = fh_gate(h)) return gate;
    FH_CHECK(hipSetDevice(h->device));
    FH_CHECK(hipStreamSynchronize(h->stream));
    if (h->side_stream) FH_CHECK(hipStreamSynchronize(h->side_stream));
    h->lu_cache.clear(hipFree);
    h->band_cache.clear(hipFree);
    fh_mf_free_buffers(h);
    return 0;
}

extern "C" int feasthip_band_plan(feasthip_handle h, int* kl, int* ku, int64_t* bytes_per_node, int* blocked) {
    if (int gate = fh_gate(h)) return gate;
    FH_CHECK(hipSetDevice(h->device));
    return fh_banded_plan(h, kl, ku, bytes_per_node, blocked);
}
extern "C" int feasthip_direct_plan_flops(feasthip_handle h, double* flops_per_node) {
    if (int gate = fh_gate(h)) return gate;
    FH_CHECK(hipSetDevice(h->device));
    return fh_banded_plan_flops(h, flops_per_node);
}

extern "C" int feasthip_set_dense(feasthip_handle h, int64_t N, int is_complex, const void* A, int64_t lda,
                                  const void* B, int64_t ldb) {
    if (!h) return FEASTHIP_ERROR_INTERNAL;
    if (N <= 0 || N > 65536) { h->last_error = "feasthip_set_dense: N out of range"; return FEASTHIP_ERROR_N; }
    if (!A || lda < N || (B && ldb < N)) { h->last_error = "feasthip_set_dense: bad A/lda/ldb"; return FEASTHIP_ERROR_N; }
    FH_CHECK(hipSetDevice(h->device));
    FH_CHECK(hipStreamSynchronize(h->stream));
    fh_free_problem(h);
    size_t es = is_complex ? sizeof(cplx) : sizeof(double);
    fh_dense& d = h->dense;
    d.N = N; d.is_complex = is_complex; d.b_identity = B ? 0 : 1;
    FH_CHECK(hipMalloc(&d.A, (size_t)N * N * es));
    FH_CHECK(hipMemcpy2D(d.A, (size_t)N * es, A, (size_t)lda * es, (size_t)N * es, (size_t)N, hipMemcpyHostToDevice));
    if (B) {
        FH_CHECK(hipMalloc(&d.B, (size_t)N * N * es));
        FH_CHECK(hipMemcpy2D(d.B, (size_t)N * es, B, (size_t)ldb * es, (size_t)N * es, (size_t)N, hipMemcpyHostToDevice));
    }
    h->kind = FH_KIND_DENSE;
    return 0;
}

// What an operator handle (FH_KIND_OPERATOR, feasthip_set_operator) cannot take; every message names the solvers it does take
const char* const fh_operator_why_adjoint =
    "an operator handle (feasthip_set_operator) has no adjoint form: the callback applies A and B only, under the Krylov solvers FEASTHIP_SOLVER_BICGSTAB, _COCG or _GMRES";
const char* fh_operator_solver_why(const feasthip_ctx* h, int kind, int factor_precision) {
    if (kind == FEASTHIP_SOLVER_LU || kind == FEASTHIP_SOLVER_BANDED)
        return "an operator handle (feasthip_set_operator) has no matrix to factor: use the Krylov solvers FEASTHIP_SOLVER_BICGSTAB, _COCG or _GMRES";
    const bool cocg = kind == FEASTHIP_SOLVER_COCG || kind == FEASTHIP_SOLVER_SHIFTED_COCG || kind == FEASTHIP_SOLVER_BLOCK_COCG;
    if (cocg && (!h->op.symmetric || h->dense.is_complex))
        return "FEASTHIP_SOLVER_COCG on an operator handle needs FEASTHIP_OP_SYMMETRIC and a real operator (A = A^T, B = B^T): of the Krylov solvers FEASTHIP_SOLVER_BICGSTAB, _COCG or _GMRES take _BICGSTAB or _GMRES";
    if (factor_precision == 32)
        return "factor_precision = 32 is not supported on an operator handle: the Krylov solvers FEASTHIP_SOLVER_BICGSTAB, _COCG or _GMRES run on complex128 panels";
    return nullptr;
}

// What a term-operator handle (FH_KIND_TERM_OPERATOR, feasthip_set_term_operator) cannot take; every message names the solvers it does take
const char* fh_termop_solver_why(const feasthip_ctx* h, int kind, int factor_precision) {
    if (kind == FEASTHIP_SOLVER_LU || kind == FEASTHIP_SOLVER_BANDED) return "there is no matrix to factor: " FH_TERMOP_TAKES;
    if (kind == FEASTHIP_SOLVER_SHIFTED_COCG || kind == FEASTHIP_SOLVER_BLOCK_COCG) return "the shifted and block COCG sweeps are pencil sweeps: " FH_TERMOP_TAKES;
    if (kind == FEASTHIP_SOLVER_COCG && !h->op.symmetric) return "FEASTHIP_SOLVER_COCG needs FEASTHIP_OP_SYMMETRIC (every A_k = A_k^T): " FH_TERMOP_TAKES;
    if (factor_precision == 32) return "factor_precision = 32 is not supported (complex128 panels): " FH_TERMOP_TAKES;
    return nullptr;
}

extern "C" int feasthip_set_contour(feasthip_handle h, int ne, const double* zne, const double* wne, double weight_scale) {
    if (!h) return FEASTHIP_ERROR_INTERNAL;
    if (ne <= 0 || !zne || !wne) { h->last_error = "feasthip_set_contour: ne <= 0 or null arrays"; return FEASTHIP_ERROR_FPM; }
    h->zne.resize(ne); h->wne.resize(ne);
    for (int e = 0; e < ne; ++e) {
        h->zne[e] = cmake(zne[2 * e], zne[2 * e + 1]);
        h->wne[e] = cmake(wne[2 * e], wne[2 * e + 1]);
    }
    h->weight_scale = weight_scale;
    if ((int)h->node_kinds.size() != ne) h->node_kinds.clear();      // feasthip_set_node_solver: kinds of another contour
    if ((int)h->pc_node_pivot.size() != ne) { h->pc_pivots.clear(); h->pc_node_pivot.clear(); }      // feasthip_set_preconditioner likewise
    h->node_first = 0;
    h->node_count = ne;
    h->node_ids.resize(ne);
    for (int e = 0; e < ne; ++e) h->node_ids[e] = e;
    // cached factors stay: slot e is reused only when its shift equals the new z_e exactly (fh_direct_solve_nodes over
    // fh_factor_cache::holds), so a repeated solve on the same contour keeps its factorisations and any other contour
    // refactors slot by slot
    return 0;
}

extern "C" int feasthip_set_node_solver(feasthip_handle h, int count, const int* kinds) {
    if (!h) return FEASTHIP_ERROR_INTERNAL;
    if (count == 0 || !kinds) { h->node_kinds.clear(); return 0; }
    if (count != (int)h->zne.size()) {
        h->last_error = "feasthip_set_node_solver: count " + std::to_string(count) + " is not the contour's node count " + std::to_string(h->zne.size());
        return FEASTHIP_ERROR_FPM;
    }
    for (int e = 0; e < count; ++e)
        if (kinds[e] != 0 && kinds[e] != FEASTHIP_SOLVER_BANDED) {
            h->last_error = "feasthip_set_node_solver: kind " + std::to_string(kinds[e]) + " of node " + std::to_string(e) + " (0 or FEASTHIP_SOLVER_BANDED)";
            return FEASTHIP_ERROR_FPM;
        }
    if (h->kind == FH_KIND_OPERATOR)
        for (int e = 0; e < count; ++e)
            if (kinds[e] != 0) {
                h->last_error = "feasthip_set_node_solver: an operator handle (feasthip_set_operator) has no matrix for a direct node; every node takes the Krylov solvers FEASTHIP_SOLVER_BICGSTAB, _COCG or _GMRES";
                return FEASTHIP_ERROR_FPM;
            }
    if (h->kind == FH_KIND_TERM_OPERATOR)
        for (int e = 0; e < count; ++e)
            if (kinds[e] != 0) { h->last_error = "feasthip_set_node_solver: there is no matrix for a direct node: " FH_TERMOP_TAKES; return FEASTHIP_ERROR_FPM; }
    h->node_kinds.assign(kinds, kinds + count);
    return 0;
}

// Only the setting's own shape is checked here; what it cannot go with (solver, handle kind, precision, adjoint, communicator,
// direct nodes) may change after this call, so the entry points that honour it look at those (fh_api.hip: fh_check_precond)
extern "C" int feasthip_set_preconditioner(feasthip_handle h, int npivots, const double* pivots, int count, const int* node_pivot) {
    if (!h) return FEASTHIP_ERROR_INTERNAL;
    if (npivots == 0) { h->pc_pivots.clear(); h->pc_node_pivot.clear(); return 0; }
    if (npivots < 0 || !pivots || !node_pivot) { h->last_error = "feasthip_set_preconditioner: npivots < 0 or null arrays"; return FEASTHIP_ERROR_FPM; }
    if (count != (int)h->zne.size()) {
        h->last_error = "feasthip_set_preconditioner: count " + std::to_string(count) + " is not the contour's node count " + std::to_string(h->zne.size());
        return FEASTHIP_ERROR_FPM;
    }
    for (int p = 0; p < npivots; ++p) {
        if (!(pivots[2 * p + 1] != 0.0) || !std::isfinite(pivots[2 * p]) || !std::isfinite(pivots[2 * p + 1])) {
            h->last_error = "feasthip_set_preconditioner: pivot " + std::to_string(p) + " must be finite with a non-zero imaginary part (z_p B - A is factored without a stop test)";
            return FEASTHIP_ERROR_FPM;
        }
        for (int q = 0; q < p; ++q)
            if (pivots[2 * q] == pivots[2 * p] && pivots[2 * q + 1] == pivots[2 * p + 1]) {
                h->last_error = "feasthip_set_preconditioner: pivots " + std::to_string(q) + " and " + std::to_string(p) + " are the same shift";
                return FEASTHIP_ERROR_FPM;
            }
    }
    for (int e = 0; e < count; ++e)
        if (node_pivot[e] < -1 || node_pivot[e] >= npivots) {
            h->last_error = "feasthip_set_preconditioner: node_pivot[" + std::to_string(e) + "] = " + std::to_string(node_pivot[e]) + " (-1 or a pivot index below " + std::to_string(npivots) + ")";
            return FEASTHIP_ERROR_FPM;
        }
    h->pc_pivots.resize(npivots);
    for (int p = 0; p < npivots; ++p) h->pc_pivots[p] = cmake(pivots[2 * p], pivots[2 * p + 1]);
    h->pc_node_pivot.assign(node_pivot, node_pivot + count);
    return 0;
}

extern "C" int feasthip_direct_plan_bytes(feasthip_handle h, int nodes, int64_t* factor_bytes, int64_t* transient_bytes) {
    if (int gate = fh_gate(h)) return gate;
    if (!(h->kind == FH_KIND_CSR || (h->kind == FH_KIND_POLYNOMIAL && h->poly.sparse)) || nodes < 0) {
        h->last_error = "feasthip_direct_plan_bytes: needs a CSR problem (or a sparse polynomial) and nodes >= 0";
        return FEASTHIP_ERROR_FPM;
    }
    FH_CHECK(hipSetDevice(h->device));
    return fh_banded_plan_bytes(h, nodes, factor_bytes, transient_bytes);
}

extern "C" int feasthip_set_real_projection(feasthip_handle h, int real_part) {
    if (!h) return FEASTHIP_ERROR_INTERNAL;
    h->real_projection = real_part ? 1 : 0;
    return 0;
}

extern "C" int feasthip_set_adjoint(feasthip_handle h, int on) {
    if (!h) return FEASTHIP_ERROR_INTERNAL;
    if (on && h->kind == FH_KIND_POLYNOMIAL) { h->last_error = "feasthip_set_adjoint: a polynomial handle has no adjoint form (the feasthip_poly_* calls are forward only)"; return FEASTHIP_ERROR_FPM; }
    if (on && h->kind == FH_KIND_OPERATOR) { h->last_error = std::string("feasthip_set_adjoint: ") + fh_operator_why_adjoint; return FEASTHIP_ERROR_FPM; }
    if (on && h->kind == FH_KIND_TERM_OPERATOR) { h->last_error = "feasthip_set_adjoint: the callback applies the A_k only, there is no adjoint form: " FH_TERMOP_TAKES; return FEASTHIP_ERROR_FPM; }
    h->adjoint = on ? 1 : 0;
    return 0;
}

extern "C" int feasthip_require_adjoint(feasthip_handle h, int on) {
    if (!h) return FEASTHIP_ERROR_INTERNAL;
    h->require_adjoint = on ? 1 : 0;
    return 0;
}

extern "C" int feasthip_set_node_range(feasthip_handle h, int first, int count) {
    if (!h) return FEASTHIP_ERROR_INTERNAL;
    if (first < 0 || count < 0 || first + count > (int)h->zne.size()) {
        h->last_error = "feasthip_set_node_range: range outside the contour";
        return FEASTHIP_ERROR_FPM;
    }
    if (h->kind == FH_KIND_TERM_OPERATOR && (first != 0 || count != (int)h->zne.size())) {
        h->last_error = "feasthip_set_node_range: the whole contour is swept on one rank: " FH_TERMOP_TAKES;
        return FEASTHIP_ERROR_FPM;
    }
    if (h->kind == FH_KIND_POLYNOMIAL && (first != 0 || count != (int)h->zne.size())) {
        h->last_error = "feasthip_set_node_range: a polynomial handle sweeps the whole contour (feasthip_poly_contour_apply_dev runs on one rank)";
        return FEASTHIP_ERROR_FPM;
    }
    h->node_first = first;
    h->node_count = count;
    h->node_ids.resize(count);
    for (int e = 0; e < count; ++e) h->node_ids[e] = first + e;
    return 0;
}

extern "C" int feasthip_set_node_list(feasthip_handle h, int count, const int* indices) {
    if (!h) return FEASTHIP_ERROR_INTERNAL;
    if (count < 0 || (count > 0 && !indices)) { h->last_error = "feasthip_set_node_list: bad arguments"; return FEASTHIP_ERROR_FPM; }
    if (h->kind == FH_KIND_TERM_OPERATOR) { h->last_error = "feasthip_set_node_list: the whole contour is swept on one rank: " FH_TERMOP_TAKES; return FEASTHIP_ERROR_FPM; }
    if (h->kind == FH_KIND_POLYNOMIAL) {
        h->last_error = "feasthip_set_node_list: a polynomial handle sweeps the whole contour (feasthip_poly_contour_apply_dev runs on one rank)";
        return FEASTHIP_ERROR_FPM;
    }
    for (int e = 0; e < count; ++e)
        if (indices[e] < 0 || indices[e] >= (int)h->zne.size()) {
            h->last_error = "feasthip_set_node_list: index outside the contour";
            return FEASTHIP_ERROR_FPM;
        }
    h->node_ids.assign(indices, indices + count);
    h->node_first = count > 0 ? indices[0] : 0;
    h->node_count = count;
    return 0;
}

extern "C" int feasthip_set_column_mask(feasthip_handle h, int64_t m, const int* mask) {
    if (!h) return FEASTHIP_ERROR_INTERNAL;
    if (m < 0 || m > (1 << 20)) { h->last_error = "set_column_mask: m out of range"; return FEASTHIP_ERROR_M0; }
    h->col_mask.clear();
    if (mask && m > 0) h->col_mask.assign(mask, mask + m);
    return 0;
}

extern "C" int feasthip_set_solver(feasthip_handle h, int kind, double rtol, double atol, int maxit, int restart,
                                   int factor_precision, int cache_factors) {
    if (!h) return FEASTHIP_ERROR_INTERNAL;
    if (kind < 0 || kind > FEASTHIP_SOLVER_BLOCK_COCG || rtol < 0 || atol < 0 || maxit <= 0 || restart < 0 ||
        (factor_precision != 64 && factor_precision != 32)) {
        h->last_error = "feasthip_set_solver: invalid option";
        return FEASTHIP_ERROR_FPM;
    }
    if (h->kind == FH_KIND_POLYNOMIAL) {
        // dense coefficients: the LU of P(z_e) only.  CSR coefficients: that (the multifrontal LU), or a Krylov solver on the
        // operator P(z_e) (fh_poly.hip: k_spmm_poly); complex128 throughout
        const bool krylov = kind == FEASTHIP_SOLVER_BICGSTAB || kind == FEASTHIP_SOLVER_COCG || kind == FEASTHIP_SOLVER_GMRES;
        if (h->poly.terms && kind != FEASTHIP_SOLVER_LU) {      // the Krylov operator k_spmm_poly forms powers of z_e
            h->last_error = "feasthip_set_solver: a term handle (feasthip_set_terms) takes FEASTHIP_SOLVER_LU only; Krylov solves on T(z) are not provided";
            return FEASTHIP_ERROR_FPM;
        }
        if (factor_precision != 64 || !(kind == FEASTHIP_SOLVER_LU || (krylov && h->poly.sparse))) {
            h->last_error = h->poly.sparse ? "feasthip_set_solver: a CSR polynomial handle needs FEASTHIP_SOLVER_LU, _BICGSTAB, _COCG or _GMRES with factor_precision = 64"
                                           : "feasthip_set_solver: a dense polynomial handle needs FEASTHIP_SOLVER_LU with factor_precision = 64";
            return FEASTHIP_ERROR_FPM;
        }
    }
    if (h->kind == FH_KIND_OPERATOR)
        if (const char* why = fh_operator_solver_why(h, kind, factor_precision)) { h->last_error = std::string("feasthip_set_solver: ") + why; return FEASTHIP_ERROR_FPM; }
    if (h->kind == FH_KIND_TERM_OPERATOR)
        if (const char* why = fh_termop_solver_why(h, kind, factor_precision)) { h->last_error = std::string("feasthip_set_solver: ") + why; return FEASTHIP_ERROR_FPM; }
    // SHIFTED_COCG is COCG with the shifted sweep where fh_contour_apply_panel finds it eligible: every other path sees COCG
    h->shifted = kind == FEASTHIP_SOLVER_SHIFTED_COCG ? 1 : 0;
    // BLOCK_COCG likewise: COCG with the block sweep where the panel is eligible
    h->block = kind == FEASTHIP_SOLVER_BLOCK_COCG ? 1 : 0;
    if (h->shifted || h->block) kind = FEASTHIP_SOLVER_COCG;
    h->solver = kind; h->rtol = rtol; h->atol = atol; h->maxit = maxit; h->restart = restart;
    h->factor_precision = factor_precision; h->cache_factors = cache_factors;
    return 0;
}
