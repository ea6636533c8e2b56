// fh_ortho.hip -- rank-revealing orthonormalisation of a subspace: Cholesky-QR, its staged form and the pivoted Gram-Schmidt.
#include "fh_host.hpp"
#include "fh_kernels.hpp"
#include "fh_dense.hpp"
#include "fh_cholqr.hpp"
#include "fh_knobs.hpp"

// ---------------------------------------------------------------------------------------
// orthonormalisation (a9)
// ---------------------------------------------------------------------------------------
// what the last orthonormalisation did (feasthip_last_ortho).  A call over several panels (fh_ortho_wide) adds up stages,
// fall-backs and rank; perm / rdiag are the last panel's.  The method reported for such a call is the staged path if any
// panel took it, else the Gram-Schmidt if any did, else the Cholesky-QR fast path.
void fh_ortho_note(feasthip_ctx* h, int used, int stages, int fell_back, int rank, const int* perm, const double* rdiag) {
    auto& o = h->ortho_last;
    auto weight = [](int u) { return u == FEASTHIP_ORTHO_CHOLQR_RR ? 2 : u == FEASTHIP_ORTHO_MGS ? 1 : 0; };
    if (o.panels == 0 || weight(used) > weight(o.used)) o.used = used;
    o.panels += 1;
    o.stages += stages; o.fell_back += fell_back; o.rank += rank;
    o.perm.assign(perm, perm + rank);
    if (rdiag) o.rdiag.assign(rdiag, rdiag + rank);
    else o.rdiag.assign(rank, 0.0);
}
void fh_ortho_note_reset(feasthip_ctx* h) {
    h->ortho_last.panels = h->ortho_last.used = h->ortho_last.stages = h->ortho_last.fell_back = h->ortho_last.rank = 0;
    h->ortho_last.perm.clear(); h->ortho_last.rdiag.clear();
}

// The staged rank-revealing Cholesky-QR (FEASTHIP_ORTHO_CHOLQR_RR) on a panel that fh_cholqr::accept rejected.  Per stage:
//   G = W^H W of the working copy W -> k_pchol_stage: the pivots this stage may judge, R^-1 with the permutation folded in
//   T = W R^-1 (the accepted columns, first pass); from the second stage on T -= K (K^H T) against the columns K kept so far
//   G = T^H T -> k_pchol_stage (refine): second pass, T2 = T R2^-1 lands in the columns [rank, rank + accepted) of a zero panel
//   Out += T2;  twice:  W -= T2 (T2^H W)
// All of it is queued for a fixed number of stages; the device decides how many run (the launches of a stage past the
// decision return at once) and the host reads the state once.  The Gram product, the panel product and the column update
// are the existing kernels (k_gram_mfma, k_small_matmul_mfma, k_axpy_cols) with a skip word: fusing gather, product and
// subtraction would save two passes over W per stage, which is not where the time of a 2-3 stage call goes (the latency
// chain of k_pchol_stage and the launch count are).  *staged = false: a non-finite Gram matrix, a stage that accepted
// nothing, a second pass that broke down, or no decision within FH_RR_MAX_STAGES; X is untouched in every case.
// colmax: the largest column norm of X (accept() has it).  The working copy is scaled by the power of two that brings it
// into [1, 2): exact, and the Gram matrices of the later stages -- squares of what is left after the projections -- stay
// clear of the denormal range for panels of any magnitude.
#define FH_RR_MAX_STAGES 6
#define FH_RR_WINDOW 1e-10
static int fh_ortho_staged(feasthip_ctx* h, int m, int ld, const cplx* X, cplx* Out, double rank_tol, double ref_scale, int big_dim,
                           double colmax, int* rank, bool* staged) {
    const int N = (int)fh_N(h);
    const size_t panel = (size_t)N * ld;
    int rc;
    *staged = false;
    cplx *W, *T, *T2, *gw, *G, *dR, *C;
    if ((rc = fh_buf(h, "rr_W", panel, &W))) return rc;
    if ((rc = fh_buf(h, "rr_T", panel, &T))) return rc;
    if ((rc = fh_buf(h, "rr_T2", panel, &T2))) return rc;
    if ((rc = fh_buf(h, "gram_work", fh_gram_work_elems(ld), &gw))) return rc;
    if ((rc = fh_buf(h, "gram_G", (size_t)ld * ld, &G))) return rc;
    if ((rc = fh_buf(h, "or_Rinv", (size_t)ld * ld, &dR))) return rc;
    if ((rc = fh_buf(h, "rr_C", (size_t)ld * ld, &C))) return rc;
    int* ist;
    double* dst;
    if ((rc = fh_buf(h, "rr_istate", FH_RR_PERM + FH_MAX_LD, &ist))) return rc;
    if ((rc = fh_buf(h, "rr_dstate", 2 + FH_MAX_LD, &dst))) return rc;
    std::vector<cplx> ones(ld, cmake(1, 0)), mones(ld, cmake(-1, 0));
    cplx *done, *dmone;
    if ((rc = fh_upload_coefs(h, "rr_one", ones, &done))) return rc;
    if ((rc = fh_upload_coefs(h, "rr_mone", mones, &dmone))) return rc;
    const double eps = 2.220446049250313e-16;
    const double big = (double)std::max(N, std::max(big_dim, m));
    const double thr = std::max(rank_tol, eps * big);                     // the threshold of k_mgs_pick
    const double scale = colmax > 0.0 && std::isfinite(colmax) ? std::ldexp(1.0, -std::ilogb(colmax)) : 1.0;
    std::vector<cplx> scl(ld, cmake(scale, 0));
    cplx* dscale;
    if ((rc = fh_upload_coefs(h, "rr_scale", scl, &dscale))) return rc;
    const int* skip = ist + FH_RR_SKIP;
    const int* decided = ist + FH_RR_DONE;
    hipStream_t st = h->stream;
    fh_prof_begin(h, "ortho");
    FH_CHECK(hipMemcpyAsync(W, X, panel * sizeof(cplx), hipMemcpyDeviceToDevice, st));
    if (scale != 1.0) fh_launch_scale_cols(W, dscale, N, ld, st);
    FH_CHECK(hipMemsetAsync(Out, 0, panel * sizeof(cplx), st));
    fh_launch_rr_init(ist, dst, ld, st);
    for (int s = 0; s < FH_RR_MAX_STAGES; ++s) {
        fh_launch_gram(W, W, N, ld, 0, gw, G, st, decided);
        fh_launch_pchol_stage(G, m, ld, 0, FH_RR_WINDOW, thr, ref_scale * scale, ist, dst, dR, st);
        fh_launch_small_matmul(W, dR, N, ld, T, st, skip);
        if (s > 0) {
            fh_launch_gram(Out, T, N, ld, 0, gw, C, st, skip);
            fh_launch_small_matmul(Out, C, N, ld, T2, st, skip);
            fh_launch_axpy_cols(T, T2, done, N, ld, st, skip);              // T -= K (K^H T)
        }
        fh_launch_gram(T, T, N, ld, 0, gw, G, st, skip);
        fh_launch_pchol_stage(G, m, ld, 1, 0.0, thr, ref_scale * scale, ist, dst, dR, st);
        fh_launch_small_matmul(T, dR, N, ld, T2, st, skip);
        fh_launch_axpy_cols(Out, T2, dmone, N, ld, st, skip);               // Out += T2
        for (int pass = 0; pass < 2; ++pass) {
            fh_launch_gram(T2, W, N, ld, 0, gw, C, st, decided);
            fh_launch_small_matmul(T2, C, N, ld, T, st, decided);
            fh_launch_axpy_cols(W, T, done, N, ld, st, decided);            // W -= T2 (T2^H W)
        }
    }
    fh_prof_end(h);
    int hst[FH_RR_PERM + FH_MAX_LD];
    double hds[2 + FH_MAX_LD];
    FH_CHECK(hipMemcpyAsync(hst, ist, (FH_RR_PERM + ld) * sizeof(int), hipMemcpyDeviceToHost, st));
    FH_CHECK(hipMemcpyAsync(hds, dst, (2 + ld) * sizeof(double), hipMemcpyDeviceToHost, st));
    FH_CHECK(hipStreamSynchronize(st));
    const int r = hst[FH_RR_RANK];
    if (hst[FH_RR_FAIL] || !hst[FH_RR_DONE] || r < 0 || r > m) return 0;
    *rank = r;
    *staged = true;
    for (int k = 0; k < r; ++k) hds[2 + k] /= scale;
    fh_ortho_note(h, FEASTHIP_ORTHO_CHOLQR_RR, hst[FH_RR_STAGES], 0, r, hst + FH_RR_PERM, hds + 2);
    return 0;
}

// Rank-revealing orthonormalisation of the m (<= ld) columns of panel X.  On success *res is the
// panel (X or Out) whose first *rank columns hold the basis.  ref_scale > 0 / big_dim: X is a
// block of a wider matrix (see k_mgs_pick).
int fh_ortho_panel(feasthip_ctx* h, int m, int ld, cplx* X, cplx* Out, double rank_tol, double ref_scale,
                          int big_dim, int* rank, cplx** res) {
    const int N = (int)fh_N(h);
    int rc;
    cplx *work, *coef;
    int* istate;
    double* dstate;
    if ((rc = fh_buf(h, "or_work", (size_t)256 * ld, &work))) return rc;
    if ((rc = fh_buf(h, "or_istate", 4 + FH_MAX_LD, &istate))) return rc;
    if ((rc = fh_buf(h, "or_dstate", 2 + FH_MAX_LD, &dstate))) return rc;
    if ((rc = fh_buf(h, "or_coef", FH_MAX_LD, &coef))) return rc;
    int fell_back = 0;
    // Fast path (Cholesky-QR, one or two passes) when the panel is far from rank deficient (fh_cholqr::accept: the pivoted
    // Cholesky pivots of the Gram matrix are the squared R_kk of the pivoted QR).  Otherwise fall through to the
    // rank-revealing pivoted Gram-Schmidt.  The Rayleigh-Ritz step that follows uses Q^H B Q anyway, so one pass suffices
    // when it is orthonormal to 1e-14.
    if (!fh_knob::no_cholqr()) {
        cplx *gw, *G, *dR;
        if ((rc = fh_buf(h, "gram_work", fh_gram_work_elems(ld), &gw))) return rc;
        if ((rc = fh_buf(h, "gram_G", (size_t)ld * ld, &G))) return rc;
        if ((rc = fh_buf(h, "or_Rinv", (size_t)ld * ld, &dR))) return rc;
        std::vector<cplx> Gh((size_t)ld * ld), Rinv;
        std::vector<double> dcol;
        bool ok = true;
        cplx* src = X;
        cplx* dst = Out;
        int npass = 2;
        const bool always_two = fh_knob::cholqr_two_pass();
        for (int pass = 0; pass < npass && ok; ++pass) {
            fh_prof_begin(h, "gram");
            fh_launch_gram(src, src, N, ld, 0, gw, G, h->stream);
            fh_prof_end(h);
            FH_CHECK(hipMemcpyAsync(Gh.data(), G, Gh.size() * sizeof(cplx), hipMemcpyDeviceToHost, h->stream));
            FH_CHECK(hipStreamSynchronize(h->stream));
            if (pass == 0) {         // equilibrates Gh: G = D G' D, D = diag(dcol)
                const fh_cholqr::Plan plan = fh_cholqr::accept(Gh, m, ld, ref_scale, rank_tol, always_two, dcol);
                if (plan == fh_cholqr::Plan::reject) { ok = false; break; }
                if (plan == fh_cholqr::Plan::one_pass) npass = 1;
            }
            if (!fh_cholqr::gram_upper_inverse(Gh, m, ld, Rinv)) { ok = false; break; }
            if (pass == 0)       // R = R' D  =>  R^-1 = D^-1 R'^-1: scale row i by 1/d_i
                for (int j = 0; j < m; ++j)
                    for (int i = 0; i < m; ++i) Rinv[(size_t)j * ld + i] = cscale(Rinv[(size_t)j * ld + i], 1.0 / dcol[i]);
            FH_CHECK(hipMemcpyAsync(dR, Rinv.data(), Rinv.size() * sizeof(cplx), hipMemcpyHostToDevice, h->stream));
            fh_prof_begin(h, "ortho");
            fh_launch_small_matmul(src, dR, N, ld, dst, h->stream);
            fh_prof_end(h);
            FH_CHECK(hipStreamSynchronize(h->stream));     // Rinv (host vector) is reused
            std::swap(src, dst);
        }
        if (ok) {       // src after the swaps: X after two passes, Out after one
            *rank = m;
            *res = src;
            std::vector<int> ident(m);
            for (int j = 0; j < m; ++j) ident[j] = j;
            fh_ortho_note(h, FEASTHIP_ORTHO_USED_CHOLQR, 0, 0, m, ident.data(), nullptr);
            return 0;
        }
        // a failure happens before the pass writes its destination: X still holds the input
        // (pass 0 writes Out, pass 1 would have written X)
        if (h->ortho_method == FEASTHIP_ORTHO_CHOLQR_RR) {
            bool staged = false;
            double colmax = 0.0;
            for (double dj : dcol) colmax = std::max(colmax, dj);
            if ((rc = fh_ortho_staged(h, m, ld, X, Out, rank_tol, ref_scale, big_dim, colmax, rank, &staged))) return rc;
            if (staged) { *res = Out; return 0; }
            fell_back = 1;                     // X is untouched: the Gram-Schmidt decides as it would have
        }
    }
    fh_mgs_args a;
    a.X = X; a.N = N; a.ld = ld; a.m = m; a.istate = istate; a.dstate = dstate; a.coef = coef; a.work = work;
    a.rank_tol = rank_tol; a.ref_scale = ref_scale; a.big_dim = big_dim;
    fh_prof_begin(h, "ortho");
    fh_mgs_run(a, h->stream);
    fh_prof_end(h);
    int hst[4 + FH_MAX_LD];
    FH_CHECK(hipMemcpyAsync(hst, istate, (4 + ld) * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    FH_CHECK(hipStreamSynchronize(h->stream));
    int r = hst[2] ? hst[1] : hst[0];
    if (r < 0) r = 0;
    if (r > m) r = m;
    *rank = r;
    fh_launch_gather_cols(X, istate + 4, r, N, ld, Out, h->stream);
    *res = Out;
    fh_ortho_note(h, FEASTHIP_ORTHO_MGS, 0, fell_back, r, hst + 4, nullptr);
    return 0;
}

// m > 64: block Gram-Schmidt over 64-column panels.  Panel j is projected twice against the kept
// columns (C = K^H X_j on the MFMA Gram kernel, X_j -= K C), then orthonormalised by fh_ortho_panel
// with the rank threshold tied to the largest column norm of the WHOLE matrix -- the R_11 of the
// reference's pivoted QR (src/core/feast_aux.jl:113-124).  Kept columns are packed to the front of
// Q.  Pivoting is per panel, not global: for a full-rank input the basis spans the same space.
static int fh_ortho_wide(feasthip_ctx* h, int m, cplx* dQ, double rank_tol, int* rank) {
    const int N = (int)fh_N(h), ld = FH_MAX_LD;
    const size_t panel = (size_t)N * ld;
    int rc;
    cplx *X, *Out, *K, *T, *gw, *C, *part, *ddots;
    if ((rc = fh_buf(h, "or_X", panel, &X))) return rc;
    if ((rc = fh_buf(h, "or_out", panel, &Out))) return rc;
    if ((rc = fh_buf(h, "ow_K", panel, &K))) return rc;
    if ((rc = fh_buf(h, "ow_T", panel, &T))) return rc;
    if ((rc = fh_buf(h, "gram_work", fh_gram_work_elems(ld), &gw))) return rc;
    if ((rc = fh_buf(h, "ow_C", (size_t)ld * ld, &C))) return rc;
    if ((rc = fh_buf(h, "ow_part", (size_t)fh_vec_nblk(N, ld) * ld, &part))) return rc;
    if ((rc = fh_buf(h, "ow_dots", (size_t)ld, &ddots))) return rc;
    std::vector<cplx> ones(ld, cmake(1, 0));
    cplx* done;
    if ((rc = fh_upload_coefs(h, "ow_one", ones, &done))) return rc;
    const int npan = (m + ld - 1) / ld;
    // largest column norm of the whole matrix
    double ref = 0.0;
    std::vector<cplx> dots(ld);
    for (int j = 0; j < npan; ++j) {
        const int mj = std::min(ld, m - j * ld);
        fh_launch_to_panel(dQ + (size_t)j * ld * N, N, N, mj, X, ld, h->stream, fh_perm(h));
        fh_launch_dot_cols(X, X, N, ld, part, ddots, h->stream);
        FH_CHECK(hipMemcpyAsync(dots.data(), ddots, ld * sizeof(cplx), hipMemcpyDeviceToHost, h->stream));
        FH_CHECK(hipStreamSynchronize(h->stream));
        for (int c = 0; c < mj; ++c) if (dots[c].x > ref * ref) ref = std::sqrt(dots[c].x);
    }
    int kept = 0;
    for (int j = 0; j < npan; ++j) {
        const int mj = std::min(ld, m - j * ld);
        fh_launch_to_panel(dQ + (size_t)j * ld * N, N, N, mj, X, ld, h->stream, fh_perm(h));
        for (int pass = 0; pass < 2; ++pass) {
            for (int k0 = 0; k0 < kept; k0 += ld) {
                const int kw = std::min(ld, kept - k0);
                fh_launch_to_panel(dQ + (size_t)k0 * N, N, N, kw, K, ld, h->stream, fh_perm(h));
                fh_prof_begin(h, "gram");
                fh_launch_gram(K, X, N, ld, 0, gw, C, h->stream);        // C = K^H X
                fh_prof_end(h);
                fh_prof_begin(h, "ortho");
                fh_launch_small_matmul(K, C, N, ld, T, h->stream);       // T = K C
                fh_launch_axpy_cols(X, T, done, N, ld, h->stream);       // X -= T
                fh_prof_end(h);
            }
        }
        int rj = 0;
        cplx* res = nullptr;
        if ((rc = fh_ortho_panel(h, mj, ld, X, Out, rank_tol, ref, m, &rj, &res))) return rc;
        if (rj > 0) fh_launch_from_panel(res, ld, N, rj, dQ + (size_t)kept * N, N, h->stream, fh_perm(h));
        kept += rj;
    }
    *rank = kept;
    FH_CHECK(hipStreamSynchronize(h->stream));
    return 0;
}

// the body of feasthip_orthonormalize_dev / feasthip_poly_orthonormalize_dev once the handle and m are checked
static int fh_orthonormalize_checked(feasthip_ctx* h, int64_t m64, void* dQ, double rank_tol, int* rank) {
    int rc;
    FH_CHECK(hipSetDevice(h->device));
    fh_ortho_note_reset(h);
    if (m64 > FH_MAX_LD) {
        rc = fh_ortho_wide(h, (int)m64, (cplx*)dQ, rank_tol, rank);
        fh_prof_collect(h);
        return rc;
    }
    const int m = (int)m64, ld = fh_pick_ld(m), N = (int)fh_N(h);
    const size_t panel = (size_t)N * ld;
    cplx *X, *Out;
    if ((rc = fh_buf(h, "or_X", panel, &X))) return rc;
    if ((rc = fh_buf(h, "or_out", panel, &Out))) return rc;
    fh_launch_to_panel((const cplx*)dQ, N, N, m, X, ld, h->stream, fh_perm(h));
    cplx* res = nullptr;
    if ((rc = fh_ortho_panel(h, m, ld, X, Out, rank_tol, 0.0, m, rank, &res))) return rc;
    fh_launch_from_panel(res, ld, N, m, (cplx*)dQ, N, h->stream, fh_perm(h));
    return fh_finish(h);
}

extern "C" int feasthip_orthonormalize_dev(feasthip_handle h, int64_t m64, void* dQ, double rank_tol, int* rank) {
    int rc = fh_check_problem(h, m64, 1);
    if (rc) return rc;
    if (!dQ || !rank) { h->last_error = "orthonormalize: null argument"; return FEASTHIP_ERROR_INTERNAL; }
    return fh_orthonormalize_checked(h, m64, dQ, rank_tol, rank);
}

// The same orthonormalisation for the N x m panels of a polynomial handle (the projected method's subspace lives in the
// N-dimensional space; feasthip_orthonormalize_dev keeps refusing such a handle, like every pencil entry point).
// unit_columns: every column is scaled to unit length first (a column of zero length is left alone), so that the rank rule
// measures directions, not the lengths the contour sum happened to give them.
extern "C" int feasthip_poly_orthonormalize_dev(feasthip_handle h, int64_t m64, void* dQ, int unit_columns, double rank_tol, int* rank) {
    if (int gate = fh_gate(h)) return gate;
    if (h->kind == FH_KIND_OPERATOR) { h->last_error = "feasthip_poly_orthonormalize_dev: an operator handle (feasthip_set_operator) has no polynomial form: it takes feasthip_orthonormalize_dev and the other pencil entry points, under the Krylov solvers FEASTHIP_SOLVER_BICGSTAB, _COCG or _GMRES"; return FEASTHIP_ERROR_FPM; }
    if (h->kind != FH_KIND_POLYNOMIAL && h->kind != FH_KIND_TERM_OPERATOR) { h->last_error = "feasthip_poly_orthonormalize_dev: needs a polynomial handle (feasthip_set_polynomial); a dense or CSR handle takes feasthip_orthonormalize_dev"; return FEASTHIP_ERROR_FPM; }
    if (m64 <= 0 || m64 > fh_N(h)) { h->last_error = "feasthip_poly_orthonormalize_dev: block width m must satisfy 1 <= m <= N"; return FEASTHIP_ERROR_M0; }
    if (!dQ || !rank) { h->last_error = "feasthip_poly_orthonormalize_dev: null argument"; return FEASTHIP_ERROR_INTERNAL; }
    if (unit_columns) {
        FH_CHECK(hipSetDevice(h->device));
        const int N = (int)fh_N(h);
        int rc;
        for (int64_t c0 = 0; c0 < m64; c0 += FH_MAX_LD) {
            const int m = (int)std::min<int64_t>(FH_MAX_LD, m64 - c0), ld = fh_pick_ld(m);
            cplx *X, *part, *ddots;
            if ((rc = fh_buf(h, "po_X", (size_t)N * ld, &X))) return rc;
            if ((rc = fh_buf(h, "po_part", (size_t)fh_vec_nblk(N, ld) * ld, &part))) return rc;
            if ((rc = fh_buf(h, "po_dots", (size_t)ld, &ddots))) return rc;
            fh_launch_to_panel((cplx*)dQ + (size_t)c0 * N, N, N, m, X, ld, h->stream);
            fh_launch_dot_cols(X, X, N, ld, part, ddots, h->stream);
            fh_launch_normalize_cols(X, ddots, N, ld, m, h->stream);
            fh_launch_from_panel(X, ld, N, m, (cplx*)dQ + (size_t)c0 * N, N, h->stream);
        }
    }
    return fh_orthonormalize_checked(h, m64, dQ, rank_tol, rank);
}

extern "C" int feasthip_orthonormalize(feasthip_handle h, int64_t m, void* Q, double rank_tol, int* rank) {
    int rc = fh_check_problem(h, m, 1);
    if (rc) return rc;
    if (!Q || !rank) { h->last_error = "orthonormalize: null argument"; return FEASTHIP_ERROR_INTERNAL; }
    FH_CHECK(hipSetDevice(h->device));
    const size_t nb = (size_t)fh_N(h) * m * sizeof(cplx);
    void* dQ;
    if ((rc = fh_stage_in(h, "host_Q", Q, nb, &dQ))) return rc;
    rc = feasthip_orthonormalize_dev(h, m, dQ, rank_tol, rank);
    if (rc) return rc;
    FH_CHECK(hipMemcpy(Q, dQ, nb, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int feasthip_set_ortho_method(feasthip_handle h, int method) {
    if (!h) return FEASTHIP_ERROR_INTERNAL;
    if (method != FEASTHIP_ORTHO_MGS && method != FEASTHIP_ORTHO_CHOLQR_RR) {
        h->last_error = "set_ortho_method: unknown method";
        return FEASTHIP_ERROR_FPM;
    }
    h->ortho_method = method;
    return 0;
}

extern "C" int feasthip_last_ortho(feasthip_handle h, int* method_used, int* stages, int* fell_back, int* rank, int* perm,
                                   double* rdiag, int n) {
    if (!h) return FEASTHIP_ERROR_INTERNAL;
    const auto& o = h->ortho_last;
    if (method_used) *method_used = o.used;
    if (stages) *stages = o.stages;
    if (fell_back) *fell_back = o.fell_back;
    if (rank) *rank = o.rank;
    for (int k = 0; k < n; ++k) {
        if (perm) perm[k] = k < (int)o.perm.size() ? o.perm[k] : -1;
        if (rdiag) rdiag[k] = k < (int)o.rdiag.size() ? o.rdiag[k] : 0.0;
    }
    return 0;
}
