// fh_ritz.hip -- the Rayleigh-Ritz step: the projections, the Ritz back-transform with its residuals, the same two on the
// resident panels, and the whole step with the reduced eigenproblem on the device.
#include "fh_host.hpp"
#include "fh_kernels.hpp"
#include "fh_dense.hpp"
#include "fh_eig.hpp"
#include "fh_cholqr.hpp"
#include "fh_knobs.hpp"

// ---------------------------------------------------------------------------------------
// Rayleigh-Ritz projection (a10)
// ---------------------------------------------------------------------------------------
// While it lives the handle applies the forward operator whatever feasthip_set_adjoint says (the projections are defined
// with A and B themselves); the switch is put back on every return path.
struct fh_forward_scope {
    feasthip_ctx* h; int was;
    explicit fh_forward_scope(feasthip_ctx* h_) : h(h_), was(h_->adjoint) { h->adjoint = 0; }
    ~fh_forward_scope() { h->adjoint = was; }
};

// What one operator-Gram step works with: the product panel W, the Gram kernel's workspace and the unit / zero coefficient
// vectors that select A or B in the operator kernel.  The projections and the resident reduce share them by name.
struct fh_op_gram {
    feasthip_ctx* h; int ld;
    cplx *W, *gw, *d1, *d0;
    int acquire(feasthip_ctx* h_, int ld_) {
        h = h_; ld = ld_;
        int rc;
        if ((rc = fh_buf(h, "pj_W", (size_t)fh_N(h) * ld, &W))) return rc;
        if ((rc = fh_buf(h, "gram_work", fh_gram_work_elems(ld), &gw))) return rc;
        const std::vector<cplx> one(ld, cmake(1, 0)), zero(ld, cmake(0, 0));
        if ((rc = fh_upload_coefs(h, "pj_one", one, &d1))) return rc;
        return fh_upload_coefs(h, "pj_zero", zero, &d0);
    }
    // queues W = op X on the first m columns, op = A (which 0) or B (which 1)
    int product(int m, const cplx* X, int which) const {
        fh_op_call oc;
        oc.m = m;
        oc.X = X; oc.Y = W;
        oc.coefA = which == 0 ? d1 : d0; oc.coefB = which == 0 ? d0 : d1; oc.skip = which == 0 ? 2 : 1;
        return fh_apply_operator(h, ld, oc) < 0 ? (int)FEASTHIP_ERROR_INTERNAL : 0;
    }
    // queues G = QL^H W (bilinear: QL^T W) as one launch of the "gram" profile class
    void gram(const cplx* QL, int bilinear, cplx* G) const {
        fh_prof_begin(h, "gram");
        fh_launch_gram(QL, W, (int)fh_N(h), ld, bilinear, gw, G, h->stream);
        fh_prof_end(h);
    }
    // the whole step, G = QL^H (op X): nothing is synchronised or downloaded; the operator's error code comes back
    int step(int m, const cplx* QL, const cplx* X, int which, int bilinear, cplx* G) const {
        const int rc = product(m, X, which);
        if (!rc) gram(QL, bilinear, G);
        return rc;
    }
};

// out (r x r column-major, host) = the leading r x r block of Gsrc (host, leading dimension ld), scaled by 1 / (d_i d_j) when
// d != null, its Hermitian part when asked
static void fh_gram_to_host(const cplx* Gsrc, int ld, int r, const double* d, bool hermitian, cplx* out) {
    for (int j = 0; j < r; ++j)
        for (int i = 0; i < r; ++i) {
            cplx g = Gsrc[(size_t)j * ld + i];
            if (d) g = cscale(g, 1.0 / (d[i] * d[j]));
            out[(size_t)j * r + i] = g;
        }
    if (hermitian) fh_cholqr::hermitian_part(out, r);
}
// out = I exactly: the B-part of an orthonormal basis when B = I (src/dense/feast_dense.jl:255-259)
static void fh_identity_to_host(int r, cplx* out) {
    for (int j = 0; j < r; ++j)
        for (int i = 0; i < r; ++i) out[(size_t)j * r + i] = cmake(i == j ? 1.0 : 0.0, 0.0);
}

// res = Q_L^H op Q_R (bilinear: Q_L^T) for op = A (which 0) or B (which 1), r x r column-major on the host, by ld-column
// panels: block (i, j) is Q_L,i^H (op Q_R,j), one operator product (fh_op_gram::product) per block column and one Gram
// launch per block.  One download and one stream synchronisation per block: a single one for r <= ld, (r / 64)^2 of them
// for the wide calls.
static int fh_project_blocks(feasthip_ctx* h, int r, int ld, const cplx* dQL, const cplx* dQR, int which, int bilinear, cplx* res) {
    const int N = (int)fh_N(h);
    const size_t panel = (size_t)N * ld;
    int rc;
    cplx *Qi, *Qj, *G;
    fh_op_gram og;
    if ((rc = fh_buf(h, "pj_Q", panel, &Qi))) return rc;
    if ((rc = fh_buf(h, "pj_Qj", panel, &Qj))) return rc;
    if ((rc = fh_buf(h, "gram_G", (size_t)ld * ld, &G))) return rc;
    if ((rc = og.acquire(h, ld))) return rc;
    const int npan = (r + ld - 1) / ld;
    std::vector<cplx> Gh((size_t)ld * ld);
    for (int j = 0; j < npan; ++j) {
        const int mj = std::min(ld, r - j * ld);
        fh_launch_to_panel(dQR + (size_t)j * ld * N, N, N, mj, Qj, ld, h->stream, fh_perm(h));
        if ((rc = og.product(mj, Qj, which))) return rc;
        for (int i = 0; i < npan; ++i) {
            const int mi = std::min(ld, r - i * ld);
            fh_launch_to_panel(dQL + (size_t)i * ld * N, N, N, mi, Qi, ld, h->stream, fh_perm(h));
            og.gram(Qi, bilinear, G);
            FH_CHECK(hipMemcpyAsync(Gh.data(), G, Gh.size() * sizeof(cplx), hipMemcpyDeviceToHost, h->stream));
            FH_CHECK(hipStreamSynchronize(h->stream));
            for (int c2 = 0; c2 < mj; ++c2)
                for (int c1 = 0; c1 < mi; ++c1)
                    res[(size_t)(j * ld + c2) * r + i * ld + c1] = Gh[(size_t)c2 * ld + c1];
        }
    }
    return 0;
}

extern "C" int feasthip_project_dev(feasthip_handle h, int64_t r64, const void* dQ, int bilinear, int hermitize,
                                    void* Aq_host, void* Bq_host) {
    const bool wide = r64 > FH_MAX_LD;                  // r > 64: 64-column panels (fh_project_blocks)
    int rc = fh_check_problem(h, r64, wide);
    if (rc) return rc;
    if (!dQ || !Aq_host) { h->last_error = "project: null argument"; return FEASTHIP_ERROR_INTERNAL; }
    FH_CHECK(hipSetDevice(h->device));
    fh_forward_scope forward(h);
    const int r = (int)r64, N = (int)fh_N(h);
    const int ld = wide ? r : fh_pick_ld(r);            // leading dimension of the Gram data on the host
    const size_t g2 = (size_t)ld * ld;
    cplx* const out_host[2] = {(cplx*)Aq_host, (cplx*)Bq_host};
    // variant A: Q is orthonormal and B = I, so Bq = I exactly and no product is formed for it
    // (B = I without orthonormal Q, variant C: the operator kernel yields W = Q, so G = Q^H Q)
    const bool b_exact = fh_b_identity(h) && hermitize && !bilinear;
    auto produced = [&](int which) { return out_host[which] && !(which == 1 && b_exact); };
    std::vector<cplx> Gh(2 * g2);
    if (wide) {
        for (int which = 0; which < 2; ++which)
            if (produced(which) && (rc = fh_project_blocks(h, r, FH_MAX_LD, (const cplx*)dQ, (const cplx*)dQ, which, bilinear,
                                                           Gh.data() + which * g2))) return rc;
    } else {
        cplx *Qp, *G;
        fh_op_gram og;
        if ((rc = fh_buf(h, "pj_Q", (size_t)N * ld, &Qp))) return rc;
        fh_launch_to_panel((const cplx*)dQ, N, N, r, Qp, ld, h->stream, fh_perm(h));
        if ((rc = og.acquire(h, ld))) return rc;
        // both Gram matrices are queued before the ONE synchronisation that brings them to the host
        if ((rc = fh_buf(h, "gram_G2", 2 * g2, &G))) return rc;
        for (int which = 0; which < 2; ++which) {
            if (!produced(which)) continue;
            if ((rc = og.step(r, Qp, Qp, which, bilinear, G + which * g2))) return rc;
            FH_CHECK(hipMemcpyAsync(Gh.data() + which * g2, G + which * g2, g2 * sizeof(cplx), hipMemcpyDeviceToHost, h->stream));
        }
        FH_CHECK(hipStreamSynchronize(h->stream));
    }
    for (int which = 0; which < 2; ++which) {
        if (!out_host[which]) continue;
        if (produced(which)) fh_gram_to_host(Gh.data() + which * g2, ld, r, nullptr, hermitize && !bilinear, out_host[which]);
        else fh_identity_to_host(r, out_host[which]);
    }
    fh_prof_collect(h);
    FH_CHECK(hipGetLastError());       // launch-configuration errors do not surface through the stream sync
    return 0;
}

extern "C" int feasthip_project(feasthip_handle h, int64_t r, const void* Q, int bilinear, int hermitize, void* Aq, void* Bq) {
    int rc = fh_check_problem(h, r, 1);
    if (rc) return rc;
    if (!Q) { h->last_error = "project: null Q"; return FEASTHIP_ERROR_INTERNAL; }
    FH_CHECK(hipSetDevice(h->device));
    void* dQ;
    if ((rc = fh_stage_in(h, "host_Q", Q, (size_t)fh_N(h) * r * sizeof(cplx), &dQ))) return rc;
    return feasthip_project_dev(h, r, dQ, bilinear, hermitize, Aq, Bq);
}

// Oblique projection of the two-sided method: Aq = Q_L^H A Q_R, Bq = Q_L^H B Q_R (Q_L^H Q_R for B = I), raw products
// (fh_project_blocks).  Forward operator whatever the adjoint switch says.
extern "C" int feasthip_project_pair_dev(feasthip_handle h, int64_t r64, const void* dQL, const void* dQR, void* Aq_host, void* Bq_host) {
    int rc = fh_check_problem(h, r64, 1);
    if (rc) return rc;
    if (!dQL || !dQR || !Aq_host) { h->last_error = "project_pair: null argument"; return FEASTHIP_ERROR_INTERNAL; }
    FH_CHECK(hipSetDevice(h->device));
    fh_forward_scope forward(h);
    const int r = (int)r64, ld = r > FH_MAX_LD ? FH_MAX_LD : fh_pick_ld(r);
    for (int which = 0; which < 2; ++which) {
        cplx* out_host = (cplx*)(which == 0 ? Aq_host : Bq_host);
        if (out_host && (rc = fh_project_blocks(h, r, ld, (const cplx*)dQL, (const cplx*)dQR, which, 0, out_host))) return rc;
    }
    fh_prof_collect(h);
    FH_CHECK(hipGetLastError());       // launch-configuration errors do not surface through the stream sync
    return 0;
}

extern "C" int feasthip_project_pair(feasthip_handle h, int64_t r, const void* QL, const void* QR, void* Aq, void* Bq) {
    int rc = fh_check_problem(h, r, 1);
    if (rc) return rc;
    if (!QL || !QR || !Aq) { h->last_error = "project_pair: null argument"; return FEASTHIP_ERROR_INTERNAL; }
    FH_CHECK(hipSetDevice(h->device));
    const size_t nb = (size_t)fh_N(h) * r * sizeof(cplx);
    void *dL, *dR;
    if ((rc = fh_stage_in(h, "host_Q", QL, nb, &dL))) return rc;
    if ((rc = fh_stage_in(h, "host_X", QR, nb, &dR))) return rc;
    return feasthip_project_pair_dev(h, r, dL, dR, Aq, Bq);
}

// ---------------------------------------------------------------------------------------
// Ritz back-transform + residual (a12, a13)
// ---------------------------------------------------------------------------------------
// R = A X - B X diag(lambda) on the first ncols columns of an ld-wide panel -- A X - X diag(lambda) when use_B = 0 and B != I
// (RCI-style residual, src/kernel/feast_kernel.jl:899-906); lambda holds (re, im) pairs.  With dots != null the squared
// column norms are queued into the pinned ring as well: *dots is valid after the caller's next stream synchronisation
// (fh_residual_norms).  No synchronisation of its own.
static int fh_panel_residual(feasthip_ctx* h, int ld, int ncols, const cplx* X, cplx* R, const double* lambda, int use_B,
                             cplx* part, cplx* ddots, const cplx** dots, std::vector<char>& fallback) {
    const int N = (int)fh_N(h);
    const bool lam_in_op = use_B || fh_b_identity(h);
    std::vector<cplx> ca(ld, cmake(1, 0)), cb(ld, cmake(0, 0));
    for (int c = 0; c < ncols; ++c) cb[c] = lam_in_op ? cmake(-lambda[2 * c], -lambda[2 * c + 1]) : cmake(0, 0);
    int rc;
    cplx *dca, *dcb;
    if ((rc = fh_upload_coefs(h, "rz_coefA", ca, &dca))) return rc;
    if ((rc = fh_upload_coefs(h, "rz_coefB", cb, &dcb))) return rc;
    fh_op_call oc;
    oc.m = ncols;
    oc.X = X; oc.Y = R; oc.coefA = dca; oc.coefB = dcb; oc.skip = lam_in_op ? 0 : 2;
    if (fh_apply_operator(h, ld, oc) < 0) return FEASTHIP_ERROR_INTERNAL;
    if (!lam_in_op) {
        std::vector<cplx> lam(ld, cmake(0, 0));
        for (int c = 0; c < ncols; ++c) lam[c] = cmake(lambda[2 * c], lambda[2 * c + 1]);
        cplx* dl;
        if ((rc = fh_upload_coefs(h, "rz_lam", lam, &dl))) return rc;
        fh_launch_axpy_cols(R, X, dl, N, ld, h->stream);   // R -= X diag(lam)
    }
    if (!dots) return 0;
    fh_launch_dot_cols(R, R, N, ld, part, ddots, h->stream);
    const void* slot = nullptr;
    if ((rc = fh_download_small(h, ddots, ld * sizeof(cplx), &slot, fallback))) return rc;
    *dots = (const cplx*)slot;
    return 0;
}

// res_j = ||R_j|| / max(|lambda_j|, 1), j < M, from the squared norms of fh_panel_residual
static void fh_residual_norms(const cplx* dots, const double* lambda, int M, double* res) {
    for (int c = 0; c < M; ++c) {
        const double la = std::hypot(lambda[2 * c], lambda[2 * c + 1]);
        res[c] = std::sqrt(dots[c].x) / std::max(la, 1.0);
    }
}

// The rz_* workspace of the Ritz back-transform X = Q V and its residual.  staged: the caller's column-major Q and X go
// through panels of their own (rz_Q, rz_X, rz_R; the resident loop has its panels already); wide: the r > 64 path sums its
// block products through rz_T.
struct fh_ritz_ws {
    cplx *Qp = nullptr, *Xp = nullptr, *Rp = nullptr, *Tp = nullptr, *dV = nullptr, *part = nullptr, *ddots = nullptr;
    int acquire(feasthip_ctx* h, int ld, bool staged, bool wide) {
        const int N = (int)fh_N(h);
        const size_t panel = (size_t)N * ld;
        int rc;
        if (staged) {
            if ((rc = fh_buf(h, "rz_Q", panel, &Qp))) return rc;
            if ((rc = fh_buf(h, "rz_X", panel, &Xp))) return rc;
            if ((rc = fh_buf(h, "rz_R", panel, &Rp))) return rc;
        }
        if (wide && (rc = fh_buf(h, "rz_T", panel, &Tp))) return rc;
        if ((rc = fh_buf(h, "rz_V", (size_t)ld * ld, &dV))) return rc;
        if ((rc = fh_buf(h, "rz_part", (size_t)std::max(fh_op_nblk(h, ld), fh_vec_nblk(N, ld)) * ld, &part))) return rc;
        return fh_buf(h, "rz_dots", (size_t)ld, &ddots);
    }
};

extern "C" int feasthip_ritz_residual_dev(feasthip_handle h, int64_t r64, const void* dQ, const void* V_host,
                                          const double* lambda_host, int64_t M, int normalize, int use_B, void* dX,
                                          double* res_host) {
    const bool wide = r64 > FH_MAX_LD;
    int rc = fh_check_adjoint(h, "ritz_residual");
    if (rc) return rc;
    if ((rc = fh_check_problem(h, r64, wide))) return rc;
    if (!dQ || !V_host || !lambda_host || !dX) { h->last_error = "ritz_residual: null argument"; return FEASTHIP_ERROR_INTERNAL; }
    if (M < 0 || M > r64) { h->last_error = "ritz_residual: M out of range"; return FEASTHIP_ERROR_M0; }
    std::vector<double> lam_conj;
    if (h->adjoint) {
        // adjoint residual A^H x - conj(lambda) B^H x: the products are adjoint through fh_apply_operator, the values here
        lam_conj.assign(lambda_host, lambda_host + 2 * (size_t)r64);
        for (size_t c = 0; c < (size_t)r64; ++c) lam_conj[2 * c + 1] = -lam_conj[2 * c + 1];
        lambda_host = lam_conj.data();
    }
    FH_CHECK(hipSetDevice(h->device));
    const int r = (int)r64, ld = wide ? FH_MAX_LD : fh_pick_ld(r), N = (int)fh_N(h);
    fh_ritz_ws ws;
    if ((rc = ws.acquire(h, ld, true, wide))) return rc;
    cplx *Qp = ws.Qp, *Xp = ws.Xp, *Rp = ws.Rp, *dV = ws.dV, *part = ws.part, *ddots = ws.ddots;
    const cplx* Vh = (const cplx*)V_host;
    std::vector<cplx> Vp;
    std::vector<char> dots_fb;
    if (wide) {
        // r > 64: X_j = sum_i Q_i V[i-block, j-block] per 64-column output panel, then the panel
        // goes through the same normalise / residual steps as the narrow path
        if (dQ == dX) { h->last_error = "ritz_residual: X must not alias Q for r > 64"; return FEASTHIP_ERROR_INTERNAL; }
        std::vector<cplx> mones(ld, cmake(-1, 0));
        cplx* dmone;
        if ((rc = fh_upload_coefs(h, "rz_mone", mones, &dmone))) return rc;
        const int npan = (r + ld - 1) / ld;
        std::vector<cplx> dots(ld);
        for (int j = 0; j < npan; ++j) {
            const int mj = std::min(ld, r - j * ld);
            for (int i = 0; i < npan; ++i) {
                const int mi = std::min(ld, r - i * ld);
                fh_pad_block(Vh, r, r, ld, i, j, nullptr, Vp);
                FH_CHECK(hipMemcpyAsync(dV, Vp.data(), Vp.size() * sizeof(cplx), hipMemcpyHostToDevice, h->stream));
                fh_launch_to_panel((const cplx*)dQ + (size_t)i * ld * N, N, N, mi, Qp, ld, h->stream, fh_perm(h));
                fh_prof_begin(h, "ritz");
                if (i == 0) {
                    fh_launch_small_matmul(Qp, dV, N, ld, Xp, h->stream);
                } else {
                    fh_launch_small_matmul(Qp, dV, N, ld, ws.Tp, h->stream);
                    fh_launch_axpy_cols(Xp, ws.Tp, dmone, N, ld, h->stream);    // X += T
                }
                fh_prof_end(h);
                FH_CHECK(hipStreamSynchronize(h->stream));                      // Vp (host) is reused
            }
            const int Mj = std::max(0, std::min(mj, (int)M - j * ld));          // columns of this panel below M
            // (unlike the narrow and resident paths, which normalise on the device with fh_launch_normalize_cols, the norms
            //  make a host round trip here; not folded in: it would change the launches and the synchronisations)
            if (normalize && Mj > 0) {
                fh_launch_dot_cols(Xp, Xp, N, ld, part, ddots, h->stream);
                FH_CHECK(hipMemcpyAsync(dots.data(), ddots, ld * sizeof(cplx), hipMemcpyDeviceToHost, h->stream));
                FH_CHECK(hipStreamSynchronize(h->stream));
                std::vector<cplx> sc(ld, cmake(1, 0));
                for (int c = 0; c < Mj; ++c) {
                    double n = std::sqrt(dots[c].x);
                    if (n > 0) sc[c] = cmake(1.0 / n, 0);
                }
                cplx* dsc;
                if ((rc = fh_upload_coefs(h, "rz_scale", sc, &dsc))) return rc;
                fh_launch_scale_cols(Xp, dsc, N, ld, h->stream);
            }
            fh_launch_from_panel(Xp, ld, N, mj, (cplx*)dX + (size_t)j * ld * N, N, h->stream, fh_perm(h));
            if (Mj > 0 && res_host) {
                const double* lam = lambda_host + 2 * (size_t)j * ld;
                const cplx* rdots = nullptr;
                if ((rc = fh_panel_residual(h, ld, mj, Xp, Rp, lam, use_B, part, ddots, &rdots, dots_fb))) return rc;
                FH_CHECK(hipStreamSynchronize(h->stream));
                fh_residual_norms(rdots, lam, Mj, res_host + (size_t)j * ld);
            }
        }
        FH_CHECK(hipStreamSynchronize(h->stream));
        fh_prof_collect(h);
        return 0;
    }
    fh_pad_block(Vh, r, r, ld, 0, 0, nullptr, Vp);
    FH_CHECK(hipMemcpyAsync(dV, Vp.data(), Vp.size() * sizeof(cplx), hipMemcpyHostToDevice, h->stream));
    fh_launch_to_panel((const cplx*)dQ, N, N, r, Qp, ld, h->stream, fh_perm(h));
    fh_prof_begin(h, "ritz");
    fh_launch_small_matmul(Qp, dV, N, ld, Xp, h->stream);
    fh_prof_end(h);
    if (normalize && M > 0) {
        // normalise the first M columns (src/dense/feast_dense.jl:301-305): norms and scaling stay on the device
        fh_launch_dot_cols(Xp, Xp, N, ld, part, ddots, h->stream);
        fh_launch_normalize_cols(Xp, ddots, N, ld, (int)M, h->stream);
    }
    fh_launch_from_panel(Xp, ld, N, r, (cplx*)dX, N, h->stream, fh_perm(h));
    if (M > 0 && res_host) {
        const cplx* rdots = nullptr;
        if ((rc = fh_panel_residual(h, ld, r, Xp, Rp, lambda_host, use_B, part, ddots, &rdots, dots_fb))) return rc;
        FH_CHECK(hipStreamSynchronize(h->stream));
        fh_residual_norms(rdots, lambda_host, (int)M, res_host);
    }
    return fh_finish(h);
}

extern "C" int feasthip_ritz_residual(feasthip_handle h, int64_t r, const void* Q, const void* V, const double* lambda,
                                      int64_t M, int normalize, int use_B, void* X, double* res) {
    int rc = fh_check_problem(h, r, 1);
    if (rc) return rc;
    if (!Q || !X) { h->last_error = "ritz_residual: null argument"; return FEASTHIP_ERROR_INTERNAL; }
    if ((rc = fh_check_adjoint(h, "ritz_residual"))) return rc;
    FH_CHECK(hipSetDevice(h->device));
    const size_t nb = (size_t)fh_N(h) * r * sizeof(cplx);
    void *dQ, *dX;
    if ((rc = fh_stage_in(h, "host_Q", Q, nb, &dQ))) return rc;
    if ((rc = fh_get_buf(h, "host_X", nb, &dX))) return rc;
    rc = feasthip_ritz_residual_dev(h, r, dQ, V, lambda, M, normalize, use_B, dX, res);
    if (rc) return rc;
    FH_CHECK(hipMemcpy(X, dX, nb, hipMemcpyDeviceToHost));
    return 0;
}

// ---------------------------------------------------------------------------------------
// Resident refinement loop (rows a7, a9-a13 of one FEAST loop without leaving the kernels' panel layout)
//
// The per-primitive entry points above speak column-major at the C ABI, so one loop of variant A crossed the boundary seven
// times (contour_apply in/out, orthonormalize in/out, project in, ritz_residual in/out: k_to_panel / k_from_panel each) and
// synchronised the stream about twenty times (every small host -> device upload).  Here the panels stay where the kernels
// left them:
//   feasthip_contour_apply_resident   (fh_api.hip) Q (imported once, or the Ritz vectors of the previous loop)  ->  Q_proj   [rs_P]
//   feasthip_rr_reduce_resident       rank + the reduced pencil  (Q_o^H A Q_o, Q_o^H B Q_o)  of the orthonormal basis Q_o of Q_proj
//   feasthip_rr_ritz_resident         X = Q_o V, normalise, residuals; X becomes the next loop's Q   [rs_X, rs_R]
//   feasthip_resident_export          column-major copy of X (the converged Ritz vectors, once per solve)
// The orthonormal basis is never formed when Q_proj is well conditioned (the steady state of FEAST): the Rayleigh-Ritz
// pairs of a subspace do not depend on the basis, so the reduced pencil is taken on Q_proj with unit columns -- three Gram
// products (Q^H Q for the test, Q^H A Q, Q^H B Q: fh_op_gram, the step the per-primitive projections use) queued behind ONE
// synchronisation, an O(m^2) scaling on the host (fh_gram_to_host) -- and
// handed to the host's generalized eigensolver, whose Cholesky factorisation of the B-part does what the Cholesky-QR did;
// the Ritz vectors are Q_proj (D^-1 V): one tall product instead of two.  The acceptance test is fh_ortho_panel's own
// (fh_cholqr::accept) and the implicit basis is taken when it decides "one pass"; anything else -- rank deficiency, a ratio
// that needs the second Cholesky-QR pass -- takes fh_ortho_panel itself on the resident panel, so the rank decisions are the
// same as the per-primitive path's.
// The eigen-residual panel A X - B X diag(lambda) the Ritz step forms for its norms is the next sweep's shared start
// residual (fh_contour_apply_panel: shared_src), which saves that sweep's first operator product.
// ---------------------------------------------------------------------------------------
int fh_rs_panels(feasthip_ctx* h, cplx** P, cplx** X, cplx** R) {
    const size_t panel = (size_t)fh_N(h) * FH_MAX_LD;
    int rc;
    if ((rc = fh_buf(h, "rs_P", panel, P))) return rc;
    if ((rc = fh_buf(h, "rs_X", panel, X))) return rc;
    return fh_buf(h, "rs_R", panel, R);
}

extern "C" int feasthip_rr_reduce_resident(feasthip_handle h, int64_t m64, double rank_tol, int hermitize, int* rank,
                                           void* Aq_host, void* Bq_host) {
    int rc = fh_check_problem(h, m64);
    if (rc) return rc;
    if (!rank || !Aq_host || !Bq_host) { h->last_error = "rr_reduce_resident: null argument"; return FEASTHIP_ERROR_INTERNAL; }
    if ((rc = fh_check_adjoint(h, "rr_reduce_resident", "the resident loop has no adjoint form"))) return rc;
    FH_CHECK(hipSetDevice(h->device));
    const int m = (int)m64, N = (int)fh_N(h);
    cplx *Pb, *Xb, *Rb;
    if ((rc = fh_rs_panels(h, &Pb, &Xb, &Rb))) return rc;
    if (h->rs_P != Pb || h->rs_m != m) { h->last_error = "rr_reduce_resident: no resident Q_proj of this width"; return FEASTHIP_ERROR_M0; }
    const int ld = h->rs_ld;
    cplx* P = h->rs_P;
    const size_t g2 = (size_t)ld * ld;
    cplx* G;
    fh_op_gram og;
    if ((rc = og.acquire(h, ld))) return rc;
    if ((rc = fh_buf(h, "gram_G3", 3 * g2, &G))) return rc;
    const bool b_id = fh_b_identity(h);
    // Gram products of `basis`: [0] basis^H basis (want_g0), [1] basis^H A basis, [2] basis^H B basis (B != I); one sync
    const cplx* Gh = nullptr;
    std::vector<char> gh_fallback;
    auto grams = [&](const cplx* basis, bool want_g0) -> int {
        if (want_g0) { fh_prof_begin(h, "gram"); fh_launch_gram(basis, basis, N, ld, 0, og.gw, G, h->stream); fh_prof_end(h); }
        int drc;
        for (int which = 0; which < (b_id ? 1 : 2); ++which)
            if ((drc = og.step(m, basis, basis, which, 0, G + (1 + which) * g2))) return drc;
        const void* slot = nullptr;
        if ((drc = fh_download_small(h, G, 3 * g2 * sizeof(cplx), &slot, gh_fallback))) return drc;
        FH_CHECK(hipStreamSynchronize(h->stream));
        Gh = (const cplx*)slot;
        return 0;
    };
    if ((rc = grams(P, true))) return rc;
    // ---- implicit basis: fh_ortho_panel's acceptance test on the Gram matrix we already have; its one-pass decision (the basis
    //      below is then as good as an orthonormalised one to 1e-14) takes the fast path ----
    std::vector<double> dcol;
    bool fast = false;
    if (!fh_knob::no_cholqr()) {
        std::vector<cplx> G0(Gh, Gh + g2);
        fast = fh_cholqr::accept(G0, m, ld, 0.0, rank_tol, fh_knob::cholqr_two_pass(), dcol) == fh_cholqr::Plan::one_pass;
    }
    if (fast) {
        fh_ortho_note_reset(h);
        std::vector<int> ident(m);
        for (int j = 0; j < m; ++j) ident[j] = j;
        fh_ortho_note(h, FEASTHIP_ORTHO_USED_CHOLQR, 0, 0, m, ident.data(), nullptr);
        // basis = Q_proj D^-1 (unit columns): its pencil is the equilibrated Gram pair; the orthonormal basis is never formed
        fh_gram_to_host(Gh + g2, ld, m, dcol.data(), hermitize, (cplx*)Aq_host);
        fh_gram_to_host(b_id ? Gh : Gh + 2 * g2, ld, m, dcol.data(), hermitize, (cplx*)Bq_host);
        h->rs_basis = P; h->rs_rank = m;
        h->rs_T.assign(m, cmake(1, 0));
        for (int j = 0; j < m; ++j) h->rs_T[j] = cmake(1.0 / dcol[j], 0.0);
        *rank = m;
        fh_prof_collect(h);
        FH_CHECK(hipGetLastError());
        return 0;
    }
    // ---- general path: the rank-revealing orthonormalisation on the resident panel, then the projections of its result ----
    cplx* Out;
    if ((rc = fh_buf(h, "or_out", (size_t)N * FH_MAX_LD, &Out))) return rc;
    cplx* res = nullptr;
    int r = 0;
    fh_ortho_note_reset(h);
    if ((rc = fh_ortho_panel(h, m, ld, P, Out, rank_tol, 0.0, m, &r, &res))) return rc;
    h->rs_P = nullptr;                            // (the orthonormalisation may have overwritten the projection panel)
    *rank = r;
    h->rs_rank = r; h->rs_T.clear(); h->rs_basis = res;
    if (r == 0) { fh_prof_collect(h); return 0; }
    if ((rc = grams(res, false))) return rc;
    fh_gram_to_host(Gh + g2, ld, r, nullptr, hermitize, (cplx*)Aq_host);
    if (b_id) fh_identity_to_host(r, (cplx*)Bq_host);       // orthonormal basis, B = I
    else fh_gram_to_host(Gh + 2 * g2, ld, r, nullptr, hermitize, (cplx*)Bq_host);
    fh_prof_collect(h);
    FH_CHECK(hipGetLastError());
    return 0;
}

extern "C" int feasthip_rr_ritz_resident(feasthip_handle h, int64_t r64, const void* V_host, const double* lambda_host, int64_t M,
                                         int normalize, int use_B, double* res_host) {
    int rc = fh_check_problem(h, r64);
    if (rc) return rc;
    if (!V_host || !lambda_host) { h->last_error = "rr_ritz_resident: null argument"; return FEASTHIP_ERROR_INTERNAL; }
    if ((rc = fh_check_adjoint(h, "rr_ritz_resident", "the resident loop has no adjoint form"))) return rc;
    if (M < 0 || M > r64) { h->last_error = "rr_ritz_resident: M out of range"; return FEASTHIP_ERROR_M0; }
    FH_CHECK(hipSetDevice(h->device));
    const int r = (int)r64, N = (int)fh_N(h);
    cplx *Pb, *Xp, *Rp;
    if ((rc = fh_rs_panels(h, &Pb, &Xp, &Rp))) return rc;
    if (!h->rs_basis || h->rs_rank != r) { h->last_error = "rr_ritz_resident: run rr_reduce_resident first (rank mismatch)"; return FEASTHIP_ERROR_M0; }
    const int ld = h->rs_ld;
    fh_ritz_ws ws;
    if ((rc = ws.acquire(h, ld, false, false))) return rc;
    cplx *dV = ws.dV, *part = ws.part, *ddots = ws.ddots;
    // V padded to ld x ld; the implicit basis is Q_proj D^-1, so X = Q_proj (D^-1 V)
    std::vector<cplx> Vp;
    fh_pad_block((const cplx*)V_host, r, r, ld, 0, 0, h->rs_T.empty() ? nullptr : h->rs_T.data(), Vp);
    if ((rc = fh_upload_small(h, dV, Vp.data(), Vp.size() * sizeof(cplx)))) return rc;
    h->rs_X = nullptr; h->rs_R = nullptr;
    fh_prof_begin(h, "ritz");
    fh_launch_small_matmul(h->rs_basis, dV, N, ld, Xp, h->stream);
    fh_prof_end(h);
    if (normalize && M > 0) {
        fh_launch_dot_cols(Xp, Xp, N, ld, part, ddots, h->stream);
        fh_launch_normalize_cols(Xp, ddots, N, ld, (int)M, h->stream);
    }
    // R for all r columns (the next sweep's start residual); its column norms only when asked for
    const cplx* dots_h = nullptr;
    std::vector<char> dots_fb;
    const bool want_res = M > 0 && res_host;
    if ((rc = fh_panel_residual(h, ld, r, Xp, Rp, lambda_host, use_B, part, ddots, want_res ? &dots_h : nullptr, dots_fb))) return rc;
    // the rank dropped below the panel's padded width (64 -> 32 / 16 columns): the next sweep works on the narrower panel
    int ldx = ld;
    if (fh_pick_ld(r) < ld) {
        ldx = fh_pick_ld(r);
        cplx* tmp;
        if ((rc = fh_buf(h, "rs_tmp", (size_t)N * FH_MAX_LD, &tmp))) return rc;
        for (cplx* pan : {Xp, Rp}) {
            fh_launch_panel_cols(pan, ld, 0, r, N, tmp, ldx, h->stream);
            FH_CHECK(hipMemcpyAsync(pan, tmp, (size_t)N * ldx * sizeof(cplx), hipMemcpyDeviceToDevice, h->stream));
        }
    }
    FH_CHECK(hipStreamSynchronize(h->stream));
    if (want_res) fh_residual_norms(dots_h, lambda_host, (int)M, res_host);
    h->rs_X = Xp; h->rs_X_m = r; h->rs_X_ld = ldx;
    h->rs_R_lambda.assign(ld, cmake(0, 0));
    if (use_B || fh_b_identity(h)) {                  // the start residual of the sweeps is the one WITH B
        for (int c = 0; c < r; ++c) h->rs_R_lambda[c] = cmake(lambda_host[2 * c], lambda_host[2 * c + 1]);
        h->rs_R = Rp;
    }
    fh_prof_collect(h);
    FH_CHECK(hipGetLastError());
    return 0;
}

extern "C" int feasthip_resident_export(feasthip_handle h, int which, int64_t ncols, void* dX) {
    if (int gate = fh_gate(h)) return gate;
    if (!dX) { h->last_error = "resident_export: null destination"; return FEASTHIP_ERROR_INTERNAL; }
    if (h->kind == FH_KIND_POLYNOMIAL) { h->last_error = "resident_export: a polynomial handle has no resident panels (use the feasthip_poly_* calls)"; return FEASTHIP_ERROR_FPM; }
    const cplx* src = which == 0 ? h->rs_X : h->rs_P;
    const int have = which == 0 ? h->rs_X_m : h->rs_m, ld = which == 0 ? h->rs_X_ld : h->rs_ld;
    if (!src || ncols < 0 || ncols > have) { h->last_error = "resident_export: no such resident panel / too many columns"; return FEASTHIP_ERROR_M0; }
    FH_CHECK(hipSetDevice(h->device));
    const int N = (int)fh_N(h);
    if (ncols > 0) fh_launch_from_panel(src, ld, N, (int)ncols, (cplx*)dX, N, h->stream, fh_perm(h));
    FH_CHECK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int feasthip_resident_import(feasthip_handle h, int which, int64_t ncols, const void* dX) {
    int rc = fh_check_problem(h, ncols);
    if (rc) return rc;
    if (!dX) { h->last_error = "resident_import: null source"; return FEASTHIP_ERROR_INTERNAL; }
    FH_CHECK(hipSetDevice(h->device));
    const int m = (int)ncols, ld = fh_pick_ld(m), N = (int)fh_N(h);
    cplx *P, *X, *R;
    if ((rc = fh_rs_panels(h, &P, &X, &R))) return rc;
    fh_launch_to_panel((const cplx*)dX, N, N, m, which == 0 ? X : P, ld, h->stream, fh_perm(h));
    FH_CHECK(hipStreamSynchronize(h->stream));
    if (which == 0) { h->rs_X = X; h->rs_X_m = m; h->rs_X_ld = ld; h->rs_R = nullptr; h->rs_R_lambda.clear(); }
    else { h->rs_P = P; h->rs_m = m; h->rs_ld = ld; h->rs_basis = nullptr; h->rs_T.clear(); h->rs_rank = 0; }
    return 0;
}

// Rayleigh-Ritz step with the reduced eigenproblem on the device: project,
// Jacobi eigensolver (fh_eig.hip) instead of host ZHEGV, stable inside-first reorder for [Emin, Emax]
// (src/core/feast_aux.jl:144-197), X = Q V, normalise the inside columns, residuals.  The host sees
// lambda[r] (reordered), M and res[M] only.  FEASTHIP_ERROR_LAPACK: the reduced B matrix is not
// positive definite -- the caller falls back to project + host eigen + ritz_residual
// (the general fallback of src/dense/feast_dense.jl:276-284).
extern "C" int feasthip_rayleigh_ritz_dev(feasthip_handle h, int64_t r64, const void* dQ, double Emin, double Emax,
                                          int use_B, void* dX, double* lambda_out, int* M_out, double* res_out) {
    int rc = fh_check_problem(h, r64);
    if (rc) return rc;
    if (!dQ || !dX || !lambda_out || !M_out) { h->last_error = "rayleigh_ritz: null argument"; return FEASTHIP_ERROR_INTERNAL; }
    if ((rc = fh_check_adjoint(h, "rayleigh_ritz", "the Hermitian reduced eigensolver has no two-sided form"))) return rc;
    const int r = (int)r64, ld = FH_MAX_LD;
    std::vector<cplx> Sq((size_t)r * r), Aq((size_t)r * r);
    if ((rc = feasthip_project_dev(h, r64, dQ, 0, 1, Sq.data(), Aq.data()))) return rc;
    bool a_identity = fh_b_identity(h) != 0;                 // project returned exactly I
    cplx *dS, *dA, *dV;
    double* dlam;
    int* dflags;
    void* scratch;                               // (laid out by the kernel: sized in bytes)
    if ((rc = fh_buf(h, "rr_S", (size_t)ld * ld, &dS))) return rc;
    if ((rc = fh_buf(h, "rr_A", (size_t)ld * ld, &dA))) return rc;
    if ((rc = fh_buf(h, "rr_V", (size_t)ld * ld, &dV))) return rc;
    if ((rc = fh_buf(h, "rr_lam", ld, &dlam))) return rc;
    if ((rc = fh_buf(h, "rr_flags", 4, &dflags))) return rc;
    if ((rc = fh_get_buf(h, "rr_scratch", fh_herm_eig_scratch_bytes(), &scratch))) return rc;
    std::vector<cplx> pad((size_t)ld * ld, cmake(0, 0));
    for (int j = 0; j < r; ++j) for (int i = 0; i < r; ++i) pad[(size_t)j * ld + i] = Sq[(size_t)j * r + i];
    FH_CHECK(hipMemcpyAsync(dS, pad.data(), pad.size() * sizeof(cplx), hipMemcpyHostToDevice, h->stream));
    FH_CHECK(hipStreamSynchronize(h->stream));
    if (!a_identity) {
        for (int j = 0; j < r; ++j) for (int i = 0; i < r; ++i) pad[(size_t)j * ld + i] = Aq[(size_t)j * r + i];
        FH_CHECK(hipMemcpyAsync(dA, pad.data(), pad.size() * sizeof(cplx), hipMemcpyHostToDevice, h->stream));
        FH_CHECK(hipStreamSynchronize(h->stream));
    }
    fh_prof_begin(h, "reduced_eig");
    fh_launch_herm_eig(r, ld, dS, a_identity ? nullptr : dA, scratch, dlam, dV, dflags, h->stream);
    fh_prof_end(h);
    std::vector<double> lam(r);
    std::vector<cplx> V((size_t)ld * ld);
    int flags[4];
    FH_CHECK(hipMemcpyAsync(flags, dflags, sizeof(flags), hipMemcpyDeviceToHost, h->stream));
    FH_CHECK(hipMemcpyAsync(lam.data(), dlam, r * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    FH_CHECK(hipMemcpyAsync(V.data(), dV, V.size() * sizeof(cplx), hipMemcpyDeviceToHost, h->stream));
    FH_CHECK(hipStreamSynchronize(h->stream));
    if (fh_knob::debug_timing()) fprintf(stderr, "[rayleigh_ritz] r=%d jacobi sweeps=%d\n", r, flags[3]);
    if (flags[0] || flags[2]) { h->last_error = "rayleigh_ritz: reduced B matrix not positive definite"; return FEASTHIP_ERROR_LAPACK; }
    // stable inside-first permutation
    std::vector<int> perm;
    for (int i = 0; i < r; ++i) if (lam[i] >= Emin && lam[i] <= Emax) perm.push_back(i);
    const int M = (int)perm.size();
    for (int i = 0; i < r; ++i) if (!(lam[i] >= Emin && lam[i] <= Emax)) perm.push_back(i);
    std::vector<cplx> Vs((size_t)r * r);
    std::vector<double> lamc(2 * (size_t)r);
    for (int k = 0; k < r; ++k) {
        lambda_out[k] = lam[perm[k]];
        lamc[2 * k] = lam[perm[k]]; lamc[2 * k + 1] = 0.0;
        for (int i = 0; i < r; ++i) Vs[(size_t)k * r + i] = V[(size_t)perm[k] * ld + i];
    }
    *M_out = M;
    return feasthip_ritz_residual_dev(h, r64, dQ, Vs.data(), lamc.data(), M, 1, use_B, dX, res_out);
}
