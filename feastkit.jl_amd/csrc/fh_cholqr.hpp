// fh_cholqr.hpp -- host half of the Cholesky-QR orthonormalisation (pure C++17, no HIP): the small dense maths that decides
// the rank of every FEAST refinement loop's subspace.  fh_ortho_panel and feasthip_rr_reduce_resident (fh_ortho.hip, fh_ritz.hip) both take
// their decision from accept() below; tests/host_cholqr_harness.cpp and tests/host_cholqr_rr_harness.cpp check this file on
// the CPU under sanitizers.
//
// Every routine is one template instantiated for a real scalar (double) and a complex one (any struct {double x, y}, such as
// fh_common.hpp's cplx).  A Gram matrix without imaginary parts (the real projection of a real-symmetric pencil) takes the
// real instantiation: the same arithmetic on a quarter of the flops.  The scalar operations below keep the operation order of
// the routines they replaced: the real ones divide by a real pivot, the complex ones multiply by its reciprocal.
#pragma once
#include <algorithm>
#include <cmath>
#include <type_traits>
#include <utility>
#include <vector>

#if defined(__HIPCC__)
#define FH_CQ_HD __host__ __device__
#else
#define FH_CQ_HD
#endif

namespace fh_cholqr {

FH_CQ_HD inline double re(double a) { return a; }
FH_CQ_HD inline double conj(double a) { return a; }
FH_CQ_HD inline double neg(double a) { return -a; }
FH_CQ_HD inline double add(double a, double b) { return a + b; }
FH_CQ_HD inline double sub(double a, double b) { return a - b; }
FH_CQ_HD inline double mul(double a, double b) { return a * b; }
FH_CQ_HD inline double div_re(double a, double r) { return a / r; }
template <class C> FH_CQ_HD inline double re(const C& a) { return a.x; }
template <class C> FH_CQ_HD inline C conj(const C& a) { return C{a.x, -a.y}; }
template <class C> FH_CQ_HD inline C neg(const C& a) { return C{-a.x, -a.y}; }
template <class C> FH_CQ_HD inline C add(const C& a, const C& b) { return C{a.x + b.x, a.y + b.y}; }
template <class C> FH_CQ_HD inline C sub(const C& a, const C& b) { return C{a.x - b.x, a.y - b.y}; }
template <class C> FH_CQ_HD inline C mul(const C& a, const C& b) { return C{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
template <class C> FH_CQ_HD inline C div_re(const C& a, double r) { const double s = 1.0 / r; return C{a.x * s, a.y * s}; }
template <class S> FH_CQ_HD inline S from_re(double v) {
    if constexpr (std::is_same_v<S, double>) return v;
    else return S{v, 0.0};
}

// Pivoted Cholesky of a Hermitian PSD matrix (m x m, column-major, leading dim ld): min/max pivot ratio, 0 when a pivot is
// not positive or not finite.  In exact arithmetic the pivots are the squares of the diagonal of R in the column-pivoted QR
// of the panel, so the ratio bounds the rank test of _feast_qr_compress! (src/core/feast_aux.jl:117-124) from the safe side.
template <class S> double pivoted_cholesky_ratio(std::vector<S> G, int m, int ld) {
    double dmax = 0.0, dmin = 0.0;
    auto at = [&](int i, int j) -> S& { return G[(size_t)j * ld + i]; };
    for (int k = 0; k < m; ++k) {
        int p = k;
        for (int j = k + 1; j < m; ++j) if (re(at(j, j)) > re(at(p, p))) p = j;
        if (p != k) {     // symmetric swap of rows/cols k and p
            for (int j = 0; j < m; ++j) std::swap(at(k, j), at(p, j));
            for (int i = 0; i < m; ++i) std::swap(at(i, k), at(i, p));
        }
        const double d = re(at(k, k));
        if (k == 0) dmax = d;
        if (!(d > 0.0) || !std::isfinite(d)) return 0.0;
        dmin = d;
        const double r = std::sqrt(d);
        for (int i = k + 1; i < m; ++i) at(i, k) = div_re(at(i, k), r);
        for (int j = k + 1; j < m; ++j)
            for (int i = j; i < m; ++i) {
                const S v = sub(at(i, j), mul(at(i, k), conj(at(j, k))));
                at(i, j) = v;
                at(j, i) = conj(v);
            }
    }
    return dmax > 0.0 ? dmin / dmax : 0.0;
}

// Rinv (ld x ld, column-major, zero padded) with G = R^H R, R upper triangular (G: m x m, leading dim ld); false if G is not
// numerically positive definite
template <class S> bool chol_upper_inverse(const std::vector<S>& G, int m, int ld, std::vector<S>& Rinv) {
    std::vector<S> R((size_t)m * m, S{});
    auto r = [&](int i, int j) -> S& { return R[(size_t)j * m + i]; };
    for (int j = 0; j < m; ++j)
        for (int i = 0; i <= j; ++i) {
            S sum = G[(size_t)j * ld + i];
            for (int k = 0; k < i; ++k) sum = sub(sum, mul(conj(r(k, i)), r(k, j)));
            if (i == j) {
                if (!(re(sum) > 0.0) || !std::isfinite(re(sum))) return false;
                r(i, i) = from_re<S>(std::sqrt(re(sum)));
            } else {
                r(i, j) = div_re(sum, re(r(i, i)));
            }
        }
    Rinv.assign((size_t)ld * ld, S{});
    for (int j = 0; j < m; ++j) {          // back substitution, column by column
        Rinv[(size_t)j * ld + j] = from_re<S>(1.0 / re(r(j, j)));
        for (int i = j - 1; i >= 0; --i) {
            S sum{};
            for (int k = i + 1; k <= j; ++k) sum = add(sum, mul(r(i, k), Rinv[(size_t)j * ld + k]));
            Rinv[(size_t)j * ld + i] = div_re(neg(sum), re(r(i, i)));
        }
    }
    return true;
}

// the real parts of G when no entry of its m x m block has an imaginary part (leading dim ld kept), else empty
template <class C> std::vector<double> real_gram(const std::vector<C>& G, int m, int ld) {
    for (int j = 0; j < m; ++j)
        for (int i = 0; i < m; ++i) if (G[(size_t)j * ld + i].y != 0.0) return {};
    std::vector<double> Gr((size_t)ld * ld, 0.0);
    for (int j = 0; j < m; ++j) for (int i = 0; i < m; ++i) Gr[(size_t)j * ld + i] = G[(size_t)j * ld + i].x;
    return Gr;
}

// the two routines on a complex Gram matrix, through the real instantiation when it has no imaginary parts
template <class C> double gram_ratio(const std::vector<C>& G, int m, int ld) {
    std::vector<double> Gr = real_gram(G, m, ld);
    return Gr.empty() ? pivoted_cholesky_ratio(G, m, ld) : pivoted_cholesky_ratio(std::move(Gr), m, ld);
}
template <class C> bool gram_upper_inverse(const std::vector<C>& G, int m, int ld, std::vector<C>& Rinv) {
    const std::vector<double> Gr = real_gram(G, m, ld);
    if (Gr.empty()) return chol_upper_inverse(G, m, ld, Rinv);
    std::vector<double> Rr;
    if (!chol_upper_inverse(Gr, m, ld, Rr)) return false;
    Rinv.resize(Rr.size());
    for (size_t k = 0; k < Rr.size(); ++k) Rinv[k] = from_re<C>(Rr[k]);
    return true;
}

enum class Plan { reject, two_pass, one_pass };

// The Cholesky-QR acceptance test.  G (the Gram matrix X^H X of m columns, leading dim ld) is equilibrated in place,
// G' = D^-1 G D^-1 with D = diag(d), d = the column norms: columns of very different length (guard columns scaled by a small
// filter value) make G ill-conditioned although the directions are fine, and Cholesky of G' is as stable as for unit
// columns.  ref_scale > 0: X is a block of a wider matrix whose largest column norm is ref_scale (0: X itself).
//   reject    a zero, non-finite or nearly dependent column: the rank-revealing pivoted Gram-Schmidt decides.  Full rank in
//             the sense of the reference's pivoted-QR rule is accepted only with a wide margin: |R_kk|/|R_11| >~
//             (d_min/d_max) sqrt(ratio') must exceed 1e3 rank_tol (ratio' = pivot ratio of G' ~ 1 / its condition number).
//   one_pass  ratio' > 1e-2: one Cholesky-QR pass is already orthonormal to 1e-14 (the FEAST panel in steady state has
//             ratio' ~ 0.4), unless always_two
//   two_pass  otherwise: the second pass squares away the orthogonality error of the first, eps / ratio'
template <class C> Plan accept(std::vector<C>& G, int m, int ld, double ref_scale, double rank_tol, bool always_two,
                               std::vector<double>& d) {
    d.resize(m);
    double dmin = 0.0, dmax = ref_scale;
    for (int j = 0; j < m; ++j) {
        const double g = G[(size_t)j * ld + j].x;
        d[j] = g > 0.0 && std::isfinite(g) ? std::sqrt(g) : 0.0;
        dmin = j == 0 ? d[j] : std::min(dmin, d[j]);
        dmax = std::max(dmax, d[j]);
    }
    if (!(dmin > 0.0)) return Plan::reject;
    for (int j = 0; j < m; ++j)
        for (int i = 0; i < m; ++i) G[(size_t)j * ld + i] = div_re(G[(size_t)j * ld + i], d[i] * d[j]);
    const double ratio = gram_ratio(G, m, ld);
    if (!(ratio > 1e-10) || !((dmin / dmax) * std::sqrt(ratio) > 1e3 * rank_tol)) return Plan::reject;
    return ratio > 1e-2 && !always_two ? Plan::one_pass : Plan::two_pass;
}

// ---- one stage of the rank-revealing Cholesky-QR (FEASTHIP_ORTHO_CHOLQR_RR) ---------------------------------------------------
// The pivots of a pivoted Cholesky of G = X^H X are the squared R_kk of the column-pivoted QR of X, but the rank threshold of
// _feast_qr_compress! (rank_tol ~ sqrt(eps), src/core/feast_aux.jl:117-124) sits at pivot ratio 1e-16, where G has no digits
// left.  So a stage only accepts the leading pivots that stay inside `window` (a ratio of squared pivots) of its first one;
// the caller orthonormalises those columns, projects them out of the rest and runs the next stage on the Gram matrix of the
// remainder, which is accurate relative to its own size.  k_pchol_stage (fh_blockops.hip) is this routine on one workgroup:
// the same operations on every entry in the same order, spread over threads.
//
// G (ld x ld, column-major) is overwritten.  decided[j] != 0: column j was accepted by an earlier stage and is ignored.
//   refine == false  equilibrate the undecided block as accept() does, then pivoted Cholesky: the next pivot is the column
//                    of largest remaining norm, |R_kk| = d_p sqrt(G'_pp).  Stops for good (done) at the first
//                    |R_kk| <= stop -- the rule of k_mgs_pick -- and for this stage at the first pivot with
//                    R_kk^2 <= window * (the stage's first R_kk^2).  *r11 < 0 on entry: first stage, *r11 = max(first |R_kk|,
//                    ref_scale) and stop = thr * *r11 from here on.
//   refine == true   the second Cholesky-QR pass of the columns a stage accepted: G is the Gram matrix of those nfix columns
//                    (already nearly orthonormal), no pivoting, no scaling; rdiag[k] is multiplied by the correction R2_kk.
// ord[k] / rdiag[k]: column and |R_kk| of the k-th accepted pivot.  Rinv (ld x ld, zero padded): X Rinv has the accepted
// columns, orthonormalised, at columns col0, col0 + 1, ... (the permutation is folded in: row ord[a] of Rinv holds row a of
// the inverse of the triangular factor).
struct Stage { int nacc = 0; bool done = false, fail = false; };

template <class S> inline bool finite_s(const S& a) {
    if constexpr (std::is_same_v<S, double>) return std::isfinite(a);
    else return std::isfinite(a.x) && std::isfinite(a.y);
}

template <class S>
Stage pivoted_stage(std::vector<S>& G, int m, int ld, double window, double thr, double ref_scale, double* r11,
                    const int* decided, bool refine, int nfix, int col0, int* ord, double* rdiag, std::vector<S>& Rinv) {
    Stage out;
    auto at = [&](int i, int j) -> S& { return G[(size_t)j * ld + i]; };
    std::vector<int> alive(ld, 0), picked(ld, 0), pos(ld, -1);
    std::vector<double> d(ld, 1.0), w(ld, 1.0), key(ld, -1.0);
    for (int j = 0; j < ld; ++j) alive[j] = refine ? j < nfix : (j < m && !decided[j]);
    Rinv.assign((size_t)ld * ld, S{});
    for (int j = 0; j < ld; ++j)
        for (int i = 0; i < ld; ++i)
            if (alive[i] && alive[j] && !finite_s(at(i, j))) { out.fail = out.done = true; return out; }
    double dref = 0.0;
    if (!refine) {
        for (int j = 0; j < ld; ++j) {
            if (!alive[j]) continue;
            const double g = re(at(j, j));
            d[j] = g > 0.0 ? std::sqrt(g) : 0.0;
            dref = std::max(dref, d[j]);
        }
        for (int j = 0; j < ld; ++j)
            for (int i = 0; i < ld; ++i)
                if (alive[i] && alive[j] && d[i] > 0.0 && d[j] > 0.0) at(i, j) = div_re(at(i, j), d[i] * d[j]);
        for (int j = 0; j < ld; ++j) if (alive[j]) w[j] = d[j] > 0.0 ? (d[j] / dref) * (d[j] / dref) : 0.0;
        if (*r11 < 0.0) *r11 = std::max(dref, ref_scale);
    } else {
        dref = 1.0;
    }
    const double stop = thr * *r11;
    for (int j = 0; j < ld; ++j) if (alive[j]) key[j] = w[j] * re(at(j, j));
    double key0 = 0.0;
    int k = 0;
    for (;; ++k) {
        int p = -1;
        for (int j = 0; j < ld; ++j) {
            if (!alive[j] || picked[j]) continue;
            if (refine) { p = j; break; }
            if (p < 0 || key[j] > key[p]) p = j;       // ties: the lowest index
        }
        if (p < 0) break;
        const double best = key[p], rkk = dref * std::sqrt(best);
        if (refine) {
            if (!(best > 0.0)) { out.fail = out.done = true; return out; }
        } else {
            if (!(rkk > stop) || rkk == 0.0) { out.done = true; break; }
            if (k == 0) key0 = best;
            else if (!(best > window * key0)) break;
        }
        const double r = std::sqrt(re(at(p, p)));
        ord[k] = p;
        rdiag[k] = refine ? rdiag[k] * r : rkk;
        picked[p] = 1;
        pos[p] = k;
        for (int i = 0; i < ld; ++i) if (alive[i] && !picked[i]) at(i, p) = div_re(at(i, p), r);
        at(p, p) = from_re<S>(r);
        for (int j = 0; j < ld; ++j) {
            if (!alive[j] || picked[j]) continue;
            for (int i = 0; i < ld; ++i)
                if (alive[i] && !picked[i]) at(i, j) = sub(at(i, j), mul(at(i, p), conj(at(j, p))));
            key[j] = w[j] * re(at(j, j));
        }
    }
    out.nacc = k;
    // inverse of the triangular factor R'[a][b] = conj(L_a[ord[b]]) (a < b), R'[a][a] = r_a, column by column
    std::vector<S> Ri((size_t)k * k, S{});
    for (int b = 0; b < k; ++b) {
        Ri[(size_t)b * k + b] = from_re<S>(1.0 / re(at(ord[b], ord[b])));
        for (int a = b - 1; a >= 0; --a) {
            S sum{};
            for (int c = a + 1; c <= b; ++c) sum = add(sum, mul(conj(at(ord[c], ord[a])), Ri[(size_t)b * k + c]));
            Ri[(size_t)b * k + a] = div_re(neg(sum), re(at(ord[a], ord[a])));
        }
    }
    for (int b = 0; b < k; ++b)
        for (int a = 0; a <= b; ++a) {
            if (col0 + b >= ld) continue;
            Rinv[(size_t)(col0 + b) * ld + ord[a]] = refine ? Ri[(size_t)b * k + a] : div_re(Ri[(size_t)b * k + a], d[ord[a]]);
        }
    return out;
}

// Hermitian part (G + G^H) / 2 in place (r x r, column-major): _feast_hermitian_part!, src/core/feast_aux.jl:84-92
template <class C> void hermitian_part(C* G, int r) {
    for (int j = 0; j < r; ++j)
        for (int i = 0; i <= j; ++i) {
            const C a = G[(size_t)j * r + i], b = conj(G[(size_t)i * r + j]);
            const C hm{0.5 * (a.x + b.x), 0.5 * (a.y + b.y)};
            G[(size_t)j * r + i] = hm;
            G[(size_t)i * r + j] = conj(hm);
        }
}

}  // namespace fh_cholqr
