// Host harness of the rank-revealing Cholesky-QR stage (csrc/fh_cholqr.hpp: pivoted_stage), built with gcc under
// AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_cholqr_rr_host.py.
//
//   host_cholqr_rr_harness <in> <out>
// <in>: one record per panel -- "N m ld cplx rank_tol ref_scale big_dim" and then the N x m panel, column-major, as
// numbers (re im pairs when cplx).  The harness runs the staged factorisation with every dense step done naively on the
// host (Gram products, panel products, projections; the stage decision is pivoted_stage) and writes per panel
// "rank stages fell_back", the pivot order and the |R_kk|.  It also checks what the kernel relies on: accepted pivots are
// distinct undecided columns, Rinv is zero outside the accepted rows and columns, and the result is finite.
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <vector>

#include "../feastkit.jl_amd/csrc/fh_cholqr.hpp"

struct cplx { double x, y; };
using cd = std::complex<double>;
using Mat = std::vector<cd>;          // column-major

static void fail(const char* what) { std::fprintf(stderr, "FAIL: %s\n", what); std::exit(1); }

// C (ra x cb) = A^H B, A: N x ra (leading dim N), B: N x cb
static Mat herm_prod(const Mat& A, int ra, const Mat& B, int cb, int N) {
    Mat C((size_t)ra * cb);
    for (int j = 0; j < cb; ++j)
        for (int i = 0; i < ra; ++i) {
            cd s = 0;
            for (int r = 0; r < N; ++r) s += std::conj(A[(size_t)i * N + r]) * B[(size_t)j * N + r];
            C[(size_t)j * ra + i] = s;
        }
    return C;
}
// C (N x cb) = A (N x ka) * B (ka x cb, leading dim ldb)
static Mat prod(const Mat& A, int ka, const Mat& B, int ldb, int cb, int N) {
    Mat C((size_t)N * cb, cd(0));
    for (int j = 0; j < cb; ++j)
        for (int k = 0; k < ka; ++k) {
            const cd b = B[(size_t)j * ldb + k];
            if (b == cd(0)) continue;
            for (int r = 0; r < N; ++r) C[(size_t)j * N + r] += A[(size_t)k * N + r] * b;
        }
    return C;
}

template <class S> static S to_s(cd v);
template <> double to_s<double>(cd v) { return v.real(); }
template <> cplx to_s<cplx>(cd v) { return cplx{v.real(), v.imag()}; }
static cd from_s(double v) { return cd(v, 0); }
static cd from_s(cplx v) { return cd(v.x, v.y); }

// one stage on the Gram matrix Gc (ld x ld) in the scalar type S; Rinv comes back as complex
template <class S>
static fh_cholqr::Stage run_stage(const Mat& Gc, int m, int ld, double window, double thr, double ref, double* r11, const int* decided,
                                  bool refine, int nfix, int col0, int* ord, double* rd, Mat& Rinv) {
    std::vector<S> G((size_t)ld * ld), Ri;
    for (size_t e = 0; e < G.size(); ++e) G[e] = to_s<S>(Gc[e]);
    fh_cholqr::Stage st = fh_cholqr::pivoted_stage(G, m, ld, window, thr, ref, r11, decided, refine, nfix, col0, ord, rd, Ri);
    Rinv.assign((size_t)ld * ld, cd(0));
    for (size_t e = 0; e < Ri.size(); ++e) Rinv[e] = from_s(Ri[e]);
    return st;
}
static bool has_imag(const Mat& G) {
    for (const cd& v : G) if (v.imag() != 0.0) return true;
    return false;
}
static fh_cholqr::Stage stage(const Mat& G, int m, int ld, double window, double thr, double ref, double* r11, const int* decided,
                              bool refine, int nfix, int col0, int* ord, double* rd, Mat& Rinv) {
    return has_imag(G) ? run_stage<cplx>(G, m, ld, window, thr, ref, r11, decided, refine, nfix, col0, ord, rd, Rinv)
                       : run_stage<double>(G, m, ld, window, thr, ref, r11, decided, refine, nfix, col0, ord, rd, Rinv);
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s <in> <out>\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    std::ofstream out(argv[2]);
    out.precision(17);
    const double window = 1e-10, eps = 2.220446049250313e-16;
    const int max_stages = 6;
    int N, m, ld, is_c, big_dim, count = 0;
    double rank_tol, ref_scale;
    while (in >> N >> m >> ld >> is_c >> rank_tol >> ref_scale >> big_dim) {
        if (m < 0 || m > ld || ld > 64) fail("bad record");
        Mat X((size_t)N * ld, cd(0));
        double colmax = 0.0;
        for (int j = 0; j < m; ++j) {
            double n2 = 0.0;
            for (int r = 0; r < N; ++r) {
                double a, b = 0.0;
                in >> a;
                if (is_c) in >> b;
                X[(size_t)j * N + r] = cd(a, b);
                n2 += a * a + b * b;
            }
            colmax = std::max(colmax, std::sqrt(n2));
        }
        const double scale = colmax > 0.0 && std::isfinite(colmax) ? std::ldexp(1.0, -std::ilogb(colmax)) : 1.0;
        Mat W = X;
        for (cd& v : W) v *= scale;
        const double thr = std::max(rank_tol, eps * std::max(N, std::max(big_dim, m)));
        Mat Q((size_t)N * ld, cd(0));
        std::vector<int> decided(ld, 0), perm;
        std::vector<double> rdiag;
        double r11 = -1.0;
        int rank = 0, stages = 0;
        bool done = false, gave_up = false;
        for (int s = 0; s < max_stages && !done && !gave_up; ++s) {
            std::vector<int> ord(ld, -1);
            std::vector<double> rd(ld, 0.0);
            Mat Rinv;
            fh_cholqr::Stage st = stage(herm_prod(W, ld, W, ld, N), m, ld, window, thr, ref_scale * scale, &r11, decided.data(), false, 0, 0,
                                        ord.data(), rd.data(), Rinv);
            if (st.fail) { gave_up = true; break; }
            if (st.nacc < 0 || rank + st.nacc > m) fail("accepted count out of range");
            for (int k = 0; k < st.nacc; ++k) {
                if (ord[k] < 0 || ord[k] >= m || decided[ord[k]]) fail("pivot is not an undecided column");
                for (int q = 0; q < k; ++q) if (ord[q] == ord[k]) fail("pivot taken twice");
                if (!(rd[k] > 0.0) || !std::isfinite(rd[k])) fail("|R_kk| not positive");
                if (k > 0 && rd[k] > rd[k - 1] * (1.0 + 1e-6)) fail("pivots not decreasing");
            }
            for (int c = 0; c < ld; ++c)
                for (int r = 0; r < ld; ++r) {
                    const cd v = Rinv[(size_t)c * ld + r];
                    if (!std::isfinite(v.real()) || !std::isfinite(v.imag())) fail("Rinv not finite");
                    bool row_ok = false;
                    for (int k = 0; k < st.nacc; ++k) row_ok |= ord[k] == r;
                    if ((c >= st.nacc || !row_ok) && v != cd(0)) fail("Rinv not zero outside the accepted block");
                }
            Mat T = prod(W, ld, Rinv, ld, ld, N);
            if (s > 0) {
                Mat C = herm_prod(Q, ld, T, ld, N), KC = prod(Q, ld, C, ld, ld, N);
                for (size_t e = 0; e < T.size(); ++e) T[e] -= KC[e];
            }
            Mat R2;
            std::vector<int> ord2(ld, -1);
            fh_cholqr::Stage s2 = stage(herm_prod(T, ld, T, ld, N), m, ld, 0.0, thr, ref_scale * scale, &r11, decided.data(), true, st.nacc,
                                        rank, ord2.data(), rd.data(), R2);
            if (s2.fail) { gave_up = true; break; }
            if (s2.nacc != st.nacc) fail("second pass changed the count");
            Mat T2 = prod(T, ld, R2, ld, ld, N);
            for (size_t e = 0; e < Q.size(); ++e) Q[e] += T2[e];
            for (int k = 0; k < st.nacc; ++k) { decided[ord[k]] = 1; perm.push_back(ord[k]); rdiag.push_back(rd[k] / scale); }
            rank += st.nacc;
            stages += 1;
            if (st.done || rank >= m) { done = true; break; }
            for (int pass = 0; pass < 2; ++pass) {
                Mat C = herm_prod(T2, ld, W, ld, N), TC = prod(T2, ld, C, ld, ld, N);
                for (size_t e = 0; e < W.size(); ++e) W[e] -= TC[e];
            }
        }
        if (!done) gave_up = true;
        if (gave_up) { out << "0 " << stages << " 1\n\n\n"; ++count; continue; }
        // the basis is orthonormal
        Mat QQ = herm_prod(Q, ld, Q, ld, N);
        for (int j = 0; j < rank; ++j)
            for (int i = 0; i < rank; ++i)
                if (std::abs(QQ[(size_t)j * ld + i] - cd(i == j ? 1.0 : 0.0)) > 1e-12) fail("basis not orthonormal");
        out << rank << " " << stages << " 0\n";
        for (int k = 0; k < rank; ++k) out << perm[k] << (k + 1 < rank ? " " : "");
        out << "\n";
        for (int k = 0; k < rank; ++k) out << rdiag[k] << (k + 1 < rank ? " " : "");
        out << "\n";
        ++count;
    }
    std::printf("ok %d\n", count);
    return 0;
}
