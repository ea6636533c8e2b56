// CPU harness for the host half of the Cholesky-QR orthonormalisation (feastkit.jl_amd/csrc/fh_cholqr.hpp), built by
// tests/test_ingest_sanitizer.py with  g++ -fsanitize=address,undefined -fno-sanitize-recover=all.  For real and complex
// Gram matrices G = X^H X, m = 1..64 columns, leading dimensions 16 / 32 / 64:
//   * well conditioned: Rinv^H G Rinv = I to 1e-12 and the decision is "one pass";
//   * graded columns: norms spread over 1e3 still give "one pass" after equilibration (and the equilibrated inverse, scaled
//     back, orthonormalises G to 1e-12); a spread of 1e8 with rank_tol = sqrt(eps) fails the 1e3 rank_tol margin: "reject";
//   * rank deficient (a zero column, half the rank) and non-finite entries: "reject", and Rinv fails cleanly;
//   * the complex instantiation on a real matrix agrees with the real one to 1e-13.
// Usage: host_cholqr_harness [seed]                    -> prints "ok <cases>" or aborts
//        host_cholqr_harness ratios <in.txt> <out.txt> -> the pivot ratio of each matrix in <in.txt> ("m is_complex" and the
//                                                         m x m entries column-major, re [im]); tests/test_ingest_sanitizer.py
//                                                         checks them against LAPACK's pivoted Cholesky (?pstrf)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "../feastkit.jl_amd/csrc/fh_cholqr.hpp"

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "CHECK failed line %d: %s\n", __LINE__, #cond); std::abort(); } } while (0)

struct cx { double x, y; };
using fh_cholqr::Plan;

static double sqrt_eps() { return std::sqrt(2.220446049250313e-16); }

// G = X^H X (m x m, leading dim ld) of an n x m panel with independent N(0, 1) entries times the column scales s
static std::vector<cx> gram(std::mt19937_64& rng, int n, int m, int ld, bool cplx, const std::vector<double>& s) {
    std::normal_distribution<double> nd;
    std::vector<cx> X((size_t)n * m), G((size_t)ld * ld, cx{0, 0});
    for (int j = 0; j < m; ++j)
        for (int i = 0; i < n; ++i) X[(size_t)j * n + i] = cx{s[j] * nd(rng), cplx ? s[j] * nd(rng) : 0.0};
    for (int j = 0; j < m; ++j)
        for (int i = 0; i < m; ++i) {
            cx a{0, 0};
            for (int t = 0; t < n; ++t) {
                const cx u = X[(size_t)i * n + t], v = X[(size_t)j * n + t];
                a = cx{a.x + u.x * v.x + u.y * v.y, a.y + u.x * v.y - u.y * v.x};
            }
            G[(size_t)j * ld + i] = a;
        }
    return G;
}

// max |Rinv^H G Rinv - I| over the m x m block
static double ortho_error(const std::vector<cx>& G, const std::vector<cx>& Rinv, int m, int ld) {
    std::vector<cx> T((size_t)m * m);
    for (int j = 0; j < m; ++j)          // T = G Rinv
        for (int i = 0; i < m; ++i) {
            cx a{0, 0};
            for (int k = 0; k < m; ++k) a = fh_cholqr::add(a, fh_cholqr::mul(G[(size_t)k * ld + i], Rinv[(size_t)j * ld + k]));
            T[(size_t)j * m + i] = a;
        }
    double err = 0.0;
    for (int j = 0; j < m; ++j)
        for (int i = 0; i < m; ++i) {
            cx a{0, 0};
            for (int k = 0; k < m; ++k) a = fh_cholqr::add(a, fh_cholqr::mul(fh_cholqr::conj(Rinv[(size_t)i * ld + k]), T[(size_t)j * m + k]));
            err = std::max(err, std::hypot(a.x - (i == j ? 1.0 : 0.0), a.y));
        }
    return err;
}

static Plan decide(std::vector<cx> G, int m, int ld, double rank_tol, std::vector<double>& d) {
    return fh_cholqr::accept(G, m, ld, 0.0, rank_tol, false, d);
}

static int ratios(const char* in, const char* out) {
    FILE* f = std::fopen(in, "r");
    FILE* g = std::fopen(out, "w");
    CHECK(f && g);
    int m, is_c, count = 0;
    while (std::fscanf(f, "%d %d", &m, &is_c) == 2) {
        CHECK(m >= 1 && m <= 64);
        const int ld = m <= 16 ? 16 : m <= 32 ? 32 : 64;
        std::vector<double> Gr((size_t)ld * ld, 0.0);
        std::vector<cx> Gc((size_t)ld * ld, cx{0, 0});
        for (int j = 0; j < m; ++j)
            for (int i = 0; i < m; ++i) {
                double re = 0.0, im = 0.0;
                CHECK(std::fscanf(f, "%lf", &re) == 1);
                if (is_c) CHECK(std::fscanf(f, "%lf", &im) == 1);
                Gr[(size_t)j * ld + i] = re;
                Gc[(size_t)j * ld + i] = cx{re, im};
            }
        const double r = is_c ? fh_cholqr::pivoted_cholesky_ratio(Gc, m, ld) : fh_cholqr::pivoted_cholesky_ratio(Gr, m, ld);
        std::fprintf(g, "%.17g\n", r);
        ++count;
    }
    std::fclose(f);
    std::fclose(g);
    std::printf("ratios %d\n", count);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && std::strcmp(argv[1], "ratios") == 0) return ratios(argv[2], argv[3]);
    std::mt19937_64 rng(argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 20260515ull);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    int cases = 0;
    for (int ld : {16, 32, 64})
        for (int m = 1; m <= ld; ++m)
            for (int cplx = 0; cplx < 2; ++cplx) {
                const int n = 6 * m + 16;
                std::vector<double> d, ones(m, 1.0);
                std::vector<cx> Rinv;
                // well conditioned
                std::vector<cx> G = gram(rng, n, m, ld, cplx, ones);
                CHECK(fh_cholqr::gram_upper_inverse(G, m, ld, Rinv));
                CHECK(Rinv.size() == (size_t)ld * ld);
                CHECK(ortho_error(G, Rinv, m, ld) < 1e-12);
                CHECK(decide(G, m, ld, sqrt_eps(), d) == Plan::one_pass);
                std::vector<cx> Gt = G;
                CHECK(fh_cholqr::accept(Gt, m, ld, 0.0, sqrt_eps(), true, d) == Plan::two_pass);        // the two-pass override
                for (int j = 0; j < ld; ++j)                        // zero padding outside the m x m block
                    for (int i = 0; i < ld; ++i)
                        if (i >= m || j >= m || i > j) CHECK(Rinv[(size_t)j * ld + i].x == 0.0 && Rinv[(size_t)j * ld + i].y == 0.0);
                if (!cplx) {        // the complex instantiation on a real matrix against the real one
                    std::vector<double> Gr((size_t)ld * ld, 0.0), Rr;
                    for (int j = 0; j < m; ++j) for (int i = 0; i < m; ++i) Gr[(size_t)j * ld + i] = G[(size_t)j * ld + i].x;
                    const double rr = fh_cholqr::pivoted_cholesky_ratio(Gr, m, ld), rc = fh_cholqr::pivoted_cholesky_ratio(G, m, ld);
                    CHECK(std::fabs(rr - rc) <= 1e-13 * std::fabs(rr));
                    std::vector<cx> Rc;
                    CHECK(fh_cholqr::chol_upper_inverse(Gr, m, ld, Rr) && fh_cholqr::chol_upper_inverse(G, m, ld, Rc));
                    double scale = 0.0;
                    for (double v : Rr) scale = std::max(scale, std::fabs(v));
                    for (size_t k = 0; k < Rr.size(); ++k) CHECK(std::fabs(Rr[k] - Rc[k].x) <= 1e-13 * scale && Rc[k].y == 0.0);
                }
                if (m >= 2) {
                    // graded column norms: a spread of 1e3 is equilibrated away, 1e8 fails the margin
                    for (double spread : {1e3, 1e8}) {
                        std::vector<double> s(m);
                        for (int j = 0; j < m; ++j) s[j] = std::pow(spread, j == 0 ? 0.0 : j == m - 1 ? 1.0 : u(rng));
                        std::vector<cx> Gg = gram(rng, n, m, ld, cplx, s), Ge = Gg;
                        const Plan p = fh_cholqr::accept(Ge, m, ld, 0.0, sqrt_eps(), false, d);
                        if (spread < 1e4) {
                            CHECK(p == Plan::one_pass);
                            CHECK(fh_cholqr::gram_upper_inverse(Ge, m, ld, Rinv));
                            for (int j = 0; j < m; ++j)       // R = R' D  =>  R^-1 = D^-1 R'^-1
                                for (int i = 0; i < m; ++i) Rinv[(size_t)j * ld + i] = fh_cholqr::div_re(Rinv[(size_t)j * ld + i], d[i]);
                            CHECK(ortho_error(Gg, Rinv, m, ld) < 1e-12);
                        } else {
                            CHECK(p == Plan::reject);
                        }
                    }
                    // rank deficient: half the columns repeat the others (exactly), or one column is zero
                    std::vector<cx> Gd = gram(rng, n, m, ld, cplx, ones);
                    for (int j = m / 2; j < m; ++j)
                        for (int i = 0; i < m; ++i) Gd[(size_t)j * ld + i] = Gd[(size_t)(j - m / 2) * ld + i];
                    for (int j = 0; j < m; ++j)
                        for (int i = m / 2; i < m; ++i) Gd[(size_t)j * ld + i] = Gd[(size_t)j * ld + i - m / 2];
                    CHECK(decide(Gd, m, ld, sqrt_eps(), d) == Plan::reject);
                    CHECK(fh_cholqr::gram_ratio(Gd, m, ld) < 1e-10);
                }
                std::vector<cx> Gz = gram(rng, n, m, ld, cplx, ones);
                const int z = (int)(u(rng) * m) % m;
                for (int i = 0; i < m; ++i) Gz[(size_t)z * ld + i] = Gz[(size_t)i * ld + z] = cx{0, 0};
                CHECK(decide(Gz, m, ld, sqrt_eps(), d) == Plan::reject);
                CHECK(!fh_cholqr::gram_upper_inverse(Gz, m, ld, Rinv));
                CHECK(fh_cholqr::gram_ratio(Gz, m, ld) == 0.0);
                // non-finite entries: on the diagonal, and off it
                for (double bad : {NAN, INFINITY}) {
                    std::vector<cx> Gn = gram(rng, n, m, ld, cplx, ones);
                    Gn[(size_t)z * ld + z] = cx{bad, 0.0};
                    CHECK(decide(Gn, m, ld, sqrt_eps(), d) == Plan::reject);
                    CHECK(!fh_cholqr::gram_upper_inverse(Gn, m, ld, Rinv));
                    if (m >= 2) {
                        Gn = gram(rng, n, m, ld, cplx, ones);
                        Gn[(size_t)(m - 1) * ld] = Gn[m - 1] = cx{bad, 0.0};
                        CHECK(decide(Gn, m, ld, sqrt_eps(), d) == Plan::reject);
                        CHECK(!fh_cholqr::gram_upper_inverse(Gn, m, ld, Rinv));
                    }
                }
                ++cases;
            }
    // the Hermitian part: (G + G^H) / 2, Hermitian to the bit
    for (int r : {1, 7, 64}) {
        std::normal_distribution<double> nd;
        std::vector<cx> H((size_t)r * r), H0;
        for (auto& v : H) v = cx{nd(rng), nd(rng)};
        H0 = H;
        fh_cholqr::hermitian_part(H.data(), r);
        for (int j = 0; j < r; ++j)
            for (int i = 0; i < r; ++i) {
                const cx a = H[(size_t)j * r + i], b = H[(size_t)i * r + j];
                CHECK(a.x == b.x && a.y == -b.y);
                CHECK(std::fabs(a.x - 0.5 * (H0[(size_t)j * r + i].x + H0[(size_t)i * r + j].x)) <= 1e-15 * (std::fabs(a.x) + 1));
            }
    }
    std::printf("ok %d\n", cases);
    return 0;
}
