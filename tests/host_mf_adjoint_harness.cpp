// host_mf_adjoint_harness.cpp -- CPU harness of the ADJOINT substitution through the multifrontal plan
// (feastkit.jl_amd/csrc/fh_mf.hpp) and of the conjugate-transposed CSR set (fh_adjoint_csr, csrc/fh_ingest.hpp).
// Part 1 executes the plan on the CPU as the device code does (padded fronts, partial pivoting inside the fully-summed block,
// extend-add through the plan's maps) and then walks the tree conjugate-transposed, in the order of mf_solve_adjoint_ld
// (fh_dense.hip):
//   ascending   z = [b1; 0] + children's boundary rows (no pivot permutation),  w1 = U11^-H z1,  z2 -= U12^H w1
//   descending  v2 = the parent's rows,  v1 = L11^-H (w1 - L21^H v2),  x1[p[i]] = v1[i] last
// against the residual of (zB - A)^H x = b, bar 1e-11 (the bar of tests/host_mf_harness.cpp for the forward solve).
// The matrices have unsymmetric VALUES (a symmetric S would not tell S^H from conj(S)) and a complex shift.
// Part 2 transposes random union-pattern sets and compares with a dense conjugate transpose, entry order included.
// Test infrastructure: built and run by tests/test_mf_adjoint_host.py under -fsanitize=address,undefined.
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include "../feastkit.jl_amd/csrc/fh_mf.hpp"

typedef std::complex<double> cd;
struct c2 { double x, y; };
static inline c2 fh_ing_zero(c2) { return c2{0.0, 0.0}; }
static inline c2 fh_ing_add(c2 a, c2 b) { return c2{a.x + b.x, a.y + b.y}; }
static inline c2 fh_ing_conj(c2 a) { return c2{a.x, -a.y}; }
#include "../feastkit.jl_amd/csrc/fh_ingest.hpp"

struct csr { int N; std::vector<int> rowptr, col; std::vector<double> a, b; bool bident; };

// 7-point stencil with a convection term: the two couplings of a grid edge differ
static csr grid3d(int nx, int ny, int nz, bool bident, unsigned seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> U(-0.4, 0.4);
    csr M; M.N = nx * ny * nz; M.bident = bident;
    M.rowptr.assign(M.N + 1, 0);
    auto id = [&](int i, int j, int k) { return (i * ny + j) * nz + k; };
    for (int i = 0; i < nx; ++i) for (int j = 0; j < ny; ++j) for (int k = 0; k < nz; ++k) {
        const int r = id(i, j, k);
        auto put = [&](int c, double v) { M.col.push_back(c); M.a.push_back(v); M.b.push_back(c == r ? 1.0 + 0.1 * v : 0.1 * v); };
        if (i > 0) put(id(i - 1, j, k), -1.0 + U(rng));
        if (j > 0) put(id(i, j - 1, k), -1.0 + U(rng));
        if (k > 0) put(id(i, j, k - 1), -1.0 + U(rng));
        put(r, 6.0 + U(rng));
        if (k + 1 < nz) put(id(i, j, k + 1), -1.0 + U(rng));
        if (j + 1 < ny) put(id(i, j + 1, k), -1.0 + U(rng));
        if (i + 1 < nx) put(id(i + 1, j, k), -1.0 + U(rng));
        M.rowptr[r + 1] = (int)M.col.size();
    }
    return M;
}

// the same stencil with random coefficients and no diagonal dominance: the pivot blocks interchange rows
static csr grid3d_random(int nx, int ny, int nz, unsigned seed) {
    csr M = grid3d(nx, ny, nz, false, seed);
    std::mt19937 rng(seed + 1000);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    for (int i = 0; i < M.N; ++i)
        for (int k = M.rowptr[i]; k < M.rowptr[i + 1]; ++k) { M.a[k] = U(rng); M.b[k] = M.col[k] == i ? 1.0 + 0.3 * std::fabs(U(rng)) : 0.0; }
    return M;
}

// random pattern (unsymmetric, optionally some rows without a stored diagonal), diagonally weighted
static csr random_pattern(int N, int per_row, unsigned seed, bool bident, bool drop_diag) {
    std::mt19937 rng(seed);
    csr M; M.N = N; M.bident = bident;
    M.rowptr.assign(N + 1, 0);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    for (int i = 0; i < N; ++i) {
        std::vector<int> cols;
        for (int q = 0; q < per_row; ++q) {
            int span = (q % 3 == 0) ? N : 40;
            int c = (i + (int)(rng() % (unsigned)(2 * span + 1)) - span) % N;
            if (c < 0) c += N;
            cols.push_back(c);
        }
        if (!(drop_diag && i % 7 == 3)) cols.push_back(i);
        std::sort(cols.begin(), cols.end());
        cols.erase(std::unique(cols.begin(), cols.end()), cols.end());
        for (int c : cols) { M.col.push_back(c); M.a.push_back(c == i ? 8.0 + U(rng) : U(rng)); M.b.push_back(c == i ? 2.0 + 0.1 * U(rng) : 0.1 * U(rng)); }
        M.rowptr[i + 1] = (int)M.col.size();
    }
    return M;
}

// the plan factored on the CPU for one shift z, then the adjoint traversal; returns the relative residual of (zB - A)^H x = rhs
static double execute_adjoint(const csr& M, const fh_mf::plan& P, cd z, int* info, int* swaps) {
    const int N = M.N;
    const size_t ng = P.groups.size();
    std::vector<std::vector<cd>> W(ng);
    std::vector<std::vector<int>> PR(ng);                           // row permutation of every pivot block (k_build_perm)
    *info = 0; *swaps = 0;
    for (size_t g = 0; g < ng; ++g) {
        const fh_mf::group& G = P.groups[g];
        const int n = G.n, np = G.np;
        W[g].assign(G.work_per * G.fronts.size(), cd(0, 0));
        PR[g].assign((size_t)np * G.fronts.size(), 0);
        for (size_t s = 0; s < G.fronts.size(); ++s)
            for (int p = P.fronts[G.fronts[s]].npiv; p < np; ++p) W[g][s * G.work_per + p + (size_t)p * n] = cd(1, 0);
        for (size_t q = G.asm_begin; q < G.asm_end; ++q) {
            const bool dg = P.asm_dst[q] < 0;
            const int d = dg ? ~P.asm_dst[q] : P.asm_dst[q];
            const int k = P.asm_src[q];
            cd v(0, 0);
            if (k >= 0) v = (M.bident ? cd(0, 0) : z * M.b[k]) - M.a[k];
            if (dg) v += z;
            W[g][d] += v;
        }
        for (int side = 0; side < 2; ++side)
            for (int c : G.kids[side]) {
                const fh_mf::front& C = P.fronts[c];
                const fh_mf::group& Gc = P.groups[C.group];
                const cd* S = W[C.group].data() + (size_t)C.slot * Gc.work_per;
                cd* F = W[g].data() + (size_t)P.fronts[C.parent].slot * G.work_per;
                for (int j = 0; j < C.nbnd; ++j)
                    for (int i = 0; i < C.nbnd; ++i)
                        F[P.rel[C.bnd_off + i] + (size_t)P.rel[C.bnd_off + j] * n] += S[(Gc.np + i) + (size_t)(Gc.np + j) * Gc.n];
            }
        for (size_t s = 0; s < G.fronts.size(); ++s) {              // partial LU, pivots among rows < np
            cd* F = W[g].data() + s * G.work_per;
            int* pr = PR[g].data() + s * np;
            for (int k = 0; k < np; ++k) pr[k] = k;
            for (int k = 0; k < np; ++k) {
                int p = k; double best = -1.0;
                for (int i = k; i < np; ++i) { const double m = std::fabs(F[i + (size_t)k * n].real()) + std::fabs(F[i + (size_t)k * n].imag()); if (m > best) { best = m; p = i; } }
                if (!(best > 0.0)) { *info = 1; return 1e300; }
                if (p != k) {
                    for (int c = 0; c < n; ++c) std::swap(F[k + (size_t)c * n], F[p + (size_t)c * n]);
                    std::swap(pr[k], pr[p]);
                    ++*swaps;
                }
                const cd inv = cd(1, 0) / F[k + (size_t)k * n];
                for (int i = k + 1; i < n; ++i) F[i + (size_t)k * n] *= inv;
                for (int c = k + 1; c < n; ++c) {
                    const cd u = F[k + (size_t)c * n];
                    if (u == cd(0, 0)) continue;
                    for (int i = k + 1; i < n; ++i) F[i + (size_t)c * n] -= F[i + (size_t)k * n] * u;
                }
            }
        }
    }
    std::mt19937 rng(7);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    std::vector<cd> rhs(N), x(N);
    for (int i = 0; i < N; ++i) rhs[i] = cd(U(rng), U(rng));
    // Z: front vectors of the ascending pass (boundary rows = what the parent adds), Y: w1, then [x1; v2]
    std::vector<std::vector<cd>> Z(ng), Y(ng);
    for (size_t g = 0; g < ng; ++g) {                               // ascending: U^H
        const fh_mf::group& G = P.groups[g];
        const int n = G.n, np = G.np;
        Z[g].assign((size_t)n * G.fronts.size(), cd(0, 0));
        Y[g].assign((size_t)n * G.fronts.size(), cd(0, 0));
        for (size_t s = 0; s < G.fronts.size(); ++s) {
            const fh_mf::front& F = P.fronts[G.fronts[s]];
            for (int p = 0; p < F.npiv; ++p) Z[g][s * n + p] = rhs[P.perm[F.piv0 + p]];     // plan order, no pivot permutation
        }
        for (int side = 0; side < 2; ++side)
            for (int c : G.kids[side]) {
                const fh_mf::front& C = P.fronts[c];
                const fh_mf::group& Gc = P.groups[C.group];
                for (int i = 0; i < C.nbnd; ++i)
                    Z[g][(size_t)P.fronts[C.parent].slot * n + P.rel[C.bnd_off + i]] += Z[C.group][(size_t)C.slot * Gc.n + Gc.np + i];
            }
        for (size_t s = 0; s < G.fronts.size(); ++s) {
            const cd* F = W[g].data() + s * G.work_per;
            cd* zz = Z[g].data() + s * n;
            cd* w = Y[g].data() + s * n;
            for (int k = 0; k < np; ++k) {                                                  // w1 = U11^-H z1, ascending
                cd sum = zz[k];
                for (int c = 0; c < k; ++c) sum -= std::conj(F[c + (size_t)k * n]) * w[c];
                w[k] = sum / std::conj(F[k + (size_t)k * n]);
            }
            for (int j = np; j < n; ++j)                                                    // z2 -= U12^H w1
                for (int k = 0; k < np; ++k) zz[j] -= std::conj(F[k + (size_t)j * n]) * w[k];
        }
    }
    for (size_t g = ng; g-- > 0;) {                                 // descending: L^H, then the row permutation
        const fh_mf::group& G = P.groups[g];
        const int n = G.n, np = G.np;
        for (size_t s = 0; s < G.fronts.size(); ++s) {
            const fh_mf::front& F = P.fronts[G.fronts[s]];
            const cd* A = W[g].data() + s * G.work_per;
            cd* y = Y[g].data() + s * n;
            const int* pr = PR[g].data() + s * np;
            if (F.parent >= 0) {
                const fh_mf::front& Pf = P.fronts[F.parent];
                const fh_mf::group& Gp = P.groups[Pf.group];
                for (int i = 0; i < F.nbnd; ++i) y[np + i] = Y[Pf.group][(size_t)Pf.slot * Gp.n + P.rel[F.bnd_off + i]];
            }
            for (int i = F.nbnd; i < G.nb; ++i) y[np + i] = cd(0, 0);
            std::vector<cd> v(np);
            for (int k = np - 1; k >= 0; --k) {                                             // v1 = L11^-H (w1 - L21^H v2)
                cd sum = y[k];
                for (int i = k + 1; i < np; ++i) sum -= std::conj(A[i + (size_t)k * n]) * v[i];
                for (int i = np; i < n; ++i) sum -= std::conj(A[i + (size_t)k * n]) * y[i];
                v[k] = sum;
            }
            for (int k = 0; k < np; ++k) y[pr[k]] = v[k];                                   // x1[p[i]] = v1[i], last
            for (int p = 0; p < F.npiv; ++p) x[P.perm[F.piv0 + p]] = y[p];
        }
    }
    // r = rhs - S^H x, S = zB - A row by row (identity B: z on the diagonal whether it is stored or not)
    std::vector<cd> r(rhs);
    for (int i = 0; i < N; ++i) {
        bool has = false;
        for (int k = M.rowptr[i]; k < M.rowptr[i + 1]; ++k) {
            const int c = M.col[k];
            if (c == i) has = true;
            const cd s = (M.bident ? (c == i ? z : cd(0, 0)) : z * M.b[k]) - M.a[k];
            r[c] -= std::conj(s) * x[i];
        }
        if (M.bident && !has) r[i] -= std::conj(z) * x[i];
    }
    double rn = 0.0, bn = 0.0;
    for (int i = 0; i < N; ++i) { rn += std::norm(r[i]); bn += std::norm(rhs[i]); }
    return std::sqrt(rn / bn);
}

// ---- part 2: the conjugate-transposed CSR set --------------------------------------------------------------------------
static inline cd as_cd(double v) { return cd(v, 0.0); }
static inline cd as_cd(c2 v) { return cd(v.x, v.y); }
static inline void rnd(std::mt19937& rng, double& v) { v = std::uniform_real_distribution<double>(-1, 1)(rng); }
static inline void rnd(std::mt19937& rng, c2& v) { std::uniform_real_distribution<double> U(-1, 1); v.x = U(rng); v.y = U(rng); }

template <typename VT>
static int transpose_case(const char* name, int N, double fill, unsigned seed, bool bident, bool empty_rows) {
    std::mt19937 rng(seed);
    std::vector<int> rowptr(N + 1, 0), col;
    std::vector<VT> av, bv;
    for (int i = 0; i < N; ++i) {
        if (!(empty_rows && i % 5 == 2)) {
            std::vector<int> cols;
            for (int c = 0; c < N; ++c)
                if (!(empty_rows && c % 7 == 4) && (rng() % 1000) < (unsigned)(1000 * fill)) cols.push_back(c);
            std::shuffle(cols.begin(), cols.end(), rng);            // the stored order inside a row is arbitrary (the ingest moves entries)
            for (int c : cols) {
                VT a, b; rnd(rng, a); rnd(rng, b);
                col.push_back(c); av.push_back(a); if (!bident) bv.push_back(b);
            }
        }
        rowptr[i + 1] = (int)col.size();
    }
    std::vector<int> rpt, clt;
    std::vector<VT> avt, bvt;
    fh_adjoint_csr<VT>(N, rowptr, col, av.data(), bident ? nullptr : bv.data(), rpt, clt, avt, bvt);
    int bad = 0;
    if ((int)rpt.size() != N + 1 || rpt[0] != 0 || rpt[N] != rowptr[N] || clt.size() != col.size() || avt.size() != col.size() ||
        bvt.size() != (bident ? 0 : col.size())) { std::printf("FAIL %s: sizes\n", name); return 1; }
    std::vector<cd> DA((size_t)N * N, cd(0, 0)), DB((size_t)N * N, cd(0, 0)), TA((size_t)N * N, cd(0, 0)), TB((size_t)N * N, cd(0, 0));
    for (int i = 0; i < N; ++i)
        for (int k = rowptr[i]; k < rowptr[i + 1]; ++k) { DA[(size_t)i * N + col[k]] = as_cd(av[k]); if (!bident) DB[(size_t)i * N + col[k]] = as_cd(bv[k]); }
    for (int i = 0; i < N; ++i) {
        if (rpt[i + 1] < rpt[i]) { std::printf("FAIL %s: rowptr\n", name); return 1; }
        for (int k = rpt[i]; k < rpt[i + 1]; ++k) {
            if (clt[k] < 0 || clt[k] >= N) { std::printf("FAIL %s: column range\n", name); return 1; }
            if (k > rpt[i] && clt[k - 1] >= clt[k]) ++bad;          // the fixed order: ascending columns in every transposed row
            TA[(size_t)i * N + clt[k]] = as_cd(avt[k]);
            if (!bident) TB[(size_t)i * N + clt[k]] = as_cd(bvt[k]);
        }
    }
    if (bad) { std::printf("FAIL %s: %d entries out of the fixed order\n", name, bad); return 1; }
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j)
            if (TA[(size_t)i * N + j] != std::conj(DA[(size_t)j * N + i]) || TB[(size_t)i * N + j] != std::conj(DB[(size_t)j * N + i])) ++bad;
    if (bad) { std::printf("FAIL %s: %d entries differ from the dense conjugate transpose\n", name, bad); return 1; }
    std::printf("%s: N %d nnz %d ok\n", name, N, rowptr[N]);
    return 0;
}

int main() {
    struct tc { const char* name; csr M; int leaf; };
    std::vector<tc> cases;
    cases.push_back({"grid 12x10x8 leaf 8", grid3d(12, 10, 8, false, 1), 8});
    cases.push_back({"grid 12x10x8 leaf 64", grid3d(12, 10, 8, false, 1), 64});
    cases.push_back({"grid 9x9x9 B=I", grid3d(9, 9, 9, true, 2), 16});
    cases.push_back({"grid 40x25x1 leaf 64", grid3d(40, 25, 1, false, 3), 64});
    cases.push_back({"grid 40x25x1 leaf 8", grid3d(40, 25, 1, false, 3), 8});
    cases.push_back({"grid 30x1x1 (path)", grid3d(30, 1, 1, false, 4), 8});
    cases.push_back({"random 700", random_pattern(700, 4, 1, false, false), 32});
    cases.push_back({"random 900 B=I, missing diagonals", random_pattern(900, 3, 2, true, true), 24});
    cases.push_back({"random 600 B=I, missing diagonals, leaf 64", random_pattern(600, 4, 5, true, true), 64});
    cases.push_back({"grid 8x7x6 random coefficients leaf 8", grid3d_random(8, 7, 6, 21), 8});
    cases.push_back({"grid 8x7x6 random coefficients leaf 64", grid3d_random(8, 7, 6, 21), 64});
    cases.push_back({"grid 24x20x1 random coefficients", grid3d_random(24, 20, 1, 22), 16});
    cases.push_back({"random dense-ish 200", random_pattern(200, 40, 3, false, false), 16});
    cases.push_back({"tiny 5", random_pattern(5, 2, 4, false, false), 8});
    int bad = 0, swaps_all = 0;
    for (tc& c : cases) {
        fh_mf::plan P;
        const int rc = fh_mf::make_plan(c.M.N, c.M.rowptr, c.M.col, c.M.bident, c.leaf, P);
        if (rc) { std::printf("FAIL make_plan %s (%d)\n", c.name, rc); ++bad; continue; }
        int info = 0, swaps = 0;
        const double res = execute_adjoint(c.M, P, cd(0.7, 0.9), &info, &swaps);
        swaps_all += swaps;
        std::printf("%s: N %d fronts %zu groups %zu row interchanges %d  adjoint residual %.2e  info %d\n", c.name, c.M.N, P.fronts.size(), P.groups.size(), swaps, res, info);
        if (info || !(res < 1e-11)) { std::printf("FAIL residual in %s\n", c.name); ++bad; }
    }
    if (swaps_all == 0) { std::printf("FAIL no case interchanged a row: the permutation step went untested\n"); ++bad; }
    bad += transpose_case<double>("transpose real, with B", 61, 0.08, 11, false, false);
    bad += transpose_case<double>("transpose real, B = I, empty rows and columns", 75, 0.05, 12, true, true);
    bad += transpose_case<c2>("transpose complex, with B, empty rows and columns", 90, 0.06, 13, false, true);
    bad += transpose_case<c2>("transpose complex, B = I", 40, 0.3, 14, true, false);
    bad += transpose_case<double>("transpose 1 x 1", 1, 1.0, 15, false, false);
    bad += transpose_case<c2>("transpose all empty", 9, 0.0, 16, false, false);
    std::printf(bad ? "FAILED (%d)\n" : "OK\n", bad);
    return bad ? 1 : 0;
}
