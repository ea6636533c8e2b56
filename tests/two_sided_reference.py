"""Host restatement of the two-sided FEAST loop of feast_hip_general_two_sided (numpy / scipy only): every shifted
system goes through scipy.linalg.lu_factor once and lu_solve with trans=0 (forward) or trans=2 (conjugate transposed) --
LAPACK's ZGETRS 'N' / 'C' on one factorisation per node, which is what the device path claims to do.

    P_R = sum_e w_e S_e^-1 B Q_R,   P_L = sum_e conj(w_e) S_e^-H B^H Q_L,   S_e = z_e B - A
    Aq = P_L^H A P_R,  Bq = P_L^H B P_R;  lam, V_L, V_R = eig(Aq, Bq);  inside-first by the contour -> M
    X_R = P_R V_R, X_L = P_L V_L with unit columns;  res_R = ||A x - lam B x||, res_L = ||A^H y - conj(lam) B^H y||, both
    over max(|lam|, 1);  epsout = max_{j < M} max(res_R, res_L);  stop at epsout <= tol or loop >= fpm[4]."""
import numpy as np
import scipy.linalg as sla

from feastkit_jl_amd.contour import feast_gcontour, feast_inside_gcontour
from feastkit_jl_amd.hip_backend import seeded_subspace
from feastkit_jl_amd.parameters import feast_tolerance, feastdefault, feastinit


def residuals(A, B, lam, X, Y):
    """(res_R, res_L) of unit-column X, Y for the values lam, in fp64 on the host."""
    BX = X if B is None else B @ X
    BhY = Y if B is None else B.conj().T @ Y
    sc = np.maximum(np.abs(lam), 1.0)
    rr = np.linalg.norm(A @ X - BX * lam[None, :], axis=0) / sc
    rl = np.linalg.norm(A.conj().T @ Y - BhY * np.conj(lam)[None, :], axis=0) / sc
    return rr, rl


def two_sided_reference(A, B, center, radius, M0, fpm=None, seed=20260515):
    """-> dict(lam, X, Y, M, info, epsout, loop, eps_hist, res_right, res_left); X unit columns, Y scaled to y^H B x = 1,
    the first M pairs sorted by |lam|^2."""
    N = A.shape[0]
    fpm = feastinit() if fpm is None else fpm
    feastdefault(fpm)
    A = np.asarray(A, dtype=np.complex128)
    Bc = None if B is None else np.asarray(B, dtype=np.complex128)
    Zne, Wne = feast_gcontour(complex(center), float(radius), fpm)
    Bm = np.eye(N) if Bc is None else Bc
    factors = [sla.lu_factor(z * Bm - A) for z in Zne]          # one factorisation per node for the whole solve
    QR = seeded_subspace(N, M0, seed)
    QL = seeded_subspace(N, M0, seed + 1, complex_values=True)
    tol, maxloop = feast_tolerance(fpm), int(fpm[4])
    hist, hr, hl = [], [], []
    loop = 0
    while True:
        rhsR = QR if Bc is None else Bc @ QR
        rhsL = QL if Bc is None else Bc.conj().T @ QL
        PR = sum(w * sla.lu_solve(f, rhsR, trans=0) for f, w in zip(factors, Wne))
        PL = sum(np.conj(w) * sla.lu_solve(f, rhsL, trans=2) for f, w in zip(factors, Wne))
        Aq = PL.conj().T @ (A @ PR)
        Bq = PL.conj().T @ (PR if Bc is None else Bc @ PR)
        lam, VL, VR = sla.eig(Aq, Bq, left=True, right=True)
        ins = [i for i in range(M0) if feast_inside_gcontour(lam[i], complex(center), float(radius), fpm)]
        M = len(ins)
        if M == 0:
            return {"M": 0, "info": 5, "loop": loop, "eps_hist": hist}
        perm = np.array(ins + [i for i in range(M0) if i not in set(ins)])
        lam = lam[perm]
        X = PR @ VR[:, perm]
        Y = PL @ VL[:, perm]
        X = X / np.linalg.norm(X, axis=0)
        Y = Y / np.linalg.norm(Y, axis=0)
        rr, rl = residuals(A, Bc, lam[:M], X[:, :M], Y[:, :M])
        epsout = float(max(rr.max(), rl.max()))
        hist.append(epsout); hr.append(float(rr.max())); hl.append(float(rl.max()))
        if epsout <= tol or loop >= maxloop:
            break
        loop += 1
        QR, QL = X, Y
    order = sorted(range(M), key=lambda i: abs(lam[i]) ** 2)
    X, Y, lam = X[:, :M][:, order], Y[:, :M][:, order], lam[:M][order]
    d = np.einsum("ij,ij->j", Y.conj(), X if Bc is None else Bc @ X)
    return {"lam": lam, "X": X, "Y": Y / np.conj(d)[None, :], "M": M, "info": 0 if epsout <= tol else 5, "epsout": epsout,
            "loop": loop, "eps_hist": hist, "res_right": hr, "res_left": hl, "overlap": np.abs(d)}


_runs = {}


def reference_run(params):
    """The restatement's result for a case of two_sided_cases (tol 1e-12, fpm[4] = 20), computed once and shared by the
    host and the GPU tests; read only."""
    import two_sided_cases as tc
    if params not in _runs:
        case = tc.make_case(*params)
        fpm = feastinit()
        fpm[3], fpm[4] = 12, 20
        _runs[params] = two_sided_reference(case["A"], case["B"], tc.CENTER, tc.RADIUS, case["M0"], fpm)
    return _runs[params]
