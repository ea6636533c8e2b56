"""User-facing entry points with the reference's names and argument meaning
(src/interfaces/feast_interfaces.jl:143-379), restricted to the ``:hip`` backend this
package provides.  Everything else of the reference API stays on the Julia host."""
from __future__ import annotations

import math
import os
import warnings

import numpy as np
import scipy.sparse as sp

from .engine import HipEngine
from .contour import feast_contour, feast_gcontour
from .hip_backend import (DIRECT_SOLVERS, ESTIMATE_SEED, check_direct_nodes, check_ortho, check_precond, check_two_sided, feast_hip_estimate,
                          feast_hip_general, feast_hip_general_two_sided, feast_hip_hermitian, feast_hip_polynomial, feast_hip_polynomial_projected,
                          POLY_METHODS, POLY_RESIDUALS, POLY_SET_ASIDE, feast_hip_nonlinear, feast_hip_poly_estimate, nep_functions,
                          nep_table)
from .ingest import polynomial_union_csr
from .parameters import feastdefault, feastinit
from .types import FEAST_UNINITIALIZED, FeastHipError, FeastResult

_BACKENDS = ("hip", "auto")   # _normalize_backend whitelist edit, feast_interfaces.jl:44


def _is_hermitian(A, tol=0.0):
    if sp.issparse(A):
        D = (A - A.conj().T)
        return D.nnz == 0 or abs(D).max() <= tol
    return np.array_equal(A, A.conj().T)


def _band_widths(A, B):
    """(kl, ku) of the union pattern of A and B in the caller's order."""
    kl = ku = 0
    for M in (A, B):
        if M is None:
            continue
        c = sp.coo_matrix(M)
        if c.nnz:
            kl = max(kl, int((c.row - c.col).max()))
            ku = max(ku, int((c.col - c.row).max()))
    return kl, ku


# kl + ku up to which the library's direct plan is the one-workgroup narrow band LU (FH_BAND_NARROW, csrc/fh_banded.hip)
_NARROW_BAND = 64


def _sparse_direct_solver(A, B, nodes, budget_bytes=32 << 30, dense_limit=12288, allow_band=True):
    """``solver=:direct`` for sparse input (UMFPACK in the reference, src/sparse/feast_sparse.jl:334-342, :943):
      "banded" -- the union pattern of A and B is a narrow band whose LU factors (2 kl + ku + 1 rows per column and
                  node, complex128) fit the budget: batched banded LU on the CSR arrays;
      "dense"  -- any other pattern up to N = dense_limit whose N x N complex128 factors (one per node, plus A and B)
                  fit the budget: the matrix is expanded on ingest and factored by the batched dense LU -- an exact
                  direct solve like the reference's, at O(N^3) per node, which the MFMA LU affords at these sizes;
      "krylov" -- everything larger: the batched Krylov solvers (north_star's iterative path).
    ``allow_band=False`` leaves the narrow-band answer out (the two-sided call: that LU has no adjoint substitution)."""
    kl, ku = _band_widths(A, B)
    ldab = 2 * kl + ku + 1
    N = A.shape[0]
    if allow_band and 2 * kl + ku + 1 <= 3500 and ldab * N * 16 * max(nodes, 1) <= budget_bytes and kl + ku <= 512:
        return "banded"
    if N <= dense_limit and (max(nodes, 1) + 2) * N * N * 16 <= budget_bytes:
        return "dense"
    return "krylov"


# `solver=:direct` on a sparse Hermitian pencil beyond the narrow-band / dense windows: the sparse direct solver (multifrontal
# LU, or the band LU) is taken outright when all its factorisations together cost at most this many flop (feasthip_direct_plan_flops
# x local nodes), else the Krylov path runs first with the direct solver as its fallback.  4e11: with the multifrontal plan a 2-D
# pencil of 50 000 unknowns (1e11 in all) is a 0.1 s direct call against 0.5 s of Krylov loops, while cfg 3 (1.7e12 in all: 0.19 s)
# stays with the Krylov path (0.16 s).  With the band LU alone (round 3) the switch was off: its block steps are a chain of panel
# kernels, ~0.4 s for N = 50 000 however thin the band.  0: never.
_DIRECT_FLOPS = float(os.environ.get("FEASTKIT_DIRECT_FLOPS", "4e11"))


def _direct_label(eng):
    """what FEASTHIP_SOLVER_BANDED runs for the problem set on the engine (feasthip_band_plan)."""
    try:
        return "multifrontal LU on a nested-dissection tree" if eng.band_plan()[3] == HipEngine.PLAN_MULTIFRONTAL else "band LU after reverse Cuthill-McKee"
    except Exception:
        return "band LU after reverse Cuthill-McKee"


def _band_direct_fits(eng, A, B, nodes, group=None, complexify=False, max_flops=1e14):
    """True when the sparse direct solver for general patterns (multifrontal LU on a nested-dissection tree, or reverse
    Cuthill-McKee + blocked band LU on the dense kernels: FEASTHIP_SOLVER_BANDED) can hold one factor per local quadrature node in the free device memory.  Sets the
    problem on the engine (a later set_problem with the same matrices is free: content fingerprint)."""
    import torch
    if complexify:
        A = A.astype(np.complex128) if not np.iscomplexobj(A.data) else A
        B = None if B is None else (B.astype(np.complex128) if not np.iscomplexobj(B.data) else B)
    world = 1
    if group is not None:
        import torch.distributed as dist
        world = dist.get_world_size(group)
    local = -(-max(int(nodes), 1) // world)
    try:
        eng.set_problem(A, B)
        kl, ku, nbytes, blocked = eng.band_plan()
        free, _total = torch.cuda.mem_get_info(eng.device)
        panels = 2 * local * A.shape[0] * 64 * 16
        # the elimination costs 8 N kl (kl + ku) flop per node: beyond ~1e14 in all (seconds of MFMA time) a band this wide
        # is no longer the cheap way to a direct solve
        # (or the multifrontal elimination's padded fronts, when the library's plan took that: blocked == 2)
        flops = eng.direct_plan_flops() * local
        fits = bool((local + 1) * nbytes + panels <= 0.85 * free and flops <= max_flops)
    except FeastHipError:
        fits = False
    if world > 1:
        # every rank decides from ITS free memory: the ranks must agree (different solvers have different tolerance
        # semantics, and a rank that alone takes the band LU would fail later in its slot allocation) -- logical AND over
        # the group, through the control plane (any backend)
        votes = [None] * world
        dist.all_gather_object(votes, fits, group=group)
        fits = all(votes)
    return fits


def _single_precision(*mats):
    """True when every matrix given is float32 / complex64: the reference preserves the element type of such input
    (test/runtests.jl:281-304) and stops at max(10^-fpm[3], sqrt(eps(Float32))) (src/core/feast_parameters.jl:398-405)."""
    dts = [np.dtype((M.dtype if not sp.issparse(M) else M.data.dtype)) for M in mats if M is not None]
    return bool(dts) and all(dt in (np.dtype(np.float32), np.dtype(np.complex64)) for dt in dts)


def _promote(M):
    """float32 / complex64 -> float64 / complex128 (the C ABI takes f64 / c128 only: the shim converts on the way in and
    casts the results back, so that single-precision callers keep their element types)."""
    if M is None:
        return None
    dt = np.complex128 if np.iscomplexobj(M.data if sp.issparse(M) else M) else np.float64
    return M.astype(dt)


def _demote(res, cplx_lambda):
    return FeastResult(res.lambda_.astype(np.complex64 if cplx_lambda else np.float32),
                       res.q.astype(np.complex64 if np.iscomplexobj(res.q) else np.float32), res.M, res.res.astype(np.float32), res.info,
                       float(res.epsout), res.loop, res.stats)


def _densify(M):
    return None if M is None else np.asfortranarray(M.toarray())


# What `solver=:direct` (the reference's default, UMFPACK for sparse input: src/sparse/feast_sparse.jl:334-342 via
# src/core/feast_backend_utils.jl:166-198) maps to when the pattern is not a narrow band: the batched Krylov path in
# the configuration that converges on large problems -- COCG for real-symmetric input (z B - A is complex symmetric:
# one operator application per iteration), BiCGStab otherwise; Ritz-pair warm starts, inexact inner solves (relative
# reduction 3e-2 per refinement loop, at most 100 iterations per loop) and, for real input, the real projection.
# The outer stop test is the reference's (max residual of the pairs inside <= 10^-fpm[3]).
_KRYLOV_DEFAULT = dict(warm_start=True, inner_rtol=3e-2, solver_maxiter=100)


_warned = set()


def _warn_substitution(sub):
    """One warning per process and configuration: the reference's `solver=:direct` means a sparse LU, which this
    backend replaces by a Krylov solver for patterns that are not a narrow band (also recorded in
    ``result.stats["solver_substitution"]``)."""
    key = (sub["used"], sub["warm_start"], sub["inner_rtol"], sub["solver_maxiter"])
    if key in _warned:
        return
    _warned.add(key)
    warnings.warn("feastkit.jl_amd: solver='direct' on a sparse pattern that is not a narrow band runs the batched "
                  f"{sub['used']} solver (warm_start={sub['warm_start']}, inner_rtol={sub['inner_rtol']}, "
                  f"<= {sub['solver_maxiter']} iterations per refinement loop) instead of a sparse LU",
                  RuntimeWarning, stacklevel=3)


def _check_direct_nodes_early(direct_nodes, A, solver, fpm, ne_slot, contour):
    """The ``direct_nodes`` keyword checked before any device work (ValueError): sparse input, a Krylov solver (or the
    default, which may resolve to one), indices inside the contour's node count (fpm[ne_slot], or the caller's contour)."""
    if direct_nodes is None:
        return
    f = feastinit() if fpm is None else np.array(fpm).copy()
    feastdefault(f)
    ne = len(contour[0]) if contour is not None else int(f[ne_slot])
    check_direct_nodes(direct_nodes, ne, sp.issparse(A), "cocg" if solver in ("direct", "krylov") else solver)


def _release_band_factors(eng, keep):
    """The sparse direct solver's factors stay on the engine across set_contour and across calls (16 x 2.8 GB on cfg 3).
    Inside one call that is the reference's factor cache; beyond it, it is device memory a later Krylov / GMRES call on
    the same engine no longer has (and that _band_direct_fits would count as taken).  Whatever path of the call created
    them -- solver='banded', the automatic choice of feast_general, the Krylov-to-direct fallback -- they go when the
    call returns unless the caller asked to keep them."""
    if keep:
        return
    try:
        eng.free_factors()
    except FeastHipError:
        pass                                   # a poisoned handle reports through the result, not from the clean-up


# ---- stochastic eigenvalue-count estimate (fpm[14] = 2) and M0 = "auto" ----------------------------------------------
ESTIMATE_TOL = 1e-8        # inner tolerance of the estimate's Krylov solves (zero start): loose solves bias every t_j
AUTO_SAMPLES = 64          # samples of the estimate behind M0 = "auto"


def _estimate_solver(eng, A, B, nodes, solver, group, general):
    """The solver of the estimate's sweep: the caller's when named, else (solver=:direct) the direct solver where it applies
    -- dense input, or a sparse pattern whose direct factors fit the device (_band_direct_fits) -- and otherwise the Krylov
    solver for the pencil (COCG for real symmetric input, BiCGStab otherwise)."""
    if solver == "sparse_direct":
        return "banded"
    if solver not in ("direct", "lu", "krylov"):
        return solver
    if not sp.issparse(A):
        return "direct"
    if solver != "krylov" and _band_direct_fits(eng, A, B, nodes, group, complexify=general):
        return "banded"
    real_input = not (np.iscomplexobj(A.data) or (B is not None and np.iscomplexobj(B.data)))
    return "cocg" if (real_input and not general) else "bicgstab"


def _run_estimate(eng, A, B, Zne, Wne, general, m, seed, solver, solver_tol, solver_maxiter, solver_restart, group):
    """(info, estimate dict or None) of feast_hip_estimate with the solver rule above; the direct factors go afterwards."""
    use = _estimate_solver(eng, A, B, len(Zne), solver, group, general)
    if general:                                     # the shifted systems of the full contour are complex (feast_hip_general)
        A = A.astype(np.complex128) if not np.iscomplexobj(A.data if sp.issparse(A) else A) else A
        B = None if B is None else (B.astype(np.complex128) if not np.iscomplexobj(B.data if sp.issparse(B) else B) else B)
    tol = float(solver_tol) if solver_tol and float(solver_tol) > 0.0 else ESTIMATE_TOL
    try:
        return feast_hip_estimate(eng, A, B, Zne, Wne, 1.0 if general else 2.0, int(m), general=general,
                                  seed=ESTIMATE_SEED if seed is None else int(seed), solver=use, solver_tol=tol,
                                  solver_maxiter=2000 if solver_maxiter is None else int(solver_maxiter),
                                  solver_restart=solver_restart, group=group)
    finally:
        _release_band_factors(eng, False)


def _estimate_result(N, info, est, real):
    """FeastResult of an fpm[14] = 2 call: no eigenpairs, M = max(0, round(Re mean)), the estimate in stats."""
    M = 0 if est is None else max(0, int(round(float(np.real(est["mean"])))))
    q = np.zeros((N, 0), dtype=np.float64 if real else np.complex128)
    lam = np.zeros(0, dtype=np.float64 if real else np.complex128)
    return FeastResult(lam, q, M, np.zeros(0), int(info), 0.0, 0, {"estimate": est})


def auto_M0(est, N):
    """M0 for a solve after an estimate: 1.5 x (mean + 2 stderr) (FEAST's sizing advice), at least 8, at most N."""
    return int(min(N, max(8, math.ceil(1.5 * (float(np.real(est["mean"])) + 2.0 * float(est["stderr"]))))))


def _estimate_fpm(fpm):
    """Parameters of the estimate behind M0 = "auto": the caller's, with fpm[14] = 2 and the estimate's own node counts
    (fpm[2] = 3, fpm[8] = 6) -- the contour shape (fpm[16], fpm[18], fpm[19]) stays the caller's."""
    e = (feastinit() if fpm is None else np.array(fpm, dtype=np.int64)).copy()
    e[14], e[2], e[8] = 2, FEAST_UNINITIALIZED, FEAST_UNINITIALIZED
    return feastdefault(e)


def _engine(engine, device):
    return engine if engine is not None else HipEngine(device)


def feast(A, B=None, interval=None, *, M0=10, fpm=None, backend="hip", solver="direct", solver_tol=0.0,
          solver_maxiter=None, solver_restart=30, warm_start=None, inner_rtol=None, real_projection=None,
          inner_precision=64, group=None, engine=None, device=0, Q0=None, contour=None, contour_policy=None,
          keep_factors=False, seed=None, direct_nodes=None, ortho="mgs", precond=None, precond_shifts=1):
    """feast(A, [B,] (Emin, Emax); M0, fpm, backend=:hip) for real-symmetric / Hermitian
    dense (numpy) or sparse (scipy) matrices.  Real input is complexified and the result is
    real.(q), exactly as feast_sygv!/feast_scsrgv! do (src/dense/feast_dense.jl:362-387).
    ``contour=(Zne, Wne)``: caller-supplied half-contour nodes and weights, the reference's "x" drivers
    (feast_hcsrgvx!/feast_heevx!, test/runtests.jl:415-440).
    ``keep_factors``: the band-LU factors of the sparse direct solver (one per quadrature node: 2.8 GB each on cfg 3) are
    cached across the refinement loops of ONE call, like the reference's per-call ``lu(zB - A)`` cache
    (src/sparse/feast_sparse.jl:335-341), and released when the call returns; ``True`` leaves them resident on the engine
    for a repeated call on the same contour (``engine.free_factors()`` releases them).
    ``fpm[14] = 2``: no eigensolve -- a stochastic estimate of the number of eigenvalues in the interval from one contour
    sweep over M0 Rademacher columns (hip_backend.feast_hip_estimate; ``seed`` picks the block, default the package seed).
    The result has no eigenpairs, M = round(mean) and ``stats["estimate"]`` = {mean, stderr, samples, nodes, solver, seed,
    seconds}; a node that fails (status 5 / 8) gives that info and ``stats["estimate"] = None``.
    ``M0="auto"``: such an estimate with 64 samples first, then the solve with M0 = min(N, max(8, ceil(1.5 (mean +
    2 stderr)))); the estimate and the chosen M0 are in ``stats["estimate"]`` / ``stats["M0_auto"]``.
    ``direct_nodes`` (sparse input on the Krylov path: solver cocg / bicgstab / iterative, or the default when it resolves to
    them): contour nodes the sweeps solve with the sparse direct solver instead of iterating (per-node solver,
    feasthip_set_node_solver) -- a list of node indices, an int k (the k slowest nodes of the first loop, from the second
    on) or "auto" (feasthip_policy_pick_direct_nodes after every loop).  ``stats["direct_nodes"]`` has one entry per loop.
    ``ortho``: what orthonormalises a rank-deficient subspace (every loop of an exact solver): "mgs", the column-pivoted
    Gram-Schmidt (default), or "cholqr_rr", the staged rank-revealing Cholesky-QR; same rank rule.  ``stats["ortho"]`` has one
    entry per loop: method used ("cholqr" = the full-rank fast path), stages, fell_back, rank.
    ``precond="shift"`` (sparse input, ``solver="gmres"``): the GMRES sweeps are preconditioned by the sparse LU of
    z_p B - A at a few pivot shifts z_p -- one factorisation serves every node of its pivot, so the call holds
    ``precond_shifts`` factors where ``solver="sparse_direct"`` holds one per node (feasthip_set_preconditioner).
    ``precond_shifts``: an int k (default 1) -- the contour's nodes in order are cut into k arcs of equal count (+-1), each
    arc's pivot is its middle node -- or a list of complex pivots off the real axis (every node takes the nearest).  Restarted
    GMRES under ONE pivot stalls when more eigenvalues lie near the contour than the restart length: raise ``solver_restart``
    or ``precond_shifts``.  Any other solver, dense input, ``inner_precision=32``, ``group=``, ``direct_nodes=``,
    ``fpm[14] = 2`` and ``M0="auto"`` raise ValueError.  ``stats["precond"]`` has one entry per loop: pivots, node_pivot,
    factorizations, substitution_sweeps, lock_steps per node, factor_bytes, fell_back.  The factors go when the call returns
    (``keep_factors``).
    """
    if isinstance(M0, str):
        if M0 != "auto":
            raise ValueError("M0 must be an integer or 'auto'")
        check_precond(precond, precond_shifts, auto_m0=True)
        return _feast_auto(feast, A, B, interval, fpm=fpm, backend=backend, solver=solver, solver_tol=solver_tol,
                           solver_maxiter=solver_maxiter, solver_restart=solver_restart, warm_start=warm_start,
                           inner_rtol=inner_rtol, real_projection=real_projection, inner_precision=inner_precision,
                           group=group, engine=engine, device=device, Q0=Q0, contour=contour, contour_policy=contour_policy,
                           keep_factors=keep_factors, seed=seed, direct_nodes=direct_nodes, ortho=ortho)
    if interval is None and B is not None and isinstance(B, tuple):
        B, interval = None, B              # feast(A, (Emin, Emax)) form
    if backend not in _BACKENDS:
        raise ValueError(f"Unknown backend '{backend}' (this package provides: hip)")
    if A.shape[0] != A.shape[1]:
        raise ValueError("Matrix A must be square")
    if B is not None and B.shape != A.shape:
        raise ValueError("Matrix B must match size of A")
    check_precond(precond, precond_shifts, sparse=sp.issparse(A), solver=solver, inner_precision=inner_precision, group=group,
                  direct_nodes=direct_nodes, estimate=fpm is not None and int(fpm[14]) == 2)
    _check_direct_nodes_early(direct_nodes, A, solver, fpm, 2, contour)
    check_ortho(ortho)
    eng = _engine(engine, device)
    # input checks and the pattern scan cost tens of milliseconds on a 50 000-unknown CSR pair (sparse transposes): a
    # repeated call with the same matrices (content fingerprint, engine.py) skips them
    fp = (HipEngine._fingerprint(A), HipEngine._fingerprint(B)) if sp.issparse(A) else None
    known = fp is not None and fp[0] and fp[1] is not False and getattr(eng, "_checked", {}).get("fp") == fp
    if not known:
        if not _is_hermitian(A):
            raise ValueError("Matrix A must be Hermitian")
        if B is not None and not _is_hermitian(B):
            raise ValueError("Matrix B must be Hermitian positive definite")
    single = _single_precision(A, B)
    if single:
        A, B = _promote(A), _promote(B)
    Emin, Emax = float(interval[0]), float(interval[1])
    fpm = feastinit() if fpm is None else fpm
    aspect_unset = int(fpm[18]) == FEAST_UNINITIALIZED      # the caller left the contour shape to the library
    feastdefault(fpm)
    N = A.shape[0]
    M0 = min(int(M0), N)
    real_input = not (np.iscomplexobj(A.data if sp.issparse(A) else A) or
                      (B is not None and np.iscomplexobj(B.data if sp.issparse(B) else B)))
    if int(fpm[14]) == 2:
        if M0 <= 0:
            return FeastResult(np.zeros(0), np.zeros((N, 0)), 0, np.zeros(0), 2, 0.0, 0, {"estimate": None})
        if not Emin < Emax:
            return FeastResult(np.zeros(0), np.zeros((N, 0)), 0, np.zeros(0), 3, 0.0, 0, {"estimate": None})
        Zne, Wne = feast_contour(Emin, Emax, fpm) if contour is None else contour
        info, est = _run_estimate(eng, A, B, Zne, Wne, False, M0, seed, solver, solver_tol, solver_maxiter, solver_restart,
                                  group)
        return _estimate_result(N, info, est, real_input)
    substituted = None
    if sp.issparse(A) and solver in ("direct", "lu"):
        # the reference's sparse default is UMFPACK; the :hip backend has a direct path for band
        # matrices (batched banded LU) and otherwise the batched Krylov solver (north_star)
        if known and eng._checked.get("nodes") == int(fpm[2]):
            solver = eng._checked["direct"]
        else:
            solver = _sparse_direct_solver(A, B, int(fpm[2]))
            if fp is not None and fp[0] and fp[1] is not False:
                eng._checked = {"fp": fp, "nodes": int(fpm[2]), "direct": solver}
        if solver == "dense":
            A, B, solver = _densify(A), _densify(B), "direct"
            substituted = {"requested": "direct", "used": "dense LU of the expanded matrix"}
        elif (solver == "krylov" and group is None and _DIRECT_FLOPS > 0 and A.shape[0] <= 400_000     # (beyond: the plan itself -- host nested dissection -- is no longer small change)
              and _band_direct_fits(eng, A, B, int(fpm[2]), max_flops=_DIRECT_FLOPS)):
            # a band the direct solver eliminates in a fraction of a second (2-D problems, thin 3-D ones): the reference's own
            # default -- a direct factorisation per node, exact solves, two or three loops -- is then also the faster one
            # (measured: DESIGN.md section 5); wider bands keep the Krylov fast path with the direct solver as its fallback
            solver = "banded"
            substituted = {"requested": "direct", "used": _direct_label(eng)}
            if fp is not None and fp[0] and fp[1] is not False:
                eng._checked = {"fp": fp, "nodes": int(fpm[2]), "direct": solver}
        elif solver == "krylov":
            solver = "cocg" if real_input else "bicgstab"
            # each default applies on its own: naming one of the three keeps the other two
            if warm_start is None:
                warm_start = _KRYLOV_DEFAULT["warm_start"]
            if inner_rtol is None and warm_start:
                inner_rtol = _KRYLOV_DEFAULT["inner_rtol"]
            # inexact solves pay for a sharper filter than they can use: unless the caller fixed fpm[18], the driver
            # picks the ellipse ratio itself (hip_backend.feast_hip_hermitian, contour_policy)
            auto = contour_policy is None and aspect_unset and contour is None and warm_start and inner_rtol is not None
            if solver_maxiter is None:
                # per-loop iteration cap: 100 on the caller's contour; 50 under the contour policy, whose taller ellipses
                # need fewer iterations and whose safeguard doubles the cap when a loop stalls on capped nodes (measured on
                # four 50 000-unknown pencils: 50 is 5-10 % ahead on three and 5 % behind on the fourth)
                solver_maxiter = (50 if auto else _KRYLOV_DEFAULT["solver_maxiter"]) if (warm_start and inner_rtol is not None) else 500
            substituted = {"requested": "direct", "used": solver, "warm_start": bool(warm_start),
                           "inner_rtol": inner_rtol, "solver_maxiter": int(solver_maxiter)}
            _warn_substitution(substituted)
            if auto:
                contour_policy = "auto"
                substituted["contour_policy"] = "auto"
    if solver == "sparse_direct":
        solver = "banded"
    abort_check = None
    if (substituted is not None and substituted.get("used") in ("cocg", "bicgstab") and group is None
            and os.environ.get("FEASTKIT_DIRECT_SWITCH", "1") != "0"):
        # (FEASTKIT_DIRECT_SWITCH=0: never leave the Krylov path before fpm[4] loops are spent.)  The Krylov path was OUR choice for the caller's solver=:direct.  After every refinement loop the time it still needs
        # is extrapolated from the contraction of the outer residual over the last two loops; when that exceeds 3 x what
        # the sparse direct solver would take from here (its factorisations: a chain of ~1.5 ms block steps plus
        # 8 N kl (kl + ku) flop per node at ~20 TFLOP/s; then one or two loops), the sweep stops and the direct solver
        # finishes from the current subspace.  Intervals inside the spectrum, where the Krylov sweeps stagnate, cost four
        # loops of them instead of fpm[4].
        plan = {}

        def abort_check(loop_idx, eps, elapsed):
            if loop_idx < 3:
                return False
            if "t_direct" not in plan:
                plan["t_direct"] = None
                if _band_direct_fits(eng, A, B, int(fpm[2])):
                    kl, ku, _nb, _blk = eng.band_plan()
                    if _blk == HipEngine.PLAN_MULTIFRONTAL:      # measured 0.19 s for cfg 3 (1.05e11 flop per node, 16 nodes)
                        plan["t_direct"] = 0.08 + eng.direct_plan_flops() * int(fpm[2]) / 1.3e13
                    else:
                        plan["t_direct"] = 0.3 + (N / 128.0) * 1.5e-3 + 8.0 * N * kl * (kl + ku) * int(fpm[2]) / 2e13
            if plan["t_direct"] is None:
                return False
            fin = [e for e in eps if np.isfinite(e) and e > 0]
            tol = 10.0 ** (-int(fpm[3]))
            if len(fin) >= 3 and len(eps) >= 3 and all(np.isfinite(e) for e in eps[-3:]):
                rho = (eps[-1] / eps[-3]) ** 0.5
                remaining = math.inf if rho >= 1.0 else max(0.0, math.log(tol / eps[-1]) / math.log(rho)) * (elapsed / (loop_idx + 1))
            else:
                remaining = math.inf                                    # no Ritz value inside after four loops
            return remaining > 3.0 * plan["t_direct"]
    warm_start = bool(warm_start)                 # an explicitly named iterative solver keeps the reference's zero guess
    solver_maxiter = 500 if solver_maxiter is None else int(solver_maxiter)
    dn_ignored = direct_nodes is not None and solver in DIRECT_SOLVERS      # the default resolved to a direct solver outright
    try:                                          # whatever happens below, the factors it cached go with the call
        res = feast_hip_hermitian(eng, A, B, Emin, Emax, M0, fpm, solver=solver, solver_tol=solver_tol,
                                  solver_maxiter=solver_maxiter, solver_restart=solver_restart,
                                  warm_start=warm_start, inner_rtol=inner_rtol, real_projection=real_projection,
                                  inner_precision=inner_precision, group=group, Q0=Q0, contour=contour,
                                  contour_policy=contour_policy, eps_floor=float(np.sqrt(np.finfo(np.float32).eps)) if single else 0.0,
                                  abort_check=abort_check, direct_nodes=None if dn_ignored else direct_nodes, ortho=ortho,
                                  precond=precond, precond_shifts=precond_shifts)
        if dn_ignored and isinstance(res.stats, dict):
            res.stats["direct_nodes"] = {"ignored": "direct solver in force"}
        if (res.info == 5 and substituted is not None and substituted.get("used") in ("cocg", "bicgstab") and group is None
                and _band_direct_fits(eng, A, B, int(fpm[2]))):
            # The Krylov sweeps did not converge (typically an interval inside the spectrum: the shifted systems are then
            # indefinite and badly conditioned).  solver=:direct was what the caller asked for, and the direct solver for general
            # patterns fits the device: run it, as the reference's default would have from the start.
            krylov_info, krylov_loops = int(res.info), int(res.loop)
            # (the direct solver starts from the caller's / the seeded subspace, not from what the Krylov loops left: measured on
            #  cfg 3's interval around 2.0, the stagnated subspace carries a spurious pair into the direct solve -- M = 41, info 5
            #  after 20 loops -- where the fresh start converges in two)
            dn_log = res.stats.get("direct_nodes") if isinstance(res.stats, dict) else None
            res = feast_hip_hermitian(eng, A, B, Emin, Emax, M0, fpm, solver="banded", solver_tol=solver_tol,
                                      real_projection=real_projection, inner_precision=inner_precision, group=group, Q0=Q0,
                                      contour=contour, eps_floor=float(np.sqrt(np.finfo(np.float32).eps)) if single else 0.0,
                                      ortho=ortho)
            if dn_log is not None and isinstance(res.stats, dict):
                res.stats["direct_nodes"] = dn_log                      # what the Krylov loops did before the hand-over
            substituted = dict(substituted, fallback=_direct_label(eng), krylov_info=krylov_info,
                               krylov_loops=krylov_loops)
        if substituted is not None and isinstance(res.stats, dict):
            res.stats["solver_substitution"] = substituted
    finally:
        _release_band_factors(eng, keep_factors)
    if real_input:
        res = FeastResult(res.lambda_, np.real(res.q), res.M, res.res, res.info, res.epsout, res.loop, res.stats)
    if single:
        res = _demote(res, cplx_lambda=False)
    return res


def _two_sided_sparse_route(A, B, solver, nodes, engine, device):
    """Where ``feast_general(A_sparse, ..., two_sided=True)`` runs -> (A, B, solver, substitution record, engine).
    ``direct`` / ``lu``: ValueError for a pattern inside the library's narrow band (kl + ku <= 64: that solver means the
    one-workgroup band LU there, which has no adjoint substitution, and a band that thin is not expanded silently: the caller
    chooses ``sparse_direct`` or dense input); else the expanded matrix under the dense LU inside _sparse_direct_solver's dense
    window, else -- as for an explicit ``sparse_direct`` / ``banded`` -- the sparse direct solver with the plan the requirement
    gives: the multifrontal LU, or the blocked band LU for a pattern that has no multifrontal plan
    (require_adjoint is set BEFORE the plan is queried, so the plan query already answers for the plan that has an adjoint
    substitution; the driver clears it), provided its factors fit the device.  Otherwise ValueError: there is no Krylov solver
    on the conjugate transpose.  The fit is that of the plan in force: a multifrontal LU that rejects a pivot during the solve
    falls back to the blocked band LU, whose factors are larger; if those do not fit, the solve raises the library's
    FeastHipError (``banded LU: ... do not fit the free device memory``), it is not turned into a result code."""
    if solver in ("direct", "lu"):
        kl, ku = _band_widths(A, B)
        if kl + ku <= _NARROW_BAND:
            # (host-only, before any engine exists: the refusal the dense-only version of this keyword gave such input stays)
            raise ValueError("two_sided with solver='direct' on a sparse matrix inside the narrow band (kl + ku <= 64): the band LU "
                             "that solver means for it has no adjoint substitution, and expanding a band this thin is not done "
                             "silently; pass solver='sparse_direct' (multifrontal LU) or dense input")
    if solver in ("direct", "lu") and _sparse_direct_solver(A, B, nodes, allow_band=False) == "dense":
        return _densify(A), _densify(B), "direct", {"requested": "direct", "used": "dense LU of the expanded matrix"}, engine
    explicit = solver in ("sparse_direct", "banded")
    engine = _engine(engine, device)
    engine.require_adjoint(True)
    try:
        fits = _band_direct_fits(engine, A, B, nodes, None, complexify=True)
        label = _direct_label(engine) if fits else None
    finally:
        engine.require_adjoint(False)
    if not fits and not explicit:
        raise ValueError("two_sided on this sparse input: the factors of the sparse direct solver do not fit the device, and "
                         "there is no Krylov solver on the conjugate transpose")
    return A, B, "banded", (None if explicit else {"requested": "direct", "used": label}), engine


def feast_general(A, B=None, center=0.0, radius=1.0, *, M0=10, fpm=None, backend="hip", solver="direct",
                  solver_tol=0.0, solver_maxiter=500, solver_restart=30, group=None, engine=None, device=0, Q0=None,
                  inner_precision=64, contour=None, keep_factors=False, seed=None, direct_nodes=None, ortho="mgs",
                  two_sided=False, QL0=None, precond=None, precond_shifts=1):
    """feast_general(A, [B,] center, radius; M0, fpm): src/interfaces/feast_interfaces.jl:274-379.
    ``two_sided=True`` (``solver="direct"``; sparse input also ``"sparse_direct"`` / ``"banded"``): the two-sided method -- a
    left subspace from conjugate-transposed solves on the LU factors of the right sweep, oblique projection, both residuals
    with B; the result carries ``q_left`` (y_j^H B x_j = 1) and ``stats["two_sided"]`` (``direct_plan`` names the factors that
    ran, ``fell_back`` whether the multifrontal LU handed the matrix to the band LU), and ``info`` is
    Feast_ERROR_NO_CONVERGENCE when the loop limit ends the run.  Sparse input runs on the multifrontal
    LU of the sparse direct solver -- on its blocked band LU where a pivot is rejected (saddle-point, zero-diagonal pencils)
    or the pattern has no multifrontal plan --, or -- ``solver="direct"`` up to N = 12 288 -- on the dense LU of the expanded matrix
    (``stats["solver_substitution"]``); ``solver="direct"`` on a narrow band (kl + ku <= 64) raises ValueError and names
    ``solver="sparse_direct"``; there is no Krylov solver on the conjugate transpose.
    ``QL0``: left start block.  The keyword is the only switch: fpm[15], which the reference validates and never reads
    (src/core/feast_parameters.jl:217-225), stays unread here too, so no existing call changes.  A Krylov
    solver, ``inner_precision=32``, ``group=`` and ``direct_nodes=`` raise ValueError.
    ``keep_factors``, ``direct_nodes``, ``ortho``: as in feast() (this variant never orthonormalises its subspace, so ``ortho``
    changes nothing it computes).  ``fpm[14] = 2`` and ``M0="auto"``: as in feast(), on the full contour of the
    circle (the samples are complex; M = round(Re mean)).
    ``precond``, ``precond_shifts``: as in feast(), on the full contour of the circle; ``two_sided=True`` raises ValueError too."""
    if isinstance(M0, str):
        if M0 != "auto":
            raise ValueError("M0 must be an integer or 'auto'")
        check_precond(precond, precond_shifts, auto_m0=True)
        return _feast_auto(feast_general, A, B, center, radius, fpm=fpm, backend=backend, solver=solver, solver_tol=solver_tol,
                           solver_maxiter=solver_maxiter, solver_restart=solver_restart, group=group, engine=engine,
                           device=device, Q0=Q0, inner_precision=inner_precision, contour=contour, keep_factors=keep_factors,
                           seed=seed, direct_nodes=direct_nodes, ortho=ortho, two_sided=two_sided, QL0=QL0)
    if backend not in _BACKENDS:
        raise ValueError(f"Unknown backend '{backend}' (this package provides: hip)")
    if A.shape[0] != A.shape[1]:
        raise ValueError("Matrix A must be square")
    if not radius > 0:
        raise ValueError("radius must be positive")
    if two_sided:
        check_two_sided(sp.issparse(A), solver, inner_precision, group, direct_nodes)
    check_precond(precond, precond_shifts, sparse=sp.issparse(A), solver=solver, inner_precision=inner_precision, group=group,
                  direct_nodes=direct_nodes, two_sided=two_sided, estimate=fpm is not None and int(fpm[14]) == 2)
    _check_direct_nodes_early(direct_nodes, A, solver, fpm, 8, contour)
    check_ortho(ortho)
    single = _single_precision(A, B)
    if single:
        A, B = _promote(A), _promote(B)
    fpm = feastinit() if fpm is None else fpm
    feastdefault(fpm)
    M0 = min(int(M0), A.shape[0])
    if int(fpm[14]) == 2:
        N = A.shape[0]
        if M0 <= 0:
            return FeastResult(np.zeros(0, complex), np.zeros((N, 0), complex), 0, np.zeros(0), 2, 0.0, 0, {"estimate": None})
        Zne, Wne = feast_gcontour(complex(center), float(radius), fpm) if contour is None else contour
        info, est = _run_estimate(_engine(engine, device), A, B, Zne, Wne, True, M0, seed, solver, solver_tol,
                                  solver_maxiter, solver_restart, group)
        return _estimate_result(N, info, est, False)
    substituted = None
    if two_sided and sp.issparse(A):
        A, B, solver, substituted, engine = _two_sided_sparse_route(A, B, solver, int(fpm[8]), engine, device)
    elif sp.issparse(A) and solver in ("direct", "lu"):
        # the reference factors z B - A with UMFPACK (src/sparse/feast_sparse.jl:943); here: banded LU for narrow
        # bands, else batched BiCGStab on the (non-symmetric) shifted systems with the reference's iterative
        # settings (zero guess, rtol = atol = 10^-fpm[3], src/sparse/feast_sparse.jl:164-203)
        solver = _sparse_direct_solver(A, B, int(fpm[8]))
        if solver == "dense":
            A, B, solver = _densify(A), _densify(B), "direct"
            substituted = {"requested": "direct", "used": "dense LU of the expanded matrix"}
        elif solver == "krylov":
            # unpreconditioned Krylov sweeps cannot solve shifted systems whose spectrum surrounds the shift (the usual case
            # for a contour inside a non-Hermitian spectrum): the direct solver for general patterns takes them whenever its
            # factors fit the device
            engine = _engine(engine, device)
            if _band_direct_fits(engine, A, B, int(fpm[8]), group, complexify=True):
                solver = "banded"
                substituted = {"requested": "direct", "used": _direct_label(engine)}
            else:
                solver = "bicgstab"
                substituted = {"requested": "direct", "used": solver, "warm_start": False, "inner_rtol": None,
                               "solver_maxiter": int(solver_maxiter)}
                _warn_substitution(substituted)
    elif solver == "krylov":
        solver = "bicgstab"
    elif solver == "sparse_direct":
        solver = "banded"
    eng = _engine(engine, device)
    dn_ignored = direct_nodes is not None and solver in DIRECT_SOLVERS
    eps_floor = float(np.sqrt(np.finfo(np.float32).eps)) if single else 0.0
    try:
        if two_sided:
            res = feast_hip_general_two_sided(eng, A, B, complex(center), float(radius), M0, fpm, solver=solver, Q0=Q0, QL0=QL0,
                                              contour=contour, eps_floor=eps_floor, **({} if seed is None else {"seed": int(seed)}))
        else:
            res = feast_hip_general(eng, A, B, complex(center), float(radius), M0, fpm, solver=solver, inner_precision=inner_precision,
                                    solver_tol=solver_tol, solver_maxiter=solver_maxiter,
                                    solver_restart=solver_restart, group=group, Q0=Q0, contour=contour, eps_floor=eps_floor,
                                    direct_nodes=None if dn_ignored else direct_nodes, ortho=ortho, precond=precond,
                                    precond_shifts=precond_shifts)
        if dn_ignored and isinstance(res.stats, dict):
            res.stats["direct_nodes"] = {"ignored": "direct solver in force"}
        if substituted is not None and isinstance(res.stats, dict):
            res.stats["solver_substitution"] = substituted
    finally:
        _release_band_factors(eng, keep_factors)          # (the dense LU factors of the two-sided sweeps among them)
    if single:
        ql = res.q_left
        res = _demote(res, cplx_lambda=True)
        res.q_left = None if ql is None else ql.astype(np.complex64)
    return res


POLY_MAX_DEGREE = 8          # FEASTHIP_POLY_MAX_DEGREE
POLY_DENSE_LIMIT = 12288     # sparse coefficients are expanded up to this size
# POLY_SET_ASIDE (hip_backend): the two thresholds of the projected method's set-aside rule, (absolute, factor)


POLY_SOLVERS = ("direct", "sparse_direct")               # the direct solvers
POLY_KRYLOV_SOLVERS = ("bicgstab", "cocg", "gmres")      # sparse coefficients under method="projected" only


def _check_poly_M0(M0, Q0):
    """M0 of feast_polynomial / feast_nonlinear: an integer, or "auto" without a start block (whose width is then not known)"""
    if isinstance(M0, str):
        if M0 != "auto":
            raise ValueError("M0 must be an integer or 'auto'")
        if Q0 is not None:
            raise ValueError('M0="auto" chooses the width of the subspace: a start block Q0 cannot be given with it')


def _poly_estimate_mode(M0, fpm):
    """(M0 is "auto", fpm[14] = 2) of a feast_polynomial / feast_nonlinear call; the two together make no sense"""
    auto, estimate_only = isinstance(M0, str), int(fpm[14]) == 2
    if auto and estimate_only:
        raise ValueError('M0="auto" sizes a solve; under fpm[14] = 2 M0 is the sample count of the estimate')
    return auto, estimate_only


def _poly_estimate_or_solve(eng, driver, mats, funcs, center, radius, M0, fpm, union, common, auto, estimate_only, seed, krylov, width):
    """One attempt of feast_polynomial / feast_nonlinear on the engine (the callers' fallback to the dense expansion wraps it):
    the solve ``driver(eng, mats, [funcs,] center, radius, M0, fpm, union_csr=union, **common)``; under fpm[14] = 2 the count
    estimate alone, M0 its sample count; under M0 = "auto" the estimate with AUTO_SAMPLES samples on the contour of the solve,
    then the solve on the same handle set-up (``prepared``: the factors the estimate cached serve it) with M0 = auto_M0, or
    ``width(auto_M0)`` where the method runs several columns per unit of M0.  The estimate's Krylov solves (``krylov`` = (solver,
    tol, maxiter, restart)) stop at solver_tol, ESTIMATE_TOL when that is 0."""
    args = (eng, mats) + (() if funcs is None else (funcs,)) + (center, radius)
    if not (auto or estimate_only):
        return driver(*args, M0, fpm, union_csr=union, **common)
    N = mats[0].shape[0]
    ekry = None if krylov is None else (krylov[0], krylov[1] if krylov[1] > 0.0 else ESTIMATE_TOL) + tuple(krylov[2:])
    info, est, _plan, nfact = feast_hip_poly_estimate(eng, mats, funcs, center, radius, M0, fpm, seed=ESTIMATE_SEED if seed is None else int(seed),
                                                      contour=common.get("contour"), union_csr=union, krylov=ekry)
    if estimate_only or est is None:
        return _estimate_result(N, info, est, False)
    M0a = auto_M0(est, N)
    if width is not None:
        M0a = width(M0a)
    res = driver(*args, M0a, fpm, union_csr=union, prepared=True, **common)
    if isinstance(res.stats, dict):
        res.stats["factorizations"] = res.stats.get("factorizations", 0) + nfact
        res.stats["estimate"] = est
        res.stats["M0_auto"] = M0a
    return res


def feast_polynomial(coeffs, center, radius, *, M0=10, fpm=None, engine=None, device=0, Q0=None, contour=None, seed=None,
                     keep_factors=False, residual="pencil", solver="direct", method="linearised", ortho="mgs", solver_tol=0.0,
                     solver_maxiter=500, solver_restart=30):
    """feast_polynomial(coeffs, center, radius; M0, fpm): src/interfaces/feast_interfaces.jl:448-462, feast_pep! /
    feast_gepev! / feast_hepev! / feast_sypev! (src/dense/feast_dense.jl:715-772, 946-979).  Eigenpairs of
    P(lambda) x = 0, P(lambda) = coeffs[0] + lambda coeffs[1] + ... + lambda^d coeffs[d], with lambda inside the circle.
    The reference builds the dN x dN companion pencil and factors it per node; here a node costs one LU of P(z_e), order N.

    ``coeffs``: d + 1 square matrices of one size, 1 <= d <= 8, real or complex (float32 / complex64 input is promoted and
    the result demoted as in feast_general).  ``M0`` (clipped to N) sizes the subspace: the loop runs M0 d columns, as
    feast_pep! does.  ``Q0``: linearised start block, (d N) x (M0 d).
    ``solver``:
      "direct" (default)  the dense LU of P(z_e).  Sparse coefficients are expanded up to N = 12 288
                          (``stats["solver_substitution"]``); beyond that ValueError.
      "sparse_direct"     every coefficient a scipy.sparse matrix, any N: the counterpart of the reference's feast_scsrpev! /
                          feast_hcsrpev! / feast_gcsrpev! (src/sparse/feast_sparse.jl), which run on the explicit sparse
                          companion.  The coefficients go on one union pattern (ingest.polynomial_union_csr) and P(z_e) is
                          factored by the multifrontal LU of the sparse direct solver.  That LU pivots only inside a front's
                          fully-summed block: when it rejects a pivot at any node, or the pattern has no multifrontal plan
                          (a front beyond 16 384 rows), the call reruns on the dense expansion if N <= 12 288
                          (``stats["polynomial"]["fell_back"]`` = True, plan = "dense", ``stats["solver_substitution"]``),
                          else raises FeastHipError naming the cause and the sizes -- as it does when the factors do not fit
                          the device.  There is no band LU for polynomials.
      "bicgstab" | "cocg" | "gmres"   no factors at all: every coefficient a scipy.sparse matrix, ``method="projected"``.  The
                          solves P(z_e) Y_e = R of the contour step run on the batched Krylov drivers of feast / feast_general
                          (the counterpart of the reference's difeast_scsrpev! / zifeast_hcsrpev! / zifeast_gcsrpev! family),
                          with the operator P(z_e) applied per nonzero on the union pattern, from a zero start, without a
                          preconditioner.  ``solver_tol`` (0 = 10^-fpm[3], the package's convention), ``solver_maxiter`` and
                          ``solver_restart`` (GMRES) as in feast.  The stop test is relative only, ||r|| <= solver_tol ||rhs||
                          (atol = 0): the right-hand side of a residual-inverse solve is P(sigma_j) x_j, which shrinks with
                          the outer residual, so an absolute floor would stop the inner solves of the late loops at once.
                          Inexact solves are enough: at solver_tol = 1e-4 the loop history stays within a few percent of the
                          exact-solve one.  A node whose column stops at ``solver_maxiter`` is a normal outcome (its iterate
                          is used; ``stats["polynomial"]["krylov"][loop]["capped_nodes"]`` counts them).  "cocg" needs every
                          coefficient exactly symmetric (A_k == A_k^T; complex symmetric qualifies, Hermitian does not), else
                          ValueError naming "bicgstab".  ``method="linearised"`` (one right-hand side per node) and dense
                          coefficients raise ValueError; a Krylov call never falls back to the dense expansion.
                          ``stats["krylov_iterations"]`` sums the slowest column of every node and loop,
                          ``stats["polynomial"]["krylov"]`` holds per loop {iterations (worst column), node_iterations,
                          capped_nodes}, ``stats["factorizations"]`` stays 0, plan = "krylov", fell_back = False.
    ``residual``: what ``res`` / ``epsout`` and the stop test measure on the unit linearised Ritz vector x of the companion
    pencil (A_lin, B_lin):
      "pencil" (default)  ||A_lin x - lambda B_lin x|| / max(|lambda|, 1)
      "reference"         ||A_lin x - lambda x|| / max(|lambda|, 1), the reference's measure, which omits B_lin
                          (src/kernel/feast_kernel.jl:899-906).  For coeffs[d] != I that measure never falls: the reference
                          on a non-monic quadratic runs every loop and returns info = 0 with epsout = 0.34 while its
                          eigenvalues are right to 6e-14.  That is why the default differs.
    Result: FeastResult with complex ``lambda_`` (feast_sort_general order), ``q`` = the first N rows of the M linearised Ritz
    vectors as the reference returns them (src/dense/feast_dense.jl:768), ``res`` in the chosen measure;
    ``stats["polynomial"]`` = {degree, columns, residual, backward_error, eps_history} with backward_error[j] =
    ||P(lambda_j) q_j|| / (sum_k |lambda_j|^k ||A_k||_F ||q_j||); ``stats["factorizations"]`` counts N x N factorisations.
    Under "sparse_direct" also plan ("multifrontal" | "dense"), plan_factor_bytes / plan_transient_bytes / plan_flops per node
    (feasthip_direct_plan_bytes / _flops; absent for "dense"), plan_nnz of the union pattern, and fell_back.
    ``keep_factors``, ``contour``, ``seed``: as in feast_general.

    ``method``:
      "linearised" (default)  the loop described above, on M0 d linearised columns that are never orthonormalised.  It carries
                          junk directions whose Ritz values can fall inside the circle, and may wander or stop at the loop
                          limit on a start block it does not like.
      "projected"         polynomial FEAST on an N-row subspace (Gavin, Miedlar, Polizzi): ``M0`` is the number of N-row
                          columns -- choose M0 >= 1.3 x the expected count, as for feast -- and ``Q0`` is (N, M0).  Per loop the
                          subspace is orthonormalised in the N-dimensional space (``ortho``: "mgs" | "cholqr_rr", as in feast),
                          the polynomial itself is projected (Q^H A_k Q) and only the small r x r polynomial is linearised, on
                          the host; the contour step is a residual-inverse sweep with the Ritz values as per-column shifts.
                          A node is still factored once per solve (``stats["factorizations"]`` = the node count) and solves
                          M0 right-hand sides per loop instead of M0 d.  The stop test, ``res`` and ``epsout`` are the backward
                          error ||P(lambda) q|| / sum_k |lambda|^k ||A_k||_F of the unit vectors ``q``, so ``residual`` must stay
                          "pencil" (the default; "reference" raises ValueError).  Of the d r candidates of a loop, those inside the
                          circle are kept in ascending backward error, then those outside by distance; a kept pair inside whose
                          backward error exceeds both POLY_SET_ASIDE[0] and POLY_SET_ASIDE[1] times the best one is set aside:
                          it stays in the subspace and is left out of M and epsout.  At the loop limit the last iterates are
                          returned with info = Feast_ERROR_NO_CONVERGENCE.  ``stats["polynomial"]`` = {degree, method, columns (M0),
                          rank, candidates, set_aside, eps_history (one entry per loop each), backward_error}, plus the plan
                          fields under "sparse_direct"; ``stats["ortho"]`` as in feast.
    ``ortho`` is checked for both methods and used by "projected" only (the linearised loop never orthonormalises).

    ``fpm[14] = 2``: no eigensolve -- a stochastic estimate of the number of eigenvalues inside the circle
    (hip_backend.feast_hip_poly_estimate): Hutchinson samples of sum_e w_e tr(P'(z_e) P(z_e)^-1) over ``M0`` Rademacher columns
    from one set of solves on the call's contour, under any ``solver`` of the call (Krylov solves stop at ``solver_tol``, 1e-8
    when that is 0; the Krylov names are accepted with either ``method`` here, since the estimate's solves share one
    right-hand-side block).  ``Q0`` is ignored; ``method``, ``residual`` and ``ortho`` are validated and unused.  The result has no
    eigenpairs, complex dtype, M = max(0, round(Re mean)) and ``stats["estimate"]`` = {mean, stderr, samples, nodes, solver, seed,
    seconds, dropped_terms}; a node that fails (status 5 / 8) gives that info and ``stats["estimate"] = None``.  feastdefault
    lowers an unset fpm[8] to 6 under fpm[14] = 2: six nodes are a blunt filter for this use, set
    fpm[8] >= 16.
    ``M0="auto"``: such an estimate with 64 samples on the contour of the solve (the caller's fpm[8], default 16 -- not the
    six-node estimate contour), then the solve on the same handle, so that under "direct" / "sparse_direct" it reuses the factors
    the estimate cached and ``stats["factorizations"]`` of the whole call is the node count.  "projected": M0 = min(N, max(8,
    ceil(1.5 (mean + 2 stderr)))); "linearised": that number divided by d, rounded up.  ``stats["estimate"]`` and
    ``stats["M0_auto"]`` as in feast; ``seed`` picks both the estimate's block and the start block.  The estimate takes
    min(64, N) samples.  When a node of the estimate fails (status 5 / 8) no solve follows: the call returns the estimate's
    result -- that info, no eigenpairs, ``stats["estimate"] = None``, no ``stats["M0_auto"]`` or ``stats["factorizations"]``.  ``Q0`` with "auto" raises
    ValueError (the width is not known), as does any other string."""
    mats = list(coeffs)
    _check_poly_M0(M0, Q0)
    if method not in POLY_METHODS:
        raise ValueError(f"method must be one of {POLY_METHODS}, not {method!r}")
    check_ortho(ortho)
    if method == "projected" and residual == "reference":
        raise ValueError('method="projected" stops on the backward error of (lambda, q): residual="reference" does not apply')
    if len(mats) < 2:
        raise ValueError("feast_polynomial needs at least two coefficient matrices (degree >= 1)")
    if len(mats) - 1 > POLY_MAX_DEGREE:
        raise ValueError(f"degree {len(mats) - 1} exceeds the supported maximum {POLY_MAX_DEGREE}")
    shape = mats[0].shape
    for c in mats:
        if len(c.shape) != 2 or c.shape[0] != c.shape[1]:
            raise ValueError("coefficient matrices must be square")
        if c.shape != shape:
            raise ValueError("coefficient matrices must have equal shapes")
    if not radius > 0:
        raise ValueError("radius must be positive")
    if residual not in POLY_RESIDUALS:
        raise ValueError(f"residual must be one of {POLY_RESIDUALS}, not {residual!r}")
    if solver not in POLY_SOLVERS + POLY_KRYLOV_SOLVERS:
        raise ValueError(f"solver must be one of {POLY_SOLVERS + POLY_KRYLOV_SOLVERS}, not {solver!r}")
    N = shape[0]
    krylov = solver in POLY_KRYLOV_SOLVERS
    if krylov:
        if not all(sp.issparse(c) for c in mats):
            raise ValueError(f'solver="{solver}" needs every coefficient as a scipy.sparse matrix; dense coefficients take '
                             'solver="direct"')
        # (the estimate of fpm[14] = 2 solves with one shared right-hand-side block whatever the method)
        if method != "projected" and not (fpm is not None and int(fpm[14]) == 2):
            raise ValueError(f'solver="{solver}" solves one right-hand-side block shared by the contour nodes: it needs '
                             'method="projected" (the linearised sweep has one right-hand side per node)')
        if solver == "cocg" and any(abs(c - c.T).max() != 0 for c in mats):
            raise ValueError('solver="cocg" needs every coefficient exactly symmetric (A_k == A_k^T; Hermitian does not '
                             'qualify); use solver="bicgstab"')
        if solver_tol < 0 or int(solver_maxiter) < 1 or int(solver_restart) < 0:
            raise ValueError("solver_tol must be >= 0, solver_maxiter >= 1, solver_restart >= 0")
    sparse_direct = solver == "sparse_direct" or krylov
    if sparse_direct and not all(sp.issparse(c) for c in mats):
        raise ValueError('solver="sparse_direct" needs every coefficient as a scipy.sparse matrix; dense coefficients take '
                         'solver="direct"')
    substituted = None
    if not sparse_direct and any(sp.issparse(c) for c in mats):
        if N > POLY_DENSE_LIMIT:
            raise ValueError(f"sparse coefficients are expanded to dense matrices up to N = {POLY_DENSE_LIMIT}; N = {N}")
        mats = [_densify(c) if sp.issparse(c) else c for c in mats]
        substituted = {"requested": "direct", "used": "dense LU of the expanded coefficients"}
    if not sparse_direct:
        mats = [np.asarray(c) for c in mats]
    single = _single_precision(*mats)
    if single:
        mats = [_promote(c) for c in mats]
    fpm = feastinit() if fpm is None else fpm
    feastdefault(fpm)
    auto, estimate_only = _poly_estimate_mode(M0, fpm)
    M0 = min(AUTO_SAMPLES if auto else int(M0), N)
    if estimate_only and M0 <= 0:
        return _estimate_result(N, 2, None, False)
    if method == "projected" and Q0 is not None and np.shape(Q0) != (N, M0):
        raise ValueError(f'method="projected": Q0 must be the N-row start block of shape ({N}, {M0}), not {np.shape(Q0)}')
    eng = _engine(engine, device)
    eps_floor = float(np.sqrt(np.finfo(np.float32).eps)) if single else 0.0
    common = dict(Q0=Q0, contour=contour, eps_floor=eps_floor, **({} if seed is None else {"seed": int(seed)}))
    if method == "projected":
        driver, common["ortho"] = feast_hip_polynomial_projected, ortho
    else:
        driver, common["residual"] = feast_hip_polynomial, residual
    kry = (solver, float(solver_tol), int(solver_maxiter), int(solver_restart)) if krylov else None
    if krylov:
        common["krylov"] = kry

    def run(mats, union):
        return _poly_estimate_or_solve(eng, driver, mats, None, complex(center), float(radius), M0, fpm, union, common, auto, estimate_only,
                                       seed, kry, (lambda M: max(1, math.ceil(M / (len(mats) - 1)))) if method == "linearised" else None)
    try:
        res = None
        if sparse_direct:
            union = polynomial_union_csr(mats)
            try:
                res = run(mats, union)
                if isinstance(res.stats, dict) and "polynomial" in res.stats:
                    res.stats["polynomial"]["fell_back"] = False
            except FeastHipError as err:
                # 9: no multifrontal plan for the pattern, 8: a rejected pivot.  (6, factors that do not fit, is not a
                # reason to try N^2 dense ones.)
                if krylov or err.code not in (8, 9) or N > POLY_DENSE_LIMIT:
                    raise
                eng.free_factors()
                substituted = {"requested": "sparse_direct", "used": "dense LU of the expanded coefficients", "reason": str(err)}
                mats = [_densify(c) for c in mats]
        if res is None:
            res = run(mats, None)
            if sparse_direct and isinstance(res.stats, dict) and "polynomial" in res.stats:
                res.stats["polynomial"].update(plan="dense", plan_nnz=int(len(union[1])), fell_back=True)
        if substituted is not None and isinstance(res.stats, dict):
            res.stats["solver_substitution"] = substituted
    finally:
        _release_band_factors(eng, keep_factors)          # (the N x N LU factors of the nodes)
    return _demote(res, cplx_lambda=True) if single else res


feast_pep = feast_polynomial


def feast_nonlinear(terms, center, radius, *, M0=10, fpm=None, solver="direct", ortho="mgs", Q0=None, contour=None, seed=None,
                    keep_factors=False, moments=2, reduced_nodes=128, engine=None, device=0):
    """Eigenpairs of the nonlinear eigenproblem T(lambda) x = 0 in split form,
        T(lambda) = sum_k f_k(lambda) A_k,
    with lambda inside the circle: the projected method of feast_polynomial (FEAST with a residual-inverse contour step on an
    N-row subspace; Gavin, Miedlar, Polizzi) with arbitrary analytic scalar functions in place of the powers of lambda.  No
    reference counterpart.

    ``terms``: 2 to 9 pairs (A_k, f_k).  The A_k are square and of one size, all numpy arrays or all scipy.sparse matrices
    (a mix is expanded under "direct"), real or complex; float32 / complex64 input is promoted and the result demoted as in
    feast_polynomial.  f_k is a callable mapping a complex numpy array to a complex array of the same shape, or a non-negative
    int p for lambda^p.  The f_k are only ever evaluated -- at the contour nodes, the reduced contour and the Ritz values -- and
    never differentiated analytically; the device sees tables of their values, not the functions.
    ``M0`` (clipped to N): the number of N-row columns; choose M0 >= 1.3 x the expected count.  ``Q0``: (N, M0).
    ``solver``: "direct" (the dense LU of T(z_e); sparse terms are expanded up to N = 12 288, ``stats["solver_substitution"]``)
    or "sparse_direct" (every A_k sparse: the multifrontal LU on the union pattern, with feast_polynomial's fallback to the
    dense expansion on a rejected pivot or a pattern without a plan, and FeastHipError where it raises one).  "bicgstab",
    "cocg" and "gmres" raise ValueError: Krylov solves on T(z) are not provided.
    Per loop the subspace is orthonormalised (``ortho`` as in feast), the terms are projected (Q^H A_k Q) and the small r x r
    problem is solved on the host: Beyn's integral method on ``reduced_nodes`` trapezoid points of the same circle with
    ``moments`` block moments (>= 2 are needed where eigenvalues inside share an eigenvector, as the branches of a delay term
    do), then a guarded Newton polish of each candidate whose derivative is a central difference of the f_k.  Candidates are
    ranked by their backward error on the device as in feast_polynomial (POLY_SET_ASIDE).  Loop 0 factors every node once;
    later loops reuse the factors.
    Result: FeastResult with complex ``lambda_`` (feast_sort_general order), unit vectors ``q``, ``res[j]`` the backward error
    ||T(lambda_j) q_j|| / sum_k |f_k(lambda_j)| ||A_k||_F, ``epsout`` the largest, ``info`` 0 or Feast_ERROR_NO_CONVERGENCE (loop
    limit, with the last iterates; or nothing found inside, M = 0).  ``stats["nonlinear"]`` = {terms, columns, rank, candidates,
    set_aside, eps_history (one entry per loop each), backward_error, moments, reduced_nodes, reduced_seconds}, plus the plan fields
    and fell_back under "sparse_direct"; ``stats["factorizations"]``, ``stats["solve_seconds"]``, ``stats["ortho"]`` as in
    feast_polynomial.  ``keep_factors``, ``contour``, ``seed``: as in feast_general.

    Known limits of the method: an eigenvalue just outside the circle slows the filter of a 16-node
    contour to a contraction of about one half per loop, so the loop limit may be reached with info = Feast_ERROR_NO_CONVERGENCE
    (more nodes cure it); a spurious candidate of the small problem inside the circle whose backward error is below
    POLY_SET_ASIDE[0] is not set aside: it is counted in M and epsout stalls at its backward error.

    ``fpm[14] = 2`` and ``M0="auto"``: as in feast_polynomial (a failed estimate node under "auto" included), with T'(z_e) = sum_k f_k'(z_e) A_k from central differences of the
    f_k (hip_backend.nep_derivative_table; the f_k are still only evaluated, at z_e +- 1e-6 max(1, |z_e|) too, and a value that is
    not finite there raises ValueError).  Under fpm[14] = 2 ``moments`` and ``reduced_nodes`` are validated and unused.  The
    estimate integrates the analytic remainder of tr(T^-1 T') by the quadrature as well, which falls with the node count; a pole
    of an f_k inside the circle would be counted negatively.

    Not covered: Krylov solves on T(z); multi-rank sweeps; complex64 factors; the two-sided form; functions with a branch cut
    that crosses the circle (keeping the cut away is the caller's responsibility); eigenvalues where some f_k has a pole inside
    the circle."""
    terms = list(terms)
    _check_poly_M0(M0, Q0)
    check_ortho(ortho)
    if len(terms) < 2 or len(terms) > POLY_MAX_DEGREE + 1:
        raise ValueError(f"feast_nonlinear needs 2 to {POLY_MAX_DEGREE + 1} terms (A_k, f_k), not {len(terms)}")
    if any(not isinstance(t, (tuple, list)) or len(t) != 2 for t in terms):
        raise ValueError("each term must be a pair (A_k, f_k)")
    mats = [t[0] for t in terms]
    funcs = nep_functions([t[1] for t in terms])
    shape = mats[0].shape
    for c in mats:
        if len(c.shape) != 2 or c.shape[0] != c.shape[1]:
            raise ValueError("the matrices A_k must be square")
        if c.shape != shape:
            raise ValueError("the matrices A_k must have equal shapes")
    if not radius > 0:
        raise ValueError("radius must be positive")
    if solver in POLY_KRYLOV_SOLVERS:
        raise ValueError(f'solver="{solver}": Krylov solves on T(z) are out of scope for feast_nonlinear; use "direct" or "sparse_direct"')
    if solver not in POLY_SOLVERS:
        raise ValueError(f"solver must be one of {POLY_SOLVERS}, not {solver!r}")
    if int(moments) < 1 or int(reduced_nodes) < 8:
        raise ValueError("moments must be >= 1 and reduced_nodes >= 8")
    N = shape[0]
    sparse_direct = solver == "sparse_direct"
    if sparse_direct and not all(sp.issparse(c) for c in mats):
        raise ValueError('solver="sparse_direct" needs every A_k as a scipy.sparse matrix (no mix of dense and sparse terms); dense terms take '
                         'solver="direct"')
    substituted = None
    if not sparse_direct and any(sp.issparse(c) for c in mats):
        if N > POLY_DENSE_LIMIT:
            raise ValueError(f"sparse terms are expanded to dense matrices up to N = {POLY_DENSE_LIMIT}; N = {N}")
        mats = [_densify(c) if sp.issparse(c) else c for c in mats]
        substituted = {"requested": "direct", "used": "dense LU of the expanded terms"}
    if not sparse_direct:
        mats = [np.asarray(c) for c in mats]
    single = _single_precision(*mats)
    if single:
        mats = [_promote(c) for c in mats]
    fpm = feastinit() if fpm is None else fpm
    feastdefault(fpm)
    auto, estimate_only = _poly_estimate_mode(M0, fpm)
    M0 = min(AUTO_SAMPLES if auto else int(M0), N)
    if estimate_only and M0 <= 0:
        return _estimate_result(N, 2, None, False)
    if Q0 is not None and np.shape(Q0) != (N, M0):
        raise ValueError(f"Q0 must be the N-row start block of shape ({N}, {M0}), not {np.shape(Q0)}")
    Zne, Wne = feast_gcontour(complex(center), float(radius), fpm) if contour is None else contour
    F_node = nep_table(funcs, Zne)
    if not np.isfinite(F_node).all():
        bad = int(np.flatnonzero(~np.isfinite(F_node).all(axis=0))[0])
        raise ValueError(f"f_{bad} is not finite at a contour node (a pole or an overflow on the circle)")
    eng = _engine(engine, device)
    eps_floor = float(np.sqrt(np.finfo(np.float32).eps)) if single else 0.0
    common = dict(Q0=Q0, contour=(Zne, Wne), eps_floor=eps_floor, ortho=ortho, moments=int(moments), reduced_nodes=int(reduced_nodes),
                  **({} if seed is None else {"seed": int(seed)}))

    def run(mats, union):
        return _poly_estimate_or_solve(eng, feast_hip_nonlinear, mats, funcs, complex(center), float(radius), M0, fpm, union, common, auto,
                                       estimate_only, seed, None, None)
    try:
        res = None
        if sparse_direct:
            union = polynomial_union_csr(mats)
            try:
                res = run(mats, union)
                if isinstance(res.stats, dict) and "nonlinear" in res.stats:
                    res.stats["nonlinear"]["fell_back"] = False
            except FeastHipError as err:
                if err.code not in (8, 9) or N > POLY_DENSE_LIMIT:          # (as feast_polynomial: 6 is no reason to try dense factors)
                    raise
                eng.free_factors()
                substituted = {"requested": "sparse_direct", "used": "dense LU of the expanded terms", "reason": str(err)}
                mats = [_densify(c) for c in mats]
        if res is None:
            res = run(mats, None)
            if sparse_direct and isinstance(res.stats, dict) and "nonlinear" in res.stats:
                res.stats["nonlinear"].update(plan="dense", plan_nnz=int(len(union[1])), fell_back=True)
        if substituted is not None and isinstance(res.stats, dict):
            res.stats["solver_substitution"] = substituted
    finally:
        _release_band_factors(eng, keep_factors)
    return _demote(res, cplx_lambda=True) if single else res


feast_nep = feast_nonlinear


def _feast_auto(driver, A, B, *where, fpm=None, engine=None, device=0, solver="direct", solver_tol=0.0,
                solver_maxiter=None, solver_restart=30, group=None, seed=None, **kw):
    """M0 = "auto" of feast / feast_general: a 64-sample estimate on the estimate's own contour (_estimate_fpm), then the
    solve with M0 = auto_M0(estimate) and the caller's parameters.  A failed estimate returns its info and no solve."""
    eng = _engine(engine, device)
    common = dict(engine=eng, solver=solver, solver_tol=solver_tol, solver_restart=solver_restart, group=group,
                  backend=kw.pop("backend", "hip"))
    if solver_maxiter is not None:
        common["solver_maxiter"] = solver_maxiter
    er = driver(A, B, *where, M0=AUTO_SAMPLES, fpm=_estimate_fpm(fpm), seed=seed, **common)
    est = er.stats.get("estimate")
    if est is None:
        return er
    M0 = auto_M0(est, A.shape[0])
    res = driver(A, B, *where, M0=M0, fpm=fpm, **common, **kw)
    if isinstance(res.stats, dict):
        res.stats["estimate"] = est
        res.stats["M0_auto"] = M0
    return res


# ---- matrix-free FEAST: the caller's operators on the device (engine.set_operator, feasthip_set_operator) ---------------------
_MATVEC_KRYLOV = ("gmres", "bicgstab", "iterative", "cocg", "shifted_cocg", "block_cocg")
HERMITIAN_PROBE_TOL = 1e-10       # |<x, A y> - <A x, y>| against the product norms, feast_matvec(check=True)


class _ShapeOnly:
    """stands where a matrix goes in a driver call on a preloaded engine: only its shape is read"""
    def __init__(self, N):
        self.shape = (N, N)


def _check_matvec(who, A_mul, B_mul, N, M0, solver, symmetric, inner_precision):
    """The argument checks of feast_matvec / feast_general_matvec; all of them run before an engine is made or used."""
    if not callable(A_mul):
        raise ValueError(f"{who}: A_mul must be callable, A_mul(Y, X) writes A X into Y")
    if B_mul is not None and not callable(B_mul):
        raise ValueError(f"{who}: B_mul must be callable or None (B = I)")
    if int(N) < 1:
        raise ValueError(f"{who}: N must be at least 1")
    if isinstance(M0, str):
        raise ValueError(f"{who}: M0 must be an integer (the count estimate of M0='auto' is not provided for operators)")
    if solver in ("direct", "lu", "sparse_direct", "banded"):
        raise ValueError(f"{who}: solver '{solver}' needs a matrix to factor; a matrix-free operator takes the Krylov solvers "
                         "'gmres', 'bicgstab' or (symmetric=True) 'cocg'")
    if solver not in _MATVEC_KRYLOV:
        raise ValueError(f"{who}: unknown solver '{solver}'; a matrix-free operator takes the Krylov solvers 'gmres', 'bicgstab' "
                         "or (symmetric=True) 'cocg'")
    if solver in ("cocg", "shifted_cocg", "block_cocg") and not symmetric:
        raise ValueError(f"{who}: solver '{solver}' needs symmetric=True (A = A^T and B = B^T); use 'bicgstab' or 'gmres' otherwise")
    if inner_precision != 64:
        raise ValueError(f"{who}: inner_precision={inner_precision} is not provided for operators (complex128 panels only)")


def _hermitian_probe(eng, N, real, names, seed):
    """|<x, M y> - <M x, y>| on one random two-column block for M = A (and B): ValueError naming the operator when they differ
    by more than HERMITIAN_PROBE_TOL of the product norms."""
    rng = np.random.default_rng(20260515 if seed is None else seed)
    XY = rng.standard_normal((N, 2)) + (0 if real else 1j * rng.standard_normal((N, 2)))
    dXY = eng.upload(XY)
    for which, name in names:
        M = eng.download(eng.matmul(which, dXY, 2), 2)
        x, y, Mx, My = XY[:, 0], XY[:, 1], M[:, 0], M[:, 1]
        gap = abs(np.vdot(x, My) - np.vdot(Mx, y))
        scale = max(np.linalg.norm(x) * np.linalg.norm(My), np.linalg.norm(Mx) * np.linalg.norm(y))
        if not gap <= HERMITIAN_PROBE_TOL * scale:
            raise ValueError(f"feast_matvec: {name} is not Hermitian: |<x, {name} y> - <{name} x, y>| = {gap:.3e} on a random pair "
                             f"(product norms {scale:.3e}); feast_general_matvec takes non-Hermitian operators")


def _operator_delta(eng, before):
    now = eng.operator_stats()
    return {k: now[k] - before[k] for k in now}


def feast_matvec(A_mul, B_mul, N, interval, *, M0=10, fpm=None, solver="gmres", solver_tol=1e-6, solver_maxiter=200,
                 solver_restart=20, real=True, symmetric=False, batched=False, check=True, Q0=None, seed=None, contour=None,
                 warm_start=True, inner_rtol=None, inner_precision=64, engine=None, device=0):
    """Matrix-free feast: feast_matvec(A_mul!, B_mul!, N, interval; M0, fpm) of src/interfaces/feast_interfaces.jl:465-481 for
    Hermitian operators that live on the device.  ``A_mul(Y, X)`` / ``B_mul(Y, X)`` write A X / B X into Y; X and Y are torch
    views of the solver's panels (engine.set_operator describes them: ``real``, ``batched``); ``B_mul=None`` means B = I.  The
    solver defaults are the reference's (GMRES(20), 1e-6, 200 steps: src/sparse/feast_sparse.jl:1287-1290); ``solver`` is
    "gmres", "bicgstab" or -- ``symmetric=True``: A = A^T, B = B^T, i.e. real symmetric operators -- "cocg".  ``real=True``
    (a real operator on the real view of the panels) also selects the real projection, as real matrices do in feast().
    ``check``: a Hermitian probe of A (and B) on one random pair before the solve; ValueError names the operator that fails.
    ``stats["operator"]`` = {A_calls, B_calls, callback_seconds} of this call, the probe included."""
    _check_matvec("feast_matvec", A_mul, B_mul, N, M0, solver, symmetric, inner_precision)
    N = int(N)
    Emin, Emax = float(interval[0]), float(interval[1])
    fpm = feastinit() if fpm is None else fpm
    feastdefault(fpm)
    eng = _engine(engine, device)
    eng.set_operator(N, A_mul, B_mul, real=real, symmetric=symmetric, batched=batched)
    before = eng.operator_stats()
    if check:
        _hermitian_probe(eng, N, real, [(0, "A")] + ([] if B_mul is None else [(1, "B")]), seed)
    kw = {} if seed is None else {"seed": seed}
    res = feast_hip_hermitian(eng, _ShapeOnly(N), None if B_mul is None else _ShapeOnly(N), Emin, Emax, min(int(M0), N), fpm,
                              solver=solver, solver_tol=solver_tol, solver_maxiter=int(solver_maxiter),
                              solver_restart=int(solver_restart), warm_start=bool(warm_start), inner_rtol=inner_rtol,
                              real_projection=None if real else False, Q0=Q0, contour=contour, preloaded=True, **kw)
    if isinstance(res.stats, dict):
        res.stats["operator"] = _operator_delta(eng, before)
    if real:
        res = FeastResult(res.lambda_, np.real(res.q), res.M, res.res, res.info, res.epsout, res.loop, res.stats)
    return res


def feast_general_matvec(A_mul, B_mul, N, center, radius, *, M0=10, fpm=None, solver="gmres", solver_tol=1e-6,
                         solver_maxiter=200, solver_restart=20, real=True, symmetric=False, batched=False, Q0=None, seed=None,
                         contour=None, inner_precision=64, engine=None, device=0):
    """Matrix-free feast_general: the eigenvalues of the caller's operators inside the circle (center, radius); the arguments
    are feast_matvec's, ``real=False`` takes complex operators (complex128 panels of shape (N, ld)), and no Hermitian probe
    runs.  ``stats["operator"]`` as in feast_matvec."""
    _check_matvec("feast_general_matvec", A_mul, B_mul, N, M0, solver, symmetric, inner_precision)
    N = int(N)
    fpm = feastinit() if fpm is None else fpm
    feastdefault(fpm)
    eng = _engine(engine, device)
    eng.set_operator(N, A_mul, B_mul, real=real, symmetric=symmetric, batched=batched)
    before = eng.operator_stats()
    kw = {} if seed is None else {"seed": seed}
    res = feast_hip_general(eng, _ShapeOnly(N), None if B_mul is None else _ShapeOnly(N), complex(center), float(radius),
                            min(int(M0), N), fpm, solver=solver, solver_tol=solver_tol, solver_maxiter=int(solver_maxiter),
                            solver_restart=int(solver_restart), Q0=Q0, contour=contour, preloaded=True, **kw)
    if isinstance(res.stats, dict):
        res.stats["operator"] = _operator_delta(eng, before)
    return res


# ---- matrix-free split forms and polynomials: the caller's term operators on the device (engine.set_term_operator) -------------
_TERM_KRYLOV = ("gmres", "bicgstab", "cocg")
NORM_SAMPLES = 32                 # +-1 columns of the norm estimate of feast_nonlinear_matvec(norms=None)
NORM_SEED = 20260515


def _check_term_matvec(who, muls, N, M0, Q0, solver, symmetric, norms, ortho):
    """The argument checks of feast_nonlinear_matvec / feast_polynomial_matvec that need no function value; all of them run
    before an engine is made or used."""
    if len(muls) < 2 or len(muls) > POLY_MAX_DEGREE + 1:
        raise ValueError(f"{who} needs 2 to {POLY_MAX_DEGREE + 1} terms, not {len(muls)}")
    for k, mul in enumerate(muls):
        if mul is not None and not callable(mul):
            raise ValueError(f"{who}: term {k} must be callable, mul(Y, X) writes A_k X into Y, or None for the identity")
    if int(N) < 1:
        raise ValueError(f"{who}: N must be at least 1")
    if isinstance(M0, str):
        raise ValueError(f"{who}: M0 must be an integer (the count estimate of M0='auto' is not provided for operators)")
    _check_poly_M0(M0, Q0)
    check_ortho(ortho)
    if solver in ("direct", "lu", "sparse_direct", "banded"):
        raise ValueError(f"{who}: solver '{solver}' needs a matrix to factor; term operators take the Krylov solvers "
                         "'gmres', 'bicgstab' or (symmetric=True) 'cocg'")
    if solver not in _TERM_KRYLOV:
        raise ValueError(f"{who}: unknown solver '{solver}'; term operators take the Krylov solvers 'gmres', 'bicgstab' or "
                         "(symmetric=True) 'cocg'")
    if solver == "cocg" and not symmetric:
        raise ValueError(f"{who}: solver 'cocg' needs symmetric=True (every A_k = A_k^T); use 'bicgstab' or 'gmres' otherwise")
    if norms is not None:
        nv = np.asarray(norms, dtype=np.float64)
        if nv.shape != (len(muls),) or not np.all(np.isfinite(nv)) or not np.all(nv > 0):
            raise ValueError(f"{who}: norms must be {len(muls)} positive numbers, one per term")


def _estimate_term_norms(eng, N, muls):
    """||A_k||_F^2 ~ (1 / NORM_SAMPLES) sum_c ||A_k v_c||^2 over NORM_SAMPLES seeded +-1 columns (E ||A v||^2 = ||A||_F^2 for
    independent +-1 entries): one callback per non-identity term, through nep_eval_cols with a unit-row table.  sqrt(N),
    exact, for an identity term."""
    m = min(NORM_SAMPLES, N)
    rng = np.random.default_rng(NORM_SEED)
    V = rng.integers(0, 2, size=(N, m)).astype(np.float64) * 2.0 - 1.0
    dV = eng.upload(V.astype(np.complex128))
    norms = np.empty(len(muls))
    for k, mul in enumerate(muls):
        if mul is None:
            norms[k] = math.sqrt(N)
            continue
        F = np.zeros((m, len(muls)), dtype=np.complex128)
        F[:, k] = 1.0
        W = eng.download(eng.nep_eval_cols(dV, F, m), m)
        norms[k] = math.sqrt(float(np.sum(np.abs(W) ** 2)) / m)
    return norms


def _term_matvec(who, key, muls, funcs, N, center, radius, M0, fpm, solver, solver_tol, solver_maxiter, solver_restart, real, symmetric,
                 batched, norms, ortho, Q0, contour, seed, engine, device, companion, extra):
    _check_term_matvec(who, muls, N, M0, Q0, solver, symmetric, norms, ortho)
    N = int(N)
    if not radius > 0:
        raise ValueError("radius must be positive")
    fpm = feastinit() if fpm is None else fpm
    feastdefault(fpm)
    M0 = min(int(M0), N)
    if Q0 is not None and np.shape(Q0) != (N, M0):
        raise ValueError(f"Q0 must be the N-row start block of shape ({N}, {M0}), not {np.shape(Q0)}")
    Zne, Wne = feast_gcontour(complex(center), float(radius), fpm) if contour is None else contour
    F_node = nep_table(funcs, Zne)
    if not np.isfinite(F_node).all():
        bad = int(np.flatnonzero(~np.isfinite(F_node).all(axis=0))[0])
        raise ValueError(f"f_{bad} is not finite at a contour node (a pole or an overflow on the circle)")
    eng = _engine(engine, device)
    eng.set_term_operator(N, muls, real=real, symmetric=symmetric, batched=batched)
    before = eng.operator_stats()
    estimated = norms is None
    nv = _estimate_term_norms(eng, N, muls) if estimated else np.asarray(norms, dtype=np.float64)
    if not np.all(nv > 0):          # (a zero operator: any positive number serves a term that adds nothing)
        nv = np.where(nv > 0, nv, 1.0)
    eng.set_term_norms(nv)
    eng.set_real_projection(False)
    eng.set_contour(Zne, Wne, 1.0)
    kw = {} if seed is None else {"seed": int(seed)}
    res = feast_hip_nonlinear(eng, [_ShapeOnly(N) for _ in muls], funcs, complex(center), float(radius), M0, fpm, Q0=Q0,
                              contour=(Zne, Wne), ortho=ortho, prepared=True, companion=companion,
                              krylov=(solver, float(solver_tol), int(solver_maxiter), int(solver_restart)), **extra, **kw)
    if isinstance(res.stats, dict):
        now = eng.operator_stats()
        res.stats["operator"] = {"term_calls": [a - b for a, b in zip(now["term_calls"], before["term_calls"])],
                                 "callback_seconds": now["callback_seconds"] - before["callback_seconds"],
                                 "norms": [float(v) for v in nv], "norms_estimated": bool(estimated)}
        rec = res.stats.get("nonlinear")
        if key == "polynomial" and rec is not None:
            del res.stats["nonlinear"]
            poly = {"degree": len(muls) - 1, "method": "projected", "columns": rec.pop("columns")}
            for drop in ("terms", "moments", "reduced_nodes", "reduced_seconds"):
                rec.pop(drop, None)
            poly.update(rec)
            res.stats["polynomial"] = poly
    return res


def feast_nonlinear_matvec(terms, N, center, radius, *, M0=10, fpm=None, solver="gmres", solver_tol=1e-6, solver_maxiter=200,
                           solver_restart=20, real=True, symmetric=False, batched=False, norms=None, ortho="mgs", Q0=None,
                           contour=None, seed=None, moments=2, reduced_nodes=128, engine=None, device=0):
    """Matrix-free feast_nonlinear: the eigenvalues of T(lambda) = sum_k f_k(lambda) A_k inside the circle, the A_k given as
    products on the device.  ``terms``: 2 to 9 pairs (A_mul_k, f_k); ``A_mul_k(Y, X)`` writes A_k X into Y on torch views of the
    solver's panels (engine.set_term_operator describes them: ``real``, ``batched``), or is None for A_k = I; f_k is a callable
    or a non-negative int p for lambda^p, as in feast_nonlinear.  The method is feast_nonlinear's with every solve T(z_e) Y = R
    done by ``solver``: "gmres" (the default, with feast_matvec's defaults GMRES(20), 1e-6, 200 steps), "bicgstab", or
    -- ``symmetric=True``: every A_k = A_k^T -- "cocg".  ``solver_tol`` = 0 means 10^-fpm[3]; the stop test is relative only,
    solves start from zero, and a node stopped at the cap is counted (``stats["nonlinear"]["krylov"][loop]["capped_nodes"]``),
    not an error.  On non-normal dense problems restarted GMRES(20) can stall: raise ``solver_restart``.
    ``norms``: one positive number per term that stands where ||A_k||_F stands in the backward errors ``res`` / ``epsout``;
    None: estimated from 32 seeded +-1 columns (one call per non-identity term; sqrt(N), exact, for an identity), recorded in
    ``stats["operator"]["norms"]`` with ``"norms_estimated": True``.
    ``stats["operator"]`` = {term_calls, callback_seconds, norms, norms_estimated}; ``stats["nonlinear"]`` as feast_nonlinear
    fills it, plus ``"plan": "krylov"`` and the per-loop ``"krylov"`` records.  All argument checks run before an engine is made
    or used.  Not covered: M0 = "auto" and the count estimate, preconditioners, complex64 panels, multi-rank sweeps."""
    terms = list(terms)
    if any(not isinstance(t, (tuple, list)) or len(t) != 2 for t in terms):
        raise ValueError("each term must be a pair (A_mul_k, f_k)")
    if int(moments) < 1 or int(reduced_nodes) < 8:
        raise ValueError("moments must be >= 1 and reduced_nodes >= 8")
    muls = [t[0] for t in terms]
    _check_term_matvec("feast_nonlinear_matvec", muls, N, M0, Q0, solver, symmetric, norms, ortho)
    funcs = nep_functions([t[1] for t in terms])
    return _term_matvec("feast_nonlinear_matvec", "nonlinear", muls, funcs, N, center, radius, M0, fpm, solver, solver_tol,
                        solver_maxiter, solver_restart, real, symmetric, batched, norms, ortho, Q0, contour, seed, engine, device, False,
                        dict(moments=int(moments), reduced_nodes=int(reduced_nodes)))


def feast_polynomial_matvec(coeff_muls, N, center, radius, *, M0=10, fpm=None, solver="gmres", solver_tol=1e-6, solver_maxiter=200,
                            solver_restart=20, real=True, symmetric=False, batched=False, norms=None, ortho="mgs", Q0=None,
                            contour=None, seed=None, engine=None, device=0):
    """Matrix-free feast_polynomial: the eigenvalues of P(lambda) = sum_k lambda^k A_k inside the circle for coefficients given
    as products on the device -- feast_polynomial(coeffs_ops::Vector{<:MatrixFreeOperator}, center, radius; solver=:gmres) of
    src/interfaces/feast_matfree.jl:607-647, by the projected method on N-row subspaces instead of the dN x dN companion
    operator.  ``coeff_muls[k](Y, X)`` writes A_k X into Y (None: A_k = I); every other argument and the statistics are
    feast_nonlinear_matvec's, with ``stats["polynomial"]`` as feast_polynomial(method="projected") fills it."""
    muls = list(coeff_muls)
    _check_term_matvec("feast_polynomial_matvec", muls, N, M0, Q0, solver, symmetric, norms, ortho)
    funcs = nep_functions(list(range(len(muls))))
    return _term_matvec("feast_polynomial_matvec", "polynomial", muls, funcs, N, center, radius, M0, fpm, solver, solver_tol,
                        solver_maxiter, solver_restart, real, symmetric, batched, norms, ortho, Q0, contour, seed, engine, device, True, {})
