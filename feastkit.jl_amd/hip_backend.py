"""The ``:hip`` backend: host-side FEAST refinement loops that keep the reference's state
machine and call the MI355X kernels through an *engine* (``engine.HipEngine``) for every
per-quadrature-node operation.

  feast_hip_hermitian  -- variant A ("QR + Rayleigh-Ritz"), mirrors
        _feast_dense_complex_hermitian  src/dense/feast_dense.jl:78-351
        _feast_sparse_hermitian         src/sparse/feast_sparse.jl:246-499
  feast_hip_general    -- variant C maths of feast_grci!/feast_gegv!
        src/kernel/feast_kernel.jl:646-962, src/dense/feast_dense.jl:402-593
  feast_hip_complex_symmetric -- complex-symmetric sibling of variant A (q^T instead of q^H)
        src/dense/feast_dense.jl:1026-1259, src/sparse/feast_sparse.jl:509-711

Quadrature nodes are block-partitioned over the ranks of the communicator attached to the engine
(``feasthip_comm_init_rank``) exactly like ``distribute_contour_points``
(src/parallel/feast_parallel.jl:433-447); each rank sweeps its nodes and the C ABI itself sums
Q_proj (and the per-node status) with ONE packed RCCL all-reduce over xGMI inside every
``contour_apply`` call -- the image of src/parallel/feast_mpi.jl:117-119 -- after which every rank
runs the reduced eigenproblem redundantly, as the MPI path does (src/parallel/feast_mpi.jl:121-139).
No ``torch.distributed`` collective is issued by this module; a ``group`` argument is only a
convenience to attach the engine's communicator through an existing process group.

The reduced M0 x M0 eigenproblem stays on host LAPACK.
"""
from __future__ import annotations

import contextlib
import ctypes
import math
import threading
import time
import warnings

import numpy as np
import scipy.linalg as sla

from . import _lib
from .contour import (balanced_contour_points, cost_balanced_contour_points, distribute_contour_points, feast_contour,
                      feast_gcontour, feast_inside_gcontour, split_balanced_assignment)
from .engine import HipEngine
from .parameters import check_feast_srci_input, feast_tolerance, feastdefault
from .types import FeastError, FeastResult

SQRT_EPS = math.sqrt(np.finfo(np.float64).eps)
DIRECT_SOLVERS = ("direct", "lu", "banded")        # every other solver name is a Krylov method

try:
    # The reduced M0 x M0 problems are far too small for threaded BLAS, and a BLAS pool that keeps spinning
    # after the call starves the thread that feeds the GPU launch queue (measured on a 256-core host:
    # 0.89 s -> 0.71 s per cfg-3 solve).
    from threadpoolctl import ThreadpoolController as _ThreadpoolController
    _BLAS_POOLS = _ThreadpoolController()
except Exception:
    _BLAS_POOLS = None


class small_lapack:
    """Context manager: run the enclosed host LAPACK calls on one BLAS thread.  Re-entrant and cheap when nested: only the
    outermost level talks to threadpoolctl (setting and restoring the limits costs 0.1-0.3 ms, as much as the 64 x 64
    eigenproblem itself), so the drivers hold it for the whole solve and the per-loop calls nest inside it for free.
    The nesting depth is process wide (the BLAS limit is) and guarded by a lock: drivers running on several host threads
    (one engine each) share one limit, released when the last of them leaves."""
    _depth = 0
    _outer = None
    _lock = threading.Lock()

    def __enter__(self):
        cls = small_lapack
        with cls._lock:
            if cls._depth == 0 and _BLAS_POOLS is not None:
                cls._outer = _BLAS_POOLS.limit(limits=1)
                cls._outer.__enter__()
            cls._depth += 1
        return self

    def __exit__(self, *exc):
        cls = small_lapack
        with cls._lock:
            cls._depth -= 1
            if cls._depth == 0 and cls._outer is not None:
                ctx, cls._outer = cls._outer, None
                ctx.__exit__(None, None, None)
        return False


def seeded_subspace(N, M0, seed=20260515, complex_values=False):
    """Initial subspace: real Gaussian columns of unit norm (src/core/feast_tools.jl:6-43).
    The Julia MersenneTwister stream is not reproducible outside Julia; the structure is."""
    rng = np.random.default_rng([seed, N, M0, int(complex_values)])
    R = rng.standard_normal((N, M0))
    I = rng.standard_normal((N, M0)) if complex_values else None
    # (same random stream and the same values as the first version of this routine, in a third of the passes over the
    #  N x M0 block: the norms are taken on the real arrays and the result is assembled directly in column-major order --
    #  at N = 50 000, M0 = 64 this is a fifth of a default feast() call)
    if complex_values:
        nrm = np.sqrt(np.einsum("ij,ij->j", R, R) + np.einsum("ij,ij->j", I, I))
    else:
        nrm = np.sqrt(np.einsum("ij,ij->j", R, R))
    nrm[nrm == 0] = 1.0
    out = np.zeros((N, M0), dtype=np.complex128, order="F")
    out.real = R / nrm
    if complex_values:
        out.imag = I / nrm
    return out


def _world(engine, group=None):
    """(rank, world) of the communicator attached to ``engine``.  When none is attached but the host runs a
    ``torch.distributed`` group of more than one rank, the engine is attached through it first (control plane
    only: the unique id travels over the group, the reductions are the library's own)."""
    if getattr(engine, "comm_size", 1) > 1:
        return engine.comm_rank, engine.comm_size
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            engine.comm_init_from_group(group)
            return engine.comm_rank, engine.comm_size
    except ImportError:
        pass
    return 0, 1


def _reorder_by_interval(lam, Emin, Emax, n):
    """Stable inside-first permutation (src/core/feast_aux.jl:144-197) -> (perm, ninside)."""
    inside = [i for i in range(n) if Emin <= lam[i] <= Emax]
    outside = [i for i in range(n) if not (Emin <= lam[i] <= Emax)]
    return np.array(inside + outside, dtype=np.int64), len(inside)


try:
    from scipy.linalg.lapack import dsygvd as _dsygvd
except Exception:                                                # pragma: no cover
    _dsygvd = None


def _reduced_hermitian_eig(Sq, Aq):
    """eigen(Hermitian(Sq), Hermitian(Aq)) with the general fallback
    (src/dense/feast_dense.jl:270-284)."""
    with small_lapack():
        try:
            if not (np.any(Sq.imag) or np.any(Aq.imag)):
                # real-symmetric pencil (real projection of real-symmetric input): dsygvd called directly -- the same
                # eigenpairs as zhegv at a third of the time, without the argument checking of the scipy wrapper
                # (eigh: 0.26 ms for 64 x 64 on one BLAS thread, of which LAPACK itself is about half)
                a = np.array(Sq.real, dtype=np.float64, order="F")
                b = np.array(Aq.real, dtype=np.float64, order="F")
                if _dsygvd is not None:
                    lam, V, info = _dsygvd(a, b, itype=1, jobz="V", uplo="L", overwrite_a=1, overwrite_b=1)
                    if info == 0:
                        return np.asarray(lam, dtype=np.float64), V.astype(np.complex128)
                    raise np.linalg.LinAlgError("dsygvd info %d" % info)
                lam, V = sla.eigh(a, b)
                return np.asarray(lam, dtype=np.float64), V.astype(np.complex128)
            lam, V = sla.eigh(Sq, Aq)
            return np.asarray(lam, dtype=np.float64), V
        except Exception:
            w, V = sla.eig(Sq, Aq)
            return np.real(w).astype(np.float64), V


def _empty_result(N, info, loop=0, *, complex_lambda=False, real_q=False, epsout=math.inf, stats=None):
    """The FeastResult of a call that returns no eigenpair: bad input, a failed sweep or nothing converged."""
    return FeastResult(np.zeros(0, complex if complex_lambda else float), np.zeros((N, 0), float if real_q else complex), 0,
                       np.zeros(0), int(info), epsout, loop, {} if stats is None else stats)


def _setup_sweep(engine, group, A, B, Zne, Wne, weight, real_projection, preloaded=False):
    """Communicator, pencil (unless the engine holds the problem already: preloaded), contour (weights weight * Wne[e]),
    projection and this rank's block of nodes -> (world, count)."""
    rank, world = _world(engine, group)
    if not preloaded:
        engine.set_problem(A, B)
    engine.set_contour(Zne, Wne, weight)
    engine.set_real_projection(real_projection)
    first, count = distribute_contour_points(len(Zne), world)[rank]
    engine.set_node_range(first, count)
    return world, count


def _configure_solver(engine, solver, fpm, solver_tol, solver_maxiter, solver_restart, **extra):
    """The standard solver setting: tol 10^-fpm[3] unless solver_tol, absolute too for Krylov -> (iterative, tol_value)."""
    iterative = solver not in DIRECT_SOLVERS
    tol_value = feast_tolerance(fpm) if solver_tol == 0.0 else float(solver_tol)
    engine.set_solver(solver, rtol=tol_value, atol=tol_value if iterative else 0.0, maxit=solver_maxiter,
                      restart=solver_restart, cache_factors=True, **extra)
    return iterative, tol_value


def _failure(status, world, count):
    """Raw failure code of a sweep (0, 5 = a Krylov solve failed, 8 = singular shift); a lone rank without nodes has none."""
    return int(np.max(status)) if (world > 1 or count > 0) else 0


def _sweep(engine, dQ, m, world, count, stats, lam_guess=None, want_moments=False, resident=False):
    """One sweep + the solve counters into stats (if kept) -> (raw failure code, the engine's tuple); each driver maps the code."""
    if resident:
        out = (None,) + tuple(engine.contour_apply_resident(dQ, m, lam_guess))
    elif want_moments:
        out = engine.contour_apply(dQ, m, lam_guess, want_moments=True)
    else:
        out = engine.contour_apply(dQ, m, lam_guess)
    st = out[2]
    if stats is not None:
        stats["krylov_iterations"] += st.get("krylov_iterations", 0)
        stats["factorizations"] += st.get("factorizations", 0)
        stats["solve_seconds"] += st.get("seconds_solve", 0.0)
    return _failure(out[1], world, count), out


def _check_circle_input(N, M0, r):
    """Input check of the general and complex-symmetric drivers -> 1 (N), 2 (M0), 4 (radius) or 0."""
    if N <= 0:
        return 1
    if M0 <= 0 or M0 > N:
        return 2
    if not r > 0:
        return 4
    return 0


def _complex_pencil(A, B):
    """A and B as complex128 (complex input as it is)."""
    Ac = A.astype(np.complex128) if not np.iscomplexobj(A) else A
    Bc = None if B is None else (B.astype(np.complex128) if not np.iscomplexobj(B) else B)
    return Ac, Bc


def _reorder_by_contour(lam, Emid, r, fpm, n):
    """Stable inside-first permutation for the contour of (Emid, r) -> (perm, ninside); cf. _reorder_by_interval."""
    ins = [i for i in range(n) if feast_inside_gcontour(lam[i], Emid, r, fpm)]
    inset = set(ins)
    return np.array(ins + [i for i in range(n) if i not in inset], dtype=np.int64), len(ins)


class _NodeLayout:
    """This rank's quadrature nodes (local_nodes, count) and right-hand-side column group (my_cg of my_cgs) in a Hermitian sweep."""

    def __init__(self, engine, n_nodes, rank, world, M0, column_groups, node_assignment, iterative):
        if column_groups == "auto":
            column_groups = 1
            if iterative and world > 1:
                for g in range(world, 0, -1):
                    if world % g == 0 and M0 // g >= 16:
                        column_groups = g
                        break
        column_groups = int(column_groups)
        if column_groups < 1 or world % column_groups != 0 or (column_groups > 1 and not iterative):
            raise ValueError("column_groups must divide the world size and needs an iterative solver")
        self.rank, self.world, self.iterative, self.node_assignment = rank, world, iterative, node_assignment
        self.node_groups, self.node_rank = world // column_groups, rank // column_groups
        balanced = node_assignment == "balanced" or callable(node_assignment)
        if balanced and self.node_groups > 1:
            nodes_here = balanced_contour_points(n_nodes, self.node_groups)[self.node_rank]
            engine.set_node_list(nodes_here)
            self.count, self.local_nodes = len(nodes_here), list(nodes_here)
        else:
            first, self.count = distribute_contour_points(n_nodes, self.node_groups)[self.node_rank]
            engine.set_node_range(first, self.count)
            self.local_nodes = list(range(first, first + self.count))
        # this rank's column group: fixed by the grid, or re-derived every loop by split_balanced_assignment, which splits
        # only the heaviest nodes by columns
        self.my_cg, self.my_cgs = rank % column_groups, column_groups
        self.split = balanced and column_groups == 1 and world > 1 and iterative
        self.node_parts = {}                         # node -> column groups it was swept in (its iteration count arrives summed)

    def column_block(self, ncols):
        """[c0, c1) of this rank's column group: blocks in multiples of 16, remainder to the last."""
        if self.my_cgs == 1:
            return 0, ncols
        per = max(16, -(-ncols // self.my_cgs // 16) * 16) if ncols >= 16 * self.my_cgs else -(-ncols // self.my_cgs)
        c0 = min(ncols, self.my_cg * per)
        c1 = ncols if self.my_cg == self.my_cgs - 1 else min(ncols, c0 + per)
        return c0, c1

    def rebalance(self, engine, loop_idx, active, stats):
        """From loop 1 on: re-derive the layout from the iteration counts the sweep just measured (identical on every rank)."""
        if loop_idx < 1 or not hasattr(engine, "last_global_node_iterations"):
            return
        if self.split:
            # node-only layout asked for: let the heaviest nodes be split by columns over several ranks when that lowers
            # the largest share (contour.split_balanced_assignment)
            costs = [float(v) / self.node_parts.get(e, 1) for e, v in enumerate(engine.last_global_node_iterations())]
            layout = (self.node_assignment(costs, self.world) if callable(self.node_assignment)
                      else split_balanced_assignment(costs, self.world, ncols=active))
            nodes_here, self.my_cg, self.my_cgs = layout[self.rank]
            self.node_parts = {e: k for nodes, _g, k in layout for e in nodes}
            stats["layout"] = [(list(map(int, nodes)), int(g), int(k)) for nodes, g, k in layout]
        elif self.node_assignment == "balanced" and self.node_groups > 1 and self.iterative:
            # re-balance the node groups: the slow near-axis nodes no longer share a group by accident
            nodes_here = cost_balanced_contour_points(engine.last_global_node_iterations(), self.node_groups)[self.node_rank]
        else:
            return
        if list(nodes_here) != list(self.local_nodes):
            engine.set_node_list(nodes_here)
            self.count, self.local_nodes = len(nodes_here), list(nodes_here)
            stats["local_nodes"] = [int(v) for v in self.local_nodes]


NODE_SOLVER_SOLVERS = ("cocg", "bicgstab", "iterative")     # handle solvers a per-node sweep can mix with direct nodes
NODE_SOLVER_DIRECT = 4                                      # FEASTHIP_SOLVER_BANDED
DIRECT_FLOP_RATE = 1.3e13                                   # flop/s of the sparse direct solver (api.feast's hand-over estimate)
# flop/s of its substitution with 64 right-hand sides inside a sweep, measured on cfg 3 (tools/node_solver_probe.py, DESIGN.md
# section 6g: a loop that factors nothing spends 14.2 ms per direct node beyond its Krylov chain, for 2.2e10 flop)
DIRECT_SOLVE_RATE = 1.55e12


def check_direct_nodes(direct_nodes, ne, sparse, solver):
    """Host-only validation of the ``direct_nodes`` keyword (no device work) -> None, "auto", an int k or a sorted index list."""
    if direct_nodes is None:
        return None
    if not sparse:
        raise ValueError("direct_nodes needs sparse input (the per-node solver mixes Krylov sweeps with sparse direct solves)")
    if solver not in NODE_SOLVER_SOLVERS:
        raise ValueError(f"direct_nodes needs solver 'cocg', 'bicgstab' or 'iterative', not '{solver}'")
    if isinstance(direct_nodes, str):
        if direct_nodes != "auto":
            raise ValueError("direct_nodes must be None, a list of node indices, an int or 'auto'")
        return "auto"
    if isinstance(direct_nodes, (bool, float, np.floating)):
        raise ValueError("direct_nodes must be None, a list of node indices, an int or 'auto'")
    if isinstance(direct_nodes, (int, np.integer)):
        if not 0 <= int(direct_nodes) <= ne:
            raise ValueError(f"direct_nodes={int(direct_nodes)}: between 0 and the node count {ne}")
        return int(direct_nodes)
    try:
        idx = [v for v in direct_nodes]
    except TypeError:
        raise ValueError("direct_nodes must be None, a list of node indices, an int or 'auto'") from None
    if any(isinstance(v, (bool, float, str)) or not isinstance(v, (int, np.integer)) for v in idx):
        raise ValueError("direct_nodes: node indices must be integers")
    if any(not 0 <= int(v) < ne for v in idx):
        raise ValueError(f"direct_nodes: node indices must lie in 0..{ne - 1}")
    return sorted(set(int(v) for v in idx))


class _DirectNodes:
    """The ``direct_nodes`` keyword of the host drivers: which contour nodes (GLOBAL indices) the sweeps solve directly
    (feasthip_set_node_solver), chosen up front (a list), after the first loop (an int k: the k slowest nodes) or after every
    loop by feasthip_policy_pick_direct_nodes ("auto").  Every rank derives the same set from the global iteration vector.
    ``log`` becomes stats["direct_nodes"]: one entry per loop."""

    def __init__(self, engine, spec, ne, m, world):
        self.engine, self.spec, self.ne, self.m, self.world = engine, spec, ne, m, world
        self.nodes, self.log, self.note = [], [], None
        self.t_iter = self.t_solve = self.t_factor = None        # "auto": the measured inputs of the selection rule
        self.max_fit = self._fit()
        if isinstance(spec, list):
            if len(spec) > self.max_fit:
                raise ValueError(f"direct_nodes: the factors of {len(spec)} nodes do not fit the free device memory "
                                 f"({self.max_fit} would)")
            self.nodes = list(spec)
        elif spec != "auto" and spec > self.max_fit:
            self.note = f"shrunk from {spec} to {self.max_fit}: device memory"
        self._apply()

    def _fit(self):
        """How many direct nodes fit: cached factors plus the transient buffers of their factorisation and sweep
        (feasthip_direct_plan_bytes, linear in the node count) within the share of the free device memory the library's own
        slot allocation accepts (0.92, band_ensure_slots); the smallest answer over the ranks."""
        import torch
        free, _total = torch.cuda.mem_get_info(self.engine.device)
        fb, tb = self.engine.direct_plan_bytes(1)
        k = min(self.ne, int(0.92 * free // max(1, fb + tb)))
        if self.world > 1:
            k = int(round(-self.engine.max_over_ranks(-k)))
        return k

    def _apply(self):
        kinds = np.zeros(self.ne, dtype=np.int32)
        kinds[self.nodes] = NODE_SOLVER_DIRECT
        self.engine.set_node_solver(kinds if self.nodes else None)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.engine.set_node_solver(None)
        return False

    def record(self, loop_idx, st, local_nodes=None):
        """One entry for the loop just swept: the nodes in force and what it factored (summed over the ranks).  Everything
        the choice below rests on is made rank-independent here: the global iteration vector, and -- one small all-reduce
        -- every rank's sweep seconds, factorisations and local direct nodes, of which the slowest rank's are kept."""
        eng = self.engine
        self.iters = np.asarray(eng.last_global_node_iterations() if self.world > 1 else eng.last_node_iterations(self.ne),
                                dtype=np.int32)
        if local_nodes is None:                       # the block partition of _setup_sweep
            first, count = distribute_contour_points(self.ne, self.world)[eng.comm_rank]
            local_nodes = range(first, first + count)
        nd = len(set(self.nodes) & set(int(v) for v in local_nodes))
        mine = [float(st.get("seconds_solve", 0.0)), float(st.get("factorizations", 0)), float(nd)]
        if self.world > 1:
            t = eng.torch.zeros((self.world, 3), dtype=eng.torch.float64, device=eng.device)
            t[eng.comm_rank] = eng.torch.tensor(mine, dtype=eng.torch.float64, device=eng.device)
            rows = eng.allreduce_sum_(t).cpu().numpy()
        else:
            rows = np.array([mine])
        self.sweep = tuple(float(v) for v in rows[int(np.argmax(rows[:, 0]))])       # (seconds, factorisations, direct nodes)
        self.log.append({"loop": int(loop_idx), "nodes": list(self.nodes), "factorizations": int(round(rows[:, 1].sum()))})
        if self.note:
            self.log[-1]["note"] = self.note

    def _loops_left(self, loop_idx, eps_hist, eps_tol, maxloop):
        """Loops still to come: from the contraction of the last two outer residuals, at most what fpm[4] leaves."""
        fin = [e for e in eps_hist if np.isfinite(e) and e > 0]
        left = maxloop - loop_idx
        if len(fin) >= 2 and fin[-1] < fin[-2]:
            left = min(left, int(math.ceil(max(1.0, math.log(eps_tol / fin[-1]) / math.log(fin[-1] / fin[-2])))))
        return max(1, left)

    def _calibrate(self):
        """The three times of the selection rule.  t_iter: the last all-Krylov sweep's seconds per iteration of its longest
        node (a sweep with direct nodes also spends their solves).  t_factor, t_solve: the flop model (feasthip_direct_plan_flops
        / DIRECT_FLOP_RATE; one complex multiply-add per factor entry and column / DIRECT_SOLVE_RATE), raised to what the sweeps
        with direct nodes spend beyond their Krylov chain: a sweep that factored nothing gives t_solve, one that factored t_factor."""
        secs, nfact, nd = self.sweep
        chain = int(self.iters.max())
        if nd == 0 or self.t_iter is None:
            self.t_iter = secs / max(1, chain)
        if self.t_solve is None:
            fb, _tb = self.engine.direct_plan_bytes(1)
            self.t_factor = self.engine.direct_plan_flops() / DIRECT_FLOP_RATE
            self.t_solve = 8.0 * (fb / 16.0) * self.m / DIRECT_SOLVE_RATE
        beyond = secs - self.t_iter * chain
        if nd and nfact == 0:
            self.t_solve = max(self.t_solve, beyond / nd)
        elif nd:
            self.t_factor = max(self.t_factor, (beyond - nd * self.t_solve) / nfact)
        return self.t_iter, self.t_solve, self.t_factor

    def choose(self, loop_idx, eps_hist, eps_tol, maxloop):
        """The nodes of the next loop, after a loop that did not converge."""
        iters, entry = self.iters, self.log[-1]
        room = self.max_fit - len(self.nodes)
        if isinstance(self.spec, list) or room <= 0 or not iters.any():
            return
        order = sorted(range(self.ne), key=lambda e: (-int(iters[e]), e))
        new = []
        if self.spec == "auto":
            left = self._loops_left(loop_idx, eps_hist, eps_tol, maxloop)
            t_iter, t_solve, t_factor = self._calibrate()
            kinds = np.zeros(self.ne, dtype=np.int32)
            it_c = np.ascontiguousarray(iters, dtype=np.int32)
            k = _lib.load_library().feasthip_policy_pick_direct_nodes(
                it_c.ctypes.data_as(ctypes.c_void_p), self.ne, int(room), t_iter, t_solve, t_factor, int(left),
                kinds.ctypes.data_as(ctypes.c_void_p))
            new = [int(e) for e in np.nonzero(kinds)[0]]
            # the rule's own prediction: the all-Krylov loop against the loop with its k nodes direct
            t_none = t_iter * int(iters[order[0]])
            t_pick = t_iter * (int(iters[order[k]]) if k < self.ne else 0) + k * (t_solve + t_factor / left)
            entry.update(t_iter=t_iter, t_solve=t_solve, t_factor=t_factor, loops_left=int(left), predicted_gain=t_none - t_pick)
        elif loop_idx == 0:
            new = [e for e in order[:min(int(self.spec), room)] if iters[e] > 0]
        if new:
            self.nodes = sorted(set(self.nodes) | set(new))         # a node once chosen stays chosen
            self._apply()


def _direct_nodes_scope(engine, direct_nodes, ne, sparse, solver, m, world, stats, inner_precision=64):
    """The drivers' ``direct_nodes`` keyword as a context: the kinds are set for the loops inside and cleared on every way
    out; ``stats["direct_nodes"]`` is the per-loop log.  None: nothing changes."""
    if direct_nodes is None:
        return contextlib.nullcontext()
    spec = check_direct_nodes(direct_nodes, ne, sparse, solver)
    if inner_precision != 64:
        raise ValueError("direct_nodes needs inner_precision=64")
    dn = _DirectNodes(engine, spec, ne, m, world)
    stats["direct_nodes"] = dn.log
    return dn


def check_precond(precond, precond_shifts=1, *, sparse=True, solver="gmres", inner_precision=64, group=None, direct_nodes=None,
                  two_sided=False, estimate=False, auto_m0=False):
    """Host-only validation of the ``precond`` / ``precond_shifts`` keywords (no device work) -> None, an int k >= 1 or a list
    of complex pivots.  Everything the shift preconditioner does not go with raises ValueError and names what to use."""
    if precond is None:
        return None
    if precond != "shift":
        raise ValueError(f"precond must be None or 'shift', not {precond!r}")
    if not sparse:
        raise ValueError("precond='shift' needs sparse input (the pivots are factored by the sparse direct solver); dense input takes solver='direct'")
    if solver != "gmres":
        raise ValueError(f"precond='shift' needs solver='gmres', not '{solver}' (BiCGStab and COCG run unpreconditioned; use solver='gmres' or drop precond)")
    if inner_precision != 64:
        raise ValueError("precond='shift' needs inner_precision=64: the identity form I + c B M^-1 needs exact pivot factors")
    if two_sided:
        raise ValueError("precond='shift' has no two-sided form; use two_sided=True with solver='sparse_direct', or drop two_sided")
    if group is not None:
        raise ValueError("precond='shift' sweeps on one rank; drop group= or use an unpreconditioned Krylov solver")
    if direct_nodes is not None:
        raise ValueError("precond='shift' does not mix with direct_nodes=; use one of them (direct_nodes= goes with solver='cocg' or 'bicgstab')")
    if estimate:
        raise ValueError("precond='shift' does not apply to the count estimate (fpm[14] = 2); run the estimate without precond")
    if auto_m0:
        raise ValueError("precond='shift' does not go with M0='auto'; estimate first (fpm[14] = 2 without precond), then pass M0")
    ps = precond_shifts
    if isinstance(ps, (bool, str, float, np.floating)):
        raise ValueError("precond_shifts must be an int k >= 1 or a list of complex pivot shifts")
    if isinstance(ps, (int, np.integer)):
        if int(ps) < 1:
            raise ValueError("precond_shifts must be an int k >= 1 or a list of complex pivot shifts")
        return int(ps)
    try:
        piv = [complex(v) for v in ps]
    except TypeError:
        raise ValueError("precond_shifts must be an int k >= 1 or a list of complex pivot shifts") from None
    if not piv:
        raise ValueError("precond_shifts: the pivot list is empty")
    if any(p.imag == 0.0 or not np.isfinite(p.real) or not np.isfinite(p.imag) for p in piv):
        raise ValueError("precond_shifts: every pivot needs a non-zero imaginary part (z_p B - A is factored; on the real axis it may be singular)")
    if len(set(piv)) != len(piv):
        raise ValueError("precond_shifts: the pivots must be distinct")
    return piv


def precond_plan(Zne, spec):
    """(pivot shifts, node -> pivot index) of a checked ``precond_shifts``: the rules of csrc/fh_precond.hpp.  An int k: the
    nodes in order cut into k arcs [a ne // k, (a + 1) ne // k), each arc's pivot its middle node (of two, the lower one in
    the first half of the arcs, the upper one in the second: 8 nodes in 2 arcs give nodes 1 and 6).  A list: every node takes
    its nearest pivot (lowest index on ties)."""
    ne = len(Zne)
    if isinstance(spec, int):
        k = max(1, min(spec, ne))
        node_pivot, pivots = [0] * ne, []
        for a in range(k):
            lo, hi = a * ne // k, (a + 1) * ne // k
            pivots.append(complex(Zne[lo + (hi - lo - 1) // 2 if 2 * a + 1 <= k else lo + (hi - lo) // 2]))
            node_pivot[lo:hi] = [a] * (hi - lo)
        return pivots, node_pivot
    return list(spec), [int(np.argmin([abs(complex(z) - p) ** 2 for p in spec])) for z in Zne]


class _Precond:
    """The drivers' ``precond`` keyword as a context: the preconditioner is set on the engine for the loops inside (after
    set_contour, which keeps it only for the same node count) and cleared on every way out.  ``log`` becomes
    stats["precond"]: one entry per loop."""

    def __init__(self, engine, spec, Zne):
        self.engine, self.log = engine, []
        self.pivots, self.node_pivot = precond_plan(Zne, spec)
        if any(p.imag == 0.0 for p in self.pivots):
            raise ValueError("precond_shifts: a contour node on the real axis cannot be a pivot; pass the pivots as a list")

    def __enter__(self):
        self.engine.set_preconditioner(self.pivots, self.node_pivot)
        return self

    def __exit__(self, *exc):
        self.engine.set_preconditioner(None)
        return False

    def record(self, count):
        last = self.engine.last_precond_sweep()
        self.log.append({"pivots": list(self.pivots), "node_pivot": list(self.node_pivot), "factorizations": last["factorizations"],
                         "substitution_sweeps": last["substitution_sweeps"],
                         "lock_steps": [int(v) for v in self.engine.last_node_iterations(count)],
                         "factor_bytes": last["factor_bytes"], "fell_back": last["fell_back"], "used": last["used"]})


def _precond_scope(engine, precond, precond_shifts, Zne, sparse, solver, stats, inner_precision=64, group=None, direct_nodes=None):
    """None: nothing changes (a null context whose value is None)."""
    spec = check_precond(precond, precond_shifts, sparse=sparse, solver=solver, inner_precision=inner_precision, group=group,
                         direct_nodes=direct_nodes)
    if spec is None:
        return contextlib.nullcontext()
    pc = _Precond(engine, spec, Zne)
    stats["precond"] = pc.log
    return pc


class _InexactPolicy(_lib.FeastHipPolicy):
    """The inexact mode's host policy under the C ABI (feasthip_policy_*, csrc/fh_policy.hpp); fields are the C struct's.
    hist, reach: fpm[18] and the subspace reach of every loop under contour steering."""

    def init(self, Emin, Emax, fpm, inner_rtol, outer_tol, maxiter, steer):
        """feasthip_policy_init -> True when the policy is in force."""
        self.hist, self.reach = [], []
        return _lib.load_library().feasthip_policy_init(
            ctypes.byref(self), float(Emin), float(Emax), int(fpm[2]), int(fpm[16]), float(inner_rtol), float(outer_tol),
            int(maxiter), int(steer), int(fpm[18])) == 0

    def update(self, epsout, M, capped, ritz, rank_q):
        """feasthip_policy_update after a loop -> (ellipse ratio changed, inner cap or tolerance changed)."""
        prev = self.aspect, self.inner_cap, self.next_rtol
        ritz_c = np.ascontiguousarray(ritz[:rank_q], dtype=np.float64)
        _lib.load_library().feasthip_policy_update(ctypes.byref(self), float(epsout), int(M), int(capped),
                                                   ritz_c.ctypes.data_as(ctypes.c_void_p), int(rank_q))
        return self.aspect != prev[0], (self.inner_cap, self.next_rtol) != prev[1:]

    def steer(self, engine, Emin, Emax, fpm, layout):
        """fpm[18] := the policy's ellipse ratio, the contour re-issued on this rank's nodes (set_contour resets them)."""
        fpm[18] = self.aspect
        Zne, Wne = feast_contour(Emin, Emax, fpm)
        engine.set_contour(Zne, Wne, 2.0)
        engine.set_node_list(layout.local_nodes)


def _policy_set_aside(engine, resident, dP, rank_q, V, lam, M, dX, res):
    """Inexact inner solves leave solver noise in the guard columns.  Its Ritz values are arbitrary; one that lands inside
    the interval has an O(1) residual that never contracts and would hold epsout up forever (variant A has no spurious-pair
    removal; with exact solves the guard columns are true eigen-directions and stay outside).  A pair is set aside when
    its relative residual is > 0.1 AND > 100x the smallest residual of the pairs inside: a true pair inside the interval
    sees a filter value >= 1/2 and contracts with the others, it cannot sit at 10 % while another pair is 100x ahead.
    Set-aside pairs stay in the subspace and are re-examined every loop (measured on a random pencil: the ten true pairs
    contract by ~1e-2 per loop while one to three noise pairs stay at residual 1).  feasthip_policy_set_aside needs no
    policy state.  -> (n set aside, dX, lam, M, res): the n pairs moved behind the M - n kept, the Ritz pairs formed again."""
    resc = np.ascontiguousarray(res, dtype=np.float64)
    flags = np.zeros(M, dtype=np.int32)
    n = int(_lib.load_library().feasthip_policy_set_aside(resc.ctypes.data_as(ctypes.c_void_p), int(M),
                                                          flags.ctypes.data_as(ctypes.c_void_p)))
    if not 0 < n < M:
        return 0, dX, lam, M, res
    flag = flags.astype(bool)
    order = np.concatenate([np.nonzero(~flag)[0], np.nonzero(flag)[0], np.arange(M, rank_q)])
    lam = lam[order]
    dX, res = _ritz_pairs(engine, resident, dP, rank_q, np.asfortranarray(V[:, order]), lam, M - n)
    return n, dX, lam, M - n, res


def _initial_block(engine, Q0, N, M0, seed):
    """The start block on the device: a device Q0 (data_ptr; only ever read), the seeded block, or the host Q0 uploaded."""
    if Q0 is not None and hasattr(Q0, "data_ptr"):
        return Q0
    if Q0 is not None:
        return engine.upload(np.asarray(Q0, dtype=np.complex128))
    # the seeded start block is a function of (N, M0, seed): generating it on the host takes 35 ms at N = 50 000, M0 = 64 --
    # a sixth of a default feast() call -- so an engine keeps the last one on the device for repeated calls
    key = (int(N), int(M0), int(seed))
    cache = getattr(engine, "_seed_cache", None)
    if cache is not None and cache[0] == key:
        return cache[1]
    dQ = engine.upload(seeded_subspace(N, M0, seed))
    try:
        engine._seed_cache = (key, dQ)
    except AttributeError:
        pass
    return dQ


def _host_reduced_eig(engine, dP, rank_q, SA, Emin, Emax, ph):
    """The reduced eigenproblem on the host, projected first unless resident panels gave (Sq, Aq) -> (lam, V, M) sorted
    inside first, or None when LAPACK fails."""
    tick = time.perf_counter
    if SA is None:
        t_ = tick()
        SA = engine.project(dP, rank_q, bilinear=False, hermitize=True)
        ph["project"] += tick() - t_
    t_ = tick()
    try:
        lam_red, v_red = _reduced_hermitian_eig(*SA)
    except Exception:
        return None
    ph["eig"] += tick() - t_
    perm, M = _reorder_by_interval(lam_red, Emin, Emax, rank_q)
    return lam_red[perm], np.asfortranarray(v_red[:, perm]), M


def _ritz_pairs(engine, resident, dP, rank_q, V, lam, M):
    """Ritz vectors and residuals of the host reduced solution -> (dX, res); resident panels keep the block (dX None)."""
    if resident:
        return None, engine.rr_ritz_resident(rank_q, V, lam, M, normalize=True, use_B=True)
    return engine.ritz_residual(dP, rank_q, V, lam, M, normalize=True, use_B=True)


class _LoopRecord:
    """The Ritz values (lam_vec), residuals of the M_found pairs inside (res_vec) and epsout of the last refinement loop;
    loops: the stats["loops"] list that gets one entry per loop, if kept."""

    def __init__(self, M0, eps_tol, maxloop, dtype=float, loops=None):
        self.lam_vec, self.res_vec = np.zeros(M0, dtype=dtype), np.zeros(M0)
        self.epsout, self.M_found = math.inf, 0
        self.eps_tol, self.maxloop, self.loops = eps_tol, maxloop, loops

    def record(self, loop_idx, n, lam, M, res, st=None, set_aside=None):
        """Keep the loop's n Ritz values and its M residuals -> None, or the info to stop with (0, or 5 after the last loop).
        set_aside: pairs the host reduced solver set aside (its entry also keeps the residuals); None for the device one."""
        self.lam_vec[:n] = lam
        if M > 0:
            self.res_vec[:M] = res[:M]
            self.epsout = float(res[:M].max())
        else:
            self.epsout = math.inf
        self.M_found = M
        if self.loops is not None:
            entry = {"loop": loop_idx, "rank": n, "M": M, "epsout": self.epsout}
            if set_aside is not None:
                entry["set_aside"] = set_aside
            entry["krylov_iterations"] = st.get("krylov_iterations", 0)
            if set_aside is not None:
                entry["res_inside"] = np.array(res[:M], dtype=float).copy() if M > 0 else np.zeros(0)
            self.loops.append(entry)
        if M > 0 and self.epsout <= self.eps_tol:
            return 0
        if loop_idx == self.maxloop:
            return int(FeastError.Feast_ERROR_NO_CONVERGENCE)
        return None

    def result(self, q, info, loop, stats=None, order=None):
        """The FeastResult of the M_found pairs, in ``order`` if given; info 5 when no pair converged and nothing failed."""
        M = self.M_found
        if M == 0 and info == 0:
            info = int(FeastError.Feast_ERROR_NO_CONVERGENCE)
        lam, res = self.lam_vec[:M], self.res_vec[:M]
        if order is not None:
            lam, res, q = lam[order], res[order], q[:, order].copy()
        return FeastResult(lam.copy(), q, M, res.copy(), info, self.epsout, loop, {} if stats is None else stats)


ORTHO_METHODS = ("mgs", "cholqr_rr")


def check_ortho(ortho):
    """Host-only validation of the ``ortho`` keyword."""
    if ortho not in ORTHO_METHODS:
        raise ValueError(f"ortho must be one of {ORTHO_METHODS}, not {ortho!r}")
    return ortho


@contextlib.contextmanager
def _ortho_scope(engine, ortho, stats):
    """The drivers' ``ortho`` keyword as a context: the engine orthonormalises rank-deficient panels by that method inside
    and by the default on every way out.  ``stats["ortho"]`` gets one entry per loop (_note_ortho)."""
    check_ortho(ortho)
    if not hasattr(engine, "set_ortho_method"):
        if ortho != "mgs":
            raise ValueError(f"ortho={ortho!r}: this engine has no choice of orthonormalisation")
        yield
        return
    stats["ortho"] = []
    engine.set_ortho_method(ortho)
    try:
        yield
    finally:
        engine.set_ortho_method("mgs")


def _note_ortho(engine, stats):
    if "ortho" in stats and hasattr(engine, "last_ortho"):
        stats["ortho"].append(engine.last_ortho())


def feast_hip_hermitian(engine, A, B, Emin, Emax, M0, fpm, *, freeze_guards_after=None, reduced_solver="host",
                        solver="direct", solver_tol=0.0,
                        solver_maxiter=500, solver_restart=30, warm_start=True, inner_rtol=None,
                        real_projection=None, group=None, Q0=None, seed=20260515, contour=None, trace=None,
                        preloaded=False, node_assignment="block", inner_precision=64, column_groups=1,
                        spurious_filter=True, contour_policy=None, eps_floor=0.0, abort_check=None, resident_panels=True,
                        direct_nodes=None, ortho="mgs", precond=None, precond_shifts=1):
    """Variant A on the :hip engine.  Returns FeastResult (complex Ritz vectors, like
    _feast_dense_complex_hermitian; real-symmetric callers take real.(q) as the reference
    does, src/dense/feast_dense.jl:372-387).

    solver: "direct" (dense batched LU), "bicgstab"/"iterative" (batched BiCGStab), "gmres".
    solver_tol: 0 -> 10^-fpm[3] like the reference.  Krylov stop test: ||r|| <= tol + tol*||r0||.
    warm_start (iterative only, not in the reference): after the first loop the Ritz pairs
      (lambda_j, q_j) seed the solves with Y0 = q_j/(z_e - lambda_j), whose residual is
      r_j/(z_e - lambda_j) -- Galerkin-orthogonal to the current subspace.  ``inner_rtol``
      then bounds the reduction relative to that initial residual (default solver_tol).
    column_groups: g > 1 (iterative solvers, multi-rank) arranges the ranks as
      (world/g node groups) x (g column groups): a rank sweeps its node group for only its
      block of right-hand-side columns (blocks of >= 16 columns).  The reference shards nodes
      only (feast_parallel.jl:433-447); with Krylov solves the near-axis nodes need 10x the
      iterations of the others, so pure node sharding is bounded by the slowest node while
      columns of one node cost the same.  "auto" picks the largest g dividing the world size
      that leaves >= 16 columns per rank.  Q_proj columns are disjoint across column groups,
      so the one all-reduce per loop is unchanged.
    inner_precision: 64 | 32 (iterative solvers on sparse matrices).  32 solves the correction
      (z_e B - A) d = r0/||r0|| of each warm-started system in complex64 and adds it back in
      fp64; valid for inexact solves only (inner_rtol >= 1e-5).  Warm start, residuals,
      orthonormalisation and Rayleigh-Ritz stay fp64, so the converged eigenpairs are unchanged.
    real_projection: None -> True for real-symmetric A, B.  Q_proj = Re(sum 2 w_e Y_e), the
      full-contour FEAST filter (what the reference's real paths do, feast_parallel.jl:38-55,
      feast_kernel.jl:183-186).  False keeps variant A's complex half-contour sum
      (feast_dense.jl:231), whose filter only decays like 1/distance: same converged
      eigenpairs, many more refinement loops.
    contour_policy: None keeps fpm[18] as given (the reference's behaviour).  "auto" (inexact iterative solves with the
      real projection only; ignored otherwise) lets the driver pick the ellipse ratio fpm[18] itself, loop by loop
      (feasthip_policy_*, csrc/fh_policy.hpp): with inner solves that reduce the residual by inner_rtol per loop the contraction of a
      refinement loop is max(filter ratio, ~2 inner_rtol), so among the candidate ratios the one minimising the
      predicted work  a^-0.6 / ln(1 / max(filter ratio(a), inner_rtol))  is taken (a^-0.6: measured fall of the
      Krylov iterations per loop with the ratio a; a taller ellipse moves every node away from the spectrum).  The
      filter ratio is evaluated at the reach of the current subspace (feasthip_policy_reach of the Ritz values; loop 0:
      the a-priori 1.4 half widths of a subspace 1.5 times the eigenvalue count).  Safeguard: when a loop contracts
      the residual by less than 0.3 although the policy promised better, then -- if inner solves stopped at the iteration
      cap -- the cap is doubled, else the ratio is halved for the next loops, down to the reference's circle.
    direct_nodes: None | list of GLOBAL node indices | int k | "auto" (sparse input, cocg / bicgstab): those contour nodes are
      solved by the sparse direct solver inside the Krylov sweep (feasthip_set_node_solver) -- the list in every loop, the k
      slowest nodes of the first loop from the second on, or what feasthip_policy_pick_direct_nodes picks after every loop.
      ``stats["direct_nodes"]`` has one entry per loop; ``stats["node_iterations"]`` shows 0 for a direct node.
    precond, precond_shifts: None | "shift" (sparse input, solver "gmres"): the GMRES sweeps run preconditioned by the LU
      factors of z_p B - A at a few pivot shifts (feasthip_set_preconditioner; check_precond, precond_plan).
      ``stats["precond"]`` has one entry per loop.
    """
    N = A.shape[0]
    feastdefault(fpm)
    info = check_feast_srci_input(N, M0, Emin, Emax)
    if info:
        return _empty_result(N, info)
    rank, world = _world(engine, group)
    iterative = solver not in DIRECT_SOLVERS

    t_setup = time.perf_counter()
    if not preloaded:                            # matrices already resident on the device
        engine.set_problem(A, B)
    Zne, Wne = feast_contour(Emin, Emax, fpm) if contour is None else contour
    engine.set_contour(Zne, Wne, 2.0)            # weight = 2*Wne[e]: src/dense/feast_dense.jl:174
    if real_projection is None:
        import scipy.sparse as _sp
        _isc = lambda M_: M_ is not None and np.iscomplexobj(M_.data if _sp.issparse(M_) else M_)
        q_real = Q0 is None or (hasattr(Q0, "data_ptr") and not bool((Q0.imag != 0).any())) or \
            (not hasattr(Q0, "data_ptr") and (not np.iscomplexobj(Q0) or not np.any(np.imag(Q0))))
        real_projection = not (_isc(A) or _isc(B)) and q_real
    engine.set_real_projection(bool(real_projection))
    layout = _NodeLayout(engine, len(Zne), rank, world, M0, column_groups, node_assignment, iterative)
    _, tol_value = _configure_solver(engine, solver, fpm, solver_tol, solver_maxiter, solver_restart)
    if inner_precision not in (32, 64):
        raise ValueError("inner_precision must be 32 or 64")
    inexact = bool(iterative and warm_start and inner_rtol is not None and float(inner_rtol) > 10.0 * tol_value)
    # block COCG with frozen guard columns: the cocg sweep (stats["block"] then reports used = False)
    eng_solver = "cocg" if (solver == "block_cocg" and freeze_guards_after is not None) else solver
    if iterative and warm_start:
        # inexact-solve mode: every loop reduces the (warm-started) residual by inner_rtol
        rt = tol_value if inner_rtol is None else float(inner_rtol)
        if inner_precision == 32 and rt < 1e-5:
            raise ValueError("inner_precision=32 needs inner_rtol >= 1e-5 (single-precision correction solves)")
        engine.set_solver(eng_solver, rtol=rt, atol=0.0, maxit=solver_maxiter, restart=solver_restart,
                          factor_precision=inner_precision)
    elif inner_precision == 32:
        if solver in DIRECT_SOLVERS:
            # dense LU / blocked band LU: complex64 factors + fp64 iterative refinement inside every solve
            engine.set_solver(eng_solver, rtol=tol_value, atol=0.0, maxit=solver_maxiter, restart=solver_restart,
                              factor_precision=32, cache_factors=True)
        else:
            raise ValueError("inner_precision=32 needs a direct solver or the warm-started inexact iterative mode")
    eps_tol = max(feast_tolerance(fpm), float(eps_floor))      # eps_floor: sqrt(eps(Float32)) for single-precision callers
    # -- the host policy of the inexact mode lives under the C ABI.  Steering only where the filter is the real-projection
    #    filter.  The spurious-pair set-aside needs no policy state.
    auto_contour = bool(contour_policy == "auto" and contour is None and inexact and real_projection and int(fpm[16]) in (0, 1))
    pol = _InexactPolicy() if inexact else None
    if pol is not None and not pol.init(Emin, Emax, fpm, inner_rtol, eps_tol, solver_maxiter, auto_contour):
        pol = None
    if auto_contour and pol is not None:
        fpm = fpm.copy()
        pol.steer(engine, Emin, Emax, fpm, layout)
        pol.hist.append(pol.aspect)
    t_setup = time.perf_counter() - t_setup

    dQ = _initial_block(engine, Q0, N, M0, seed)
    maxloop = int(fpm[4])
    info, loop_count, active, ritz_lambda, dX = 0, 0, M0, None, None
    stats = {"setup_seconds": t_setup, "krylov_iterations": 0, "spmm_calls": 0, "factorizations": 0,
             "solve_seconds": 0.0, "loops": [], "node_iterations": [], "node_lists": [],
             "local_nodes": [int(v) for v in layout.local_nodes],
             "phase_seconds": {"apply": 0.0, "reduce": 0.0, "ortho": 0.0, "project": 0.0, "eig": 0.0, "ritz": 0.0}}
    ph = stats["phase_seconds"]
    tick = time.perf_counter
    done = _LoopRecord(M0, eps_tol, maxloop, loops=stats["loops"])

    t_loops = time.perf_counter()
    # The refinement loop with resident panels (engine.contour_apply_resident / rr_reduce_resident / rr_ritz_resident): one
    # 64-column panel, reduced eigenproblem on the host.  The per-primitive calls remain for wide subspaces (M0 > 64), the
    # device eigensolver and engines without the resident entry points.
    resident = bool(getattr(engine, "resident", False)) and M0 <= 64 and reduced_solver != "device" and resident_panels
    # one BLAS thread for the whole solve; the `with` releases the process-wide limit on every way out, including an
    # exception from the engine inside the loop (FeastHipError, a poisoned handle)
    import scipy.sparse as _sp
    if precond is not None and contour_policy is not None:
        raise ValueError("precond='shift' keeps the contour it planned its pivots on; drop contour_policy=")
    with small_lapack(), _ortho_scope(engine, ortho, stats), \
            _direct_nodes_scope(engine, direct_nodes, len(Zne), _sp.issparse(A), solver, M0, world, stats, inner_precision) as dn, \
            _precond_scope(engine, precond, precond_shifts, Zne, _sp.issparse(A), solver, stats, inner_precision, group, direct_nodes) as pc:
        for loop_idx in range(0, maxloop + 1):
            loop_count = loop_idx
            # -- sweep
            t_ = tick()
            lam_guess = ritz_lambda if (iterative and warm_start) else None
            col_mask = None
            if lam_guess is not None and freeze_guards_after is not None and loop_idx > freeze_guards_after:
                # guard columns (Ritz value outside the interval) keep their warm start q/(z - lambda): they
                # stay in the subspace, scaled by the filter value, but no solves are spent on them
                col_mask = np.array([1 if Emin <= lam_guess[c] <= Emax else 0 for c in range(active)], dtype=np.int32)
            if hasattr(engine, "set_column_mask"):
                engine.set_column_mask(col_mask)                    # one-shot: consumed by the sweep below
            if layout.my_cgs > 1:
                c0, c1 = layout.column_block(active)
                engine.set_column_block(c0, c1 - c0)
            if inner_precision == 32 and not iterative:
                # inexact FEAST on complex64 factors: the solves are refined only as far as the current outer residual needs
                # (no refinement in the first loop; the last loops reach the full tolerance)
                ref_tol = 1.0 if not math.isfinite(done.epsout) else min(1.0, max(tol_value, 1e-2 * done.epsout))
                engine.set_solver(eng_solver, rtol=ref_tol, atol=0.0, maxit=solver_maxiter, restart=solver_restart,
                                  factor_precision=32, cache_factors=True)
            # one call = this rank's (nodes x column block) sweep + the packed all-reduce inside the C ABI: dP and status
            # come back summed over all ranks (status indexed by contour node when world > 1).  Resident panels: Q_proj
            # stays in the library in the kernels' layout; after the first loop the subspace is the Ritz block the
            # previous loop left there (dQ is None)
            fail, (dP, status, st) = _sweep(engine, dQ, active, world, layout.count, stats, lam_guess, resident=resident)
            if layout.my_cgs > 1:
                engine.set_column_block(0, -1)
            ph["apply"] += tick() - t_
            stats["spmm_calls"] += st.get("spmm_calls", 0)
            if hasattr(engine, "last_node_iterations"):
                stats["node_iterations"].append([int(v) for v in engine.last_node_iterations(layout.count)])
                stats["node_lists"].append([int(v) for v in layout.local_nodes])
            if solver == "shifted_cocg" and hasattr(engine, "last_shifted_sweep"):
                used, seed_node, seed_its, _ = engine.last_shifted_sweep()
                stats.setdefault("shifted", []).append({"used": used, "seed_node": seed_node, "seed_iterations": seed_its})
            if solver == "block_cocg" and hasattr(engine, "last_block_sweep"):
                used, steps_max, brk, passes = engine.last_block_sweep()
                stats.setdefault("block", []).append({"used": used, "node_steps_max": steps_max, "breakdown_nodes": brk,
                                                      "spmm_node_passes": passes})
            if dn is not None:
                dn.record(loop_idx, st, layout.local_nodes)
            if pc is not None:
                pc.record(layout.count)
            layout.rebalance(engine, loop_idx, active, stats)
            # direct: singular shift -> info 8 (src/dense/feast_dense.jl:199-203); reference GMRES failure -> info 5
            # (src/dense/feast_dense.jl:221-225).  Warm-started solves go on past a Krylov failure (5): the next loop
            # starts from where this one stopped.
            if fail == 8 or (fail == 5 and not warm_start):
                info = int(FeastError.Feast_ERROR_LAPACK if fail == 8 else FeastError.Feast_ERROR_NO_CONVERGENCE)
                break

            # -- reduce
            t_ = tick()
            if resident:
                # _feast_qr_compress! and the projections in one call: rank + (Q_o^H A Q_o, Q_o^H B Q_o)
                rank_q, Sq, Aq = engine.rr_reduce_resident(active, SQRT_EPS)
                ph["project"] += tick() - t_
            else:
                rank_q = engine.orthonormalize(dP, active, SQRT_EPS)       # _feast_qr_compress!
                ph["ortho"] += tick() - t_
            _note_ortho(engine, stats)
            if rank_q == 0:
                info = int(FeastError.Feast_ERROR_NO_CONVERGENCE)
                break

            # -- reduced eigenproblem, Ritz pairs and residuals: on the device in one call, or on the host
            rr = None
            if reduced_solver == "device" and rank_q <= 64 and trace is None and hasattr(engine, "rayleigh_ritz"):
                # project + reduced eigenproblem (Jacobi in LDS) + reorder + Ritz vectors + residuals in one call;
                # None: reduced B not positive definite -> the host path below (general fallback of the reference)
                t_ = tick()
                rr = engine.rayleigh_ritz(dP, rank_q, Emin, Emax, use_B=True)
                ph["ritz"] += tick() - t_
            if rr is not None:
                dX, lam_sorted, M, res = rr
                if M == 0 and not (iterative and warm_start):
                    info = int(FeastError.Feast_ERROR_NO_CONVERGENCE)
                    break
            else:
                red = _host_reduced_eig(engine, dP, rank_q, (Sq, Aq) if resident else None, Emin, Emax, ph)
                if red is None:
                    info = int(FeastError.Feast_ERROR_LAPACK)
                    break
                lam_sorted, V_sorted, M = red
                if trace is not None:
                    trace.append({"loop": loop_idx, "rank": rank_q, "M": M, "lambda": lam_sorted.copy(), "status": status.copy(),
                                  "stats": dict(st),
                                  "node_iterations": engine.last_node_iterations(layout.count) if hasattr(engine, "last_node_iterations") else None,
                                  "column_iterations": engine.last_column_iterations(layout.count, active) if hasattr(engine, "last_column_iterations") else None})
                if M == 0 and not (iterative and warm_start):
                    info = int(FeastError.Feast_ERROR_NO_CONVERGENCE)
                    break
                t_ = tick()
                dX, res = _ritz_pairs(engine, resident, dP, rank_q, V_sorted, lam_sorted, M)
                n_spurious = 0
                if inexact and spurious_filter and loop_idx >= 1 and M > 1:      # solver noise inside the interval
                    n_spurious, dX, lam_sorted, M, res = _policy_set_aside(engine, resident, dP, rank_q, V_sorted, lam_sorted,
                                                                           M, dX, res)
                ph["ritz"] += tick() - t_

            # -- stop test
            # (the device reduced solver sets no pair aside)
            stop = done.record(loop_idx, rank_q, lam_sorted, M, res, st, set_aside=None if rr is not None else n_spurious)
            if stop is not None:
                info = stop
                break
            if rr is None:                          # the device reduced solver has neither the abort test nor the policy
                if abort_check is not None and world == 1 and abort_check(loop_idx, [l["epsout"] for l in stats["loops"]],
                                                                          time.perf_counter() - t_loops):
                    # the caller has a cheaper way to finish (api.feast: the sparse direct solver): stop here
                    info = int(FeastError.Feast_ERROR_NO_CONVERGENCE)
                    stats["aborted"] = True
                    break
                if pol is not None:
                    # one call decides the next sweep: iteration cap (stagnation guard; capped nodes under the contour
                    # policy), inner tolerance (relaxed when the outer tolerance is within reach), and -- under the contour
                    # policy -- fpm[18]
                    new_aspect, new_solve = pol.update(done.epsout, M, int(np.max(status)) == 5, lam_sorted, rank_q)
                    if new_solve:
                        engine.set_solver(eng_solver, rtol=pol.next_rtol, atol=0.0, maxit=pol.inner_cap, restart=solver_restart,
                                          factor_precision=inner_precision)
                        if pol.inner_cap != int(solver_maxiter):
                            stats["inner_cap"] = pol.inner_cap
                    if auto_contour:
                        if new_aspect:
                            pol.steer(engine, Emin, Emax, fpm, layout)
                        pol.hist.append(pol.aspect)
                        pol.reach.append(None if pol.last_reach < 0 else round(pol.last_reach, 3))

            if dn is not None:
                dn.choose(loop_idx, [l["epsout"] for l in stats["loops"]], eps_tol, maxloop)

            # -- next loop
            active = rank_q
            dQ = dX                                   # Q_basis[:, 1:rank] = solutions[:, 1:rank]
            ritz_lambda = lam_sorted.copy()

    if auto_contour and pol is not None:
        stats["contour_policy"] = {"fpm18_per_loop": pol.hist, "cap": pol.cap, "reach": pol.reach}
    if hasattr(engine, "set_column_mask"):
        engine.set_column_mask(None)
    M_found = done.M_found
    # only the M converged Ritz vectors cross PCIe (the block is column-major: the first M rows of the tensor)
    if resident and M_found > 0:
        q = engine.download(engine.export_resident(M_found), M_found)
    else:
        q = engine.download(dX[:M_found], M_found) if (dX is not None and M_found > 0) else np.zeros((N, 0), dtype=np.complex128)
    return done.result(q, info, loop_count, stats)


ESTIMATE_SEED = 20260515          # default seed of the estimate's Rademacher block (the package seed)


def feast_hip_estimate(engine, A, B, Zne, Wne, weight_scale, m, *, general=False, seed=ESTIMATE_SEED, solver="direct",
                       solver_tol=1e-8, solver_maxiter=2000, solver_restart=30, group=None):
    """Stochastic estimate of the eigenvalue count inside the contour (Zne, Wne): fpm[14] = 2, which the reference
    validates (src/core/feast_parameters.jl:69-75) but never computes.  One sweep over m Rademacher columns V generated on
    the device, then Hutchinson's samples t_j = v_j^T Q_proj[:, j] (engine.estimate_count).

    Hermitian (general=False): half contour with the real projection, Q_proj = Re(sum_e 2 w_e (z_e B - A)^{-1} B) V, so
      t_j samples sum_i f(lambda_i) with f(x) = Re sum_e 2 w_e / (z_e - x) -- also for complex Hermitian input, since
      v_j is real and the full contour's trace is the real part of the half contour's.
    General (general=True): full contour, weight_scale 1, no projection: the t_j are complex and Re mean(t) estimates
      the count inside the circle.
    The estimate is of a sum of filter values, not of an integer: eigenvalues near the ends of the interval (or just
    outside) contribute fractions.  Krylov solves start from zero and stop at ||r|| <= solver_tol ||b||.

    Returns (info, estimate): info 0 with the dict {mean, stderr, samples, nodes, solver, seed, seconds}, or the node
    status 5 / 8 of a failed node and None."""
    t0 = time.perf_counter()
    world, count = _setup_sweep(engine, group, A, B, Zne, Wne, float(weight_scale), not general)
    engine.set_solver(solver, rtol=float(solver_tol), atol=0.0, maxit=int(solver_maxiter), restart=int(solver_restart),
                      cache_factors=True)
    samples, status, _st = engine.estimate_count(m, seed)
    fail = _failure(status, world, count)
    if fail:
        return (int(FeastError.Feast_ERROR_LAPACK) if fail == 8 else int(FeastError.Feast_ERROR_NO_CONVERGENCE)), None
    t = samples if general else samples.real
    mean = complex(np.mean(t)) if general else float(np.mean(t))
    stderr = float(np.std(t, ddof=1) / math.sqrt(m)) if m > 1 else math.inf
    est = {"mean": mean, "stderr": stderr, "samples": t.copy(), "nodes": len(Zne), "solver": solver, "seed": int(seed),
           "seconds": time.perf_counter() - t0}
    if solver not in DIRECT_SOLVERS:
        est["solver_tol"] = float(solver_tol)
    return 0, est


def feast_hip_general(engine, A, B, Emid, r, M0, fpm, *, solver="direct", solver_tol=0.0, solver_maxiter=500,
                      solver_restart=30, group=None, Q0=None, seed=20260515, inner_precision=64, contour=None, eps_floor=0.0,
                      direct_nodes=None, ortho="mgs", preloaded=False, precond=None, precond_shifts=1):
    """Variant C (general, full contour, no factor 2, no orthonormalisation, residual
    without B): src/kernel/feast_kernel.jl:752-950 driven as in src/dense/feast_dense.jl:468-584.
    ``preloaded``: the engine holds the problem already (engine.set_operator); A and B are then read for their shape only.
    ``ortho`` is checked and set on the engine for the solve like in the other drivers; this variant never orthonormalises
    its subspace, so ``stats["ortho"]`` stays empty.  ``precond``, ``precond_shifts``: as in feast_hip_hermitian."""
    N = A.shape[0]
    feastdefault(fpm)
    info = _check_circle_input(N, M0, r)
    if info:
        return _empty_result(N, info, complex_lambda=True)
    Ac, Bc = (A, B) if preloaded else _complex_pencil(A, B)
    # caller-supplied nodes/weights: the reference's "x" drivers (feast_gcsrgvx!/feast_gegvx!, src/sparse/feast_sparse.jl:1008-)
    Zne, Wne = feast_gcontour(Emid, r, fpm) if contour is None else contour
    world, count = _setup_sweep(engine, group, Ac, Bc, Zne, Wne, 1.0, False, preloaded)
    if inner_precision == 32 and solver not in DIRECT_SOLVERS:
        raise ValueError("inner_precision=32 (complex64 LU factors + fp64 refinement) needs a direct solver")
    _configure_solver(engine, solver, fpm, solver_tol, solver_maxiter, solver_restart,
                      factor_precision=32 if inner_precision == 32 else 64)
    Q_host = seeded_subspace(N, M0, seed) if Q0 is None else np.asarray(Q0, dtype=np.complex128)
    dQ = engine.upload(Q_host)
    eps_tol = max(feast_tolerance(fpm), float(eps_floor))
    maxloop = int(fpm[4])
    loop = 0
    stats = {"krylov_iterations": 0, "factorizations": 0, "solve_seconds": 0.0}
    epsout, eps_hist = math.inf, []
    import scipy.sparse as _sp
    with _ortho_scope(engine, ortho, stats), \
            _direct_nodes_scope(engine, direct_nodes, len(Zne), _sp.issparse(A), solver, M0, world, stats, inner_precision) as dn, \
            _precond_scope(engine, precond, precond_shifts, Zne, _sp.issparse(A), solver, stats, inner_precision, group, direct_nodes) as pc:
        while True:
            if inner_precision == 32:
                # inexact FEAST: the complex64 solves are refined only as far as the current outer residual needs
                ref_tol = 1.0 if not math.isfinite(epsout) else min(1.0, max(1e-14, 1e-2 * epsout))
                engine.set_solver(solver, rtol=ref_tol, atol=0.0, maxit=solver_maxiter, restart=solver_restart,
                                  cache_factors=True, factor_precision=32)
            fail, (dq, status, st) = _sweep(engine, dQ, M0, world, count, stats)
            if dn is not None:
                dn.record(loop, st)
            if pc is not None:
                pc.record(count)
            if fail:
                return _empty_result(N, FeastError.Feast_ERROR_LAPACK if fail == 8 else FeastError.Feast_ERROR_NO_CONVERGENCE,
                                     loop, complex_lambda=True, stats=stats)
            Aq, Sq = engine.project(dq, M0, bilinear=False, hermitize=False)   # Aq = q^H A q, Sq = q^H B q
            try:
                with small_lapack():
                    lam_red, v_red = sla.eig(Aq, Sq)                            # feast_kernel.jl:812
            except Exception:
                return _empty_result(N, FeastError.Feast_ERROR_LAPACK, loop, complex_lambda=True, stats=stats)
            perm, M = _reorder_by_contour(lam_red, Emid, r, fpm, M0)
            if M == 0:
                return _empty_result(N, FeastError.Feast_ERROR_NO_CONVERGENCE, loop, complex_lambda=True, stats=stats)
            lam = lam_red[perm]
            V = np.asfortranarray(v_red[:, perm])
            # normalise ALL M0 columns (feast_kernel.jl:864-876); residual WITHOUT B (:899-906)
            dX, res = engine.ritz_residual(dq, M0, V, lam, M0, normalize=True, use_B=False)
            res = res[:M]
            epsout = float(res.max())
            if epsout <= eps_tol or loop >= maxloop:
                order = sorted(range(M), key=lambda i: abs(lam[i]) ** 2)         # feast_sort_general!
                X = engine.download(dX, M0)
                return FeastResult(lam[:M][order].copy(), X[:, :M][:, order].copy(), M, res[order].copy(), 0, epsout, loop, stats)
            if dn is not None:
                eps_hist.append(epsout)
                dn.choose(loop, eps_hist, eps_tol, maxloop)
            loop += 1
            dQ = dX


POLY_RESIDUALS = ("pencil", "reference")


def _poly_setup(engine, coeffs, Emid, r, fpm, contour, union_csr, krylov=None, terms=False, prepared=False):
    """What both polynomial drivers do before their loop: the polynomial (dense, or sparse from ``union_csr``) becomes the engine's
    problem with the direct solver, cached fp64 factors, no real projection and the full contour -> the plan fields of
    ``stats["polynomial"]`` for sparse coefficients, else None.  ``krylov`` = (solver, tol, maxiter, restart), sparse
    coefficients only: that Krylov solver on P(z_e) instead, relative stop test (tol 0 = 10^-fpm[3]) -> {"plan": "krylov"}.
    ``terms``: the matrices are the A_k of a split form and the handle becomes a term handle (feast_hip_nonlinear).
    ``prepared``: the engine holds this problem and this contour already (the estimate behind M0 = "auto" set them and cached
    the factors): only the solver is set again."""
    Zne, Wne = feast_gcontour(Emid, r, fpm) if contour is None else contour
    if not prepared and union_csr is None:
        engine.set_polynomial(coeffs, terms=terms)
    elif not prepared:
        engine.set_polynomial_csr(*union_csr, terms=terms)
    if krylov is not None:
        solver, tol, maxiter, restart = krylov
        engine.set_solver(solver, rtol=feast_tolerance(fpm) if tol == 0.0 else float(tol), atol=0.0, maxit=maxiter, restart=restart,
                          factor_precision=64)
    else:
        engine.set_solver("direct", cache_factors=True, factor_precision=64)
    if not prepared:
        engine.set_real_projection(False)
        engine.set_contour(Zne, Wne, 1.0)
    if krylov is not None:
        return {"plan": "krylov"}
    if union_csr is None:
        return None
    factor_bytes, transient_bytes = engine.direct_plan_bytes(1)
    return {"plan": "multifrontal", "plan_factor_bytes": factor_bytes, "plan_transient_bytes": transient_bytes,
            "plan_flops": engine.direct_plan_flops(), "plan_nnz": int(len(union_csr[1]))}


def feast_hip_polynomial(engine, coeffs, Emid, r, M0, fpm, *, Q0=None, seed=20260515, contour=None, residual="pencil",
                         eps_floor=0.0, union_csr=None, prepared=False):
    """P(lambda) x = 0 inside a circle: feast_hip_general's loop on the first companion linearisation with M0 d columns
    (feast_pep!, src/dense/feast_dense.jl:715-772, driving feast_gegv! :763) -- full contour, no factor 2, no
    orthonormalisation -- with the companion pencil replaced by the engine's poly_* calls: one N x N LU per node.
    ``residual``: "pencil" measures ||A_lin x - lambda B_lin x|| / max(|lambda|, 1), "reference" omits B_lin as the
    reference's kernel does (src/kernel/feast_kernel.jl:899-906).  q: the first N rows of the M linearised Ritz vectors
    (src/dense/feast_dense.jl:768).
    ``union_csr`` = (rowptr, col, vals) of ingest.polynomial_union_csr(coeffs): the coefficients stay sparse
    (engine.set_polynomial_csr), P(z_e) is factored by the multifrontal LU and ``stats["polynomial"]`` gains plan =
    "multifrontal", plan_factor_bytes / plan_transient_bytes / plan_flops per node and plan_nnz of the union pattern.  A
    pattern without a plan, factors that do not fit and a rejected pivot raise FeastHipError (codes 9, 6, 8): there is no
    band LU for polynomials, the caller decides what to do instead.  ``prepared``: as in _poly_setup."""
    d = len(coeffs) - 1
    N = coeffs[0].shape[0]
    cols = M0 * d
    feastdefault(fpm)
    info = _check_circle_input(N, M0, r)
    if info:
        return _empty_result(N, info, complex_lambda=True)
    plan = _poly_setup(engine, coeffs, Emid, r, fpm, contour, union_csr, prepared=prepared)
    Q_host = seeded_subspace(d * N, cols, seed) if Q0 is None else np.asarray(Q0, dtype=np.complex128)
    if Q_host.shape != (d * N, cols):
        raise ValueError(f"Q0 must be the linearised start block of shape ({d * N}, {cols})")
    dQ = engine.upload(Q_host)
    eps_tol = max(feast_tolerance(fpm), float(eps_floor))
    maxloop = int(fpm[4])
    use_B = residual == "pencil"
    loop = 0
    eps_hist = []
    stats = {"krylov_iterations": 0, "factorizations": 0, "solve_seconds": 0.0,
             "polynomial": {"degree": d, "method": "linearised", "columns": cols, "residual": residual, "backward_error": np.zeros(0), "eps_history": eps_hist}}
    if plan is not None:
        stats["polynomial"].update(plan)
    while True:
        dq, status, st = engine.poly_contour_apply(dQ, cols)
        stats["factorizations"] += st.get("factorizations", 0)
        stats["solve_seconds"] += st.get("seconds_total", 0.0)
        if int(np.max(status)):
            return _empty_result(N, FeastError.Feast_ERROR_LAPACK, loop, complex_lambda=True, stats=stats)
        Aq, Sq = engine.poly_project(dq, cols)
        try:
            with small_lapack():
                lam_red, v_red = sla.eig(Aq, Sq)                                # feast_kernel.jl:812
        except Exception:
            return _empty_result(N, FeastError.Feast_ERROR_LAPACK, loop, complex_lambda=True, stats=stats)
        perm, M = _reorder_by_contour(lam_red, Emid, r, fpm, cols)
        if M == 0:
            return _empty_result(N, FeastError.Feast_ERROR_NO_CONVERGENCE, loop, complex_lambda=True, stats=stats)
        lam = lam_red[perm]
        V = np.asfortranarray(v_red[:, perm])
        # all columns normalised (feast_kernel.jl:864-876)
        dX, res, bwd = engine.poly_ritz_residual(dq, cols, V, lam, cols, normalize=True, use_B=use_B)
        res, bwd = res[:M], bwd[:M]
        epsout = float(res.max())
        eps_hist.append(epsout)
        if epsout <= eps_tol or loop >= maxloop:
            order = sorted(range(M), key=lambda i: abs(lam[i]) ** 2)             # feast_sort_general!
            X = engine.download(dX, cols)
            stats["polynomial"]["backward_error"] = bwd[order].copy()
            return FeastResult(lam[:M][order].copy(), X[:N, :M][:, order].copy(), M, res[order].copy(), 0, epsout, loop, stats)
        loop += 1
        dQ = dX


POLY_METHODS = ("linearised", "projected")
# Set-aside rule of the projected method: a selected pair inside the circle whose backward error exceeds BOTH the absolute
# threshold and `factor` times the smallest backward error inside is kept in the subspace but left out of M and epsout (the
# shape of feasthip_policy_set_aside's rule).  (absolute, factor)
POLY_SET_ASIDE = (1e-3, 100.0)


def _poly_companion(Ahat):
    """First companion pencil (A_lin, B_lin) of the small polynomial sum_k lambda^k Ahat[k], r x r coefficients."""
    d, r = len(Ahat) - 1, Ahat[0].shape[0]
    Al = np.zeros((d * r, d * r), dtype=np.complex128)
    Bl = np.eye(d * r, dtype=np.complex128)
    for i in range(d - 1):
        Al[i * r:(i + 1) * r, (i + 1) * r:(i + 2) * r] = np.eye(r)
    for j in range(d):
        Al[(d - 1) * r:, j * r:(j + 1) * r] = -Ahat[j]
    Bl[(d - 1) * r:, (d - 1) * r:] = Ahat[d]
    return Al, Bl


def poly_select(theta, be, center, radius, keep):
    """Selection and set-aside of the projected method.  The reduced polynomial has d r Ritz values for r columns, and the
    surplus ones fall inside a circle that the spectrum surrounds; "nearest to the centre" picks them and stagnates.  So:
    the candidates inside the circle in ascending backward error, then those outside in ascending distance, `keep` in all;
    among the selected inside ones a pair is set aside under POLY_SET_ASIDE.
    -> (selected indices, mask over them: inside and not set aside, number set aside)"""
    dist = np.abs(np.where(np.isfinite(theta), theta, np.inf) - center)
    inside = dist <= radius
    ins = np.flatnonzero(inside)
    ins = ins[np.argsort(be[ins], kind="stable")]
    out = np.flatnonzero(~inside)
    out = out[np.argsort(dist[out], kind="stable")]
    sel = np.concatenate([ins, out])[:keep]
    good = inside[sel].copy()
    aside = 0
    if good.any():
        best = be[sel][good].min()
        bad = good & (be[sel] > POLY_SET_ASIDE[0]) & (be[sel] > POLY_SET_ASIDE[1] * best)
        aside = int(bad.sum())
        good &= ~bad
    return sel, good, aside


class ReducedSolveError(Exception):
    """Host LAPACK failed on the small projected problem of a projected-method loop (-> Feast_ERROR_LAPACK)."""


def _projected_loop(engine, N, M0, Emid, r, fpm, Q0, seed, eps_floor, ortho, stats, rec, sweep, reduced, evaluate, krylov=False):
    """The loop of the projected method, shared by feast_hip_polynomial_projected and feast_hip_nonlinear; the problem is the
    engine's already.  Per loop: ``sweep(dX, m, sigma)`` -> (dQ, status, stats) is the contour step (sigma None: the plain sweep
    of loop 0), then unit columns and the rank-revealing orthonormalisation of ``ortho``, the projected matrices Q^H A_k Q,
    ``reduced(Ahat, rank)`` -> (theta, Y) the candidates of the small problem (it raises ReducedSolveError when host LAPACK
    fails; whatever else it raises is the caller's), ``evaluate(dQ, rank, Y, theta)`` -> (dXc, backward errors) on the device,
    poly_select.  Stop test: the largest backward error among the kept pairs inside the circle.  At the loop limit the last
    iterates are returned with info = Feast_ERROR_NO_CONVERGENCE; no candidate at all ends the loop with M = 0.  ``rec``: the
    method's entry of ``stats``, which gets eps_history, rank, candidates, set_aside (one entry per loop) and backward_error;
    ``krylov``: the sweeps are inexact Krylov solves, recorded per loop in rec["krylov"], and a node status 5 is no failure."""
    X_host = seeded_subspace(N, M0, seed) if Q0 is None else np.asarray(Q0, dtype=np.complex128)
    if X_host.shape != (N, M0):
        raise ValueError(f"Q0 must be the start block of shape ({N}, {M0})")
    dX = engine.upload(X_host)
    eps_tol = max(feast_tolerance(fpm), float(eps_floor))
    maxloop = int(fpm[4])
    center = complex(Emid)
    loop, m, sigma = 0, M0, None
    rec.update({"backward_error": np.zeros(0), "eps_history": [], "rank": [], "candidates": [], "set_aside": []})
    if krylov:
        rec["krylov"] = []
    no_conv = FeastError.Feast_ERROR_NO_CONVERGENCE
    with _ortho_scope(engine, ortho, stats):
        while True:
            dQ, status, st = sweep(dX, m, sigma)
            stats["factorizations"] += st.get("factorizations", 0)
            stats["solve_seconds"] += st.get("seconds_total", 0.0)
            if krylov:
                stats["krylov_iterations"] += int(st.get("krylov_iterations", 0))
                node_it = engine.last_node_iterations(len(status))
                rec["krylov"].append({"iterations": int(node_it.max()) if len(node_it) else 0,
                                      "node_iterations": [int(v) for v in node_it], "capped_nodes": int(np.sum(status == 5))})
                status = np.where(status == 5, 0, status)
            if int(np.max(status)):
                return _empty_result(N, FeastError.Feast_ERROR_LAPACK, loop, complex_lambda=True, stats=stats)
            rank_q = engine.poly_orthonormalize(dQ, m, SQRT_EPS, unit_columns=True)
            _note_ortho(engine, stats)
            if rank_q == 0:
                return _empty_result(N, no_conv, loop, complex_lambda=True, stats=stats)
            Ahat = engine.poly_project_reduced(dQ, rank_q)
            try:
                with small_lapack():
                    theta, Y = reduced(Ahat, rank_q)
            except ReducedSolveError:
                return _empty_result(N, FeastError.Feast_ERROR_LAPACK, loop, complex_lambda=True, stats=stats)
            ncand = len(theta)
            rec["rank"].append(int(rank_q))
            rec["candidates"].append(int(ncand))
            if ncand == 0:
                rec["eps_history"].append(math.inf)
                rec["set_aside"].append(0)
                return _empty_result(N, no_conv, loop, complex_lambda=True, stats=stats)
            dXc, be = evaluate(dQ, rank_q, np.asfortranarray(Y), theta)
            keep = min(M0, ncand)
            sel, good, aside = poly_select(theta, be, center, r, keep)
            M = int(good.sum())
            epsout = float(be[sel][good].max()) if M else math.inf
            rec["eps_history"].append(epsout)
            rec["set_aside"].append(aside)
            done = M > 0 and epsout <= eps_tol
            if done or loop >= maxloop:
                if M == 0:
                    return _empty_result(N, no_conv, loop, complex_lambda=True, stats=stats)
                idx = sel[good]
                idx = idx[np.argsort(np.abs(theta[idx]) ** 2, kind="stable")]                 # feast_sort_general!
                Xall = engine.download(dXc, ncand)
                rec["backward_error"] = be[idx].copy()
                return FeastResult(theta[idx].copy(), Xall[:, idx].copy(), M, be[idx].copy(), 0 if done else int(no_conv), epsout,
                                   loop, stats)
            dX = dXc[engine.torch.as_tensor(sel, device=dXc.device)].contiguous()
            sigma = np.where(np.isfinite(theta[sel]), theta[sel], center)
            m = keep
            loop += 1


def feast_hip_polynomial_projected(engine, coeffs, Emid, r, M0, fpm, *, Q0=None, seed=20260515, contour=None, eps_floor=0.0,
                                   union_csr=None, ortho="mgs", krylov=None, prepared=False):
    """P(lambda) x = 0 inside a circle on an N-row subspace of M0 columns: polynomial FEAST with a residual-inverse contour
    step (Gavin, Miedlar, Polizzi).  Per loop (_projected_loop): the contour step on the N x m block (loop 0 the plain sweep,
    which factors P(z_e) once per node and fills the cache; afterwards R_j = P(sigma_j) x_j, Y_e = P(z_e)^-1 R, Q_j = sum_e w_e
    (x_j - Y_e,j) / (z_e - sigma_j) on the cached factors), unit columns and the rank-revealing orthonormalisation of ``ortho``,
    the projected polynomial Q^H A_k Q, its dr x dr companion pencil solved on the host, the backward error of ALL dr candidates,
    poly_select.  Stop test: the largest backward error among the kept pairs inside the circle.  At the loop limit the last
    iterates are returned with info = Feast_ERROR_NO_CONVERGENCE.  ``union_csr`` and the exceptions: as feast_hip_polynomial.
    ``krylov`` = (solver, tol, maxiter, restart) with ``union_csr``: the solves of the contour step run on that Krylov solver
    (_poly_setup) and are inexact.  A node whose column stopped at maxiter (status 5) is the normal outcome of such a sweep and
    the loop goes on with its iterate; ``stats["polynomial"]["krylov"]`` gets one entry per loop, {iterations (worst column),
    node_iterations, capped_nodes}, ``stats["krylov_iterations"]`` the engine's count, and nothing is factored.
    ``prepared``: as in _poly_setup."""
    d = len(coeffs) - 1
    N = coeffs[0].shape[0]
    feastdefault(fpm)
    info = _check_circle_input(N, M0, r)
    if info:
        return _empty_result(N, info, complex_lambda=True)
    if krylov is not None and union_csr is None:
        raise ValueError("a Krylov solver on P(z) needs sparse coefficients (union_csr)")
    plan = _poly_setup(engine, coeffs, Emid, r, fpm, contour, union_csr, krylov, prepared=prepared)
    poly = {"degree": d, "method": "projected", "columns": M0}
    stats = {"krylov_iterations": 0, "factorizations": 0, "solve_seconds": 0.0, "polynomial": poly}
    if plan is not None:
        poly.update(plan)

    def reduced(Ahat, rank_q):
        try:
            theta, V = sla.eig(*_poly_companion(Ahat))
        except Exception as err:
            raise ReducedSolveError(str(err)) from err
        return theta, V[:rank_q, :]

    return _projected_loop(engine, N, M0, Emid, r, fpm, Q0, seed, eps_floor, ortho, stats, poly, engine.poly_resinv_apply, reduced,
                           engine.poly_ritz_eval, krylov=krylov is not None)


# Host rules of feast_hip_nonlinear's reduced solve.  Beyn: singular values of the block Hankel matrix H0 below BEYN_RANK_TOL
# times the largest are cut; a largest one below BEYN_NOISE max_j ||That(z_j)^-1||_F means an empty circle (the moments are then
# the rounding left over by a sum that cancels) and nothing is returned.  Newton polish of a candidate: at most NEWTON_STEPS steps, derivative by a central difference of
# the f_k with step NEWTON_FD max(1, |theta|), stop at a reduced backward error NEWTON_DONE; a polished pair that moved further
# than NEWTON_REACH radius is rejected.
BEYN_RANK_TOL = 1e-10
BEYN_NOISE = 1e-10
NEWTON_STEPS = 6
NEWTON_FD = 1e-6
NEWTON_DONE = 1e-14
NEWTON_REACH = 0.1


def nep_functions(funcs):
    """The scalar functions of a split form as callables: a non-negative int p stands for lambda^p."""
    out = []
    for f in funcs:
        if callable(f):
            out.append(f)
        elif isinstance(f, (int, np.integer)) and not isinstance(f, bool) and f >= 0:
            out.append(lambda z, p=int(f): np.asarray(z, dtype=np.complex128) ** p)
        else:
            raise ValueError("each f_k must be a callable or a non-negative int p (for lambda^p)")
    return out


def nep_table(funcs, z):
    """F[i, k] = f_k(z_i), complex128, for a 1-D array z: the only place the f_k are evaluated (never differentiated)."""
    z = np.atleast_1d(np.asarray(z, dtype=np.complex128))
    F = np.empty((len(z), len(funcs)), dtype=np.complex128)
    with np.errstate(all="ignore"):
        for k, f in enumerate(funcs):
            v = np.asarray(f(z), dtype=np.complex128)
            if v.shape not in ((), z.shape):
                raise ValueError(f"f_{k} must map an array to an array of the same shape")
            F[:, k] = v
    return F


def poly_derivative_table(degree, z):
    """D[i, k] = k z_i^(k-1), k = 0 .. degree: P'(z_i) = sum_k D[i, k] A_k for a polynomial, exact.  Column 0 is zero."""
    z = np.atleast_1d(np.asarray(z, dtype=np.complex128))
    D = np.zeros((len(z), int(degree) + 1), dtype=np.complex128)
    for k in range(1, int(degree) + 1):
        D[:, k] = k * z ** (k - 1)
    return D


def nep_derivative_table(funcs, z):
    """D[i, k] ~ f_k'(z_i) for a 1-D array z, as the central difference (f_k(z + h) - f_k(z - h)) / 2h with h = NEWTON_FD
    max(1, |z|) -- the quantity nep_newton_polish forms for the small problem, here for T'(z_i) = sum_k D[i, k] A_k of the count
    estimate.  The f_k are still only evaluated.  Error: h^2 |f'''| / 6 of truncation plus eps |f| / h of rounding, 1e-10-class
    for functions of unit scale (on the delay cases the trace built on it agrees with one built on a Cauchy-integral derivative
    to the four digits printed).  A constant f_k gives an exactly zero column.  A value f_k(z_i +- h) that is not finite raises
    ValueError, as a node value that is not finite does."""
    z = np.atleast_1d(np.asarray(z, dtype=np.complex128))
    h = NEWTON_FD * np.maximum(1.0, np.abs(z))
    Fp, Fm = nep_table(funcs, z + h), nep_table(funcs, z - h)
    bad = ~(np.isfinite(Fp) & np.isfinite(Fm))
    if bad.any():
        k = int(np.flatnonzero(bad.any(axis=0))[0])
        raise ValueError(f"f_{k} is not finite next to a contour node (the central difference of the count estimate needs it there)")
    return (Fp - Fm) / (2.0 * h[:, None])


def _nep_at(Ahat, frow):
    return sum(f * A for f, A in zip(frow, Ahat))


def nep_beyn(Ahat, funcs, center, radius, moments, reduced_nodes):
    """Beyn's integral method for the small problem sum_k f_k(lambda) Ahat[k] on the circle, in the scaled variable
    u = (z - center) / radius: the block moments M_p = (1 / n) sum_j u_j^{p+1} That(z_j)^-1, p < 2 moments, by the trapezoid rule
    on reduced_nodes points with the full identity as probe, the block Hankel pair (H0, H1), the SVD of H0 cut at BEYN_RANK_TOL,
    the eigenvalues of U0^H H1 V0 S0^-1 mapped back -> (theta[ncand], Y[r, ncand]), Y the first r rows of U0 S.  Two or more
    moments let it return eigenvalues that share an eigenvector (one moment cannot: its rank is that of the vectors).  An
    empty circle (BEYN_NOISE) returns no candidates."""
    r = Ahat[0].shape[0]
    K, n = int(moments), int(reduced_nodes)
    u = np.exp(2j * np.pi * (np.arange(n) + 0.5) / n)
    F = nep_table(funcs, center + radius * u)
    Mp = np.zeros((2 * K, r, r), dtype=np.complex128)
    scale = 0.0
    try:          # (no f_k is called from here on: what LAPACK refuses is a ReducedSolveError)
        for j in range(n):
            Tinv = sla.inv(_nep_at(Ahat, F[j]), check_finite=False)
            scale = max(scale, float(np.linalg.norm(Tinv)))
            for p in range(2 * K):
                Mp[p] += (u[j] ** (p + 1) / n) * Tinv
        H0 = np.block([[Mp[i + j] for j in range(K)] for i in range(K)])
        H1 = np.block([[Mp[i + j + 1] for j in range(K)] for i in range(K)])
        U, s, Vh = sla.svd(H0)
        k = int(np.sum(s > BEYN_RANK_TOL * s[0])) if s[0] > BEYN_NOISE * scale else 0
        if k == 0:
            return np.zeros(0, dtype=np.complex128), np.zeros((r, 0), dtype=np.complex128)
        U0, V0 = U[:, :k], Vh[:k].conj().T
        mu, S = sla.eig((U0.conj().T @ H1 @ V0) / s[None, :k])
    except (np.linalg.LinAlgError, ValueError) as err:
        raise ReducedSolveError(str(err)) from err
    return center + radius * mu, (U0 @ S)[:r]


def _nep_reduced_error(Ahat, fro, funcs, theta, v):
    f = nep_table(funcs, theta)[0]
    if not np.isfinite(f).all():
        return math.inf, math.inf
    res = float(np.linalg.norm(_nep_at(Ahat, f) @ v))
    den = float(np.abs(f) @ fro)
    return res, (res / den if den > 0 else math.inf)


def nep_newton_polish(Ahat, funcs, theta0, v0, radius):
    """Guarded Newton polish of one pair of the small problem: steps on the bordered system [That(theta), That'(theta) v; v^H, 0]
    with That' from central differences of the f_k (the residual is exact, so the root is).  The polished pair is returned only
    if it stayed finite and within NEWTON_REACH radius of its start AND (reached a reduced backward error NEWTON_DONE or ended
    with a smaller reduced residual than it began with); otherwise the start pair, with unit v.  (An unguarded fixed number of
    steps carries junk candidates to points of small but not converged residual inside the circle, where the loop stagnates.)"""
    fro = np.array([np.linalg.norm(A) for A in Ahat])
    r = len(v0)
    nv = np.linalg.norm(v0)
    if not (np.isfinite(theta0) and nv > 0 and np.isfinite(nv)):
        return theta0, v0
    v0 = v0 / nv
    res0, be0 = _nep_reduced_error(Ahat, fro, funcs, theta0, v0)
    theta, v, res, be = theta0, v0, res0, be0
    for _ in range(NEWTON_STEPS):
        if not be > NEWTON_DONE:
            break
        h = NEWTON_FD * max(1.0, abs(theta))
        F = nep_table(funcs, [theta, theta + h, theta - h])
        if not np.isfinite(F).all():
            return theta0, v0
        Jb = np.zeros((r + 1, r + 1), dtype=np.complex128)
        Jb[:r, :r] = _nep_at(Ahat, F[0])
        Jb[:r, r] = _nep_at(Ahat, (F[1] - F[2]) / (2.0 * h)) @ v
        Jb[r, :r] = v.conj()
        rhs = np.zeros(r + 1, dtype=np.complex128)
        rhs[r] = 1.0
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                sol = sla.solve(Jb, rhs, check_finite=False)
        except (np.linalg.LinAlgError, ValueError):          # a singular or non-finite bordered matrix: keep what there is
            break
        nrm = np.linalg.norm(sol[:r])
        if not (np.isfinite(sol).all() and nrm > 0):
            return theta0, v0
        theta, v = theta + sol[r], sol[:r] / nrm
        res, be = _nep_reduced_error(Ahat, fro, funcs, theta, v)
    ok = np.isfinite(theta) and np.isfinite(res) and abs(theta - theta0) <= NEWTON_REACH * radius and (be <= NEWTON_DONE or res < res0)
    return (theta, v) if ok else (theta0, v0)


def feast_hip_nonlinear(engine, mats, funcs, Emid, r, M0, fpm, *, Q0=None, seed=20260515, contour=None, eps_floor=0.0,
                        union_csr=None, ortho="mgs", moments=2, reduced_nodes=128, prepared=False, krylov=None, companion=False):
    """T(lambda) x = 0, T(lambda) = sum_k f_k(lambda) mats[k], inside a circle: feast_hip_polynomial_projected's loop
    (_projected_loop) on a term handle (engine.set_terms), with two changes.  The scalars are host tables of the f_k -- at the
    contour nodes once, at the shifts and the candidates once per loop -- so the device never sees the functions.  The reduced
    r x r problem sum_k f_k(lambda) Q^H A_k Q is solved on the host by nep_beyn and each candidate polished by
    nep_newton_polish; the candidates then go through the polynomial method's ranking by device backward error (poly_select,
    POLY_SET_ASIDE).  Loop 0 is the plain sweep, which factors T(z_e) once per node; later loops are residual-inverse sweeps on
    the cached factors.  Stop test, loop limit and ``union_csr``: as feast_hip_polynomial_projected.  A circle in which the
    reduced problem finds nothing returns Feast_ERROR_NO_CONVERGENCE with M = 0.  What an f_k raises is the caller's to see.
    ``prepared``: as in _poly_setup (the node values are set again, which changes nothing when they are the same).
    ``krylov`` = (solver, tol, maxiter, restart): the solves of the contour step run on that Krylov solver and are inexact, as in
    feast_hip_polynomial_projected (``stats["nonlinear"]["krylov"]`` per loop, a capped node is no failure, nothing is factored).
    That is the path of a term-operator handle (engine.set_term_operator) on a ``prepared`` engine, where ``mats`` are shape-only
    stand-ins.  ``companion``: the f_k are the powers lambda^k, and the reduced problem is the polynomial method's companion
    pencil (_poly_companion) instead of Beyn's method and the polish."""
    N = mats[0].shape[0]
    feastdefault(fpm)
    info = _check_circle_input(N, M0, r)
    if info:
        return _empty_result(N, info, complex_lambda=True)
    center = complex(Emid)
    Zne, Wne = feast_gcontour(Emid, r, fpm) if contour is None else contour
    F_node = nep_table(funcs, Zne)
    if not np.isfinite(F_node).all():
        k = int(np.flatnonzero(~np.isfinite(F_node).all(axis=0))[0])
        raise ValueError(f"f_{k} is not finite at a contour node")
    plan = _poly_setup(engine, mats, Emid, r, fpm, (Zne, Wne), union_csr, krylov, terms=True, prepared=prepared)
    engine.nep_set_node_values(F_node)
    nep = {"terms": len(mats), "columns": M0, "moments": int(moments), "reduced_nodes": int(reduced_nodes), "reduced_seconds": 0.0}
    stats = {"krylov_iterations": 0, "factorizations": 0, "solve_seconds": 0.0, "nonlinear": nep}
    if plan is not None:
        nep.update(plan)

    def sweep(dX, m, sigma):
        return engine.nep_resinv_apply(dX, m, sigma, None if sigma is None else nep_table(funcs, sigma))

    def reduced(Ahat, rank_q):
        t0 = time.perf_counter()
        if companion:
            try:
                theta, V = sla.eig(*_poly_companion(Ahat))
            except Exception as err:
                raise ReducedSolveError(str(err)) from err
            nep["reduced_seconds"] += time.perf_counter() - t0
            return theta, V[:rank_q, :]
        theta, Y = nep_beyn(Ahat, funcs, center, r, moments, reduced_nodes)
        theta, Y = theta.copy(), np.array(Y, dtype=np.complex128)
        for i in range(len(theta)):
            theta[i], Y[:, i] = nep_newton_polish(Ahat, funcs, theta[i], Y[:, i], r)
        nep["reduced_seconds"] += time.perf_counter() - t0
        return theta, Y

    def evaluate(dQ, rank_q, Y, theta):
        return engine.nep_ritz_eval(dQ, rank_q, Y, nep_table(funcs, theta))

    return _projected_loop(engine, N, M0, Emid, r, fpm, Q0, seed, eps_floor, ortho, stats, nep, sweep, reduced, evaluate,
                           krylov=krylov is not None)


def feast_hip_poly_estimate(engine, mats, funcs, Emid, r, m, fpm, *, seed=ESTIMATE_SEED, contour=None, union_csr=None, krylov=None):
    """Stochastic estimate of the number of eigenvalues of P(lambda) = sum_k lambda^k mats[k] (``funcs`` None) or T(lambda) =
    sum_k f_k(lambda) mats[k] inside the contour: fpm[14] = 2 of feast_polynomial / feast_nonlinear.  For a regular T the count
    is (1 / 2 pi i) oint tr(T(z)^-1 T'(z)) dz; with the contour's nodes and weights it is sum_e w_e tr(T'(z_e) T(z_e)^-1), and
    Hutchinson's samples of that trace over m Rademacher columns come from one set of solves T(z_e)^-1 V
    (engine.poly_estimate_count).  T'(z_e) = sum_k g_k(z_e) A_k goes to the device as the table G[e, k] = w_e g_k(z_e):
    poly_derivative_table (exact) or nep_derivative_table (central differences of the f_k).
    The estimate is a sum of filter values counted with algebraic multiplicity, not an integer; for a non-normal problem its
    variance grows with the departure of the eigenvector basis from orthogonality.  ``union_csr`` / ``krylov``: as _poly_setup.
    The engine keeps the problem, the contour and (direct solvers) the cached factors, so a solve that follows with
    ``prepared=True`` factors nothing.

    Returns (info, estimate, plan, factorizations): info 0 with the dict {mean, stderr, samples, nodes, solver, seed, seconds,
    dropped_terms} -- stderr = std(t) / sqrt(m) of the complex samples, as feast_hip_estimate(general=True) reports it: it counts
    the spread of the imaginary parts too, so it overstates the standard error of Re mean, which is what M is rounded from -- or the status 5 / 8 of a failed node as info and None; plan: what _poly_setup returned."""
    t0 = time.perf_counter()
    feastdefault(fpm)
    Zne, Wne = feast_gcontour(Emid, r, fpm) if contour is None else contour
    Zne, Wne = np.asarray(Zne, dtype=np.complex128), np.asarray(Wne, dtype=np.complex128)
    F_node = None
    if funcs is None:
        D = poly_derivative_table(len(mats) - 1, Zne)
    else:
        F_node = nep_table(funcs, Zne)
        if not np.isfinite(F_node).all():
            k = int(np.flatnonzero(~np.isfinite(F_node).all(axis=0))[0])
            raise ValueError(f"f_{k} is not finite at a contour node")
        D = nep_derivative_table(funcs, Zne)
    G = Wne[:, None] * D
    plan = _poly_setup(engine, mats, Emid, r, fpm, (Zne, Wne), union_csr, krylov, terms=funcs is not None)
    if F_node is not None:
        engine.nep_set_node_values(F_node)
    samples, status, st = engine.poly_estimate_count(int(m), seed, G)
    nfact = int(st.get("factorizations", 0))
    fail = int(np.max(status))
    if fail:
        return (int(FeastError.Feast_ERROR_LAPACK) if fail == 8 else int(FeastError.Feast_ERROR_NO_CONVERGENCE)), None, plan, nfact
    solver = krylov[0] if krylov is not None else ("direct" if union_csr is None else "sparse_direct")
    est = {"mean": complex(np.mean(samples)), "stderr": float(np.std(samples, ddof=1) / math.sqrt(m)) if m > 1 else math.inf,
           "samples": samples.copy(), "nodes": len(Zne), "solver": solver, "seed": int(seed), "seconds": time.perf_counter() - t0,
           "dropped_terms": [int(k) for k in np.flatnonzero(~G.any(axis=0))]}
    if krylov is not None:
        est["solver_tol"] = float(krylov[1])
    return 0, est, plan, nfact


TWO_SIDED_SOLVERS = ("direct", "lu")
TWO_SIDED_SPARSE_SOLVERS = ("direct", "lu", "sparse_direct", "banded")


def check_two_sided(sparse, solver, inner_precision=64, group=None, direct_nodes=None):
    """Host-only validation of ``feast_general(..., two_sided=True)`` (no device work): the adjoint sweep exists for the
    direct solvers in fp64 on one rank -- the dense LU, and for sparse input the sparse direct solver (its multifrontal
    plan; there is no Krylov solver on the conjugate transpose)."""
    if sparse and solver not in TWO_SIDED_SPARSE_SOLVERS:
        raise ValueError(f"two_sided on sparse input needs a direct solver (solver='direct' or 'sparse_direct'), not '{solver}'")
    if not sparse and solver not in TWO_SIDED_SOLVERS:
        raise ValueError(f"two_sided needs the dense direct solver (solver='direct'), not '{solver}'")
    if inner_precision == 32:
        raise ValueError("two_sided does not support inner_precision=32 (the adjoint substitution runs on complex128 factors)")
    if group is not None:
        raise ValueError("two_sided does not support group= (single-rank sweeps only)")
    if direct_nodes is not None:
        raise ValueError("two_sided does not support direct_nodes= (every node is solved directly already)")


def feast_hip_general_two_sided(engine, A, B, Emid, r, M0, fpm, *, solver="direct", Q0=None, QL0=None, seed=20260515,
                                contour=None, eps_floor=0.0):
    """Two-sided FEAST on a dense pencil, or on a sparse one under the sparse direct solver (``solver="banded"``: the
    multifrontal plan, or the blocked band LU where that plan is missing or rejects a pivot, declared with
    engine.require_adjoint): right and left subspaces from the same cached LU factors, oblique projection.
    ``stats["two_sided"]["direct_plan"]`` names the factors that ran, ``fell_back`` whether they are not the ones planned.

        P_R = sum_e w_e S_e^-1 B Q_R                (forward sweep; factors cached per node)
        P_L = sum_e conj(w_e) S_e^-H B^H Q_L        (adjoint sweep: conjugate-transposed substitution, no factorisation)
        Aq = P_L^H A P_R,  Bq = P_L^H B P_R;   lam, V_L, V_R = eig(Aq, Bq)
        X_R = P_R V_R,  X_L = P_L V_L  (unit columns);  epsout = max_{j < M} max(res_R, res_L), both residuals with B

    The reference validates fpm[15] (one- or two-sided contour, src/core/feast_parameters.jl:217-225) and never reads it, so
    this driver mirrors nothing: it reports Feast_ERROR_NO_CONVERGENCE when the loop limit ends the run (the last iterates
    are still returned).  ``q`` holds unit-norm right vectors, ``q_left`` left vectors scaled to y_j^H B x_j = 1; ``res`` is
    the larger of the two residuals of each pair."""
    N = A.shape[0]
    feastdefault(fpm)
    info = _check_circle_input(N, M0, r)
    if info:
        return _empty_result(N, info, complex_lambda=True)
    import scipy.sparse as _sp
    sparse = _sp.issparse(A)
    check_two_sided(sparse, solver)
    if sparse and solver != "banded":
        raise ValueError("two_sided on sparse input runs on the sparse direct solver (solver='banded')")
    Ac, Bc = _complex_pencil(A, B)
    Zne, Wne = feast_gcontour(Emid, r, fpm) if contour is None else contour
    engine.set_adjoint(False)
    engine.require_adjoint(sparse)              # before the problem's direct plan is made or queried
    try:
        world, count = _setup_sweep(engine, None, Ac, Bc, Zne, Wne, 1.0, False)
        _configure_solver(engine, solver, fpm, 0.0, 500, 30, factor_precision=64)
    except BaseException:
        engine.require_adjoint(False)
        raise
    dQR = engine.upload(seeded_subspace(N, M0, seed) if Q0 is None else np.asarray(Q0, dtype=np.complex128))
    dQL = engine.upload(seeded_subspace(N, M0, seed + 1, complex_values=True) if QL0 is None
                        else np.asarray(QL0, dtype=np.complex128))
    eps_tol = max(feast_tolerance(fpm), float(eps_floor))
    maxloop = int(fpm[4])
    loop = 0
    stats = {"krylov_iterations": 0, "factorizations": 0, "solve_seconds": 0.0}
    ts = {"res_right": [], "res_left": [], "adjoint_factorizations": 0,
          "seconds": {"forward_sweep": 0.0, "adjoint_sweep": 0.0, "rayleigh_ritz": 0.0}}
    stats["two_sided"] = ts
    tick = time.perf_counter
    def plan_name():
        if not sparse:
            return "dense LU"
        return ("multifrontal LU on a nested-dissection tree" if engine.band_plan()[3] == HipEngine.PLAN_MULTIFRONTAL
                else "band LU after reverse Cuthill-McKee")

    try:
        # the plan as made; a multifrontal LU that rejects a pivot hands the matrix to the band LU inside the first sweep, so
        # the name is read again after every pair of sweeps: it names the factors that ran
        planned = ts["direct_plan"] = plan_name()
        ts["fell_back"] = False
        with small_lapack():
            while True:
                t0 = tick()
                fail, (dPR, _, _) = _sweep(engine, dQR, M0, world, count, stats)
                t1 = tick()
                if not fail:
                    engine.set_adjoint(True)
                    fail, (dPL, _, st) = _sweep(engine, dQL, M0, world, count, stats)
                    engine.set_adjoint(False)
                    ts["adjoint_factorizations"] += int(st.get("factorizations", 0))
                t2 = tick()
                ts["seconds"]["forward_sweep"] += t1 - t0
                ts["seconds"]["adjoint_sweep"] += t2 - t1
                if sparse:
                    ts["direct_plan"] = plan_name()
                    ts["fell_back"] = ts["fell_back"] or ts["direct_plan"] != planned
                if fail:
                    return _empty_result(N, FeastError.Feast_ERROR_LAPACK if fail == 8 else FeastError.Feast_ERROR_NO_CONVERGENCE,
                                         loop, complex_lambda=True, stats=stats)
                Aq, Bq = engine.project_pair(dPL, dPR, M0)
                try:
                    lam_red, vl_red, vr_red = sla.eig(Aq, Bq, left=True, right=True)
                except Exception:
                    return _empty_result(N, FeastError.Feast_ERROR_LAPACK, loop, complex_lambda=True, stats=stats)
                perm, M = _reorder_by_contour(lam_red, Emid, r, fpm, M0)
                if M == 0:
                    return _empty_result(N, FeastError.Feast_ERROR_NO_CONVERGENCE, loop, complex_lambda=True, stats=stats)
                lam = lam_red[perm]
                # (Ritz values of the directions the filter has removed come back infinite or undefined from the singular
                #  reduced pencil; they lie outside the contour and only their vectors are carried along)
                lam_safe = np.where(np.isfinite(lam), lam, 0.0)
                dXR, res_r = engine.ritz_residual(dPR, M0, np.asfortranarray(vr_red[:, perm]), lam_safe, M0, normalize=True, use_B=True)
                engine.set_adjoint(True)
                dXL, res_l = engine.ritz_residual(dPL, M0, np.asfortranarray(vl_red[:, perm]), lam_safe, M0, normalize=True, use_B=True)
                engine.set_adjoint(False)
                res_r, res_l = res_r[:M], res_l[:M]
                ts["res_right"].append(float(res_r.max()))
                ts["res_left"].append(float(res_l.max()))
                epsout = float(max(res_r.max(), res_l.max()))
                ts["seconds"]["rayleigh_ritz"] += tick() - t2
                if epsout <= eps_tol or loop >= maxloop:
                    break
                loop += 1
                dQR, dQL = dXR, dXL
    finally:
        engine.set_adjoint(False)
        engine.require_adjoint(False)
    order = sorted(range(M), key=lambda i: abs(lam[i]) ** 2)             # feast_sort_general!
    X = engine.download(dXR, M0)[:, :M][:, order]
    Y = engine.download(dXL, M0)[:, :M][:, order]
    G = Y.conj().T @ (X if Bc is None else Bc @ X)                          # Y^H B X, M x M, once per solve
    d = np.diag(G).copy()
    ts["overlap"] = np.abs(d)
    with np.errstate(divide="ignore", invalid="ignore"):
        Y = Y / np.conj(d)[None, :]                                         # y_j^H B x_j = 1
        Gs = G / d[:, None]
    ts["biorthogonality"] = float(np.abs(Gs - np.diag(np.diag(Gs))).max()) if M > 1 else 0.0
    info = 0 if epsout <= eps_tol else int(FeastError.Feast_ERROR_NO_CONVERGENCE)
    return FeastResult(lam[:M][order].copy(), X.copy(), M, np.maximum(res_r, res_l)[order].copy(), info, epsout, loop, stats,
                       q_left=Y.copy())


def feast_hip_complex_symmetric(engine, A, B, Emid, r, M0, fpm, *, solver="direct", solver_tol=0.0,
                                solver_maxiter=500, solver_restart=30, group=None, Q0=None, seed=20260515, direct_nodes=None,
                                ortho="mgs"):
    """Complex-symmetric sibling of variant A (A == A^T, B == B^T, complex): the loop of
    _feast_dense_complex_symmetric / its sparse twin (src/dense/feast_dense.jl:1026-1259,
    src/sparse/feast_sparse.jl:509-711).  Same kernels as the Hermitian path with the full
    contour (weights unscaled), pivoted-QR compression, the BILINEAR projection q^T A q, q^T B q
    (feasthip_project bilinear=1), general reduced eigenproblem on the host, inside-first
    reorder by the contour, all rank columns normalised, residual with B, sort by |lambda|^2.
    Sparse input may use solver="cocg": z B - A is complex symmetric for complex-symmetric A, B
    -- the COCG kernels need real A, B, so complex input goes through "bicgstab"/"gmres"."""
    import scipy.sparse as _sp
    N = A.shape[0]
    feastdefault(fpm)
    info = _check_circle_input(N, M0, r)
    if info:
        return _empty_result(N, info, complex_lambda=True)
    for name, Mx in (("A", A), ("B", B)):
        if Mx is None:
            continue
        sym = (abs(Mx - Mx.T).max() == 0) if _sp.issparse(Mx) else np.array_equal(Mx, Mx.T)
        if not sym:                                          # check_complex_symmetric, feast_dense.jl:1038
            raise ValueError(f"Matrix {name} must be complex symmetric ({name} == transpose({name}))")
    Ac, Bc = _complex_pencil(A, B)
    Zne, Wne = feast_gcontour(Emid, r, fpm)
    world, count = _setup_sweep(engine, group, Ac, Bc, Zne, Wne, 1.0, False)
    _configure_solver(engine, solver, fpm, solver_tol, solver_maxiter, solver_restart)
    dQ = engine.upload(seeded_subspace(N, M0, seed, complex_values=True) if Q0 is None else np.asarray(Q0, dtype=np.complex128))
    done = _LoopRecord(M0, feast_tolerance(fpm), int(fpm[4]), dtype=np.complex128)
    info, active, loop_count, dX, eps_hist = 0, M0, 0, None, []
    stats = {"krylov_iterations": 0, "factorizations": 0, "solve_seconds": 0.0}
    with _ortho_scope(engine, ortho, stats), \
            _direct_nodes_scope(engine, direct_nodes, len(Zne), _sp.issparse(A), solver, M0, world, stats) as dn:
        for loop_idx in range(0, done.maxloop + 1):
            loop_count = loop_idx
            fail, (dP, status, st) = _sweep(engine, dQ, active, world, count, stats)
            if dn is not None:
                dn.record(loop_idx, st)
            if fail:
                info = int(FeastError.Feast_ERROR_LAPACK if fail == 8 else FeastError.Feast_ERROR_NO_CONVERGENCE)
                break
            rank_q = engine.orthonormalize(dP, active, SQRT_EPS)                  # _feast_qr_compress!, :1163
            _note_ortho(engine, stats)
            if rank_q == 0:
                info = int(FeastError.Feast_ERROR_NO_CONVERGENCE)
                break
            Ared, Bred = engine.project(dP, rank_q, bilinear=True, hermitize=False)   # q^T A q, q^T B q
            try:
                with small_lapack():
                    lam_red, v_red = sla.eig(Ared, Bred)
            except Exception:
                info = int(FeastError.Feast_ERROR_LAPACK)
                break
            perm, M = _reorder_by_contour(lam_red, Emid, r, fpm, rank_q)
            if M == 0:
                info = int(FeastError.Feast_ERROR_NO_CONVERGENCE)
                break
            lam_sorted = lam_red[perm]
            V = np.asfortranarray(v_red[:, perm])
            dX, res = engine.ritz_residual(dP, rank_q, V, lam_sorted, rank_q, normalize=True, use_B=True)
            stop = done.record(loop_idx, rank_q, lam_sorted, M, res)
            if stop is not None:
                info = stop
                break
            if dn is not None:
                eps_hist.append(done.epsout)
                dn.choose(loop_idx, eps_hist, done.eps_tol, done.maxloop)
            active = rank_q
            dQ = dX
    M_found = done.M_found
    X = engine.download(dX, M_found) if M_found > 0 else np.zeros((N, 0), complex)
    order = sorted(range(M_found), key=lambda i: abs(done.lam_vec[i]) ** 2)         # feast_sort_general!
    return done.result(X, info, loop_count, stats, order)


def pfeast_hip_moments(engine, A, B, Emin, Emax, M0, fpm, *, group=None, Q0=None, seed=20260515):
    """Variant B ("moments") on the :hip engine -- the loop of the reference's parallel drivers
    pfeast_sygv!/pfeast_scsrgv! (src/parallel/feast_parallel.jl:58-207, 450-572) with the
    per-node worker pfeast_solve_sparse_single_point (:717-751) replaced by one
    feasthip_contour_apply call that also returns the moment matrices
        Aq = Re sum_e 2 w_e Q^T Y_e,   Sq = Re sum_e 2 w_e z_e Q^T Y_e,   Q_proj = Re sum_e 2 w_e Y_e.
    Real-symmetric A, B only (as in the reference).  No orthonormalisation: the reduced pencil
    (Sq, Aq) is solved as is and X = Q_proj V; all M0 columns are carried to the next loop.
    The reference itself routes high-level dense calls away from this variant because it "does
    not currently match serial results" (src/core/feast_backend_utils.jl:115); it is mirrored for
    the seam, variant A (feast_hip_hermitian) is the robust path.
    """
    import scipy.sparse as _sp
    N = A.shape[0]
    feastdefault(fpm)
    info = check_feast_srci_input(N, M0, Emin, Emax)
    if info:
        return _empty_result(N, info, real_q=True)
    Bm = B if B is not None else (_sp.identity(N, format="csr") if _sp.issparse(A) else np.eye(N))
    Zne, Wne = feast_contour(Emin, Emax, fpm)
    _setup_sweep(engine, group, A, Bm, Zne, Wne, 2.0, True)      # real.(...) of feast_parallel.jl:38-55
    engine.set_solver("direct" if not _sp.issparse(A) else "bicgstab", rtol=1e-13, atol=0.0, maxit=5000)
    work = np.real(seeded_subspace(N, M0, seed)) if Q0 is None else np.real(np.asarray(Q0))
    eps_tol = feast_tolerance(fpm)
    max_loops = int(fpm[4])
    lam = np.zeros(M0)
    res = np.zeros(M0)
    q = np.zeros((N, M0))
    for loop in range(1, max_loops + 1):
        dQ = engine.upload(work.astype(np.complex128))
        # Q_proj and both moment matrices come back summed over the ranks (feast_mpi.jl:117-119)
        dP, status, st, Aq, Sq = engine.contour_apply(dQ, M0, None, want_moments=True)
        Aq, Sq = np.real(Aq), np.real(Sq)
        Q_proj = np.real(engine.download(dP, M0))
        try:
            Su = np.triu(Sq) + np.triu(Sq, 1).T               # Symmetric(X) reads the upper triangle
            Au = np.triu(Aq) + np.triu(Aq, 1).T
            with small_lapack():
                lam_red, v_red = sla.eigh(Su, Au)
        except Exception:
            with small_lapack():
                w_, v_red = sla.eig(Sq, Aq)
            lam_red, v_red = np.real(w_), np.real(v_red)
        q = Q_proj @ v_red
        perm, M = _reorder_by_interval(lam_red, Emin, Emax, M0)
        lam = np.asarray(lam_red)[perm]
        q = q[:, perm]
        if M == 0:
            return _empty_result(N, FeastError.Feast_ERROR_NO_CONVERGENCE, loop, real_q=True, epsout=0.0)
        for j in range(M):
            nrm = np.linalg.norm(q[:, j])
            if nrm > 0:
                q[:, j] /= nrm
        for j in range(M):                                    # feast_residual!, src/core/feast_tools.jl:726-755
            r_ = A @ q[:, j] - lam[j] * (Bm @ q[:, j])
            res[j] = np.linalg.norm(r_) / max(abs(lam[j]), 1.0)
        epsout = float(res[:M].max())
        if epsout <= eps_tol:
            order = np.argsort(lam[:M], kind="stable")        # feast_sort!
            return FeastResult(lam[:M][order].copy(), q[:, :M][:, order].copy(), M, res[:M][order].copy(), 0, epsout, loop)
        work = q[:, :M0].copy()
    M = int(sum(1 for i in range(M0) if Emin <= lam[i] <= Emax))
    return FeastResult(lam[:M].copy(), q[:, :M].copy(), M, res[:M].copy(), int(FeastError.Feast_ERROR_NO_CONVERGENCE),
                       float(res[:M].max()) if M else 0.0, max_loops)


def feast_hip_symmetric_kernel(engine, A, B, Emin, Emax, M0, fpm, *, solver="direct", solver_tol=0.0, solver_maxiter=500,
                               solver_restart=30, group=None, Q0=None, seed=20260515, contour=None):
    """What the real-symmetric RCI kernel ``feast_srci!`` (src/kernel/feast_kernel.jl:7-275) returns when its jobs are
    served -- the maths behind ``feast_sbgv!`` (src/banded/feast_banded.jl:87-175) -- as ONE device sweep per refinement
    loop instead of a FACTORIZE / SOLVE round trip per quadrature node: ``contour_apply(want_moments)`` yields
        Q_proj = Re sum_e 2 w_e Y_e,  Aq = Re sum_e 2 w_e Q^T Y_e,  Sq = Re sum_e 2 w_e z_e Q^T Y_e   (:146-169)
    summed over the ranks; then, as the kernel does: ``eigen(Sq, Aq)`` of the general reduced pencil (:175) with LAPACK's
    eigenvector scaling (the residuals below are taken on un-normalised Ritz vectors and depend on it), q = Q_proj Re(V)
    with no normalisation (:183-187), stable inside-first reorder (:189-215), residual ||A q - lambda q|| / max(|lambda|, 1)
    WITHOUT B (:244-252: generalized problems therefore run all fpm[4] loops and return info = 0), stop test with
    loop >= fpm[4] (:258), all M0 Ritz vectors carried to the next loop (:269), feast_sort! at the end."""
    N = A.shape[0]
    feastdefault(fpm)
    info = check_feast_srci_input(N, M0, Emin, Emax)
    if info:
        return _empty_result(N, info, real_q=True, epsout=0.0)
    Zne, Wne = feast_contour(Emin, Emax, fpm) if contour is None else contour
    # weight = 2 * Wne[e] (feast_kernel.jl:150); real(...) after the sweep (:166-169)
    world, count = _setup_sweep(engine, group, A, B, Zne, Wne, 2.0, True)
    _configure_solver(engine, solver, fpm, solver_tol, solver_maxiter, solver_restart)
    if Q0 is not None:                                    # fpm[5] = 1: the caller's columns, normalised (:68-80)
        work = np.array(np.real(Q0), dtype=np.float64)
        nrm = np.linalg.norm(work, axis=0)
        nrm[nrm == 0] = 1.0
        work = work / nrm
    else:
        work = np.real(seeded_subspace(N, M0, seed))
    eps_tol = feast_tolerance(fpm)
    maxloop = int(fpm[4])
    stats = {"krylov_iterations": 0, "factorizations": 0, "solve_seconds": 0.0}
    empty = lambda code, loop: _empty_result(N, code, loop, real_q=True, epsout=0.0, stats=stats)
    loop = 0
    with small_lapack():
        while True:
            dQ = engine.upload(work)
            fail, (dP, status, st, Aq, Sq) = _sweep(engine, dQ, M0, world, count, stats, want_moments=True)
            if fail:                                      # any failed SOLVE job, whatever its code: feast_banded.jl:137-147
                return empty(FeastError.Feast_ERROR_LAPACK, loop)
            try:
                w, V = sla.eig(np.real(Sq), np.real(Aq))
            except Exception:
                return empty(FeastError.Feast_ERROR_LAPACK, loop)
            V = np.array(V, copy=True)
            for j in range(V.shape[1]):                                     # LAPACK ggev scaling: max |re| + |im| = 1
                s_ = np.max(np.abs(V[:, j].real) + np.abs(V[:, j].imag))
                if s_ > 0:
                    V[:, j] /= s_
            lam = np.real(w)
            perm, M = _reorder_by_interval(lam, Emin, Emax, M0)
            if M == 0:
                return empty(FeastError.Feast_ERROR_NO_CONVERGENCE, loop)
            lam = lam[perm]
            Vp = np.asfortranarray(np.real(V)[:, perm].astype(np.complex128))
            # q = Q_proj Re(V) for all M0 columns, residuals of the first M without B and without normalisation
            dX, res = engine.ritz_residual(dP, M0, Vp, lam, M, normalize=False, use_B=False)
            epsout = float(res.max())
            if epsout <= eps_tol or loop >= maxloop:
                X = np.real(engine.download(dX[:M], M))
                order = np.argsort(lam[:M], kind="stable")                  # feast_sort!
                return FeastResult(lam[:M][order].copy(), X[:, order].copy(), M, res[order].copy(), 0, epsout, loop, stats)
            loop += 1
            work = np.real(engine.download(dX, M0))


def pfeast_hip_hermitian_moments(engine, A, B, Emin, Emax, M0, fpm, *, solver="direct", solver_tol=0.0, solver_maxiter=500,
                                 solver_restart=30, group=None, Q0=None, seed=20260515):
    """Variant B for COMPLEX HERMITIAN input on the :hip engine -- the loop of the reference's MPI driver
    _mpi_feast_complex_hermitian! (src/parallel/feast_mpi.jl:796-909) with the per-rank worker
    mpi_compute_complex_hermitian_moments (:523-571) replaced by one ``contour_apply(want_moments)`` call:
        zAq = sum_e 2 w_e Q^H Y_e,  zSq = sum_e 2 w_e z_e Q^H Y_e,  Q_proj = sum_e 2 w_e Y_e   (complex, no real part),
    already summed over the ranks inside the C ABI (the three MPI.Allreduce of :856-858 are ONE packed reduce).
    Then, as the reference does: Hermitian parts of the moments, eigen(Hermitian(Sq), Hermitian(Aq)) with the general
    fallback, X = Q_proj V, inside-first reorder, the first M columns normalised, residuals with B, and ALL M0
    columns carried to the next loop (no orthonormalisation, no compression).  Any M0 (wider than 64 columns: the
    moment matrices are assembled block column by block column on the device).
    Sparse input with ``solver="direct"``: there is no sparse LU on the device, the systems go through the device
    GMRES with a purely relative 1e-13 stop.  This un-normalised iteration amplifies solver error (about 50x in the
    first loop, 3x per further loop: measured on the reference's fixture), so with Krylov solves the outer tolerance
    fpm[3] should not be asked below ~1e-10; dense input (batched LU) reaches 1e-12 like the reference."""
    import scipy.sparse as _sp
    N = A.shape[0]
    feastdefault(fpm)
    info = check_feast_srci_input(N, M0, Emin, Emax)
    if info:
        return _empty_result(N, info)
    sparse = _sp.issparse(A)
    Ac = A.astype(np.complex128)
    Bc = B.astype(np.complex128) if B is not None else (_sp.identity(N, dtype=np.complex128, format="csr") if sparse else np.eye(N, dtype=np.complex128))
    Zne, Wne = feast_contour(Emin, Emax, fpm)
    world, count = _setup_sweep(engine, group, Ac, Bc, Zne, Wne, 2.0, False)   # weight = 2 * local_Wne[e], feast_mpi.jl:548
    if solver in ("direct", "lu") and sparse:
        # no sparse LU on the device: the reference's own iterative option, restarted GMRES
        # (solve_shifted_iterative!, feast_sparse.jl:164-203), device resident here, standing in for a DIRECT solve:
        # purely relative stop at 1e-13 per column.  (The reference's iterative option stops at atol + rtol*||b|| with
        # atol = rtol = tol; columns of this un-normalised iteration shrink to 1e-8 and an absolute 1e-12 then leaves them
        # at 1e-4 relative -- measured: the outer residual grows 3x per loop.)
        iterative = True
        tol_value = feast_tolerance(fpm) if solver_tol == 0.0 else float(solver_tol)
        engine.set_solver("gmres", rtol=min(tol_value, 1e-13), atol=0.0, maxit=max(solver_maxiter, 2000), restart=solver_restart)
    else:
        iterative, _ = _configure_solver(engine, solver, fpm, solver_tol, solver_maxiter, solver_restart)
    Q_basis = seeded_subspace(N, M0, seed, complex_values=True) if Q0 is None else np.asarray(Q0, dtype=np.complex128)
    dQ = engine.upload(Q_basis)
    done = _LoopRecord(M0, feast_tolerance(fpm), int(fpm[4]))
    info, loop_count, dX = 0, 0, None
    for loop_idx in range(0, done.maxloop + 1):
        loop_count = loop_idx
        fail, (dP, status, st, zAq, zSq) = _sweep(engine, dQ, M0, world, count, None, want_moments=True)
        if fail:                                          # _mpi_success_count(...) != size, feast_mpi.jl:849-852
            # any failed node: LAPACK for direct solves, NO_CONVERGENCE for Krylov solves, whatever its code
            info = int(FeastError.Feast_ERROR_LAPACK if not iterative else FeastError.Feast_ERROR_NO_CONVERGENCE)
            break
        Aq = 0.5 * (zAq + zAq.conj().T)                   # _feast_hermitian_part!
        Sq = 0.5 * (zSq + zSq.conj().T)
        try:
            lam_red, v_red = _reduced_hermitian_eig(Sq, Aq)
        except Exception:
            info = int(FeastError.Feast_ERROR_LAPACK)
            break
        perm, M = _reorder_by_interval(lam_red, Emin, Emax, M0)
        if M == 0:
            info = int(FeastError.Feast_ERROR_NO_CONVERGENCE)
            break
        lam_sorted = lam_red[perm]
        V_sorted = np.asfortranarray(np.asarray(v_red, dtype=np.complex128)[:, perm])
        # X = Q_proj V, the first M columns normalised, residual ||A x - lambda B x|| / max(|lambda|, 1) for them
        dX, res = engine.ritz_residual(dP, M0, V_sorted, lam_sorted, M, normalize=True, use_B=True)
        stop = done.record(loop_idx, M0, lam_sorted, M, res)
        if stop is not None:
            info = stop
            break
        dQ = dX                                           # copyto!(Q_basis, solutions): all M0 columns
    M_found = done.M_found
    X = engine.download(dX, M_found) if M_found > 0 else np.zeros((N, 0), complex)
    order = np.argsort(done.lam_vec[:M_found], kind="stable")  # feast_sort!
    return done.result(X, info, loop_count, order=order)
