"""TEST-ONLY numpy restatement of the per-node solver's selection rule (the product's copy lives under the C ABI:
feastkit.jl_amd/csrc/fh_policy.hpp, feasthip_policy_pick_direct_nodes).  tests/test_node_solver_host.py pins the library
against it."""
import numpy as np

DIRECT = 4          # FEASTHIP_SOLVER_BANDED


def pick_direct_nodes(node_iters, max_direct, t_iter, t_solve, t_factor, loops_left):
    """-> (k, kinds).  Nodes ordered by iterations descending, ties to the lower index; with the first k of them direct one
    further loop is predicted to take  t_iter * max(iterations of the others) + k * (t_solve + t_factor / max(loops_left, 1));
    the smallest k in 0..max_direct that minimises it is taken."""
    it = np.asarray(node_iters, dtype=np.int64)
    ne = len(it)
    order = np.argsort(-it, kind="stable")
    per_node = float(t_solve) + float(t_factor) / float(max(int(loops_left), 1))
    best, best_t = 0, None
    for k in range(0, min(max(int(max_direct), 0), ne) + 1):
        rest = float(it[order[k]]) if k < ne else 0.0
        t = float(t_iter) * rest + float(k) * per_node
        if best_t is None or t < best_t:
            best, best_t = k, t
    kinds = np.zeros(ne, dtype=np.int32)
    kinds[order[:best]] = DIRECT
    return best, kinds
