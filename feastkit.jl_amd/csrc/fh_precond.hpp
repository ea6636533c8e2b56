// fh_precond.hpp -- the host-only rules of the shift preconditioner (feasthip_set_preconditioner): which pivot a contour
// node takes.  No device code and no HIP types: tests/host_precond_harness.cpp compiles it alone under the sanitizers.
// The Python driver (hip_backend.py: precond_plan) states the same two rules; tests/test_precond_harness_host.py compares the plans.
#pragma once
#include <vector>

namespace fh_precond {

// The contour's nodes, in order, cut into k arcs of equal count (+-1): arc a is [a ne / k, (a + 1) ne / k) in integer
// arithmetic, its pivot the middle node; an arc of even count has two, and takes the one towards the nearer end of the
// contour (the lower one in the first half of the arcs, 2 a + 1 <= k, the upper one in the second), so that the pivots
// mirror each other as the nodes do: 8 nodes in 2 arcs give the nodes 1 and 6.  k is clamped to [1, ne].
// node_pivot[e]: the arc of node e; pivot_node[a]: the contour node whose shift is pivot a.
inline void arc_pivots(int ne, int k, std::vector<int>& node_pivot, std::vector<int>& pivot_node) {
    node_pivot.assign(ne > 0 ? ne : 0, -1);
    pivot_node.clear();
    if (ne <= 0) return;
    if (k < 1) k = 1;
    if (k > ne) k = ne;
    for (int a = 0; a < k; ++a) {
        const int lo = (int)((long long)a * ne / k), hi = (int)((long long)(a + 1) * ne / k);
        pivot_node.push_back(2 * a + 1 <= k ? lo + (hi - lo - 1) / 2 : lo + (hi - lo) / 2);
        for (int e = lo; e < hi; ++e) node_pivot[e] = a;
    }
}

// The pivot nearest to the shift (zr, zi) among np (re, im) pairs: the smallest squared distance, the lowest index on ties;
// -1 when there is none.
inline int nearest_pivot(double zr, double zi, const double* pivots, int np) {
    int best = -1;
    double bd = 0.0;
    for (int p = 0; p < np; ++p) {
        const double dx = pivots[2 * p] - zr, dy = pivots[2 * p + 1] - zi, d = dx * dx + dy * dy;
        if (best < 0 || d < bd) { best = p; bd = d; }
    }
    return best;
}

}  // namespace fh_precond
