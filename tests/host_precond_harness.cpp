// CPU harness of the shift preconditioner's host-only rules (csrc/fh_precond.hpp): the arc rule of precond_shifts = k and the
// nearest-pivot map of an explicit pivot list, swept over node and arc counts.  Built with -fsanitize=address,undefined by
// tests/test_precond_harness_host.py; prints the plans the Python driver is compared with, then OK.
#include <cstdio>
#include <vector>

#include "../feastkit.jl_amd/csrc/fh_precond.hpp"

static int fails = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++fails; } \
    } while (0)

int main() {
    std::vector<int> node_pivot, pivot_node;
    for (int ne = 0; ne <= 40; ++ne)
        for (int k = -1; k <= ne + 3; ++k) {
            fh_precond::arc_pivots(ne, k, node_pivot, pivot_node);
            EXPECT((int)node_pivot.size() == ne);
            if (ne == 0) { EXPECT(pivot_node.empty()); continue; }
            const int kk = k < 1 ? 1 : (k > ne ? ne : k);
            EXPECT((int)pivot_node.size() == kk);
            std::vector<int> count(kk, 0);
            for (int e = 0; e < ne; ++e) {
                EXPECT(node_pivot[e] >= 0 && node_pivot[e] < kk);
                if (node_pivot[e] >= 0 && node_pivot[e] < kk) count[node_pivot[e]] += 1;
                if (e > 0) EXPECT(node_pivot[e] >= node_pivot[e - 1]);            // arcs are runs of consecutive nodes
            }
            int lo = ne, hi = 0;
            for (int a = 0; a < kk; ++a) { lo = count[a] < lo ? count[a] : lo; hi = count[a] > hi ? count[a] : hi; }
            EXPECT(lo >= 1 && hi - lo <= 1);                                       // equal count (+-1)
            for (int a = 0; a < kk; ++a) {
                EXPECT(pivot_node[a] >= 0 && pivot_node[a] < ne);
                if (pivot_node[a] >= 0 && pivot_node[a] < ne) EXPECT(node_pivot[pivot_node[a]] == a);   // a pivot lies in its own arc
            }
            if (kk == 2 && ne % 2 == 0) EXPECT(pivot_node[1] == ne - 1 - pivot_node[0]);
        }
    for (int ne : {8, 16, 7}) {
        for (int k : {1, 2, 3, 4}) {
            fh_precond::arc_pivots(ne, k, node_pivot, pivot_node);
            std::printf("arcs ne=%d k=%d pivots", ne, k);
            for (int p : pivot_node) std::printf(" %d", p);
            std::printf(" map");
            for (int p : node_pivot) std::printf(" %d", p);
            std::printf("\n");
        }
    }
    const double piv[] = {3.0, 0.5, 1.0, 0.5, 1.0, 0.5};
    EXPECT(fh_precond::nearest_pivot(1.0, 1.0, piv, 3) == 1);                      // ties: the lowest index
    EXPECT(fh_precond::nearest_pivot(2.5, 2.0, piv, 3) == 0);
    EXPECT(fh_precond::nearest_pivot(2.0, 0.5, piv, 2) == 0);                      // equidistant
    EXPECT(fh_precond::nearest_pivot(0.0, 0.0, piv, 0) == -1);
    EXPECT(fh_precond::nearest_pivot(0.0, 0.0, nullptr, 0) == -1);
    if (fails) { std::printf("%d failures\n", fails); return 1; }
    std::printf("OK\n");
    return 0;
}
