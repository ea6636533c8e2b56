// fh_factor_cache.hpp -- the host-only bookkeeping of the LU factor caches (feasthip_ctx::lu_cache for the dense LU,
// ::band_cache for the sparse direct solver): which slot holds which shift, what has to be factored, which slot a shift takes.
// No device code and no HIP types: tests/host_factor_cache_harness.cpp compiles it alone under the sanitizers.  A shift is any
// type with double members x and y; memory comes from the caller's callables (the library: hipMalloc / hipFree).
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

enum fh_slot_state { FH_SLOT_EMPTY = 0, FH_SLOT_VALID = 1, FH_SLOT_SINGULAR = -1 };
enum fh_grow_result { FH_GROW_OK = 0, FH_GROW_NO_FACTOR = 1, FH_GROW_NO_PIVOTS = 2 };      // which allocation failed

// (zr, zi): the shift of the factors, meaningful unless the slot is empty
struct fh_factor_slot { void* factor = nullptr; int* pivots = nullptr; int state = FH_SLOT_EMPTY; double zr = 0.0, zi = 0.0; };

struct fh_factor_cache {
    std::vector<fh_factor_slot> slots;
    int prec = 64;                // element type of the factors: 64 = complex128, 32 = complex64

    int size() const { return (int)slots.size(); }
    bool valid(int s) const { return s >= 0 && s < size() && slots[s].state == FH_SLOT_VALID; }

    // Reuse test: slot s holds the factors of z.  == on both parts: -0.0 matches 0.0, a NaN shift is never held.
    template <typename Z> bool holds(int s, const Z& z, bool cache_on) const {
        return cache_on && slots[s].state == FH_SLOT_VALID && slots[s].zr == z.x && slots[s].zi == z.y;
    }

    // Of the pairs (which[e], z[e]), those whose slot does not hold its shift: listed in need / zneed and marked empty
    template <typename Z> void stale(const std::vector<int>& which, const std::vector<Z>& z, bool cache_on, std::vector<int>& need, std::vector<Z>& zneed) {
        need.clear(); zneed.clear();
        for (size_t e = 0; e < which.size(); ++e)
            if (!holds(which[e], z[e], cache_on)) { need.push_back(which[e]); zneed.push_back(z[e]); slots[which[e]].state = FH_SLOT_EMPTY; }
    }
    // A factored batch: slot need[q] now has the factors of zneed[q], singular where info[q] != 0
    template <typename Z> void commit(const std::vector<int>& need, const std::vector<Z>& zneed, const std::vector<int>& info) {
        for (size_t q = 0; q < need.size(); ++q) {
            fh_factor_slot& s = slots[need[q]];
            s.zr = zneed[q].x; s.zi = zneed[q].y;
            s.state = info[q] == 0 ? FH_SLOT_VALID : FH_SLOT_SINGULAR;
        }
    }
    // The pairs whose slot is empty after a batch: every slot was re-made inside it (the sparse solver changed its plan)
    template <typename Z> void unfactored(const std::vector<int>& which, const std::vector<Z>& z, std::vector<int>& need, std::vector<Z>& zneed) const {
        need.clear(); zneed.clear();
        for (size_t e = 0; e < which.size(); ++e)
            if (slots[which[e]].state == FH_SLOT_EMPTY) { need.push_back(which[e]); zneed.push_back(z[e]); }
    }
    // status[e] = 0 where slot which[e] has factors, else `error`
    void status(const std::vector<int>& which, int error, std::vector<int>& out) const {
        out.assign(which.size(), 0);
        for (size_t e = 0; e < which.size(); ++e) if (slots[which[e]].state != FH_SLOT_VALID) out[e] = error;
    }

    // Slots by shift for a subset of the nodes (size() >= z.size()): a cached equal shift is claimed first, then the free or
    // singular slots in index order, then the cached ones nobody claimed -- a node whose z is cached keeps its slot whatever
    // else joined or left the subset.  No slot is handed out twice.
    template <typename Z> void match(const std::vector<Z>& z, bool cache_on, std::vector<int>& out) const {
        const int nd = (int)z.size(), ns = size();
        std::vector<char> taken(ns, 0);
        out.assign(nd, -1);
        for (int d = 0; d < nd; ++d)
            for (int s = 0; s < ns; ++s)
                if (!taken[s] && holds(s, z[d], cache_on)) { out[d] = s; taken[s] = 1; break; }
        for (int pass = 0; pass < 2; ++pass)
            for (int d = 0; d < nd; ++d)
                for (int s = 0; s < ns && out[d] < 0; ++s)
                    if (!taken[s] && (pass == 1 || slots[s].state != FH_SLOT_VALID)) { out[d] = s; taken[s] = 1; }
    }

    // Grow to n empty slots of factor_bytes + pivot_bytes each.  alloc(bytes) returns null on failure; a slot whose pivots
    // cannot be had gives its factor back, and the slots made so far stay.
    template <typename Alloc, typename Free> fh_grow_result grow(int n, size_t factor_bytes, size_t pivot_bytes, Alloc alloc, Free release) {
        while (size() < n) {
            fh_factor_slot s;
            if (!(s.factor = alloc(factor_bytes))) return FH_GROW_NO_FACTOR;
            if (!(s.pivots = (int*)alloc(pivot_bytes))) { release(s.factor); return FH_GROW_NO_PIVOTS; }
            slots.push_back(s);
        }
        return FH_GROW_OK;
    }
    template <typename Free> void clear(Free release) {      // every factor, then every pivot array
        for (fh_factor_slot& s : slots) release(s.factor);
        for (fh_factor_slot& s : slots) release(s.pivots);
        slots.clear();
    }
    // Factors of another element type are of no use: a change of precision drops every slot
    template <typename Free> void set_precision(int p, Free release) { if (p != prec) { clear(release); prec = p; } }
};

// The slot of a one-off shift: a shift equal to local quadrature node e (zne[node_ids[e]], e < node_count) takes that node's
// slot, so an RCI sweep over the contour keeps one factorisation per node across refinement loops, as the reference's drivers
// do (factor_cache, src/dense/feast_dense.jl:458, 487-497); any other shift shares slot node_count.
template <typename Z> inline int fh_one_off_slot(const Z& z, const std::vector<Z>& zne, const std::vector<int>& node_ids, int node_count) {
    for (int e = 0; e < node_count && e < (int)node_ids.size(); ++e)
        if (zne[node_ids[e]].x == z.x && zne[node_ids[e]].y == z.y) return e;
    return node_count;
}
inline int fh_one_off_slot_count(int slot, int node_count) { return std::max(slot, node_count) + 1; }
