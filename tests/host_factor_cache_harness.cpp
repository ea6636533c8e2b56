// CPU harness of the factor caches' host-only rules (csrc/fh_factor_cache.hpp): growing and clearing, the reuse test, what a
// batch has to factor and what it commits, the slot of a one-off shift and the slots matched by shift, on malloc / free
// allocators that count.  Built with -fsanitize=address,undefined by tests/test_factor_cache_harness_host.py; prints OK last.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../feastkit.jl_amd/csrc/fh_factor_cache.hpp"

static int fails = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++fails; } \
    } while (0)

struct zz { double x, y; };
typedef std::vector<int> ints;
typedef std::vector<zz> shifts;

static int allocs = 0, frees = 0, fail_at = 0;      // fail_at: the allocation (counted from 1, since it was set) that fails; 0: none
static void* count_alloc(size_t bytes) {
    if (fail_at && --fail_at == 0) return nullptr;
    ++allocs;
    return std::malloc(bytes);
}
static void count_free(void* p) { ++frees; std::free(p); }

// a cache of n slots with the given states and shifts
static void fill(fh_factor_cache& c, const ints& state, const shifts& z) {
    c.clear(count_free);
    EXPECT(c.grow((int)state.size(), 8, 8, count_alloc, count_free) == FH_GROW_OK);
    for (size_t s = 0; s < state.size(); ++s) { c.slots[s].state = state[s]; c.slots[s].zr = z[s].x; c.slots[s].zi = z[s].y; }
}

// today's three loops of the slot matching, restated literally on plain arrays
static ints match_reference(const ints& valid, const shifts& held, bool cache_on, const shifts& z) {
    const int nd = (int)z.size(), nslots = (int)valid.size();
    ints taken(nslots, 0), slots(nd, -1);
    for (int d = 0; d < nd; ++d)
        for (int s = 0; s < nslots && cache_on; ++s)
            if (!taken[s] && valid[s] == 1 && held[s].x == z[d].x && held[s].y == z[d].y) { slots[d] = s; taken[s] = 1; break; }
    for (int pass = 0; pass < 2; ++pass)
        for (int d = 0; d < nd; ++d)
            for (int s = 0; s < nslots && slots[d] < 0; ++s)
                if (!taken[s] && (pass == 1 || valid[s] != 1)) { slots[d] = s; taken[s] = 1; }
    return slots;
}

int main() {
    const zz za = {1.0, 0.5}, zb = {2.0, 0.5}, zc = {3.0, -0.25}, zx = {7.0, 7.0};
    ints need, out;
    shifts zneed;

    // grow and clear
    {
        fh_factor_cache c;
        EXPECT(c.grow(3, 64, 16, count_alloc, count_free) == FH_GROW_OK && c.size() == 3);
        EXPECT(c.grow(5, 64, 16, count_alloc, count_free) == FH_GROW_OK && c.size() == 5);
        EXPECT(c.grow(2, 64, 16, count_alloc, count_free) == FH_GROW_OK && c.size() == 5);      // never shrinks
        EXPECT(allocs == 10 && frees == 0);
        for (const fh_factor_slot& s : c.slots) EXPECT(s.factor && s.pivots && s.state == FH_SLOT_EMPTY);
        c.clear(count_free);
        EXPECT(frees == 10 && c.size() == 0);
        c.clear(count_free);
        EXPECT(frees == 10);
        // the pivots of the fourth slot cannot be had: its factor goes back, three slots stay
        EXPECT(c.grow(3, 64, 16, count_alloc, count_free) == FH_GROW_OK);
        allocs = frees = 0;
        fail_at = 2;
        EXPECT(c.grow(5, 64, 16, count_alloc, count_free) == FH_GROW_NO_PIVOTS);
        EXPECT(c.size() == 3 && allocs == 1 && frees == 1);
        fail_at = 1;
        EXPECT(c.grow(5, 64, 16, count_alloc, count_free) == FH_GROW_NO_FACTOR);
        EXPECT(c.size() == 3 && allocs == 1 && frees == 1 && fail_at == 0);
        c.clear(count_free);                          // (the sanitizer's leak check sees the rest)
    }

    // precision
    {
        fh_factor_cache c;
        fill(c, {1, -1, 0}, {za, zb, zc});
        allocs = frees = 0;
        c.set_precision(64, count_free);
        EXPECT(c.size() == 3 && frees == 0 && c.prec == 64);
        EXPECT(c.slots[0].state == 1 && c.slots[1].state == -1 && c.slots[2].state == 0 && c.slots[1].zr == zb.x && c.slots[2].zi == zc.y);
        c.set_precision(32, count_free);
        EXPECT(c.size() == 0 && frees == 6 && c.prec == 32);
    }

    // stale, commit, status, and the fallback that empties every slot
    {
        fh_factor_cache c;
        fill(c, {0, 0, 0}, {za, za, za});
        const ints which = {0, 1, 2};
        shifts z = {za, zb, zc};
        c.stale(which, z, true, need, zneed);
        EXPECT(need == which && zneed.size() == 3);
        c.commit(need, zneed, {0, 3, 0});
        EXPECT(c.slots[0].state == FH_SLOT_VALID && c.slots[1].state == FH_SLOT_SINGULAR && c.slots[2].state == FH_SLOT_VALID);
        EXPECT(c.slots[1].zr == zb.x && c.slots[2].zi == zc.y);
        EXPECT(c.valid(0) && !c.valid(1) && c.valid(2) && !c.valid(-1) && !c.valid(3));
        c.status(which, 8, out);
        EXPECT(out == ints({0, 8, 0}));
        c.stale(which, z, true, need, zneed);
        EXPECT(need == ints({1}) && zneed.size() == 1 && zneed[0].x == zb.x && c.slots[1].state == FH_SLOT_EMPTY);
        c.status(which, 8, out);
        EXPECT(out == ints({0, 8, 0}));              // empty reports the error as singular does
        c.unfactored(which, z, need, zneed);
        EXPECT(need == ints({1}));
        z[2].y = std::nextafter(zc.y, 1.0);          // one ulp off: not the same shift
        c.stale(which, z, true, need, zneed);
        EXPECT(need == ints({1, 2}) && zneed.size() == 2 && zneed[1].y == z[2].y);
        c.commit(need, zneed, {0, 0});
        c.stale(which, z, true, need, zneed);
        EXPECT(need.empty());
        c.stale(which, z, false, need, zneed);       // cache switched off: everything is factored
        EXPECT(need == which);
        c.commit(need, zneed, {0, 0, 0});
        // a fallback inside the batch: two slots were cached, one is factored, then every slot is re-made
        z[0] = zx;
        c.stale(which, z, true, need, zneed);
        EXPECT(need == ints({0}));
        long long done = (long long)need.size();
        for (fh_factor_slot& s : c.slots) s.state = FH_SLOT_EMPTY;
        c.commit(need, zneed, {0});
        c.unfactored(which, z, need, zneed);
        EXPECT(need == ints({1, 2}) && zneed[0].x == zb.x && zneed[1].x == zc.x);
        c.commit(need, zneed, {0, 0});
        done += (long long)need.size();
        EXPECT(done == 3);
        c.unfactored(which, z, need, zneed);
        EXPECT(need.empty());
        // signed zero and NaN
        const zz zero_im = {1.0, 0.0}, minus_zero_im = {1.0, -0.0}, nan_re = {std::numeric_limits<double>::quiet_NaN(), 1.0};
        c.commit({0, 1}, shifts({zero_im, nan_re}), {0, 0});
        EXPECT(c.holds(0, minus_zero_im, true) && !c.holds(0, minus_zero_im, false));
        EXPECT(c.valid(1) && !c.holds(1, nan_re, true));
        c.stale({0, 1}, shifts({minus_zero_im, nan_re}), true, need, zneed);
        EXPECT(need == ints({1}));
        c.clear(count_free);
    }

    // one-off shift
    {
        const shifts zne = {zx, za, zb, zc};
        const ints ids = {1, 2, 3};
        int s = fh_one_off_slot(zb, zne, ids, 3);
        EXPECT(s == 1 && fh_one_off_slot_count(s, 3) == 4);
        s = fh_one_off_slot(zx, zne, ids, 3);        // zx is a contour node, but no local one
        EXPECT(s == 3 && fh_one_off_slot_count(s, 3) == 4);
        EXPECT(fh_one_off_slot(zc, zne, ints({1, 2}), 3) == 3);      // a node-id list shorter than node_count
        EXPECT(fh_one_off_slot(zc, zne, ints(), 3) == 3 && fh_one_off_slot(zc, zne, ids, 0) == 0);
    }

    // match by shift, by hand
    {
        fh_factor_cache c;
        fill(c, {0, 0}, {za, za});
        c.match(shifts({za, zb}), true, out);
        EXPECT(out == ints({0, 1}));
        fill(c, {1, 1, 1}, {za, zb, zc});
        c.match(shifts({zc, za}), true, out);
        EXPECT(out == ints({2, 0}));
        c.match(shifts({zc, zx}), true, out);
        EXPECT(out == ints({2, 0}));
        c.match(shifts({zc, za}), false, out);       // cache off: nothing is matched by shift
        EXPECT(out == ints({0, 1}));
        c.slots[1].state = FH_SLOT_SINGULAR;
        c.match(shifts({zx}), true, out);
        EXPECT(out == ints({1}));
        fill(c, {1, 1, 1}, {zb, za, zc});
        c.match(shifts({za, za}), true, out);
        EXPECT(out.size() == 2 && out[0] == 1 && out[1] != 1 && out[1] >= 0 && out[1] < 3);
        c.clear(count_free);
    }

    // match by shift against the literal loops
    {
        const zz pool[4] = {za, zb, zc, zx};
        unsigned long long lcg = 12345;
        auto next = [&](int n) { lcg = lcg * 6364136223846793005ULL + 1442695040888963407ULL; return (int)((lcg >> 33) % (unsigned)n); };
        fh_factor_cache c;
        for (int trial = 0; trial < 4000; ++trial) {
            const int ns = next(7), nd = next(std::min(ns, 6) + 1);
            ints state(ns);
            shifts held(ns), z(nd);
            for (int s = 0; s < ns; ++s) { state[s] = next(3) - 1; held[s] = pool[next(4)]; }
            for (int d = 0; d < nd; ++d) z[d] = pool[next(4)];
            const bool on = next(4) != 0;
            fill(c, state, held);
            c.match(z, on, out);
            EXPECT(out == match_reference(state, held, on, z));
            ints seen(ns, 0);
            for (int d = 0; d < nd; ++d) {
                EXPECT(out[d] >= 0 && out[d] < ns);
                if (out[d] >= 0 && out[d] < ns) { EXPECT(!seen[out[d]]); seen[out[d]] = 1; }
            }
        }
        c.clear(count_free);
    }
    if (fails) { std::printf("%d failures\n", fails); return 1; }
    std::printf("OK\n");
    return 0;
}
