// fh_direct.hip -- the sequences of the direct solvers over their factor cache (fh_factor_cache.hpp), one copy for the dense
// LU (fh_dense.hip) and the sparse direct solver (fh_banded.hip), which differ in the operations of fh_direct_ops only.  Host code.
#include "fh_banded.hpp"
#include "fh_dense.hpp"
#include "fh_host.hpp"

static const fh_direct_ops& direct_ops(bool banded) { return banded ? fh_banded_direct_ops() : fh_dense_direct_ops(); }

// Factor the pairs (slots[e], z[e]) whose slot does not already hold the shift; status[e]: 0 or FEASTHIP_ERROR_LAPACK
static int direct_factor_slots(feasthip_ctx* h, const fh_direct_ops& ops, const std::vector<int>& slots, const std::vector<cplx>& z,
                               std::vector<int>& status, int64_t* nfact) {
    fh_factor_cache& cache = h->*ops.cache;
    std::vector<int> need, info;
    std::vector<cplx> zl;
    int64_t done = 0;
    cache.stale(slots, z, h->cache_factors != 0, need, zl);
    // (a second batch only after the sparse solver fell back to the band plan inside the first: every slot was re-made)
    for (int batch = 0; batch < 2 && (batch == 0 || !need.empty()); ++batch) {
        const int rc = ops.factor(h, need, zl, info);
        if (rc) return rc;
        cache.commit(need, zl, info);
        done += (int64_t)need.size();
        cache.unfactored(slots, z, need, zl);
    }
    if (nfact) *nfact = done;
    cache.status(slots, FEASTHIP_ERROR_LAPACK, status);
    return 0;
}

int fh_direct_solve_nodes(feasthip_ctx* h, bool banded, int ld, int m, int nodes, const std::vector<cplx>& z, const cplx* RHS, size_t rhs_stride,
                          cplx* Y, size_t stride, std::vector<int>& status, int64_t* nfact) {
    const fh_direct_ops& ops = direct_ops(banded);
    int rc = ops.ensure_slots(h, nodes, false);
    if (rc) return rc;
    std::vector<int> slots(nodes);
    for (int e = 0; e < nodes; ++e) slots[e] = e;
    if ((rc = direct_factor_slots(h, ops, slots, z, status, nfact))) return rc;
    return ops.solve(h, ld, m, slots, RHS, rhs_stride, Y, stride);
}

int fh_direct_solve_single(feasthip_ctx* h, bool banded, int ld, int m, cplx z, const cplx* RHS, cplx* Y, int* status, int64_t* nfact) {
    const fh_direct_ops& ops = direct_ops(banded);
    const int slot = fh_one_off_slot(z, h->zne, h->node_ids, h->node_count);
    int rc = ops.ensure_slots(h, fh_one_off_slot_count(slot, h->node_count), false);
    if (rc) return rc;
    fh_factor_cache& cache = h->*ops.cache;
    const std::vector<int> need(1, slot);
    if (!cache.holds(slot, z, h->cache_factors != 0)) {
        const std::vector<cplx> zl(1, z);
        std::vector<int> info;
        if ((rc = ops.factor(h, need, zl, info))) return rc;
        cache.commit(need, zl, info);
        if (nfact) *nfact = 1;
    }
    if ((rc = ops.solve(h, ld, m, need, RHS, 0, Y, (size_t)fh_N(h) * ld))) return rc;
    *status = cache.valid(slot) ? 0 : FEASTHIP_ERROR_LAPACK;
    return 0;
}

int fh_direct_factor_matched(feasthip_ctx* h, bool banded, const std::vector<cplx>& z, std::vector<int>& slots, std::vector<int>& status, int64_t* nfact) {
    const fh_direct_ops& ops = direct_ops(banded);
    const int rc = ops.ensure_slots(h, (int)z.size(), true);      // (as many slots as there were come back after a change of precision)
    if (rc) return rc;
    (h->*ops.cache).match(z, h->cache_factors != 0, slots);
    return direct_factor_slots(h, ops, slots, z, status, nfact);
}

int fh_direct_solve_slots(feasthip_ctx* h, bool banded, int ld, int m, const std::vector<int>& slots, const cplx* RHS, size_t rhs_stride, cplx* Y, size_t stride) {
    const fh_direct_ops& ops = direct_ops(banded);
    for (int s : slots)
        if (!(h->*ops.cache).valid(s)) { h->last_error = "internal: preconditioner substitution on a slot without factors"; return FEASTHIP_ERROR_INTERNAL; }
    return ops.solve(h, ld, m, slots, RHS, rhs_stride, Y, stride);
}

int fh_direct_solve_subset(feasthip_ctx* h, bool banded, int ld, int m, const std::vector<cplx>& z, const cplx* RHS, cplx* Y, size_t stride,
                           std::vector<int>& status, int64_t* nfact) {
    std::vector<int> slots;
    const int rc = fh_direct_factor_matched(h, banded, z, slots, status, nfact);
    return rc ? rc : direct_ops(banded).solve(h, ld, m, slots, RHS, 0, Y, stride);
}
