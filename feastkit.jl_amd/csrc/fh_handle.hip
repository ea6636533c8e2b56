// fh_handle.hip -- the handle of libfeasthip.so: its workspace cache, the sampled profile, create / destroy and the
// feasthip_last_* / feasthip_profile_* queries.
#include "fh_host.hpp"
#include "fh_banded.hpp"
#include "fh_comm.hpp"
#include "fh_knobs.hpp"

// ---------------------------------------------------------------------------------------
// workspace + profiling helpers
// ---------------------------------------------------------------------------------------
int fh_get_buf(feasthip_ctx* h, const char* name, size_t bytes, void** out) {
    auto it = h->bufs.find(name);
    if (it != h->bufs.end() && it->second.second >= bytes) {
        *out = it->second.first;
        return 0;
    }
    if (it != h->bufs.end()) {
        hipStreamSynchronize(h->stream);
        hipFree(it->second.first);
        h->bufs.erase(it);
    }
    void* p = nullptr;
    size_t alloc = bytes < 256 ? 256 : bytes;
    hipError_t e = hipMalloc(&p, alloc);
    if (e != hipSuccess) {
        h->last_error = std::string("hipMalloc(") + name + ", " + std::to_string(alloc) + "): " + hipGetErrorString(e);
        return FEASTHIP_ERROR_MEMORY;
    }
    h->bufs[name] = {p, alloc};
    *out = p;
    return 0;
}

void fh_free_bufs(feasthip_ctx* h) {
    for (auto& kv : h->bufs) hipFree(kv.second.first);
    h->bufs.clear();
}

// Sampled event timing (1 launch in 13: a period coprime to the iteration caps, so the samples do not alias with
// the position inside a solve, where kernel durations shrink as nodes converge): every FH_PROF_PERIOD-th launch of a class is bracketed by two events
// on the launch stream; the class average is (sum of sampled durations)/(samples).
#define FH_PROF_PERIOD 13
static thread_local int fh_prof_open = 0;
void fh_prof_begin(feasthip_ctx* h, const char* cls) {
    fh_prof_open = 0;
    if (!h->profiling) return;
    fh_prof_class& pc = h->prof[cls];
    pc.launches += 1;
    const int period = h->prof_period > 0 ? h->prof_period : fh_knob::prof_period(FH_PROF_PERIOD);
    const long eff = (long)period * h->prof_mult;
    if (eff > 1 && (pc.launches % eff) != 1) return;
    if (h->pending_events.size() > 60000) return;
    const double t_in = fh_now_s();
    fh_event_pair ep;
    ep.cls = cls;
    // events are recycled through a pool: creating and destroying a pair per sample cost more than recording it
    if (!fh_knob::prof_nopool() && h->event_pool.size() >= 2) {
        ep.a = h->event_pool.back(); h->event_pool.pop_back();
        ep.b = h->event_pool.back(); h->event_pool.pop_back();
    } else {
        if (hipEventCreate(&ep.a) != hipSuccess) return;
        if (hipEventCreate(&ep.b) != hipSuccess) { hipEventDestroy(ep.a); return; }
    }
    hipEventRecord(ep.a, h->stream);
    h->pending_events.push_back(ep);
    fh_prof_open = 1;
    h->prof_host_s += fh_now_s() - t_in;
}
void fh_prof_end(feasthip_ctx* h) {
    if (!fh_prof_open) return;
    const double t_in = fh_now_s();
    hipEventRecord(h->pending_events.back().b, h->stream);
    fh_prof_open = 0;
    h->prof_host_s += fh_now_s() - t_in;
}
void fh_prof_collect(feasthip_ctx* h) {
    if (h->pending_events.empty()) return;
    hipStreamSynchronize(h->stream);
    const double t_in = fh_now_s();
    for (auto& ep : h->pending_events) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ep.a, ep.b) == hipSuccess) {
            fh_prof_class& pc = h->prof[ep.cls + std::string("#sampled")];
            pc.total_ms += ms;
            pc.launches += 1;
        }
        if (h->event_pool.size() < 8192) { h->event_pool.push_back(ep.a); h->event_pool.push_back(ep.b); }
        else { hipEventDestroy(ep.a); hipEventDestroy(ep.b); }
    }
    h->pending_events.clear();
    // Event calls are cheap on most hosts (0.7 % of a bench step at 1 launch in 13) but were seen to cost ~90 us each
    // on a loaded box: when sampling has taken more than 1 % of the wall time since it was switched on, sample 7x
    // less often (91 stays coprime to the iteration caps), up to 1 launch in 637.
    h->prof_host_s += fh_now_s() - t_in;
    const double wall = fh_now_s() - h->prof_t0;
    if ((h->prof_period > 0 ? h->prof_period : fh_knob::prof_period(FH_PROF_PERIOD)) > 1 && wall > 0.05 && h->prof_host_s > 0.01 * wall && h->prof_mult < 49) {   // period 1 = exact timing requested
        h->prof_mult *= 7;
        h->prof_host_s = 0.0;
        h->prof_t0 = fh_now_s();
    }
}

// ---------------------------------------------------------------------------------------
// lifecycle
// ---------------------------------------------------------------------------------------
extern "C" int feasthip_version(int* major, int* minor) {
    if (major) *major = FEASTHIP_VERSION_MAJOR;
    if (minor) *minor = FEASTHIP_VERSION_MINOR;
    return 0;
}

extern "C" int feasthip_create(feasthip_handle* out, int device_id) {
    if (!out) return FEASTHIP_ERROR_INTERNAL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return FEASTHIP_ERROR_INTERNAL;
    if (device_id < 0 || device_id >= ndev) return FEASTHIP_ERROR_INTERNAL;
    feasthip_ctx* h = new (std::nothrow) feasthip_ctx();
    if (!h) return FEASTHIP_ERROR_MEMORY;
    h->device = device_id;
    h->lu_outer_block = fh_knob::lu_kb(h->lu_outer_block);
    h->lu_solve_legacy = fh_knob::lu_solve_32();
    h->lu_gemm_staged = fh_knob::lu_gemm_staged();
    h->lu_lookahead = fh_knob::lu_lookahead();
    h->sum_mode = fh_knob::no_sum_mode() ? 0 : 1;
    h->lu_panel_legacy = fh_knob::lu_panel_legacy();
    if (hipSetDevice(device_id) != hipSuccess) { delete h; return FEASTHIP_ERROR_INTERNAL; }
    if (hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess) { delete h; return FEASTHIP_ERROR_INTERNAL; }
    h->stream = h->own_stream;
    if (hipHostMalloc((void**)&h->pin, (size_t)1 << 20, hipHostMallocDefault) == hipSuccess) h->pin_cap = (size_t)1 << 20;
    else { h->pin = nullptr; h->pin_cap = 0; hipGetLastError(); }
    if (hipMalloc((void**)&h->d_counters, 8 * sizeof(unsigned long long)) != hipSuccess) { hipStreamDestroy(h->own_stream); delete h; return FEASTHIP_ERROR_MEMORY; }
    hipMemset(h->d_counters, 0, 8 * sizeof(unsigned long long));
    {
        void* hp = nullptr;
        if (hipHostMalloc(&hp, 64, hipHostMallocMapped) != hipSuccess) { hipFree(h->d_counters); hipStreamDestroy(h->own_stream); delete h; return FEASTHIP_ERROR_MEMORY; }
        h->h_progress = (volatile unsigned long long*)hp;
        *h->h_progress = 0ull;
        void* dp = nullptr;
        if (hipHostGetDevicePointer(&dp, hp, 0) != hipSuccess) { hipHostFree(hp); hipFree(h->d_counters); hipStreamDestroy(h->own_stream); delete h; return FEASTHIP_ERROR_INTERNAL; }
        h->d_progress = (unsigned long long*)dp;
    }
    *out = h;
    return 0;
}

void fh_free_adjoint_csr(feasthip_ctx* h) {
    for (void* p : {(void*)h->csr_adj.rowptr, (void*)h->csr_adj.col, h->csr_adj.aval, h->csr_adj.bval}) if (p) hipFree(p);
    h->csr_adj = fh_csr();
}

void fh_free_problem(feasthip_ctx* h) {
    if (h->csr.rowptr) hipFree(h->csr.rowptr);
    if (h->csr.col) hipFree(h->csr.col);
    if (h->csr.aval) hipFree(h->csr.aval);
    if (h->csr.bval) hipFree(h->csr.bval);
    if (h->csr.perm) hipFree(h->csr.perm);
    if (h->csr.rp8) hipFree(h->csr.rp8);
    if (h->csr.col8) hipFree(h->csr.col8);
    if (h->csr.a8) hipFree(h->csr.a8);
    if (h->csr.b8) hipFree(h->csr.b8);
    if (h->csr.blk_start) hipFree(h->csr.blk_start);
    if (h->csr.ext_ptr) hipFree(h->csr.ext_ptr);
    if (h->csr.ext_idx) hipFree(h->csr.ext_idx);
    if (h->csr.lcol) hipFree(h->csr.lcol);
    h->csr = fh_csr();
    fh_free_adjoint_csr(h);
    if (h->dense.A) hipFree(h->dense.A);
    if (h->dense.B) hipFree(h->dense.B);
    h->dense = fh_dense();
    for (void* p : h->poly.coef) if (p) hipFree(p);
    h->poly = fh_poly();
    h->op = fh_operator();
    h->top = fh_termop();
    h->lu_cache.clear(hipFree);
    fh_banded_free(h);
    h->kind = FH_KIND_NONE;
    h->rs_P = h->rs_basis = h->rs_X = h->rs_R = nullptr;
    h->rs_m = h->rs_ld = h->rs_rank = h->rs_X_m = h->rs_X_ld = 0;
    h->rs_T.clear(); h->rs_R_lambda.clear();
}

extern "C" int feasthip_destroy(feasthip_handle h) {
    if (!h) return 0;
    hipSetDevice(h->device);
    if (h->poisoned) {
        // kernels of a failed call may still be running on the workspaces: neither wait for them (a wedged kernel
        // never ends) nor free what they touch.  The memory goes back to the driver when the process exits.
        fh_comm_mark_failed(h);
        delete h;
        return 0;
    }
    hipStreamSynchronize(h->stream);
    fh_comm_destroy(h);
    fh_prof_collect(h);
    fh_free_problem(h);
    fh_free_bufs(h);
    if (h->d_counters) hipFree(h->d_counters);
    for (auto& ep : h->pending_events) { hipEventDestroy(ep.a); hipEventDestroy(ep.b); }
    for (hipEvent_t e : h->event_pool) hipEventDestroy(e);
    if (h->h_progress) hipHostFree((void*)h->h_progress);
    if (h->pin) hipHostFree(h->pin);
    if (h->lu_ev_next) hipEventDestroy(h->lu_ev_next);
    if (h->lu_ev_rest) hipEventDestroy(h->lu_ev_rest);
    if (h->side_stream) hipStreamDestroy(h->side_stream);
    if (h->own_stream) hipStreamDestroy(h->own_stream);
    delete h;
    return 0;
}

extern "C" const char* feasthip_last_error(feasthip_handle h) { return h ? h->last_error.c_str() : "null handle"; }

extern "C" int feasthip_set_stream(feasthip_handle h, void* hip_stream) {
    if (int gate = fh_gate(h)) return gate;
    hipStreamSynchronize(h->stream);
    h->stream = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
    return 0;
}

extern "C" int feasthip_synchronize(feasthip_handle h) {
    if (int gate = fh_gate(h)) return gate;
    FH_CHECK(hipSetDevice(h->device));
    return fh_finish(h);
}

// ---------------------------------------------------------------------------------------
// measurement support
// ---------------------------------------------------------------------------------------
extern "C" int feasthip_last_node_iterations(feasthip_handle h, int* out, int n) {
    if (!h || !out) return FEASTHIP_ERROR_INTERNAL;
    for (int e = 0; e < n; ++e) out[e] = e < (int)h->last_node_iters.size() ? h->last_node_iters[e] : 0;
    return 0;
}

extern "C" int feasthip_last_global_node_iterations(feasthip_handle h, int* out, int n) {
    if (!h || !out) return FEASTHIP_ERROR_INTERNAL;
    for (int e = 0; e < n; ++e) out[e] = e < (int)h->global_node_iters.size() ? h->global_node_iters[e] : 0;
    return 0;
}

extern "C" int feasthip_last_shifted_sweep(feasthip_handle h, int* used, int* seed_node, int* seed_iterations, int* spmm_node_passes) {
    if (!h) return FEASTHIP_ERROR_INTERNAL;
    const bool u = h->shift_panels > 0 && h->shift_used == h->shift_panels;
    if (used) *used = u ? 1 : 0;
    if (seed_node) *seed_node = u ? h->shift_seed : -1;
    if (seed_iterations) *seed_iterations = u ? h->shift_seed_iters : 0;
    if (spmm_node_passes) *spmm_node_passes = u ? h->shift_seed_iters : 0;
    return 0;
}

extern "C" int feasthip_last_block_sweep(feasthip_handle h, int* used, int* node_steps_max, int* breakdown_nodes, int* spmm_node_passes) {
    if (!h) return FEASTHIP_ERROR_INTERNAL;
    const bool u = h->block_panels > 0 && h->block_used == h->block_panels;
    if (used) *used = u ? 1 : 0;
    if (node_steps_max) *node_steps_max = u ? h->block_steps_max : 0;
    if (breakdown_nodes) *breakdown_nodes = u ? h->block_breakdowns : 0;
    if (spmm_node_passes) *spmm_node_passes = u ? h->block_passes : 0;
    return 0;
}

extern "C" int feasthip_last_precond_sweep(feasthip_handle h, int* used, int* pivots, int64_t* factorizations, int64_t* substitution_sweeps,
                                           int64_t* factor_bytes, int* fell_back) {
    if (!h) return FEASTHIP_ERROR_INTERNAL;
    const bool u = h->pc_last.panels > 0 && h->pc_last.used == h->pc_last.panels;
    if (used) *used = u ? 1 : 0;
    if (pivots) *pivots = h->pc_last.pivots;
    if (factorizations) *factorizations = h->pc_last.factorizations;
    if (substitution_sweeps) *substitution_sweeps = h->pc_last.sweeps;
    if (factor_bytes) *factor_bytes = h->pc_last.factor_bytes;
    if (fell_back) *fell_back = h->pc_last.fell_back;
    return 0;
}

extern "C" int feasthip_last_column_iterations(feasthip_handle h, int* out, int n) {
    if (!h || !out) return FEASTHIP_ERROR_INTERNAL;
    for (int e = 0; e < n; ++e) out[e] = e < (int)h->last_col_iters.size() ? h->last_col_iters[e] : 0;
    return 0;
}

extern "C" int feasthip_profile_enable(feasthip_handle h, int enable) {
    if (!h) return FEASTHIP_ERROR_INTERNAL;
    h->profiling = enable ? 1 : 0;
    if (enable) { h->prof_host_s = 0.0; h->prof_t0 = fh_now_s(); }
    return 0;
}
extern "C" int feasthip_profile_reset(feasthip_handle h) {
    if (!h) return FEASTHIP_ERROR_INTERNAL;
    fh_prof_collect(h);
    h->prof.clear();
    h->prof_work.clear();
    h->prof_mult = 1;
    hipMemset(h->d_counters, 0, 8 * sizeof(unsigned long long));
    return 0;
}
extern "C" int feasthip_profile_set_period(feasthip_handle h, int period) {
    if (!h || period < 0) return FEASTHIP_ERROR_INTERNAL;
    h->prof_period = period;
    return 0;
}
extern "C" int feasthip_profile_get_work(feasthip_handle h, const char* kernel_class, double* work) {
    if (!h || !kernel_class || !work) return FEASTHIP_ERROR_INTERNAL;
    auto it = h->prof_work.find(kernel_class);
    *work = it == h->prof_work.end() ? 0.0 : it->second;
    return 0;
}
extern "C" int feasthip_profile_get(feasthip_handle h, const char* kernel_class, double* total_ms, int64_t* launches) {
    if (!h || !kernel_class) return FEASTHIP_ERROR_INTERNAL;
    fh_prof_collect(h);
    // device-side work counters: [0] active node-sweeps of the SpMM, [1] its active column x vector passes, [2] columns that
    // took a step in an update kernel, [3] of those the columns that go on iterating (the fused vector kernel reads and
    // writes five panels for them, one for a column on its last step), [4] distinct columns whose accumulator entries a
    // sum-mode launch read and wrote, [5] the part of [3] counted in the first vector launch of a lazy start (four passes)
    static const char* const names[] = {"spmm.node_launches", "spmm.column_passes", "update.active_columns", "update.continuing_columns",
                                        "update.accumulator_columns", "update.first_launch_columns"};
    for (int k = 0; k < 6; ++k)
        if (!strcmp(kernel_class, names[k])) {
            unsigned long long c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            hipStreamSynchronize(h->stream);
            hipMemcpy(c, h->d_counters, sizeof(c), hipMemcpyDeviceToHost);
            if (launches) *launches = (int64_t)c[k];
            if (total_ms) *total_ms = 0.0;
            return 0;
        }
    auto it = h->prof.find(kernel_class);
    auto is = h->prof.find(std::string(kernel_class) + "#sampled");
    int64_t n = it == h->prof.end() ? 0 : it->second.launches;
    double avg = 0.0;
    if (is != h->prof.end() && is->second.launches > 0) avg = is->second.total_ms / (double)is->second.launches;
    if (total_ms) *total_ms = avg * (double)n;   // estimated total = sampled average x launches
    if (launches) *launches = n;
    return 0;
}
