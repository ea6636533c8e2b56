// Host harness of the library's environment switches (csrc/fh_knobs.hpp), built with g++ under AddressSanitizer +
// UndefinedBehaviorSanitizer and run as a child process by tests/test_knobs_host.py.
//
//   host_knobs_harness <step> ...
// Each step is the name of an environment variable -- its accessor is called and "NAME value" is printed (booleans as 0 / 1,
// a null string as "(null)") -- or NAME=VALUE / NAME= (setenv) or -NAME (unsetenv), which change the environment between two
// reads: a once-per-process switch can only show its read time inside one run.  "--list" prints every name the harness knows.
// Accessors that take their default from the caller get the marker values below.
#include <cstdio>
#include <cstring>

#include "../feastkit.jl_amd/csrc/fh_knobs.hpp"

static const int PROF_PERIOD_DEFAULT = 13, LU_KB_DEFAULT = 0, LU_CHUNKS_DEFAULT = 7, NODES_PER_CALL_CAP = 21;
static const size_t GMRES_BUDGET_DEFAULT = 12345;
static const double MAX_MULTIPLIER_DEFAULT = 1e3;

static void put(const char* k, bool v) { std::printf("%s %d\n", k, v ? 1 : 0); }
static void put(const char* k, int v) { std::printf("%s %d\n", k, v); }
static void put(const char* k, size_t v) { std::printf("%s %zu\n", k, v); }
static void put(const char* k, double v) { std::printf("%s %.17g\n", k, v); }
static void put(const char* k, const char* v) { std::printf("%s %s\n", k, v ? v : "(null)"); }

struct entry { const char* name; void (*show)(const char*); };
static const entry ENTRIES[] = {
    {"FH_DEBUG_TIMING", [](const char* k) { put(k, fh_knob::debug_timing()); }},
    {"FH_PROF_PERIOD", [](const char* k) { put(k, fh_knob::prof_period(PROF_PERIOD_DEFAULT)); }},
    {"FH_PROF_NOPOOL", [](const char* k) { put(k, fh_knob::prof_nopool()); }},
    {"FH_REORDER", [](const char* k) { put(k, fh_knob::reorder()); }},
    {"FH_SPMM_ROW", [](const char* k) { put(k, fh_knob::spmm_row()); }},
    {"FH_LDS_SPMM", [](const char* k) { put(k, fh_knob::lds_spmm()); }},
    {"FH_COCG_FUSED", [](const char* k) { put(k, fh_knob::cocg_fused()); }},
    {"FH_NO_SUM_MODE", [](const char* k) { put(k, fh_knob::no_sum_mode()); }},
    {"FH_NO_SHARED_START", [](const char* k) { put(k, fh_knob::no_shared_start()); }},
    {"FH_NO_LAZY_START", [](const char* k) { put(k, fh_knob::no_lazy_start()); }},
    {"FH_CHECK_EVERY", [](const char* k) { put(k, fh_knob::check_every()); }},
    {"FH_GMRES_BUDGET_MB", [](const char* k) { put(k, fh_knob::gmres_budget_bytes(GMRES_BUDGET_DEFAULT)); }},
    {"FH_NO_CHOLQR", [](const char* k) { put(k, fh_knob::no_cholqr()); }},
    {"FH_CHOLQR_TWO_PASS", [](const char* k) { put(k, fh_knob::cholqr_two_pass()); }},
    {"FH_SMALL_MATMUL_VALU", [](const char* k) { put(k, fh_knob::small_matmul_valu()); }},
    {"FH_DENSE_OP_VALU", [](const char* k) { put(k, fh_knob::dense_op_valu()); }},
    {"FH_EIG_NO_LDS", [](const char* k) { put(k, fh_knob::eig_no_lds()); }},
    {"FH_LU_KB", [](const char* k) { put(k, fh_knob::lu_kb(LU_KB_DEFAULT)); }},
    {"FH_LU_SOLVE_32", [](const char* k) { put(k, fh_knob::lu_solve_32()); }},
    {"FH_LU_GEMM_STAGED", [](const char* k) { put(k, fh_knob::lu_gemm_staged()); }},
    {"FH_LU_LOOKAHEAD", [](const char* k) { put(k, fh_knob::lu_lookahead()); }},
    {"FH_LU_PANEL_LEGACY", [](const char* k) { put(k, fh_knob::lu_panel_legacy()); }},
    {"FH_LU_RESERVE", [](const char* k) { put(k, fh_knob::lu_reserve()); }},
    {"FH_LU_CHUNKS", [](const char* k) { put(k, fh_knob::lu_chunks(LU_CHUNKS_DEFAULT)); }},
    {"FH_LU_TRSM_SUBST", [](const char* k) { put(k, fh_knob::lu_trsm_subst()); }},
    {"FH_LU_3M", [](const char* k) { put(k, fh_knob::lu_3m()); }},
    {"FH_LU_BLOCKINV", [](const char* k) { put(k, fh_knob::lu_blockinv()); }},
    {"FH_WBAND_BLOCKINV", [](const char* k) { put(k, fh_knob::wband_blockinv()); }},
    {"FH_WBAND", [](const char* k) { put(k, fh_knob::wband()); }},
    {"FH_MF", [](const char* k) { put(k, fh_knob::mf()); }},
    {"FH_MF_LEAF", [](const char* k) { put(k, fh_knob::mf_leaf()); }},
    {"FH_MF_STORE_SLACK", [](const char* k) { put(k, fh_knob::mf_store_slack()); }},
    {"FH_MF_STREAMS", [](const char* k) { put(k, fh_knob::mf_streams()); }},
    {"FH_MF_SIDE", [](const char* k) { put(k, fh_knob::mf_side()); }},
    {"FH_MF_NODES_PER_CALL", [](const char* k) { put(k, fh_knob::mf_nodes_per_call(NODES_PER_CALL_CAP)); }},
    {"FH_MF_MAX_MULTIPLIER", [](const char* k) { put(k, fh_knob::mf_max_multiplier(MAX_MULTIPLIER_DEFAULT)); }},
    {"FEASTHIP_COMM_TRANSPORT", [](const char* k) { put(k, fh_knob::comm_transport()); }},
    {"FEASTHIP_COMM_TIMEOUT_S", [](const char* k) { put(k, fh_knob::comm_timeout_s()); }},
    {"FEASTHIP_COMM_STAGING_MB", [](const char* k) { put(k, fh_knob::comm_staging_bytes()); }},
    {"FEASTHIP_RCCL_LIB", [](const char* k) { put(k, fh_knob::rccl_lib()); }},
};

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        const char* step = argv[a];
        if (!std::strcmp(step, "--list")) {
            for (const entry& e : ENTRIES) std::printf("%s\n", e.name);
            continue;
        }
        if (step[0] == '-') { unsetenv(step + 1); continue; }
        if (const char* eq = std::strchr(step, '=')) {
            char name[64] = {0};
            if ((size_t)(eq - step) >= sizeof(name)) { std::fprintf(stderr, "FAIL: name too long: %s\n", step); return 1; }
            std::memcpy(name, step, eq - step);
            setenv(name, eq + 1, 1);
            continue;
        }
        bool found = false;
        for (const entry& e : ENTRIES)
            if (!std::strcmp(step, e.name)) { e.show(e.name); found = true; }
        if (!found) { std::fprintf(stderr, "FAIL: unknown switch %s\n", step); return 1; }
    }
    return 0;
}
