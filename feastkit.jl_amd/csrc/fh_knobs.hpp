// fh_knobs.hpp -- every environment switch of libfeasthip.so (DESIGN.md section 9 is written from this file).
// Host only, standard library only (tests/host_knobs_harness.cpp compiles it alone with g++).  One accessor per variable
// owns its name, its parse convention, its default, its clamp and its READ TIME:
//   per call      a plain read; the caller decides how often (each accessor says when)
//   per process   cached in a function-local static of the inline accessor: one cache per process, whichever file asks first
//   per handle    read by feasthip_create into a field of feasthip_ctx
// None of them is needed for normal use; they select the comparison paths of DESIGN.md.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdlib>

namespace fh_knob {

// ---- parse primitives: nothing else in csrc/ reads the environment ----
inline const char* str_or_null(const char* name) { return std::getenv(name); }
inline bool present(const char* name) { return str_or_null(name) != nullptr; }                                 // any value, "0" and "" too
inline bool off(const char* name) { const char* e = str_or_null(name); return e && std::atoi(e) == 0; }       // set and zero ("" is zero)
inline bool on(const char* name) { const char* e = str_or_null(name); return e && std::atoi(e) != 0; }        // set and non-zero
inline int int_or(const char* name, int dflt) { const char* e = str_or_null(name); return e ? std::atoi(e) : dflt; }
inline double double_or(const char* name, double dflt) { const char* e = str_or_null(name); return e ? std::atof(e) : dflt; }

// ---- diagnostics and the in-library profiler ----
// host-side phase timings and plan decisions on stderr.  Per call.
inline bool debug_timing() { return present("FH_DEBUG_TIMING"); }
// HIP-event sampling period of the profiler (1 = every launch; dflt is the macro of the same name in fh_handle.hip).  Per process.
inline int prof_period(int dflt) { static const int v = std::max(1, int_or("FH_PROF_PERIOD", dflt)); return v; }
// profiler creates and destroys an event pair per sample instead of recycling them through a pool.  Per process.
inline bool prof_nopool() { static const bool v = present("FH_PROF_NOPOOL"); return v; }

// ---- sparse operator ----
// ingest-time row-block renumbering: 0 caller's order, 1 wide patterns only (default), 2 whenever there are two blocks.  Per process.
inline int reorder() { static const int v = int_or("FH_REORDER", 1); return v; }
// =0: full-width real panels through the 4-rows-per-wave gather kernel instead of the row-per-wave kernel.  Per process.
inline bool spmm_row() { static const bool v = !off("FH_SPMM_ROW"); return v; }
// =1: the LDS-window SpMM on renumbered matrices (opt-in, slower); it also keeps the lazy COCG start out.  Per process.
inline bool lds_spmm() { static const bool v = on("FH_LDS_SPMM"); return v; }

// ---- Krylov sweeps ----
// =0: the five-launch COCG iteration instead of the fused one.  Per process.
inline bool cocg_fused() { static const bool v = !off("FH_COCG_FUSED"); return v; }
// one solution panel per node instead of the shared accumulator.  Per handle (feasthip_ctx::sum_mode).
inline bool no_sum_mode() { return present("FH_NO_SUM_MODE"); }
// one start residual per node instead of the shared one.  Per call (each contour_apply).
inline bool no_shared_start() { return present("FH_NO_SHARED_START"); }
// materialise the start residual / direction panels of a shared start.  Per call (each sweep start).
inline bool no_lazy_start() { return present("FH_NO_LAZY_START"); }
// iterations queued between two looks at the device's progress word (>= 1).  Per call (each sweep).
inline int check_every() { return std::max(1, int_or("FH_CHECK_EVERY", 16)); }
// workspace budget of the device GMRES in MiB (>= 1), returned in bytes; dflt is what the caller sized from free memory.  Per call.
inline size_t gmres_budget_bytes(size_t dflt) { return present("FH_GMRES_BUDGET_MB") ? (size_t)std::max(1, int_or("FH_GMRES_BUDGET_MB", 1)) << 20 : dflt; }

// ---- orthonormalisation and small dense products ----
// pivoted Gram-Schmidt only, no Cholesky-QR fast path.  Per call.
inline bool no_cholqr() { return present("FH_NO_CHOLQR"); }
// always run the second Cholesky-QR pass.  Per call.
inline bool cholqr_two_pass() { return present("FH_CHOLQR_TWO_PASS"); }
// VALU form of Q V.  Per process.
inline bool small_matmul_valu() { static const bool v = present("FH_SMALL_MATMUL_VALU"); return v; }
// VALU form of the dense operator products.  Per process.
inline bool dense_op_valu() { static const bool v = present("FH_DENSE_OP_VALU"); return v; }
// Jacobi eigensolver with its matrices in global memory instead of LDS.  Per process.
inline bool eig_no_lds() { static const bool v = present("FH_EIG_NO_LDS"); return v; }

// ---- blocked LU (dense, band, fronts) ----
// outer block column of the two-level LU, rounded down to a multiple of 32, at least 32; dflt 0 = by size.  Per handle (lu_outer_block).
inline int lu_kb(int dflt) { return present("FH_LU_KB") ? std::max(32, int_or("FH_LU_KB", 0) / 32 * 32) : dflt; }
// 32-column one-launch substitution steps of the dense LU (forward solves only: the adjoint substitutions of
// feasthip_set_adjoint -- dense, multifrontal and blocked band alike -- always take the 128-column path).  Per handle (lu_solve_legacy).
inline bool lu_solve_32() { return present("FH_LU_SOLVE_32"); }
// trailing update with both panels staged through LDS.  Per handle (lu_gemm_staged).
inline bool lu_gemm_staged() { return present("FH_LU_GEMM_STAGED"); }
// =0: no overlap of the next block column's panels with the rest of the trailing update.  Per handle (lu_lookahead).
inline int lu_lookahead() { return int_or("FH_LU_LOOKAHEAD", 1); }
// =1: per-column global-memory panel kernel.  Per handle (lu_panel_legacy).
inline int lu_panel_legacy() { return int_or("FH_LU_PANEL_LEGACY", 0); }
// CUs per XCD kept out of the look-ahead side stream's mask (0 = a plain low-priority side stream).  Per factorisation.
inline int lu_reserve() { return int_or("FH_LU_RESERVE", 4); }
// column chunks of the look-ahead's rest update (>= 1); dflt depends on the reserve.  Per factorisation.
inline int lu_chunks(int dflt) { return present("FH_LU_CHUNKS") ? std::max(1, int_or("FH_LU_CHUNKS", 1)) : dflt; }
// U block row by in-place substitution instead of the product with L11^-1.  Per factorisation.
inline bool lu_trsm_subst() { return present("FH_LU_TRSM_SUBST"); }
// =0: four-product complex MFMA form of the trailing update (dense, band and front LU alike).  Per process.
inline bool lu_3m() { static const bool v = !off("FH_LU_3M"); return v; }
// =0: dense LU's U block row by 32-row products instead of 128-row slabs with the 128 x 128 inverse.  Per process.
inline bool lu_blockinv() { static const bool v = !off("FH_LU_BLOCKINV"); return v; }
// =0: the same for the band LU.  Per process.
inline bool wband_blockinv() { static const bool v = !off("FH_WBAND_BLOCKINV"); return v; }

// ---- plans of the direct sparse solver ----
// =1: every matrix to the blocked band LU, narrow bands too (keeps the multifrontal plan out unless FH_MF=1).  Per plan.
inline bool wband() { return on("FH_WBAND"); }
// multifrontal plan: 0 never, 1 always, unset (-1) by predicted work.  Per plan.
inline int mf() { return int_or("FH_MF", -1); }
// largest leaf subset of the nested dissection (>= 8).  Per plan.
inline int mf_leaf() { return std::max(8, int_or("FH_MF_LEAF", 64)); }
// padded factor store a group may take over its members' own; values under 1 give the default.  Per plan.
inline double mf_store_slack() { const double v = double_or("FH_MF_STORE_SLACK", 0.0); return v >= 1.0 ? v : 1.25; }
// streams the groups of one tree height are spread over (1 .. 4).  Per plan.
inline int mf_streams() { return std::max(1, std::min(4, int_or("FH_MF_STREAMS", 1))); }
// =0: every second group of a level does not go to the LU look-ahead's side stream.  Per process.
inline bool mf_side() { static const bool v = !off("FH_MF_SIDE"); return v; }
// quadrature nodes per factorisation / substitution batch, 1 .. cap (cap: what the grid limit allows).  Per factorisation and per solve.
inline int mf_nodes_per_call(int cap) { return std::max(1, std::min(cap, int_or("FH_MF_NODES_PER_CALL", cap))); }
// largest boundary multiplier accepted before a matrix falls back to the band LU (dflt: fh_mf::max_boundary_multiplier).  Per factorisation.
inline double mf_max_multiplier(double dflt) { return double_or("FH_MF_MAX_MULTIPLIER", dflt); }

// ---- communicator (all read by feasthip_comm_init_rank; the RCCL path once, when the library is first resolved) ----
// "shm": shared-device transport when the caller passes FEASTHIP_COMM_AUTO (anything else: RCCL).
inline const char* comm_transport() { return str_or_null("FEASTHIP_COMM_TRANSPORT"); }
// barrier timeout of the shared-device transport in seconds (>= 1).
inline double comm_timeout_s() { return std::max(1.0, double_or("FEASTHIP_COMM_TIMEOUT_S", 120.0)); }
// staging buffer of the shared-device transport in MiB (>= 1), returned in bytes.
inline size_t comm_staging_bytes() { return (size_t)std::max(1, int_or("FEASTHIP_COMM_STAGING_MB", 32)) << 20; }
// path of librccl.so when it is neither mapped already nor on the loader path.
inline const char* rccl_lib() { return str_or_null("FEASTHIP_RCCL_LIB"); }

}  // namespace fh_knob
