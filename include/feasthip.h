/*
 * feasthip.h -- C ABI of libfeasthip.so: the MI355X (gfx950) FEAST contour-integration
 * inner loop that drops in behind FeastKit.jl's feast()/feast_general()/pfeast_* and RCI
 * surfaces as a new `:hip` backend.
 *
 * The reference (subhk/FeastKit.jl v1.0.11) is pure Julia with no FFI of its own; the
 * boundary below is derived from the seams an accelerator can sit behind without
 * touching src/core or src/interfaces.  Each entry point cites
 * the reference code it replaces (paths relative to the reference checkout).
 *
 * Conventions
 *   - POD arguments only.  No callbacks, no ownership transfer, no exceptions.
 *   - Host matrices are COLUMN-MAJOR (Julia/Fortran); complex data is interleaved
 *     (re,im) double pairs (Julia ComplexF64 / C99 double _Complex layout).
 *   - "_dev" variants take DEVICE pointers in the same column-major layout and run
 *     asynchronously on the handle's stream; the plain variants take host pointers,
 *     copy in/out synchronously and never retain the pointer after return.
 *   - Return value: 0 on success, else the reference's FeastError codes
 *     (src/core/feast_types.jl:257-268): 1 N, 2 M0, 3 Emin/Emax, 4 Emid/r,
 *     5 no convergence, 6 memory, 7 internal (HIP runtime), 8 LAPACK/singular, 9 fpm.
 *     feasthip_last_error() returns a human-readable string for the last failure.
 *   - One handle = one GPU = one host thread at a time (the reference's :threads
 *     backend must not share a handle across Julia threads).
 */
#ifndef FEASTHIP_H
#define FEASTHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FEASTHIP_VERSION_MAJOR 0
#define FEASTHIP_VERSION_MINOR 1

/* FeastError, src/core/feast_types.jl:257-268 */
enum {
    FEASTHIP_SUCCESS = 0,
    FEASTHIP_ERROR_N = 1,
    FEASTHIP_ERROR_M0 = 2,
    FEASTHIP_ERROR_EMIN_EMAX = 3,
    FEASTHIP_ERROR_EMID_R = 4,
    FEASTHIP_ERROR_NO_CONVERGENCE = 5,
    FEASTHIP_ERROR_MEMORY = 6,
    FEASTHIP_ERROR_INTERNAL = 7,
    FEASTHIP_ERROR_LAPACK = 8,
    FEASTHIP_ERROR_FPM = 9
};

/* shifted-system solver kinds: keyword `solver` of feast_sygv!/feast_scsrgv!
 * (src/dense/feast_dense.jl:81-84, src/sparse/feast_sparse.jl:249-252).          */
enum {
    FEASTHIP_SOLVER_LU = 0,        /* :direct  -- dense only (batched complex LU)          */
    FEASTHIP_SOLVER_BICGSTAB = 1,  /* :iterative -- batched BiCGStab (Krylov.bicgstab,
                                      src/interfaces/feast_matfree.jl:716)                 */
    FEASTHIP_SOLVER_GMRES = 2,     /* :gmres   -- batched restarted GMRES(m)
                                      (src/sparse/feast_sparse.jl:183-188)                 */
    FEASTHIP_SOLVER_BANDED = 4,    /* sparse DIRECT solver for CSR input: one LU of z B - A per quadrature node, factors
                                      cached across refinement loops.  The direct solver of the banded drivers
                                      (src/banded/feast_banded.jl:100-150) and the build's counterpart of the sparse
                                      drivers' default `lu(z B - A)` (UMFPACK, src/sparse/feast_sparse.jl:339-342).
                                      A narrow band is eliminated as stored (ZGBTRF/ZGBTRS semantics); any other
                                      pattern by a multifrontal LU on a nested-dissection tree (batched dense fronts on
                                      the MFMA LU kernels, partial pivoting inside the fully-summed blocks) when that is
                                      less than half the work of the alternative: reverse Cuthill-McKee + a blocked band
                                      LU on the same kernels (fill confined to the band, 16 N (2 kl + ku + 256) bytes
                                      per node).  feasthip_band_plan / feasthip_direct_plan_flops say which, and what
                                      it costs                                                               */
    FEASTHIP_SOLVER_COCG = 3,      /* conjugate-orthogonal CG for the complex-SYMMETRIC shifted
                                      systems that real-symmetric A, B produce (one operator
                                      application per iteration); not in the reference      */
    FEASTHIP_SOLVER_BLOCK_COCG = 6,  /* COCG whose contour sweep lets the columns of a node share ONE block Krylov space
                                      (block COCG with residual orthonormalisation: the live columns of the panel are one
                                      block right-hand side of z_e B - A; the nodes still advance side by side).  Replaces
                                      the per-column recurrences of the solve loop, src/sparse/feast_sparse.jl:318-369 and
                                      :164-203, for real CSR A and B (or B = I), fp64 panels, feasthip_contour_apply without
                                      moments or direct nodes; a node whose block breaks down (rank loss, a small pivot) is
                                      finished by the per-column sweep; every other case runs exactly as
                                      FEASTHIP_SOLVER_COCG.  feasthip_last_block_sweep reports what ran                 */
    FEASTHIP_SOLVER_SHIFTED_COCG = 5 /* COCG whose contour sweep shares ONE Krylov space among the local nodes when
                                      B = I (shifted COCG: the matrices z_e I - A differ by multiples of the identity, so
                                      only a seed node applies the operator, the others follow by scalar recurrences).
                                      Replaces the solve loop over the nodes, src/sparse/feast_sparse.jl:318-369 and
                                      :164-203, for real CSR A without B, fp64 panels, feasthip_contour_apply without
                                      moments; every other case runs exactly as FEASTHIP_SOLVER_COCG                */
};

enum { FEASTHIP_STORAGE_CSR = 0, FEASTHIP_STORAGE_CSC = 1 };

typedef struct feasthip_ctx* feasthip_handle;

/* Per-call statistics of feasthip_contour_apply (no reference counterpart; replaces the
 * @warn/@debug diagnostics of src/parallel/feast_parallel.jl:266-273).                  */
typedef struct feasthip_stats {
    double  seconds_total;       /* wall time of the call (host clock)                       */
    double  seconds_solve;       /* device time inside shifted solves (HIP events)            */
    int64_t krylov_iterations;   /* sum over local nodes of max-over-columns iterations       */
    int64_t spmm_calls;          /* operator applications (block of m columns each)           */
    int64_t factorizations;      /* dense LU factorizations performed in this call            */
    double  max_rel_residual;    /* max over nodes/columns of ||b - S y|| / ||b|| (iterative) */
} feasthip_stats;

/* ---- lifecycle ------------------------------------------------------------------- */
int  feasthip_version(int* major, int* minor);
/* device_id: HIP ordinal (one process per GPU: LOCAL_RANK). */
int  feasthip_create(feasthip_handle* out, int device_id);
int  feasthip_destroy(feasthip_handle h);
const char* feasthip_last_error(feasthip_handle h);
/* Run all work on an externally owned hipStream_t (e.g. torch's current stream). NULL
 * restores the handle's own stream. */
int  feasthip_set_stream(feasthip_handle h, void* hip_stream);
int  feasthip_synchronize(feasthip_handle h);

/* ---- multi-GPU: one handle per GPU, one process (or task) per handle ---------------------------- */
/* The reference reduces inside its parallel backends: MPI.Allreduce(local_Aq/local_Sq/local_Q, +, comm)
 * (src/parallel/feast_mpi.jl:117-119, 856-858, 1001) and the master sum over worker results
 * (src/parallel/feast_parallel.jl:497-503).  Here the handle owns the collective: once a communicator is
 * attached, feasthip_contour_apply[_dev] returns Qproj (and zAq/zSq, node_status) already summed over all
 * ranks -- ONE packed RCCL all-reduce over xGMI per refinement loop, ordered on the handle's stream.
 *
 * feasthip_comm_unique_id: rank 0 calls it (ncclGetUniqueId) and ships the 128 bytes to the other ranks by
 *   whatever the host has (MPI.bcast in a Julia host, a TCP store in Python).
 * feasthip_comm_init_rank: collective; attaches rank `rank` of `nranks` to the handle's device.
 *   transport FEASTHIP_COMM_RCCL: librccl (resolved at run time), one rank per GPU.
 *   transport FEASTHIP_COMM_SHM : for ranks that SHARE a HIP device (RCCL refuses that); rendezvous through
 *     POSIX shared memory, peers' staging buffers mapped with HIP IPC, summed in rank order by a kernel
 *     (bitwise identical on every rank).  A rehearsal transport for one-GPU test rigs, host-synchronous.
 *   transport FEASTHIP_COMM_AUTO: RCCL unless the environment says FEASTHIP_COMM_TRANSPORT=shm.
 * feasthip_allreduce_sum_dev: in-place SUM of `count` doubles at device pointer dptr over the ranks (the
 *   reduction contour_apply uses, exposed for the host's own small reductions, e.g. residual blocks
 *   src/parallel/feast_mpi.jl:264-284).  Returns after the result is visible.                          */
#define FEASTHIP_UNIQUE_ID_BYTES 128
enum { FEASTHIP_COMM_AUTO = 0, FEASTHIP_COMM_RCCL = 1, FEASTHIP_COMM_SHM = 2 };
int  feasthip_comm_unique_id(char* uid /* FEASTHIP_UNIQUE_ID_BYTES */);
int  feasthip_comm_init_rank(feasthip_handle h, int nranks, int rank, const char* uid, int transport);
int  feasthip_comm_destroy(feasthip_handle h);
int  feasthip_comm_info(feasthip_handle h, int* nranks, int* rank, int* transport);
int  feasthip_allreduce_sum_dev(feasthip_handle h, void* dptr, int64_t count);

/* ---- problem definition ---------------------------------------------------------- */
/* Dense A (and B, NULL => identity), column-major, lda/ldb >= N.
 * Replaces the Matrix arguments of feast_sygv!/feast_hegv!/feast_gegv!
 * (src/dense/feast_dense.jl:356, 402).  is_complex: 0 => double, 1 => interleaved c128. */
int  feasthip_set_dense(feasthip_handle h, int64_t N, int is_complex,
                        const void* A, int64_t lda, const void* B, int64_t ldb);

/* Sparse A (and B, ptrB==NULL => identity).  Julia passes SparseMatrixCSC{T,Int64}
 * (index_base 1, storage CSC); scipy passes CSR base 0.  For CSC input the library
 * transposes on ingest, so results are for the matrix as the CALLER defines it
 * (no silent conj/transpose).
 * Replaces the SparseMatrixCSC arguments of feast_scsrgv!/feast_hcsrgv!/feast_gcsrgv!
 * (src/sparse/feast_sparse.jl:713, 873) and pfeast_scsrgv! (src/parallel/feast_parallel.jl:450). */
int  feasthip_set_csr(feasthip_handle h, int64_t N, int is_complex, int index_base, int storage,
                      int64_t nnzA, const int64_t* ptrA, const int64_t* idxA, const void* valA,
                      int64_t nnzB, const int64_t* ptrB, const int64_t* idxB, const void* valB);

/* Matrix-free problem: an OPERATOR handle.  The library holds no matrix; wherever it needs A X or B X it calls `apply`.
 * Replaces the A_mul! / B_mul! arguments of feast_matvec (src/interfaces/feast_interfaces.jl:465-481) and the
 * MatrixFreeOperator of src/interfaces/feast_matfree.jl.
 *
 * The callback:  apply(user, which, nodes, ld, N, dX, x_node_stride, dY, y_node_stride, stream)  forms Y_e = A X_e (which 0)
 * or Y_e = B X_e (which 1) for e = 0 .. nodes-1 and returns 0.
 *   - dX and dY are DEVICE pointers to `nodes` panels of N x ld complex128 values in the library's panel layout: element
 *     (i, c) of a panel is at i * ld + c, node e starts at e * stride elements (x_node_stride for dX, y_node_stride for dY;
 *     both at least N * ld).  ld is 16, 32 or 64.
 *   - The padding columns (beyond the block width of the call) are part of the panel: the operator is linear, so applying it
 *     to them is harmless, and the library keeps uninitialised memory out of every panel it hands out (padding is zero or
 *     the image of zero).  The callback writes all ld columns of dY, or leaves the padding of dY alone -- either is fine.
 *   - The work is enqueued on `stream` (a hipStream_t: the stream the handle runs on), or finished before the callback
 *     returns.  dX is read only; dY is scratch of the handle and holds nothing on entry.
 *   - All `nodes` panels are multiplied whatever the solver's state: which nodes have finished is known on the device only.
 *   - The callback must not call back into the same handle.
 *   - A non-zero return ends the entry point that made the call: it returns FEASTHIP_ERROR_INTERNAL with feasthip_last_error =
 *     "operator callback failed (which=..., code=...)", launches nothing more, and leaves the handle usable (not poisoned).
 *     The outputs of that entry point are undefined.
 * flags: FEASTHIP_OP_B_IDENTITY -- B = I, `which` = 1 is never called; FEASTHIP_OP_COMPLEX -- the operator is not real (a real
 * operator maps the real and the imaginary parts of a panel separately; the flag feeds the COCG admission below and the
 * callers' choice of the real projection, nothing else); FEASTHIP_OP_SYMMETRIC -- A = A^T and B = B^T (not conjugated),
 * which is what COCG needs.
 * An operator handle takes every path a dense handle takes under the Krylov solvers FEASTHIP_SOLVER_BICGSTAB, _COCG (also
 * asked for as _SHIFTED_COCG or _BLOCK_COCG: the cocg sweep) and _GMRES: feasthip_contour_apply[_dev] and the resident
 * calls, feasthip_shifted_solve[_dev], feasthip_matmul[_dev], feasthip_project[_dev] / _project_pair[_dev],
 * feasthip_ritz_residual[_dev], feasthip_rayleigh_ritz_dev, feasthip_orthonormalize[_dev], feasthip_estimate_count.
 * FEASTHIP_ERROR_FPM, with a message that names the Krylov solvers, answers: FEASTHIP_SOLVER_LU and _BANDED; a COCG kind
 * without FEASTHIP_OP_SYMMETRIC or with FEASTHIP_OP_COMPLEX; factor_precision 32; feasthip_set_adjoint(1);
 * feasthip_set_node_solver with a direct node; an attached communicator (feasthip_comm_init_rank on the handle, or
 * feasthip_set_operator on a handle that has one); every feasthip_poly_* / feasthip_nep_* call.
 * N: 1 .. INT32_MAX / 64, else FEASTHIP_ERROR_N (also for a null callback).  feasthip_set_dense / feasthip_set_csr restore an
 * ordinary handle.  A Julia `@cfunction` or any C function pointer serves this ABI.                     */
typedef int (*feasthip_apply_fn)(void* user, int which /* 0: A, 1: B */, int nodes, int ld, int64_t N,
                                 const void* dX, int64_t x_node_stride, void* dY, int64_t y_node_stride, void* stream);
enum {
    FEASTHIP_OP_B_IDENTITY = 1,
    FEASTHIP_OP_COMPLEX = 2,
    FEASTHIP_OP_SYMMETRIC = 4
};
int  feasthip_set_operator(feasthip_handle h, int64_t N, feasthip_apply_fn apply, void* user, int flags);

/* Term-operator handle: a split form whose matrices are the caller's products,
 *     T(z) X = sum_k f_k(z) (A_k X),   k = 0 .. nterms-1,   2 <= nterms <= FEASTHIP_POLY_MAX_DEGREE + 1.
 * `apply` is the callback of feasthip_set_operator with which = k, the term index: all nodes of a call in one invocation, the
 * same panel layout and stream rules.  The scalars f_k(.) stay host tables as on a term handle (feasthip_set_terms); a
 * polynomial is the case f_k(z) = z^k.
 * flags: FEASTHIP_OP_COMPLEX and FEASTHIP_OP_SYMMETRIC (every A_k = A_k^T).  Bit k of identity_mask: A_k = I -- no callback and
 * no scratch for that term, the combine kernel reads X.  scratch_bytes bounds the product scratch (nt' * nodes * 16 N ld bytes,
 * nt' the non-identity terms a call keeps; 0: the library's default): when the nodes of a call do not fit, the operator is
 * applied in node chunks -- the callback sees the chunk's node count, one kernel launch per chunk.
 * The handle is a TERM handle for the feasthip_nep_* family under the Krylov solvers FEASTHIP_SOLVER_BICGSTAB, _GMRES and (with
 * FEASTHIP_OP_SYMMETRIC) _COCG: feasthip_nep_set_node_values, feasthip_nep_solve_dev, feasthip_nep_eval_cols_dev,
 * feasthip_nep_resinv_apply_dev, feasthip_poly_project_reduced_dev, feasthip_nep_ritz_eval_dev and
 * feasthip_poly_orthonormalize_dev.  A solve's shift must be a node of the contour the node values were set for.  A term
 * whose table entries are zero for every node (or column) of a call is neither produced (no callback) nor read.
 * FEASTHIP_ERROR_FPM, with a message that names the three Krylov solvers, answers: the LU, banded and sparse-direct solvers;
 * factor_precision 32; shifted and block COCG; _COCG without FEASTHIP_OP_SYMMETRIC; the adjoint switch; per-node solvers; a
 * communicator; node ranges and lists; every other feasthip_poly_* call (they form powers of lambda or linearised columns);
 * feasthip_poly_estimate_count; the pencil entry points.  A failed callback behaves as on an operator handle.
 * feasthip_set_term_norms: nterms positive doubles that stand where ||A_k||_F stands in the backward error of
 * feasthip_nep_ritz_eval_dev, which returns FEASTHIP_ERROR_FPM until they are set.                                        */
int  feasthip_set_term_operator(feasthip_handle h, int64_t N, int nterms, feasthip_apply_fn apply, void* user, int flags,
                                unsigned identity_mask, int64_t scratch_bytes);
int  feasthip_set_term_norms(feasthip_handle h, const double* norms /* nterms */);

/* Contour nodes/weights as produced by feast_contour / feast_gcontour
 * (src/core/feast_tools.jl:212-371): zne/wne are 2*ne doubles (re,im interleaved).
 * weight_scale = 2.0 for the Hermitian half contour (src/dense/feast_dense.jl:174),
 * 1.0 for the general full contour (src/kernel/feast_kernel.jl:762-766).              */
int  feasthip_set_contour(feasthip_handle h, int ne, const double* zne, const double* wne,
                          double weight_scale);

/* real_part = 1: Qproj (and zAq/zSq) receive only the REAL part of the weighted sum,
 * Qproj = Re( sum_e 2 w_e Y_e ).  For real-symmetric A, B and a real Q this equals the sum
 * over the full contour (the conjugate half is the complex conjugate), i.e. the true FEAST
 * rational filter -- what the reference's real paths do: _pfeast_store_real_moments!
 * (src/parallel/feast_parallel.jl:38-55), feast_srci! (src/kernel/feast_kernel.jl:143,183-186).
 * real_part = 0 (default) keeps the complex half-contour sum of the complexified variant A
 * (src/dense/feast_dense.jl:231).                                                        */
int  feasthip_set_real_projection(feasthip_handle h, int real_part);

/* Restrict this handle to nodes [first, first+count) -- the block partition of
 * distribute_contour_points (src/parallel/feast_parallel.jl:433-447) /
 * MPIFeastState (src/parallel/feast_mpi.jl:36-43).  Default: all nodes.              */
int  feasthip_set_node_range(feasthip_handle h, int first, int count);
/* Arbitrary node subset (0-based contour indices).  Used by the iterative solvers to pair
 * near-axis (slow) with far-axis (fast) nodes per GPU instead of contiguous blocks; the
 * summed result is independent of the assignment.                                       */
int  feasthip_set_node_list(feasthip_handle h, int count, const int* indices);

/* Column block of this handle: the following contour_apply calls sweep only columns [first, first+count) of the
 * m columns they are given (the rest of Qproj is zero on this rank and filled in by the all-reduce); count < 0
 * restores "all columns".  The reference shards quadrature nodes only (src/parallel/feast_parallel.jl:433-447);
 * with Krylov solves the iteration counts of the nodes differ by 10x while the columns of a node cost the same,
 * so ranks are arranged as (node groups) x (column groups).                                                  */
int  feasthip_set_column_block(feasthip_handle h, int64_t first, int64_t count);

/* Inexact-FEAST extension (not in the reference): columns c < m with mask[c] == 0 keep their initial
 * guess (the Ritz warm start q_c/(z - lambda_c) when ritz_lambda is given) and are never iterated by
 * the BiCGStab / COCG solvers of the following contour_apply calls (the restarted GMRES path ignores the
 * mask: all columns of a node advance in lock-step through one Arnoldi basis).  Used to stop spending solves on the
 * guard columns (Ritz values outside the interval) once the subspace has settled.  mask == NULL or
 * m == 0 clears it.  Ignored by the LU path.  The mask is ONE-SHOT: it is consumed by the next
 * contour_apply call (cleared when that call returns, whatever its outcome) and never applies to
 * feasthip_shifted_solve.                                                                    */
int  feasthip_set_column_mask(feasthip_handle h, int64_t m, const int* mask);

/* Error 7 with "handle poisoned" in feasthip_last_error: a Krylov sweep missed its progress deadline or the device
 * queue faulted, and kernels of the failed call may still be in flight.  Every later call on the handle fails fast;
 * feasthip_destroy then neither waits for the stream nor frees the workspaces.  The host must end the process with a
 * non-zero status (or continue in a fresh child process) -- never re-exec a process that has touched the GPU.  */

/* Solver options: keyword args solver/solver_tol/solver_maxiter/solver_restart
 * (src/dense/feast_dense.jl:81-84).  Iterative stop test is Krylov.jl's
 * ||r_k|| <= atol + rtol*||r_0|| per column.  factor_precision 64|32: 32 = mixed precision.  Dense LU:
 * complex64 factors and substitutions (f32 MFMA) inside an fp64 iterative-refinement loop (residual by the
 * fp64 operator kernel, stop at 1e-14 relative, <= 8 steps) -- fp64-accurate solves while
 * cond(zB-A)*eps32 < 1 (the reference has no counterpart; BASELINE config 5 asks for it).
 * BiCGStab/COCG: correction solve on complex64 panels around an fp64 residual (inexact-solve mode).
 * restart: the GMRES restart length (basis panels per cycle); 0 and 1 are taken as 2.  GMRES counts maxit in lock-steps of a
 * node batch (all columns of the batch's nodes advance together) and spmm_calls in products that ran.
 * cache_factors: keep LU factors per
 * node across calls (src/dense/feast_dense.jl:147,188).                                 */
/* Free the cached factorisations of the direct solvers (dense LU, band LU): the reference keeps `lu(z B - A)` per node for
 * the life of a driver call (factor cache, src/dense/feast_dense.jl:458, 487-497) and the garbage collector takes them;
 * here they live until the problem changes, the handle is destroyed, or this call.  The next direct solve factors again.  */
int  feasthip_release_factors(feasthip_handle h);

/* The band FEASTHIP_SOLVER_BANDED would eliminate for the current CSR problem (after its reordering) and the device memory
 * of ONE node's factor; *blocked = 1 when the blocked band LU on the dense kernels is used (2: multifrontal, below).  A host shim uses it to decide
 * between the direct and the iterative solvers (the reference decides by keyword only: src/sparse/feast_sparse.jl:249-252).
 * Returns 0, FEASTHIP_ERROR_FPM when no CSR problem is set or the band is beyond the solver's reach.                     */
int  feasthip_band_plan(feasthip_handle h, int* kl, int* ku, int64_t* bytes_per_node, int* blocked);
/* Real flops of ONE node's factorisation under the plan feasthip_band_plan reports (*blocked = 2: the multifrontal
 * elimination on a nested-dissection tree, the counterpart of the reference's UMFPACK call src/sparse/feast_sparse.jl:334-342,
 * taken when its work is under half the band elimination's; kl / ku are then the band it replaced and bytes_per_node the
 * multifrontal factors).                                                                                                 */
int  feasthip_direct_plan_flops(feasthip_handle h, double* flops_per_node);

int  feasthip_set_solver(feasthip_handle h, int kind, double rtol, double atol, int maxit,
                         int restart, int factor_precision, int cache_factors);

/* Per-node solver: a sparse direct solve for chosen quadrature nodes of a Krylov sweep.  The reference picks ONE solver per
 * driver call by keyword -- the iterative branch src/sparse/feast_sparse.jl:164-203, `lu(zB - A)` per node :334-342 -- so a
 * sweep whose chain length is set by the one or two nodes nearest the real axis pays their iteration count on every node.
 * kinds[e], indexed by GLOBAL contour node (like node_status under a communicator): 0 = the handle's solver
 * (feasthip_set_solver), FEASTHIP_SOLVER_BANDED = factor z_e B - A and solve directly; anything else: FEASTHIP_ERROR_FPM.
 * count == 0 or kinds == NULL clears the setting; otherwise count must be the contour's node count (FEASTHIP_ERROR_FPM).
 * Persistent until cleared; feasthip_set_contour with another node count clears it.  Honoured by feasthip_contour_apply,
 * _dev, _resident and feasthip_estimate_count for a CSR problem whose handle solver is COCG or BICGSTAB with
 * factor_precision = 64; with GMRES, a dense problem or factor_precision = 32 and at least one local direct node the sweep
 * returns FEASTHIP_ERROR_FPM (a handle whose own solver is BANDED solves every node directly: the kinds change nothing).
 * feasthip_shifted_solve ignores it.  Direct nodes share the factor cache of FEASTHIP_SOLVER_BANDED, matched by z_e: a
 * repeated sweep on the same contour factors nothing (cache_factors), a moved contour factors them again, and
 * feasthip_stats.factorizations counts what the call factored; feasthip_release_factors frees them.  They ignore the column
 * mask and the warm start, report node_status 0 or 8, and 0 iterations in feasthip_last_[global_]node_iterations.        */
int  feasthip_set_node_solver(feasthip_handle h, int count, const int* kinds);
/* Device memory `nodes` direct nodes take under the plan feasthip_band_plan reports: *factor_bytes for the cached factors and
 * pivots, *transient_bytes for what lives only while they are factored and swept (multifrontal work arena and substitution
 * panels).  A host shim sizes the direct subset of feasthip_set_node_solver with it.                                       */
int  feasthip_direct_plan_bytes(feasthip_handle h, int nodes, int64_t* factor_bytes, int64_t* transient_bytes);

/* Shift preconditioner of the restarted GMRES sweep (not in the reference, whose iterative branch src/sparse/feast_sparse.jl:164-203
 * runs unpreconditioned): M = z_p B - A is factored at a few PIVOT shifts z_p off the real axis, and node e, whose pivot is p,
 * solves in the variable u = M x with the operator
 *     S_e M^-1 = (z_e B - A)(z_p B - A)^-1 = I + (z_e - z_p) B M^-1,
 * whose eigenvalues (z_e - lambda)/(z_p - lambda) sit at 1 for every lambda far from the contour.  One factorisation serves
 * every node of its pivot: the sweep holds npivots factors where FEASTHIP_SOLVER_BANDED holds one per node.
 * pivots: npivots (re, im) pairs with a non-zero imaginary part; node_pivot[e], indexed by GLOBAL contour node: the pivot of
 * node e, or -1 for a node that stays unpreconditioned.  npivots == 0 clears the setting; otherwise count must be the
 * contour's node count (FEASTHIP_ERROR_FPM).  Persistent until cleared; feasthip_set_contour with another node count clears it.
 * Honoured by feasthip_contour_apply, _dev, _resident and feasthip_shifted_solve[_dev] (a single shift takes the nearest pivot)
 * for a CSR problem whose solver is FEASTHIP_SOLVER_GMRES with factor_precision = 64.  While it is set, those calls return
 * FEASTHIP_ERROR_FPM, with the reason in feasthip_last_error, for any other solver, a dense / operator / term / polynomial
 * handle, factor_precision = 32, the adjoint switch, a communicator with more than one rank, and a node-solver setting with a
 * direct node.  The identity form needs exact factors, which is why complex64 factors are out: with M~ != M the operator is
 * S_e M~^-1, not I + c_e B M~^-1.
 * The pivots are factored through the factor cache of FEASTHIP_SOLVER_BANDED, matched by shift (all three direct plans): a
 * repeated sweep factors nothing, a factor a direct node left at the same shift is reused, feasthip_release_factors frees them.
 * A pivot that cannot be factored gives its nodes node_status 8.  The reported residual is the true b - S_e x of x = M^-1 u;
 * feasthip_stats.spmm_calls counts operator products (the preconditioned operator included), the substitution sweeps are
 * reported by feasthip_last_precond_sweep.                                                                                    */
int  feasthip_set_preconditioner(feasthip_handle h, int npivots, const double* pivots /* re,im pairs */, int count,
                                 const int* node_pivot);
/* What the last sweep (or shifted solve) did under the preconditioner, summed over its 64-column panels: used = 1 when every
 * panel ran preconditioned; the distinct pivots it named; the factorisations it made (0 when the cache held them); the
 * substitution sweeps (one batched M^-1 per cycle start, per lock-step that ran and per final x = M^-1 u); the device memory of the pivot
 * factors (pivots x bytes_per_node of feasthip_band_plan); fell_back = 1 when the multifrontal LU rejected a pivot and the band
 * LU took over (a normal outcome).  Any pointer may be null.                                                                  */
int  feasthip_last_precond_sweep(feasthip_handle h, int* used, int* pivots, int64_t* factorizations, int64_t* substitution_sweeps,
                                 int64_t* factor_bytes, int* fell_back);

/* ---- host policy of the inexact FEAST mode (no device work; needs no problem and no GPU) -----------------------------
 * What the :hip backend adds to the reference's driver loop when `solver = :direct` on large sparse input is served by the
 * warm-started, inexact Krylov sweeps (not in the reference; DESIGN.md sections 2 and 5): which ellipse ratio fpm[18] to put
 * the Gauss / trapezoid nodes on, how many inner iterations and which inner tolerance the next sweep gets, and which Ritz
 * pairs are solver noise.  Kept here so that a host shim CALLS it instead of re-porting it:
 *   feasthip_policy_init     state for one solve.  steer != 0: the library picks fpm[18] itself (the caller left it unset),
 *                            p->aspect holds the a-priori choice; steer == 0: p->aspect = fpm18 stays, only the guards act.
 *   feasthip_policy_update   after every refinement loop that did not converge: epsout, the count M of Ritz values inside,
 *                            whether a node stopped at the iteration cap (node_status 5), the rank Ritz values ordered
 *                            inside-first.  On return p->aspect (changed: recompute the contour with it, feasthip_set_contour),
 *                            p->inner_cap and p->next_rtol (feasthip_set_solver) describe the NEXT sweep.
 *   feasthip_policy_set_aside  flags[j] = 1 for pairs inside the interval that are solver noise (residual > 0.1 and > 100 x
 *                            the smallest residual inside); returns their number (0 when all M would be flagged).
 *   feasthip_policy_filter_ratio / _reach: the filter model the steering rests on (for tests and diagnostics).        */
typedef struct feasthip_policy {
    double Emin, Emax, inner_rtol, outer_tol;
    int ne, quadrature;          /* fpm[2], fpm[16] (0 Gauss, 1 trapezoid)                                              */
    int steer;                   /* 1: the policy picks fpm[18]; 0: guards only                                          */
    int aspect, cap;             /* fpm[18] of the next sweep; upper bound the safeguard has put on it (8000 at first)  */
    int inner_cap, base_cap;     /* Krylov iteration cap per loop: next sweep / as given                                */
    int n_hist;
    double eps_prev;             /* outer residual of the previous loop (inf before the first)                          */
    double eps_hist[3];          /* stagnation guard                                                                    */
    double next_rtol;            /* inner relative tolerance of the next sweep                                          */
    double last_reach;           /* subspace reach the last update steered by (< 0: none)                               */
} feasthip_policy;
int    feasthip_policy_init(feasthip_policy* p, double Emin, double Emax, int ne, int quadrature, double inner_rtol,
                            double outer_tol, int solver_maxiter, int steer, int fpm18);
int    feasthip_policy_update(feasthip_policy* p, double epsout, int M, int any_node_capped, const double* ritz, int nritz);
int    feasthip_policy_set_aside(const double* res, int M, int* flags);
/* Which nodes feasthip_set_node_solver should make direct (host arithmetic only).  Nodes ordered by node_iters descending,
 * ties to the lower index; with the first k of them direct one further loop is predicted to take
 *   t_iter * max(node_iters of the others) + k * (t_solve + t_factor / max(loops_left, 1))   seconds
 * (t_iter: one Krylov iteration of the sweep, t_solve / t_factor: one node's substitution / factorisation).  Takes the
 * smallest k in 0..max_direct that minimises it, writes kinds[e] = FEASTHIP_SOLVER_BANDED for the chosen nodes and 0 for the
 * rest, returns k (0: the all-Krylov sweep is predicted fastest).                                                          */
int    feasthip_policy_pick_direct_nodes(const int* node_iters, int ne, int max_direct, double t_iter, double t_solve,
                                         double t_factor, int loops_left, int* kinds);
double feasthip_policy_filter_ratio(double Emin, double Emax, int ne, int quadrature, int fpm18, double reach,
                                    const double* inside, int n_inside);
double feasthip_policy_reach(const double* ritz, int n, double Emin, double Emax, double quantile);

/* ---- the hot path ------------------------------------------------------------------ */
/* One contour sweep over this handle's node range:
 *     for e in local nodes:  Y_e = (z_e B - A)^{-1} (B Q);   Qproj += weight_scale*w_e*Y_e
 *     optionally  zAq += weight_scale*w_e * Q^H Y_e,  zSq += weight_scale*w_e*z_e * Q^H Y_e
 * Q, Qproj: N x m c128 column-major (ldq = N), 1 <= m <= N; m > 64 is processed in 64-column
 * panels (this holds for every entry point below; zAq/zSq need m <= 64).  Qproj is OVERWRITTEN with this handle's
 * partial sum (callers reduce across handles/ranks: src/parallel/feast_parallel.jl:497-503,
 * src/parallel/feast_mpi.jl:117-119).  zAq/zSq: m x m c128 or NULL.
 * ritz_lambda: NULL => zero initial guess (reference behaviour, Krylov.jl gmres);
 *   else m doubles (real Ritz values paired with the columns of Q, as in
 *   Q_basis <- solutions of src/dense/feast_dense.jl:336-337): iterative solvers start
 *   from Y0[:,j] = Q[:,j]/(z_e - lambda_j).  Ignored by the LU solver.
 * node_status[e_local]: 0 ok, 5 not converged, 8 singular.  With a communicator attached node_status is
 *   GLOBAL: ne entries indexed by contour node (every rank receives the same vector).
 * Replaces: loop bodies src/dense/feast_dense.jl:171-232, src/sparse/feast_sparse.jl:318-370,
 * workers pfeast_solve_sparse_single_point (src/parallel/feast_parallel.jl:717-751) and
 * mpi_compute_local_moments (src/parallel/feast_mpi.jl:206-253).                          */
int  feasthip_contour_apply(feasthip_handle h, int64_t m, const void* Q, const double* ritz_lambda,
                            void* Qproj, void* zAq, void* zSq, int* node_status,
                            feasthip_stats* stats);
int  feasthip_contour_apply_dev(feasthip_handle h, int64_t m, const void* dQ,
                                const double* ritz_lambda_host, void* dQproj,
                                void* dzAq, void* dzSq, int* node_status, feasthip_stats* stats);

/* ---- stochastic estimate of the eigenvalue count (fpm[14] = 2) ------------------------------------------------------
 * The reference validates fpm[14] in {0,1,2} (src/core/feast_parameters.jl:69-75) and sets the estimate's defaults
 * fpm[2] = 3 (:108-110), fpm[8] = 6 (:166-168), fpm[15] = 1 (:223-225), but no kernel of it reads the parameter.
 * feasthip_estimate_count: ONE contour sweep (the sweep of feasthip_contour_apply_dev, zero initial guess) over m
 *   Rademacher columns V (entries +-1, generated on the device), then t_j = v_j^T Q_proj[:, j] for every column in one
 *   pass over Q_proj.  Q_proj = rho V with rho = sum_e weight_scale w_e (z_e B - A)^{-1} B (its real part under the real
 *   projection), so every t_j is an unbiased sample of tr rho = sum_i f(lambda_i), f the rational filter of the contour
 *   in force: mean(t) estimates the number of eigenvalues inside the contour (a sum of filter values, not an integer),
 *   std(t)/sqrt(m) its standard error.  Uses the problem, contour, real-projection flag, solver and node range set on the
 *   handle; with a communicator attached Q_proj is summed by the sweep's all-reduce before the dots, so every rank
 *   returns the same samples.  samples: 2*m doubles (re, im of t_j; im = 0 under the real projection).  node_status as
 *   in feasthip_contour_apply_dev (the samples are written whatever the statuses: the caller discards them when a node
 *   reports 5 or 8).  m > 64 runs in 64-column panels; 1 <= m <= min(N, 65535).
 * feasthip_random_block_dev: the N x m block V of feasthip_estimate_count for the same seed (c128, column-major, device).
 *   v_ij is a pure function of (seed, row i, column j) -- the splitmix64 finaliser mix64 applied twice:
 *   b = mix64(mix64(seed + 0x9E3779B97F4A7C15 (i + 1)) ^ 0xD1B54A32D192ED03 (j + 1)) mod 2^64, v_ij = 1 - 2 (b >> 63) --
 *   independent of the node range, the rank, the row renumbering of a sparse matrix and the launch geometry.         */
int  feasthip_estimate_count(feasthip_handle h, int64_t m, uint64_t seed, double* samples /* 2*m: t_j re,im */,
                             int* node_status, feasthip_stats* stats);
int  feasthip_random_block_dev(feasthip_handle h, int64_t m, uint64_t seed, void* dX /* N x m c128 col-major */);

/* ---- the refinement loop with resident panels ---------------------------------------------------------------------
 * One loop of variant A -- contour sweep, _feast_qr_compress!, the reduced pencil, Ritz vectors, residuals
 * (src/dense/feast_dense.jl:171-337, src/sparse/feast_sparse.jl:318-478) -- as three calls whose N x m blocks never
 * leave the device NOR the kernels' own layout between them (m <= 64, no moment matrices).  The per-primitive entry
 * points below compute the same quantities through column-major blocks at every call; a shim that does not need the
 * intermediate blocks on the host should prefer these.
 *
 * feasthip_contour_apply_resident: the sweep of feasthip_contour_apply_dev.  dQ != NULL: the N x m subspace (column
 *   major, device) is imported; dQ == NULL: the Ritz vectors left by the last feasthip_rr_ritz_resident are the subspace
 *   (m must be that call's r) and, when ritz_lambda equals that call's lambda, its residual panel A X - B X diag(lambda)
 *   starts the warm-started Krylov sweeps (one operator product saved).  Q_proj stays resident, summed over the ranks of
 *   an attached communicator (node_status as in feasthip_contour_apply_dev).
 * feasthip_rr_reduce_resident: *rank = numerical rank of the resident Q_proj under the reference's rule
 *   (src/core/feast_aux.jl:101-131); Aq and Bq receive the rank x rank pencil (Q_b^H A Q_b, Q_b^H B Q_b) (column-major, host;
 *   Hermitian parts when hermitize != 0, src/core/feast_aux.jl:84-92) of a basis Q_b of its range, to be handed to the
 *   generalized reduced eigensolver as the reference does (eigen(Hermitian(Sq), Hermitian(Aq)), src/dense/feast_dense.jl:272).
 *   Q_b is Q_proj with its columns scaled to unit length when that basis is well conditioned (the steady state of FEAST:
 *   the test is the one-pass condition of the Cholesky-QR, pivot ratio of the equilibrated Gram matrix > 1e-2) -- no
 *   orthonormal basis is formed, Bq is then the equilibrated Gram-type matrix, not I; otherwise Q_b is the orthonormal
 *   basis of the rank-revealing orthonormalisation (Bq = exactly I for B = I, src/dense/feast_dense.jl:255-259).
 * feasthip_rr_ritz_resident: X = Q_b V for the r = rank columns of V (r x r, host, column-major), the first M columns
 *   normalised when normalize != 0, res[j] = ||A x_j - lambda_j B x_j|| / max(|lambda_j|, 1) for j < M (use_B = 0: without
 *   B, the RCI kernels' residual); lambda: r complex values (2 r doubles).  X stays resident as the next sweep's subspace.
 *   May be called again with another V / M for the same reduction (spurious-pair reordering).
 * feasthip_resident_export: column-major copy (N x ncols, device) of the first ncols resident Ritz vectors (which = 0) or
 *   of the resident Q_proj (which = 1): the converged eigenvectors leave the device once per solve.
 * Replaces the bodies of src/dense/feast_dense.jl:234-337 and src/sparse/feast_sparse.jl:372-478 between two sweeps.      */
int  feasthip_contour_apply_resident(feasthip_handle h, int64_t m, const void* dQ, const double* ritz_lambda_host,
                                     int* node_status, feasthip_stats* stats);
int  feasthip_rr_reduce_resident(feasthip_handle h, int64_t m, double rank_tol, int hermitize, int* rank,
                                 void* Aq_host, void* Bq_host);
int  feasthip_rr_ritz_resident(feasthip_handle h, int64_t r, const void* V_host, const double* lambda_host, int64_t M,
                               int normalize, int use_B, double* res_host);
int  feasthip_resident_export(feasthip_handle h, int which, int64_t ncols, void* dX);
/* The counterpart: a column-major N x ncols device block becomes the resident subspace (which = 0: resume from a saved
 * subspace, the reference's fpm[5] = 1 start) or the resident Q_proj (which = 1: a projection computed elsewhere). */
int  feasthip_resident_import(feasthip_handle h, int which, int64_t ncols, const void* dX);

/* Rank-revealing orthonormalisation of Q[:, 0:m] in place.  Column-pivoted
 * Gram-Schmidt with re-orthogonalisation; rank = #{ |R_ii| > max(rank_tol, eps*max(N,m))*|R_11| },
 * the rule of _feast_qr_compress! (src/core/feast_aux.jl:101-131).  On return the first
 * `rank` columns of Q hold the orthonormal basis.                                         */
int  feasthip_orthonormalize(feasthip_handle h, int64_t m, void* Q, double rank_tol, int* rank);
int  feasthip_orthonormalize_dev(feasthip_handle h, int64_t m, void* dQ, double rank_tol, int* rank);

/* What a panel takes when the Cholesky-QR fast path rejects it as (nearly) rank deficient -- every refinement loop of an
 * exact solver, where Q_proj has more columns than eigenvalues inside the contour.  The rank rule is the same for both, that
 * of _feast_qr_compress! (src/core/feast_aux.jl:101-131).
 *   FEASTHIP_ORTHO_MGS        the column-pivoted Gram-Schmidt, one chain of launches per column (default)
 *   FEASTHIP_ORTHO_CHOLQR_RR  staged rank-revealing Cholesky-QR: a pivoted Cholesky of the Gram matrix decides the columns
 *                             whose pivots it still resolves, they are orthonormalised and projected out, the remainder is
 *                             judged by the next stage.  Falls back to the Gram-Schmidt on the untouched input when a Gram
 *                             matrix is not finite or the stage budget runs out.
 * Applies to feasthip_orthonormalize[_dev] and feasthip_rr_reduce_resident, at every width; the setting persists on the
 * handle.  Any other value: FEASTHIP_ERROR_FPM.  Full-rank panels take the fast path under either setting.                 */
enum {
    FEASTHIP_ORTHO_MGS = 0,
    FEASTHIP_ORTHO_CHOLQR_RR = 1,
    FEASTHIP_ORTHO_USED_CHOLQR = 2     /* reported by feasthip_last_ortho only: the Cholesky-QR fast path */
};
int  feasthip_set_ortho_method(feasthip_handle h, int method);
/* The last orthonormalisation on this handle: the path taken (one of the three values above), the stages the staged path
 * ran, whether it gave up and the Gram-Schmidt decided (fell_back), the rank, and the first n entries of the pivot order
 * (columns of the panel; -1 past the rank) and of |R_kk| (staged path only, else 0).  A call wider than 64 columns reports
 * sums over its 64-column panels, perm / rdiag of the last panel, and the staged path if any panel took it.  Any pointer
 * may be NULL.                                                                                                            */
int  feasthip_last_ortho(feasthip_handle h, int* method_used, int* stages, int* fell_back, int* rank, int* perm,
                         double* rdiag, int n);

/* Rayleigh-Ritz projection: Aq = herm(Q^H A Q), Bq = herm(Q^H B Q) (Bq = I when
 * B is the identity).  bilinear=1 uses Q^T (complex-symmetric siblings) and skips the
 * Hermitian symmetrisation.  hermitize=0 returns the raw products, Bq = Q^H Q for B = I (variant C,
 * src/kernel/feast_kernel.jl:790,805).  Replaces src/dense/feast_dense.jl:252-265,
 * src/sparse/feast_sparse.jl:392-405.  Aq, Bq: r x r c128 column-major HOST buffers.       */
int  feasthip_project(feasthip_handle h, int64_t r, const void* Q, int bilinear, int hermitize,
                      void* Aq, void* Bq);
int  feasthip_project_dev(feasthip_handle h, int64_t r, const void* dQ, int bilinear, int hermitize,
                          void* Aq_host, void* Bq_host);

/* Ritz back-transform + residuals (SURVEY a12,a13):  X = Q*V (N x r), optional column
 * normalisation of the first M columns, then res_j = ||A x_j - lambda_j B x_j||_2 / max(|lambda_j|,1)
 * for j < M (use_B=0 drops B as the RCI kernels do, src/kernel/feast_kernel.jl:899-906).
 * V: r x r c128 column-major host; lambda: r c128 host (re,im).
 * Replaces src/dense/feast_dense.jl:287-322, src/core/feast_tools.jl:726-755.              */
int  feasthip_ritz_residual(feasthip_handle h, int64_t r, const void* Q, const void* V,
                            const double* lambda, int64_t M, int normalize, int use_B,
                            void* X, double* res);
int  feasthip_ritz_residual_dev(feasthip_handle h, int64_t r, const void* dQ, const void* V_host,
                                const double* lambda_host, int64_t M, int normalize, int use_B,
                                void* dX, double* res_host);

/* ---- two-sided FEAST: the adjoint switch and the oblique projection ---------------------------------------------------
 * FEAST's fpm[15] selects a two-sided or a one-sided contour; the reference validates the slot and never reads it
 * (src/core/feast_parameters.jl:217-225), so nothing here has a counterpart there.
 * feasthip_set_adjoint: persistent on the handle, off by default.  While it is on
 *   feasthip_contour_apply[_dev]   Y_e = (z_e B - A)^{-H} (B^H Q),  Qproj = sum_e weight_scale conj(w_e) Y_e  (node range, node
 *                                  list, node_status as in the forward sweep, weights by global node); zAq / zSq must be NULL;
 *   feasthip_shifted_solve[_dev]   Y = (z B - A)^{-H} X;
 *   feasthip_matmul[_dev]          Y = op^H X;
 *   feasthip_ritz_residual[_dev]   X = Q V,  res_j = ||A^H x_j - conj(lambda_j) B^H x_j|| / max(|lambda_j|, 1)  (use_B = 0 omits
 *                                  B^H as the forward form omits B).
 *   The solves are conjugate-transposed substitutions (ZGETRS 'C') on the LU factors the forward solves cache, matched by z_e
 *   in the same slots: an adjoint sweep after a forward sweep on the same contour reports stats.factorizations == 0.
 *   A dense problem needs FEASTHIP_SOLVER_LU.  A CSR problem needs FEASTHIP_SOLVER_BANDED with the MULTIFRONTAL direct plan
 *   (feasthip_band_plan: blocked == 2) or the BLOCKED BAND LU (blocked == 1).  Multifrontal: the substitution walks the front
 *   tree conjugate-transposed (U^H leaves first, L^H and the fronts' row permutations root first).  Blocked band LU: ZGBTRS 'C'
 *   on the band factors -- U^H block by block ascending, then per block descending L^H (left-looking) and the block's row
 *   interchanges undone in reverse order; gather and scatter by the band order as in the forward solve.  The products run on a
 *   conjugate-transposed copy of the CSR set, built at the first adjoint product (one device-to-host copy of the values) and
 *   kept until the problem changes.
 *   While it is on, FEASTHIP_ERROR_FPM (feasthip_last_error names the reason, nothing is computed) answers: FEASTHIP_SOLVER_LU on
 *   a CSR problem, the Krylov solvers, the narrow band plan (plan 1; the message names it), feasthip_set_node_solver kinds,
 *   factor_precision = 32, the real projection, a non-NULL moment matrix, an attached communicator, the resident entry points,
 *   feasthip_estimate_count and feasthip_rayleigh_ritz_dev.
 *   Every other entry point is unaffected: feasthip_project[_dev] and feasthip_project_pair[_dev] always apply A and B
 *   themselves, feasthip_orthonormalize[_dev] applies no operator.
 * feasthip_project_pair[_dev]: the raw products Aq = Q_L^H A Q_R and Bq = Q_L^H B Q_R (Q_L^H Q_R for B = I) of two N x r
 *   blocks (c128 column-major; r > 64 in 64-column panels); Aq, Bq: r x r c128 column-major HOST buffers, Bq may be NULL.
 *   Independent of the adjoint switch.
 * feasthip_require_adjoint: persistent on the handle, off by default; a capability the driver declares, not a tuning switch.
 *   While it is on, the direct plan of a CSR problem is the multifrontal one whenever one can be made (as FH_MF=1 does), because
 *   the narrow band plan has no adjoint substitution: a cached plan of another kind for the same matrix that was not made under
 *   the requirement is dropped with its factors when the plan is next needed.  A pivot rejection falls back to the blocked band
 *   LU as it does without the requirement, and a pattern with no multifrontal plan (a front beyond 16 384 rows) takes the
 *   blocked band LU from the start; such a band plan is kept while the requirement stays on (no re-planning, the cached
 *   factors serve both directions).  Set it before the first plan query or solve.  A plan made while it was on is dropped in
 *   turn, with its factors, when the plan is next needed with the requirement off: calls that never asked for an adjoint keep
 *   the plan and the results they had.  No effect on dense problems.                                                        */
int  feasthip_set_adjoint(feasthip_handle h, int on);
int  feasthip_require_adjoint(feasthip_handle h, int on);
int  feasthip_project_pair(feasthip_handle h, int64_t r, const void* QL, const void* QR, void* Aq, void* Bq);
int  feasthip_project_pair_dev(feasthip_handle h, int64_t r, const void* dQL, const void* dQR, void* Aq_host, void* Bq_host);

/* ---- RCI / matrix-free seams -------------------------------------- */
/* Rayleigh-Ritz step with the reduced eigenproblem on the device:
 * feasthip_project, then the Hermitian-definite r x r pencil is solved by a Jacobi eigensolver in LDS
 * (instead of eigen(Hermitian(Sq), Hermitian(Aq)), src/dense/feast_dense.jl:272), stable inside-first
 * reorder for [Emin, Emax] (src/core/feast_aux.jl:144-197), then feasthip_ritz_residual.  r <= 64.
 * Out: X (N x r device), lambda[r] (reordered, inside first), *M, res[M].  Returns 8 when the reduced
 * B matrix is not positive definite (use project + a host general eigensolver + ritz_residual then,
 * the fallback of src/dense/feast_dense.jl:276-284).                                            */
int  feasthip_rayleigh_ritz_dev(feasthip_handle h, int64_t r, const void* dQ, double Emin, double Emax,
                                int use_B, void* dX, double* lambda_out, int* M_out, double* res_out);

/* Y = op * X for op = A (which=0) or B (which=1): RCI jobs 30 / 40
 * (src/core/feast_types.jl:227-249; callers src/dense/feast_dense.jl:561-573).          */
int  feasthip_matmul(feasthip_handle h, int which, int64_t m, const void* X, void* Y);
int  feasthip_matmul_dev(feasthip_handle h, int which, int64_t m, const void* dX, void* dY);

/* Y = (z B - A)^{-1} X, all m columns: RCI jobs 10+11 and the matrix-free
 * linear_solver(Y, z, X) callback contract (src/interfaces/feast_matfree.jl:149, 697).
 * Unlike contour_apply the right-hand side is X itself (the caller applies B).          */
int  feasthip_shifted_solve(feasthip_handle h, double z_re, double z_im, int64_t m,
                            const void* X, void* Y, feasthip_stats* stats);
int  feasthip_shifted_solve_dev(feasthip_handle h, double z_re, double z_im, int64_t m,
                                const void* dX, void* dY, feasthip_stats* stats);

/* ---- polynomial eigenproblems: P(lambda) x = 0, P(lambda) = A_0 + lambda A_1 + ... + lambda^d A_d ------------------------
 * The reference's feast_pep! builds the dN x dN first companion form (src/dense/feast_dense.jl:745-760)
 *     A_lin = [0 I . ; . . I ; -A_0 ... -A_{d-1}],   B_lin = diag(I, ..., I, A_d)
 * and hands it to feast_gegv! (:763), one LU of order dN per node.  Here the companion matrix is never formed: a node costs one
 * LU of P(z_e), order N (d^3 times fewer flops, d^2 times less factor memory), and the linearised vectors exist only as the
 * dN x m blocks the caller sees.  Device blocks are column-major complex128 like the other _dev entry points; block i of a
 * column is its rows i N .. (i + 1) N - 1.  m > 64 runs in 64-column panels.
 * feasthip_set_polynomial: dense coefficients A_0 .. A_degree (host, column-major, ld[k] >= N; all double or all interleaved
 *   complex128), 1 <= degree <= FEASTHIP_POLY_MAX_DEGREE.  Replaces the coeffs argument of feast_pep!
 *   (src/dense/feast_dense.jl:715-744) and of feast_gepev! / feast_hepev! / feast_sypev! (:946-979).  The handle becomes a
 *   POLYNOMIAL handle: feasthip_set_contour, feasthip_set_solver (FEASTHIP_SOLVER_LU with factor_precision 64 only; a CSR
 *   polynomial handle also takes the Krylov solvers, see "Krylov solvers on P(z)" below),
 *   feasthip_release_factors, the stream and the profile calls work on it; every other entry point above returns
 *   FEASTHIP_ERROR_FPM and names the feasthip_poly_* calls (feasthip_set_adjoint(1), a node range or list, a communicator and
 *   factor_precision 32 included: a polynomial sweep is one rank, forward, fp64).  feasthip_set_dense / feasthip_set_csr
 *   restore an ordinary handle.  A feasthip_poly_* call on any other handle returns FEASTHIP_ERROR_FPM.
 * feasthip_set_polynomial_csr: the same handle for SPARSE coefficients, the counterpart of the reference's sparse polynomial
 *   family feast_scsrpev! / feast_hcsrpev! / feast_gcsrpev! (src/sparse/feast_sparse.jl), which runs feast on the explicit
 *   sparse dN x dN companion.  The degree + 1 coefficients share ONE CSR pattern (host arrays, 0-based: rowptr N + 1 entries
 *   starting at 0 and monotone, col in 0 .. N - 1 and strictly increasing inside a row -- anything else is FEASTHIP_ERROR_N);
 *   vals[k] holds the nnz = rowptr[N] values of A_k on that pattern, explicit zeros where A_k has no entry (all double or all
 *   interleaved complex128).  The pattern should hold the whole diagonal (the multifrontal LU pivots there).  Every
 *   feasthip_poly_* call below works on such a handle with the same meaning, and everything a polynomial handle refuses stays
 *   refused.  P(z_e) is factored by the multifrontal LU of the sparse direct solver -- always: FH_MF / FH_WBAND do not apply,
 *   FH_MF_LEAF does -- with its per-node factor cache; feasthip_direct_plan_flops / feasthip_direct_plan_bytes /
 *   feasthip_band_plan describe the plan.  There is NO band LU behind it: a pattern without a multifrontal plan (a front beyond
 *   16 384 rows) makes those calls and every solve return FEASTHIP_ERROR_FPM, and a factorisation whose pivots the multifrontal
 *   LU rejects (zero pivot, or a boundary multiplier beyond the bound: it pivots only inside a front's fully-summed block)
 *   makes the solve or sweep return FEASTHIP_ERROR_LAPACK with nothing computed; feasthip_last_error names the cause and the
 *   sizes.  Factors that do not fit the device: FEASTHIP_ERROR_MEMORY.
 *   Krylov solvers on P(z): feasthip_set_solver also accepts FEASTHIP_SOLVER_BICGSTAB, _COCG (every coefficient symmetric,
 *   A_k == A_k^T, real or complex: the caller's promise) and _GMRES on a CSR polynomial handle, factor_precision 64.  Then
 *   feasthip_poly_solve_dev and feasthip_poly_resinv_apply_dev solve with the batched Krylov drivers on the operator P(z_e)
 *   (formed per nonzero by Horner, never stored): zero start, no preconditioner, the handle's rtol / atol / maxit / restart, no
 *   factors (stats.factorizations = 0).  stats.krylov_iterations, stats.spmm_calls, feasthip_last_node_iterations and
 *   feasthip_last_column_iterations report as for a pencil; a node with a column that stopped at maxit has status
 *   FEASTHIP_ERROR_NO_CONVERGENCE (5), its iterate is still used.  feasthip_poly_contour_apply_dev returns FEASTHIP_ERROR_FPM
 *   under a Krylov solver (one right-hand side per node: use the projected method).  A dense polynomial handle refuses them.
 * feasthip_poly_solve_dev: Y = P(z)^-1 R, N x m (the shifted solve inside the companion elimination; no reference
 *   counterpart).  Factors are cached per contour node and matched by z, as in feasthip_shifted_solve.  Returns 0 or 8
 *   (Krylov solver: 0 or 5).
 * feasthip_poly_contour_apply_dev: Qproj = sum_e weight_scale w_e (z_e B_lin - A_lin)^-1 (B_lin Q), dN x m: the loop body
 *   of feast_grci! as feast_gegv! drives it on the companion pencil (src/dense/feast_dense.jl:468-584).  node_status[e]: 0 or 8,
 *   ne entries.  stats.factorizations counts the N x N factorisations of the call (0 on a repeated contour).
 * feasthip_poly_matmul_dev: Y = A_lin X (which 0) or B_lin X (which 1), dN x m (RCI jobs 30 / 40 on the companion pencil).
 *   which 2, 3, 4 (CSR coefficients, a contour of ne nodes, m <= 64): the operator of the Krylov solvers as a product of its
 *   own.  X and Y hold ne blocks of N x m one behind the other;  2: Y_e = P(z_e) X_e;  3: Y_e = B - P(z_e) X_e with B = block 0
 *   of Y on entry;  4: Y_e = B_e - P(z_e) X_e with B_e = block e of Y on entry.
 * feasthip_poly_project_dev: the raw products Aq = Q^H A_lin Q and Sq = Q^H B_lin Q (src/kernel/feast_kernel.jl:790, 805),
 *   r x r column-major host buffers.
 * feasthip_poly_ritz_residual_dev: X = Q V (dN x r; V r x r column-major, host), the first M columns scaled to unit length
 *   when normalize != 0 (src/kernel/feast_kernel.jl:864-876); for j < M
 *     res[j]            = ||A_lin x_j - lambda_j B_lin x_j||_2 / max(|lambda_j|, 1)  (use_B = 0 omits B_lin, as the reference
 *                         does, src/kernel/feast_kernel.jl:899-906: for A_d != I that measure does not fall),
 *     backward_error[j] = ||P(lambda_j) x_j||_2 / (sum_k |lambda_j|^k ||A_k||_F ||x_j||_2),  x_j the first block of column j
 *   (no reference counterpart).  lambda: r complex values; res, backward_error: M doubles each, either may be NULL; X must
 *   not alias Q.                                                                                                        */
#define FEASTHIP_POLY_MAX_DEGREE 8
int  feasthip_set_polynomial(feasthip_handle h, int64_t N, int degree, int is_complex,
                             const void* const* coeffs /* degree + 1, column-major */, const int64_t* ld);
int  feasthip_set_polynomial_csr(feasthip_handle h, int64_t N, int degree, int is_complex, const int64_t* rowptr,
                                 const int64_t* col, const void* const* vals /* degree + 1 arrays of rowptr[N] values */);
int  feasthip_poly_solve_dev(feasthip_handle h, double z_re, double z_im, int64_t m, const void* dR, void* dY, feasthip_stats* stats);
int  feasthip_poly_contour_apply_dev(feasthip_handle h, int64_t m, const void* dQ, void* dQproj, int* node_status,
                                     feasthip_stats* stats);
int  feasthip_poly_matmul_dev(feasthip_handle h, int which /* 0 A_lin, 1 B_lin, 2 .. 4 node products */, int64_t m, const void* dX, void* dY);
int  feasthip_poly_project_dev(feasthip_handle h, int64_t r, const void* dQ, void* Aq_host, void* Sq_host);
int  feasthip_poly_ritz_residual_dev(feasthip_handle h, int64_t r, const void* dQ, const void* V_host, const void* lambda, int64_t M,
                                     int normalize, int use_B, void* dX, double* res, double* backward_error);

/* ---- polynomial eigenproblems, projected method: the subspace is N x m, the small r x r polynomial is linearised on the host --
 * (polynomial FEAST with a residual-inverse contour step, Gavin, Miedlar, Polizzi; no reference counterpart).  Every call works
 * on dense and sparse polynomial handles, refuses what the calls above refuse, and takes any m >= 1 in 64-column panels.
 * feasthip_poly_eval_cols_dev: R[:, j] = P(lambda_j) X[:, j], N x m; lambda: m complex values on the host.
 * feasthip_poly_resinv_apply_dev: the contour step.  sigma == NULL: Q = sum_e weight_scale w_e P(z_e)^-1 X (plain sweep).
 *   Otherwise, with sigma: m complex shifts on the host,
 *     R[:, j] = P(sigma_j) x_j,  Y_e = P(z_e)^-1 R,  Q[:, j] = sum_e weight_scale w_e (x_j - Y_e[:, j]) / (z_e - sigma_j).
 *   Factors come from the per-node cache (stats.factorizations as in feasthip_poly_contour_apply_dev); node_status[e]: 0 or 8
 *   (Krylov solver: 0 or 5, and the sums use the iterates the capped nodes stopped with).
 *   A shift that is not finite or that coincides with a contour node to working precision: FEASTHIP_ERROR_FPM.
 * feasthip_poly_project_reduced_dev: Ahat_k = Q^H A_k Q, k = 0 .. degree, for an N x r block Q; Ahat_host: degree + 1 r x r
 *   column-major matrices one behind the other.
 * feasthip_poly_ritz_eval_dev: X = Q Y (Y: r x ncand column-major, host) with every column scaled to unit length, and
 *     backward_error[i] = ||P(theta_i) x_i||_2 / sum_k |theta_i|^k ||A_k||_F      (||A_k||_F from ingest)
 *   for i < ncand; +inf for a theta_i that is not finite and for a column of zero length.  backward_error may be NULL (then
 *   theta may be too).  X must not alias Q.
 * feasthip_poly_orthonormalize_dev: feasthip_orthonormalize_dev (method of feasthip_set_ortho_method, report through
 *   feasthip_last_ortho) for the N x m block of a polynomial handle, which feasthip_orthonormalize_dev itself refuses like every
 *   pencil entry point; unit_columns != 0 scales every column to unit length first.                                    */
int  feasthip_poly_eval_cols_dev(feasthip_handle h, int64_t m, const void* lambda, const void* dX, void* dR);
int  feasthip_poly_resinv_apply_dev(feasthip_handle h, int64_t m, const void* sigma /* host, or NULL */, const void* dX, void* dQ,
                                    int* node_status, feasthip_stats* stats);
int  feasthip_poly_project_reduced_dev(feasthip_handle h, int64_t r, const void* dQ, void* Ahat_host);
int  feasthip_poly_ritz_eval_dev(feasthip_handle h, int64_t r, const void* dQ, int64_t ncand, const void* Y_host, const void* theta,
                                 void* dX, double* backward_error);
int  feasthip_poly_orthonormalize_dev(feasthip_handle h, int64_t m, void* dQ, int unit_columns, double rank_tol, int* rank);

/* ---- nonlinear eigenproblems in split form: T(lambda) x = 0, T(lambda) = sum_{k < nterms} f_k(lambda) A_k ----------------------
 * The f_k are scalar functions that only the caller evaluates: the library never sees them, it takes tables of their values.
 * A TERM HANDLE is a polynomial handle whose scalars come from such tables instead of the powers of lambda; it keeps the
 * storage, the per-node factor cache, the dense / multifrontal LU of the solver FEASTHIP_SOLVER_LU and the restrictions of a
 * polynomial handle (complex128 factors, one rank, the whole contour, no adjoint).  (No reference counterpart.)
 * feasthip_set_terms / feasthip_set_terms_csr: the arguments and checks of feasthip_set_polynomial / _csr with nterms = 2 ..
 *   FEASTHIP_POLY_MAX_DEGREE + 1 matrices A_k in place of the degree + 1 coefficients; ||A_k||_F is kept for the backward error.
 * feasthip_nep_set_node_values: F_host[e * nterms + k] = f_k(z_e) for the contour set before (feasthip_set_contour; set the
 *   values again after every new contour).  ne other than the contour's node count, or a value that is not finite:
 *   FEASTHIP_ERROR_FPM.  Values that differ from the ones set before drop the cached factors.
 * feasthip_nep_solve_dev: Y = T(z_e)^-1 R for the contour node index `node`, N x m column-major; the factor is cached in the
 *   node's slot; returns 0 or 8 (T(z_e) singular to working precision).
 * feasthip_nep_eval_cols_dev: R[:, j] = sum_k F[j * nterms + k] A_k X[:, j], N x m; F: m x nterms on the host.
 * feasthip_nep_resinv_apply_dev: the contour step of feasthip_poly_resinv_apply_dev with T in place of P.  sigma and F_sigma
 *   both NULL: the plain sweep Q = sum_e weight_scale w_e T(z_e)^-1 X.  Both given (sigma: m shifts, F_sigma[j * nterms + k] =
 *   f_k(sigma_j), host):  R[:, j] = sum_k F_sigma[j][k] A_k x_j,  Y_e = T(z_e)^-1 R,
 *   Q[:, j] = sum_e weight_scale w_e (x_j - Y_e[:, j]) / (z_e - sigma_j).  One of the two NULL, a shift or a table row that is
 *   not finite, a shift that coincides with a contour node to working precision: FEASTHIP_ERROR_FPM.  node_status and stats as
 *   in feasthip_poly_resinv_apply_dev.
 * feasthip_nep_ritz_eval_dev: X = Q Y (Y: r x ncand column-major, host) with unit columns, and
 *     backward_error[i] = ||sum_k F_theta[i][k] A_k x_i||_2 / sum_k |F_theta[i][k]| ||A_k||_F,   F_theta: ncand x nterms, host;
 *   +inf for a row of the table that is not finite and for a column of zero length.  backward_error may be NULL (then F_theta
 *   may be too).  X must not alias Q.
 * feasthip_poly_project_reduced_dev (Ahat_k = Q^H A_k Q, k < nterms) and feasthip_poly_orthonormalize_dev take a term handle
 * as they are.  Every other feasthip_poly_* call forms powers of lambda and returns FEASTHIP_ERROR_FPM on a term handle
 * (feasthip_last_error names the call to use instead), as does feasthip_set_solver with any solver but FEASTHIP_SOLVER_LU;
 * the pencil entry points refuse a term handle as they refuse a polynomial handle.  All calls take any m >= 1 in 64-column
 * panels.                                                                                                              */
int  feasthip_set_terms(feasthip_handle h, int64_t N, int nterms, int is_complex, const void* const* mats /* nterms pointers */,
                        const int64_t* ld /* nterms leading dimensions */);
int  feasthip_set_terms_csr(feasthip_handle h, int64_t N, int nterms, int is_complex, const int64_t* rowptr, const int64_t* col,
                            const void* const* vals /* nterms arrays of rowptr[N] values */);
int  feasthip_nep_set_node_values(feasthip_handle h, int ne, const void* F_host /* ne x nterms complex */);
int  feasthip_nep_solve_dev(feasthip_handle h, int node, int64_t m, const void* dR, void* dY, feasthip_stats* stats);
int  feasthip_nep_eval_cols_dev(feasthip_handle h, int64_t m, const void* F_host /* m x nterms */, const void* dX, void* dR);
int  feasthip_nep_resinv_apply_dev(feasthip_handle h, int64_t m, const void* sigma /* host, or NULL */,
                                   const void* F_sigma /* host m x nterms, or NULL */, const void* dX, void* dQ, int* node_status,
                                   feasthip_stats* stats);
int  feasthip_nep_ritz_eval_dev(feasthip_handle h, int64_t r, const void* dQ, int64_t ncand, const void* Y_host, const void* F_theta,
                                void* dX, double* backward_error);

/* ---- stochastic estimate of the eigenvalue count of a polynomial or term handle (fpm[14] = 2 of feast_polynomial / feast_nonlinear) --
 * For a regular T the number of eigenvalues inside the contour is (1 / 2 pi i) oint tr(T(z)^-1 T'(z)) dz, with the handle's
 * quadrature sum_e w_e tr(T'(z_e) T(z_e)^-1); for T = z B - A that is the trace feasthip_estimate_count samples.
 * feasthip_poly_estimate_count: t_c = v_c^T [sum_e weight_scale w_e T'(z_e) T(z_e)^-1 v_c] for the m Rademacher columns of `seed`
 *   (the (seed, i, j) rule of feasthip_random_block_dev), so mean(t) estimates the count (a sum of filter values counted with
 *   algebraic multiplicity, not an integer) and std(t) / sqrt(m) its standard error.  T'(z) = sum_k g_k(z) A_k is given by the
 *   host table G_host[e * (degree + 1) + k] = weight_scale w_e g_k(z_e) -- g_k(z) = k z^(k-1) for a polynomial handle, f_k' for a term
 *   handle (nterms = degree + 1 columns) -- and a term whose column is zero at every node is left out of the work.  A value of G
 *   that is not finite: FEASTHIP_ERROR_FPM, feasthip_last_error names the node and the term.  Serves a polynomial handle and a
 *   term handle (which needs the node values of the current contour, feasthip_nep_set_node_values) under every solver the handle
 *   takes; FEASTHIP_SOLVER_LU factors through the per-node cache, so a following sweep on the same contour factors nothing
 *   (stats.factorizations counts what this call factored; the Krylov counts as in feasthip_poly_resinv_apply_dev).
 *   samples: 2 * m doubles (re, im of t_c), written whatever the statuses; node_status[e]: 0, 5 or 8 as in
 *   feasthip_poly_resinv_apply_dev.  dV (may be NULL): receives the block V the samples were taken with, N x m c128
 *   column-major on the device (feasthip_random_block_dev itself refuses a polynomial handle).  m > 64 runs in 64-column
 *   panels; 1 <= m <= min(N, 65535), else FEASTHIP_ERROR_M0.  The result is reproducible bit for bit.
 *   feasthip_estimate_count keeps refusing a polynomial handle.                                                          */
int  feasthip_poly_estimate_count(feasthip_handle h, int64_t m, uint64_t seed,
                                  const void* G_host /* ne x (degree+1) c128, row e = w_e g_k(z_e) */,
                                  double* samples /* 2*m: t_c re, im */, void* dV /* N x m c128 col-major, may be NULL */,
                                  int* node_status, feasthip_stats* stats);

/* ---- measurement support ---------------------------------------------------------- */
/* Average device time (ms, HIP events on the handle's stream) and launch count of the
 * named kernel class since the last reset; classes: "spmm", "bicg_update", "dot_finalize",
 * "lu_panel", "lu_gemm", "trsm", "gram", "ortho".  Used by bench.py's roofline object.     */
/* Per local node: iterations of the slowest column in the last iterative sweep. */
int  feasthip_last_node_iterations(feasthip_handle h, int* out, int n);
/* With a communicator: Krylov iterations of the last sweep per CONTOUR node (ne entries), summed over the ranks that
 * worked on the node (they travel in the tail of the packed all-reduce).  Identical on every rank, so hosts can
 * re-balance the node lists between refinement loops deterministically (nodes next to the real axis need 10x the
 * iterations of the others).                                                                              */
int  feasthip_last_global_node_iterations(feasthip_handle h, int* out, int n);
/* Whether the last feasthip_contour_apply[_resident] took the shifted COCG sweep (FEASTHIP_SOLVER_SHIFTED_COCG and an
 * eligible problem) on this rank, and what it cost: the seed's contour node, the iterations of the seed recurrence (one
 * operator product each; the last one may only find every node converged) and the SpMM node-passes of the sweep -- the
 * seed's alone, where the solve loop over the nodes (src/sparse/feast_sparse.jl:318-369, :164-203) makes one per node and
 * iteration.  Sums over the 64-column panels of a wide sweep.  used = 0: seed_node = -1, the counts are 0.  Any pointer
 * may be null.                                                                                              */
int  feasthip_last_shifted_sweep(feasthip_handle h, int* used, int* seed_node, int* seed_iterations, int* spmm_node_passes);
/* Whether the last feasthip_contour_apply[_resident] took the block COCG sweep (FEASTHIP_SOLVER_BLOCK_COCG and an eligible
 * problem) on this rank, and what it cost: the most block steps any node took (steps that ran on the device, not steps
 * queued), the nodes whose block broke down and were finished by the per-column sweep (a normal outcome, never an error
 * status), and the operator node-passes that ran (one per node and block step, plus those of the fallbacks).  Sums over the
 * 64-column panels of a wide sweep (node_steps_max: the maximum).  used = 0: the counts are 0.  Any pointer may be null. */
int  feasthip_last_block_sweep(feasthip_handle h, int* used, int* node_steps_max, int* breakdown_nodes, int* spmm_node_passes);
/* [local node][m] iterations per column of the last iterative sweep (row-major, n entries). */
int  feasthip_last_column_iterations(feasthip_handle h, int* out, int n);
int  feasthip_profile_enable(feasthip_handle h, int enable);
int  feasthip_profile_reset(feasthip_handle h);
int  feasthip_profile_get(feasthip_handle h, const char* kernel_class, double* total_ms,
                          int64_t* launches);
/* Sampling period of the event timing: 0 = default (1 launch in 13), 1 = every launch (classes with few, very
 * different launches: the dense LU).  feasthip_profile_get_work: algorithmic flops issued by a dense MFMA class
 * ("lu_gemm", "lu_gemm_in") since the last reset, for the MFMA roofline of bench.py.                        */
int  feasthip_profile_set_period(feasthip_handle h, int period);
int  feasthip_profile_get_work(feasthip_handle h, const char* kernel_class, double* work);

#ifdef __cplusplus
}
#endif
#endif /* FEASTHIP_H */
