// fh_krylov.hpp -- the batched Krylov drivers of fh_api.hip for the other .hip units, and the operators that fh_apply_operator
// launches for a sparse polynomial handle (fh_poly.hip) and for an operator handle (fh_operator.hip).
#pragma once
#include "fh_common.hpp"
#include <vector>

// What a batched solve reports (filled by fh_collect_columns)
struct fh_solve_result {
    std::vector<int> node_iters, col_iters;
    int64_t iters_sum = 0;      // sum over nodes of max column iterations
    int64_t op_calls = 0;
    int max_iters = 0;
    std::vector<int> status;    // per node
    double max_rel_res = 0.0;
};

// The optional parts of a fh_krylov call; default-constructed: a plain solve from the guess in X.
// sum_acc and wnode (COCG only): "sum mode" -- X keeps the initial guess, every step alpha p of every node is added, weighted
// with wnode[e], to the N x ld accumulator sum_acc (zeroed by the caller): sum_e w_e X_e(final) = sum_e w_e X_e(initial) + sum_acc.
// shared_src (sum mode, prec 64): the initial residual of every node is  f_node,c * shared_src  with f = 1/(z_node -
// shared_lambda[c]) (Ritz warm start: the values on the device and on the host, dznode: the nodes on the device) or 1 (no
// shared_lambda: zero guess, the source is RHS).  X and RHS are then never read: no warm-start panels, no residual product.
struct fh_krylov_opts {
    cplx* sum_acc = nullptr;
    const std::vector<cplx>* wnode = nullptr;
    const cplx *shared_src = nullptr, *dznode = nullptr;
    const double *shared_lambda = nullptr, *shared_lambda_host = nullptr;
};

// S_e X_e = RHS for e in [0, nodes), S_e = z_e B - A of a pencil handle or P(z_e) of a sparse polynomial handle; one
// right-hand-side panel shared by the nodes, X (`stride` = N ld elements apart) holds the guess on entry.  The handle's rtol,
// atol, maxit (and restart) apply.  fh_krylov: BiCGStab (method 0) or COCG (method 1); fh_gmres: restarted GMRES.
int fh_krylov(feasthip_ctx* h, int method, int prec, int ld, int m, int nodes, const std::vector<cplx>& z, const cplx* RHS,
              cplx* X, size_t stride, fh_solve_result& res, const fh_krylov_opts& opt);
// Shift preconditioner of a fh_gmres call (feasthip_set_preconditioner): node e runs in the variable u = M_e x with
// M_e = zp[e] B - A, whose factors sit in slot[e] of the band / multifrontal cache (fh_banded_precond_factor).  zero_guess: X
// holds zeros (u0 = M x0 is not formed).  sweeps: substitution sweeps the call made (out).
struct fh_gmres_precond {
    std::vector<int> slot;
    std::vector<cplx> zp;
    bool zero_guess = false;
    int64_t sweeps = 0;
};
int fh_gmres(feasthip_ctx* h, int ld, int m, int nodes_all, const std::vector<cplx>& z, const cplx* RHS, cplx* X, size_t stride,
             fh_solve_result& res, fh_gmres_precond* pc = nullptr);

// Y_e = [Bvec -] P(z_e) X_e on a sparse polynomial handle (fh_poly.hip: k_spmm_poly), complex128 panels; the fields are those
// of fh_spmm_args.  z_e = znode[e * z_stride].  Returns the partial-sum rows per node it wrote (fh_poly_op_nblk).
struct fh_polyop_call {
    const cplx* X; size_t x_node_stride;
    cplx* Y; size_t y_node_stride;
    const cplx* znode; int z_stride;
    const cplx* Bvec; size_t b_node_stride;
    const cplx* U; size_t u_node_stride;
    int dot_mode; cplx* partial1; cplx* partial2;     // modes 0 .. 4 of fh_sparse.hip
    const int* node_active;
    int nodes, m;
};
int fh_poly_op_nblk(int N, int ld);
int fh_launch_spmm_poly(feasthip_ctx* h, int ld, const fh_polyop_call& c);

// Y_e = [Bvec -] (coefB[e] B X_e + coefA[e] A X_e) on an operator handle (fh_operator.hip): the caller's callback forms A X
// and B X for all nodes, k_op_combine does the rest; complex128 panels, the fields are those of fh_spmm_args.  skip: what the
// host knows about the coefficients -- bit 0: coefA is zero everywhere, bit 1: coefB is -- so that the unused callback is not
// made.  Returns the partial-sum rows per node it wrote (fh_op_combine_nblk), or -1 with last_error set: a failed callback
// (h->op.failed is then set and every later call returns -1 at once) or a workspace that could not be had.
struct fh_userop_call {
    const cplx* X; size_t x_node_stride;
    cplx* Y; size_t y_node_stride;
    const cplx* coefA; const cplx* coefB;             // [nodes][ld]
    const cplx* Bvec; size_t b_node_stride;
    const cplx* U; size_t u_node_stride;
    int dot_mode; cplx* partial1; cplx* partial2;     // modes 0 .. 4 of fh_sparse.hip
    const int* node_active;
    int nodes, skip;
};
int fh_op_combine_nblk(int N, int ld);
int fh_apply_user_operator(feasthip_ctx* h, int ld, const fh_userop_call& c);

// Y_e = [Bvec -] sum_k F(e, c, k) A_k X_e on a term-operator handle (fh_termop.hip): the caller's callback forms A_k X for the
// kept terms, k_terms_combine does the rest; complex128 panels, the fields are those of fh_userop_call.  F: the DEVICE table --
// cols = 0: the node table F[e * nt + k] (nt = the handle's term count), uniform over the columns; cols = 1 (nodes = 1): the
// column table F[k * ld + c].  terms: bit k set when term k has a non-zero entry in the table; the others are neither produced
// nor read.  Returns the partial-sum rows per node it wrote (fh_op_combine_nblk), or -1 as fh_apply_user_operator does.
struct fh_termop_call {
    const cplx* X; size_t x_node_stride;
    cplx* Y; size_t y_node_stride;
    const cplx* F; int cols; unsigned terms;
    const cplx* Bvec; size_t b_node_stride;
    const cplx* U; size_t u_node_stride;
    int dot_mode; cplx* partial1; cplx* partial2;     // modes 0 .. 4 of fh_sparse.hip
    const int* node_active;
    int nodes;
};
int fh_apply_term_operator(feasthip_ctx* h, int ld, const fh_termop_call& c);
// W + k N ld = A_k X for every term k of the handle on one N x ld panel (an identity term: a copy of X); 0, or -1 as above
int fh_term_products(feasthip_ctx* h, int ld, const cplx* X, cplx* W);
