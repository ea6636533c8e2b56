// fh_dense.hpp -- dense shifted systems: operator application on panels and the batched
// complex LU (form z B - A, factor with partial pivoting, solve) for the FEAST contour sweep.
#pragma once
#include "fh_common.hpp"
#include <vector>

struct fh_dense_op_args {
    const void* A; const void* B;   // N x N column-major, double or cplx; B may be null (identity)
    int N; int is_complex; int nodes;
    const cplx* X; size_t x_node_stride;
    cplx* Y; size_t y_node_stride;
    const cplx* coefA; const cplx* coefB;
    const cplx* Bvec; size_t b_node_stride;
    const cplx* U; size_t u_node_stride;
    int dot_mode; cplx* partial1; cplx* partial2;
    const int* node_active;
};
int fh_dense_op_nblk(int N);
void fh_launch_dense_op(const fh_dense_op_args& a, int ld, int nblk, hipStream_t st);
// Y = (cb*B^H + ca*A^H) X, plain products only (dot_mode 0, MFMA kernel)
void fh_launch_dense_op_adjoint(const fh_dense_op_args& a, int ld, hipStream_t st);

// R -= X diag(lam)
void fh_launch_axpy_cols(cplx* R, const cplx* X, const cplx* lam, int N, int ld, hipStream_t st, const int* skip = nullptr);

// Polynomial handle (h->kind == FH_KIND_POLYNOMIAL, fh_poly.hip): LUs[e] = P(z_e) for the nf matrices lu_factor_batch is about to factor, in one
// pass over the coefficients; prec 64: complex128 factors, 32: complex64.
// A term handle (fh_poly::terms) forms T(z_e) = sum_k f_k(z_e) A_k from its node table instead; a shift that is no contour
// node of that table is an error.
int fh_poly_form(feasthip_ctx* h, void* const* dlus, const cplx* dz, int nf, int prec);
// Term handle: *dF = the nf x (degree + 1) device table of the rows f_k(z) of the node table that belong to the shifts dz (device,
// each one a node of the table's contour, matched exactly) -- what the forming kernels of both direct solvers read.
int fh_poly_term_table(feasthip_ctx* h, const cplx* dz, int nf, const cplx** dF);

const fh_direct_ops& fh_dense_direct_ops();          // the dense LU's operations for the sequences of fh_direct.hip

// Blocked band LU on the dense kernels (fh_dense.hip, "wide band"): storage per node fh_wband_elems complex128 values, the
// matrix pointer the kernels take is storage + fh_wband_base_offset.
size_t fh_wband_elems(int N, int kl, int ku);
size_t fh_wband_base_offset(int N, int kl, int ku);
// prec: 64 = complex128 factors, 32 = complex64 factors (storage elements of that type; refinement is the caller's)
int fh_wband_factor(feasthip_ctx* h, int prec, int nf, void* const* abs_host, void** dbases, int** dpvs, const cplx* dz, int* dinfo,
                    const int* d_iperm, int kl, int ku);
int fh_wband_solve(feasthip_ctx* h, int prec, int nf, void** dbases, int** dpvs, int** dperms, const int* d_perm, const cplx* RHS, size_t rhs_stride,
                   cplx* Y, size_t stride, void* Yb, void* Zb, int ld, int m, int kl, int ku);
// Y[node] = (z_node B - A)^-H RHS on the same factors (ZGBTRS 'C'; complex128 factors only), same arguments
int fh_wband_solve_adjoint(feasthip_ctx* h, int nf, void** dbases, int** dpvs, int** dperms, const int* d_perm, const cplx* RHS, size_t rhs_stride,
                           cplx* Y, size_t stride, void* Yb, void* Zb, int ld, int m, int kl, int ku);

// Multifrontal sparse LU (fh_dense.hip, symbolic phase fh_mf.hpp): plan from the host pattern, batched numeric factorisation
// of nf shifted matrices into per-node stores, substitution through the elimination tree.  prec 64: complex128 factors; 32: complex64 factors (refinement is the caller's).
int fh_mf_make_plan(feasthip_ctx* h, int leaf);
void fh_mf_free(feasthip_ctx* h);
void fh_mf_free_buffers(feasthip_ctx* h);
double fh_mf_plan_flops(feasthip_ctx* h);
int fh_mf_max_front(feasthip_ctx* h);
int fh_mf_max_group(feasthip_ctx* h);
size_t fh_mf_store_bytes(feasthip_ctx* h, int prec);
size_t fh_mf_pivot_ints(feasthip_ctx* h);
size_t fh_mf_work_bytes(feasthip_ctx* h, int prec);
int fh_mf_factor(feasthip_ctx* h, int prec, int nf, void* const* stores, int* const* pivs, const cplx* dz, std::vector<int>& info_out,
                 std::vector<double>& multiplier_out);
int fh_mf_solve(feasthip_ctx* h, int prec, int nf, void* const* stores, int* const* pivs, const cplx* RHS, size_t rhs_stride, cplx* OUT, size_t out_stride, int ld, int m);
// (z_q B - A)^-H RHS[q] on the same factors (h->adjoint; complex128 factors only): the conjugate-transposed walk through the tree
int fh_mf_solve_adjoint(feasthip_ctx* h, int prec, int nf, void* const* stores, int* const* pivs, const cplx* RHS, size_t rhs_stride, cplx* OUT, size_t out_stride, int ld, int m);
