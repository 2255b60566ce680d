/* petal_hip_probe.h -- TEST AIDS: the fp64 small-matrix operations every fit rests on (Cholesky / triangular solves, the fp64 GEMM
 * forms, the symmetric eigen-solvers, the one-sided Jacobi SVD), each through an entry of its own, so that a test can hold one
 * kernel to a long-double reference instead of a whole fit to 1e-5 -- and, further down, the composite operations that steer the
 * optimistic RandomizedPca fit (re-basing, the means fold).  Declared beside petal_hip.h, whose set of entry points mirrors
 * the crate's public interface one to one; nothing here is part of that interface, and there is no Rust binding.
 *
 * Every matrix argument is HOST memory, fp64, row-major, with an explicit leading dimension.  Each entry stages its inputs on the
 * device, fills every output buffer with NaN (whatever PETAL_OPT_POISON says), calls the device operation the way the fit drivers do
 * and copies the result back.  A shape the operation would refuse or that no kernel takes is PETAL_INVALID_INPUT and launches nothing.
 */
#ifndef PETAL_HIP_PROBE_H
#define PETAL_HIP_PROBE_H

#include "petal_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* G (L x L, ldg; upper triangle read) = R^T R with the dependence rule r_jj^2 <= rel_tol G_jj -> column j dropped.
 * Lz (0 = L): the padded extent of the result.  ndead_cols: as op_chol_inv.  *ndead: in / out, the device word the operation takes
 * the maximum into (pass 0 for the plain count).  *rt: 1 when the factor came back in RT form.
 *   route 0  op_chol_inv:                         out (Lz x Lz, ldo) = T = R^-1
 *   route 1  op_chol_rt, then op_trsm_right (RT form) or op_dgemm with the explicit inverse:
 *                                                 out (b_rows x Lz, ldo) = B R^-1;  B (b_rows x Lz, ldb), NULL = the Lz x Lz identity
 *   route 2  op_chol_rt, then the left solve inside op_gemm_xp_prod_absmax(a_rt) (RT form) or op_dgemm with the explicit inverse:
 *                                                 out (Lz x b_cols, ldo) = R^-1 B;  B (Lz x b_cols, ldb), not NULL
 * Where the RT form can come back (L <= 140, Lz a multiple of 16 <= 144) route 1 needs b_rows % 16 == 0 and route 2 b_cols % 16 == 0. */
int petal_probe_chol(petal_ctx* ctx, const double* G, int64_t L, int64_t ldg, double rel_tol, int64_t Lz, int64_t ndead_cols, int route,
                     const double* B, int64_t b_rows, int64_t b_cols, int64_t ldb, double* out, int64_t ldo, int* ndead, int* rt);

/* op_eigh on a copy of A (L x L, lda): w (L, descending), V (Lm x Lm, ldv, Lm = max(L, Lz)): eigenvectors in the columns, rows /
 * columns L .. Lz - 1 zero.  verdict_mode 0: no verdict word (*verdict_out = -1);  1: the word starts at verdict_in and is accumulated
 * into;  2: the word starts at verdict_in and the operation is told to clear it first (verdict_fresh).  L <= 2048. */
int petal_probe_eigh(petal_ctx* ctx, const double* A, int64_t L, int64_t lda, double tol_rel, int clustered, int64_t Lz, int64_t ncheck,
                     int verdict_mode, int verdict_in, double gap_tol_override, double* w, double* V, int64_t ldv, int* verdict_out);

/* op_jacobi_svd_rows on a copy of A (L x L, lda): U (L x L, ldu), s_inv (L), *nonconv (starts at 0).  L <= 1024. */
int petal_probe_jacobi_svd_rows(petal_ctx* ctx, const double* A, int64_t L, int64_t lda, double* U, int64_t ldu, double* s_inv,
                                int* nonconv);

/* op_dgemm: C (M x N, ldc; in / out) = alpha op(A) op(B) [* colscale_j] + beta C.  op(A): M x K (A is K x M when ta), op(B): K x N.
 * B == A with ldb == lda: the operation sees ONE device buffer (the symmetric rank-k form).  colscale (nullable, N values; beta
 * must be 0).  With beta == 0 the device C is NaN when the operation starts; the words between the rows of C (ldc > N) come back
 * as they went in. */
int petal_probe_dgemm(petal_ctx* ctx, int ta, int tb, int64_t M, int64_t N, int64_t K, double alpha, const double* A, int64_t lda,
                      const double* B, int64_t ldb, double beta, double* C, int64_t ldc, const double* colscale);

/* ---- the top-k subspace eigen-solver (topk_eigh: Pca, FastICA's whitening, IncrementalPca, the wide Pca and KernelPca take their
 * eigenpairs from it) and its one-launch residual verdict.  A sharded ctx is PETAL_INVALID_INPUT. */

/* op_ritz_residual by itself: CV (rows x ldc) and Vr (rows x ldv) go to the device with their WHOLE rows, nc <= ldc, ldv columns count;
 * theta (nc).  flag / flag2: NULL = the operation gets no such word, else the value the device word starts at.
 *   out3[0] = max_{j < nc} sum_i (CV_ij - theta_j Vr_ij)^2, out3[1] = theta[0] (0 when nc == 0), out3[2] = 1 if one of those nc sums is
 *   not below 1e300 (NaN included) or a given flag word is non-zero, else 0
 *   w_out (w_len >= max(nc, 1) words): theta[0 .. nc), NaN behind */
int petal_probe_ritz_residual(petal_ctx* ctx, const double* CV, int64_t ldc, const double* Vr, int64_t ldv, int64_t rows, int64_t nc,
                              const double* theta, const int* flag, const int* flag2, double* out3, double* w_out, int64_t w_len);

/* C (d x d, ldc; 1 <= d <= 2048) staged as the dp x dp zero-padded matrix a fit holds, dp = d rounded up to 16; nc <= d pairs wanted;
 * dtype PETAL_F32 | PETAL_F64: the type of the data C was formed from (closeness threshold 1e-8 | 1e-5, residual tolerance 1e-12 | 3e-14).
 *   mode 0  gram_topk_eigh, synchronous: *delivered, w (nc), V (dp x nc, ldv), *checks = the Rayleigh-Ritz steps taken
 *   mode 1  gram_topk_eigh, optimistic:  *delivered (the shape qualified), w, V, r3 (the verdict triple), *verdict = 1 when the
 *           library's own reading of r3 accepts the result
 *   mode 2  gram_eigen as Pca calls it:  *delivered (the iteration answered; 0: the full eigen-solver), w (dp), V (dp x dp, ldv),
 *           diag (dp; may be NULL in modes 0 / 1)
 * In modes 0 / 1 the device V and w hold NaN when the operation starts: a shape that does not qualify returns them so.  Outputs a mode
 * does not produce: *checks = 0, *verdict = 0, r3 = NaN. */
int petal_probe_topk_eigh(petal_ctx* ctx, const double* C, int64_t d, int64_t ldc, int64_t nc, int32_t dtype, int mode, int* delivered,
                          double* w, double* V, int64_t ldv, int* checks, double* r3, int* verdict, double* diag);

/* ---- the composite operations that steer the optimistic RandomizedPca fit, each called the way rpca_fit calls it ---------------------
 * X (n x K, ldx) and mu (K values) are HOST memory in `dtype` (PETAL_F32 | PETAL_F64); X goes to the device the way a fit's input does
 * (the row padding of PETAL_OPT_ROW_PAD included).  K and the column counts N / M are the PADDED extents a fit passes: multiples of 16.
 * Every fp64 argument is as above; muT, mu0 and Z come back WIDENED to fp64 (exactly: they are values of `dtype`).  A sharded ctx is
 * PETAL_INVALID_INPUT (these operations belong to the single-rank path). */

/* op_power_pass_means: the first fused pass of a fit with the means pass folded in.  X: d real columns, columns d .. K - 1 zero.
 * P (K x N, ldp; columns L .. N - 1 zero), L < N real columns.  *done: what the operation returned; 0 = nothing launched and EVERY
 * output below still holds the NaN it was filled with -- except mu0.
 *   Y (K x N, ldy), mu64 (K), muT (K: the means in dtype), *tv: the operation's results
 *   mu0 (K): the provisional centre the pass was taken about -- the operation overwrites it with the true means, so the probe forms it
 *            again with the operation's own first step (op_colmean over the same strided row sample) into a buffer of its own */
int petal_probe_power_pass_means(petal_ctx* ctx, const void* X, int32_t dtype, int64_t n, int64_t K, int64_t d, int64_t ldx, const double* P,
                                 int64_t N, int64_t ldp, int64_t L, int* done, double* Y, int64_t ldy, double* mu64, double* muT, double* mu0,
                                 double* tv);

/* One re-basing step: G (L x L, ldg; upper triangle read) = R^T R, P_out (K x M, ldpo) = A R^-1 (A: K x M, lda; columns L .. M - 1 of
 * the result zero), Z (n x M, ldz) = (X - mu) P_out, Y (K x M, ldy) = (X - mu)^T Z.  mu nullable.  *ndead: in / out, as petal_probe_chol.
 *   route 0  op_rebase_xp(p_planes, steering):                      P_out, Z         (*done = 1 always; Y is not touched)
 *   route 1  op_rebase_power_pass(steering) without Z:              P_out, Y         (Z is not touched)
 *   route 2  op_rebase_power_pass storing Z (never a steering pass): P_out, Z, Y
 * Routes 1 and 2 hand the operation ONE device buffer as A and Y, as the fit does (its Yp).  *done = 0 (routes 1, 2): the operation
 * returned false, nothing was launched, P_out / Z hold NaN, Y is NaN provided the buffer it shares with A still holds A bit for bit
 * (otherwise what the device holds), and *ndead is as it came in.  p_planes: 2 or 3 (routes 1, 2: ignored). */
int petal_probe_rebase(petal_ctx* ctx, const void* X, int32_t dtype, int64_t n, int64_t K, int64_t ldx, const void* mu, const double* G,
                       int64_t L, int64_t ldg, double rel_tol, const double* A, int64_t M, int64_t lda, int p_planes, int steering, int route,
                       int* done, double* P_out, int64_t ldpo, double* Z, int64_t ldz, double* Y, int64_t ldy, int* ndead);

#ifdef __cplusplus
}
#endif

#endif /* PETAL_HIP_PROBE_H */
