/* petal_hip_kpca.h -- KernelPca: kernel principal component analysis, the library's first non-linear estimator.  An extension beyond the
 * crate's interface (DESIGN.md sections 4 and 7), declared beside petal_hip.h.  The model is scikit-learn's KernelPCA.
 *
 * Kernels on rows x, y of width d (gamma <= 0 or NaN means 1 / d; defaults: linear, degree 3, coef0 1):
 *
 *     PETAL_KERNEL_LINEAR    <x, y>
 *     PETAL_KERNEL_POLY      (gamma <x, y> + coef0)^degree     integer degree >= 1, by repeated multiplication: integer inputs give
 *                                                              exact integers
 *     PETAL_KERNEL_RBF       exp(-gamma |x - y|^2)             |x - y|^2 = |x|^2 + |y|^2 - 2 <x, y>, clamped at zero
 *     PETAL_KERNEL_SIGMOID   tanh(gamma <x, y> + coef0)
 *     PETAL_KERNEL_COSINE    <x, y> / (|x| |y|)                0 where either norm is 0
 *
 * (laplacian is not included: an L1 distance is not a Gram product.)
 *
 * The fit, on X (n x d):
 *
 *     G = (X - c)(X - c)^T       the row Gram matrix of petal_hip_wide.h (k_row_gram).  c = the float64 column mean for rbf -- the kernel
 *                                is translation invariant, and centring removes the cancellation in |x|^2 + |y|^2 - 2 <x, y> -- and
 *                                c = 0 for the other four
 *     K_ij = phi(G_ij, G_ii, G_jj)
 *     K~ = K - 1 rbar^T - rbar 1^T + tbar       rbar the column means of K, tbar its grand mean; row sums in a fixed order
 *     K~ = V diag(lambda) V^T    the top k eigenpairs, descending; signs as svd_flip takes them from V (the dual route of exact Pca)
 *
 *     fit_transform  = V sqrt(lambda)
 *     transform(Xq)  = K~q V lambda^(-1/2),     K~q = Kq - 1 rbar^T - (row means of Kq) 1^T + tbar
 *
 * transform is ONE fused pass over the query rows (k_kapply): phi(Xq Xt^T) A' with A' = [V lambda^(-1/2) | 1], two chained fp64 MFMA
 * products whose m x n kernel matrix never touches memory, and an epilogue on its k + 1 output columns.
 *
 * Results contract.  Everything is float64 inside: data are widened before c is subtracted, every product and sum is float64, outputs
 * are rounded once to the data's type.  No floating-point atomics: the same input gives the same bytes.
 *   Undetermined components.  A component whose sqrt(lambda) is at or below the relative threshold of the Gram route (1e-6 float32,
 *   1e-10 float64, times sqrt(lambda_1)) comes back as a ZERO COLUMN of fit_transform and of transform, its eigenvalue as computed, and
 *   nothing is raised.  That covers every non-positive eigenvalue of the sigmoid kernel, which is not positive semi-definite, and the
 *   n-th eigenvalue of a centred K (K~ 1 = 0 by structure: cleared whatever its computed size) -- the rule exact Pca's dual route
 *   discloses.
 *   The handle keeps ITS OWN device copy of the training rows: the model outlives a caller's zero-copy tensor.
 *
 * Not in this version: sharded fits, sparse input, precomputed kernels, an approximate pre-image (inverse_transform), float32 /
 * split-bf16 products for the cross Gram matrix, an incremental or Nystroem fit.
 */
#ifndef PETAL_HIP_KPCA_H
#define PETAL_HIP_KPCA_H

#include "petal_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PETAL_KERNEL_LINEAR 0
#define PETAL_KERNEL_POLY 1
#define PETAL_KERNEL_RBF 2
#define PETAL_KERNEL_SIGMOID 3
#define PETAL_KERNEL_COSINE 4

/* petal_ctx_set_option: non-zero = the map G -> K~ and transform's phi(Xq Xt^T) A' are built from the library's other products (widen,
 * rank-one centring, fp64 GEMM) and a phi loop on the host over a read-back copy, in row blocks of bounded size, instead of k_kmap /
 * k_kapply -- a test and A/B aid like PETAL_OPT_PCA_DUAL_FALLBACK; no environment variable.  The same path is taken where the
 * device-op layer lacks the kernels or a matrix does not allow their 16-byte loads.  (36, not 35: tests/test_wide_host.py holds 35, the
 * number after petal_hip_wide.h's options, to "unknown option".) */
#define PETAL_OPT_KPCA_FALLBACK 36

typedef struct petal_kernel_spec {
    int32_t kernel;   /* PETAL_KERNEL_* */
    int32_t degree;   /* poly: >= 1 (checked for every kernel) */
    double gamma;     /* <= 0 or NaN: 1 / d */
    double coef0;
} petal_kernel_spec;

typedef struct petal_kpca petal_kpca;

/* Fits on x (n x d; float32 or float64, host or device, any strides petal_pca_fit takes) and returns a handle that lives with the ctx.
 * y_out (nullable, n x k in x's dtype): fit_transform.  Errors: k > n PETAL_INVALID_INPUT "every dimension should be at least k"
 * (d < k is legal here); n = 0, d = 0, n > 32768 "too many rows" (K~ and V are n x n float64), an unknown kernel, degree < 1,
 * non-finite kernel parameters, a sharded ctx PETAL_INVALID_INPUT; NaN or infinity in x
 * PETAL_LINALG_ERROR "did not converge" (from the traces of G and K~, before the eigen-solve: tanh and exp map an infinity to a
 * finite number, so K~ alone would not show it). */
int petal_kpca_fit(petal_ctx* ctx, const petal_matrix* x, int64_t k, const petal_kernel_spec* spec, petal_kpca** out,
                   const petal_matrix* y_out);
void petal_kpca_destroy(petal_kpca* h);

/* y_out (m x k, the fit's dtype) = transform(x), x: m x d in the fit's dtype.  Another width: "# of columns should be d". */
int petal_kpca_transform(petal_ctx* ctx, petal_kpca* h, const petal_matrix* x, const petal_matrix* y_out);

/* eigenvalues (nullable): HOST float64, k values, as computed.  scaled_vectors (nullable): HOST float64, n x k row-major, V lambda^(-1/2)
 * with the signs applied, zero columns where undetermined.  info8 (nullable) = { n, d, k, kernel ran on the fit's map (1) or the
 * fallback built K~ (0), kernel ran on the last transform (1 / 0; -1 before the first), order of the eigenproblem, PETAL_KERNEL_*,
 * eigen-solver of the fit (1: the top-k subspace iteration of the Gram route delivered the eigenpairs; 0: it gave up or did not apply and
 * the full eigen-solver of order n ran -- the slower fit) }. */
int petal_kpca_get(const petal_kpca* h, double* eigenvalues, double* scaled_vectors, int64_t* info8);

/* The fused pass by itself (a test aid in the manner of petal_row_gram): out (HOST float64, m x cols row-major) =
 * phi((xq - centre)(xt - centre)^T) A, with A HOST float64 (n x cols row-major) and centre HOST float64 (d values, or NULL).  No double
 * centring and no epilogue.  xq (m x d) and xt (n x d): the same dtype, host or device, any strides.  The device result is formed
 * inside a guard (an odd pitch, one more row, every byte 0xFF beforehand): PETAL_DEVICE_ERROR "kernel_apply wrote outside the m x cols
 * block" if the guard changed.  info1 (nullable) = { k_kapply ran }.  A sharded ctx is PETAL_INVALID_INPUT. */
int petal_kernel_apply(petal_ctx* ctx, const petal_matrix* xq, const petal_matrix* xt, const petal_kernel_spec* spec, const double* a,
                       int64_t cols, const double* centre, double* out, int64_t* info1);

#ifdef __cplusplus
}
#endif

#endif /* PETAL_HIP_KPCA_H */
