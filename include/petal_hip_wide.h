/* petal_hip_wide.h -- exact Pca on WIDE data: a few hundred to a few thousand samples of very wide rows (eigenfaces, spectra, expression
 * tables, flattened images).  An extension beyond the crate's interface (DESIGN.md sections 4 and 7), declared beside petal_hip.h; the
 * fit itself needs no new entry: petal_pca_fit on a wide matrix simply takes this route.
 *
 * petal_pca_fit is the Gram route: the d x d float64 matrix (X - mu)^T (X - mu) and an eigenproblem of order d.  For n < d its dual is
 * used instead:
 *
 *     K = Xc Xc^T            n x n float64, the ROW Gram matrix: x is WIDENED to float64 before mu is subtracted, every product and
 *                            sum is float64 (k_row_gram contracts over the contiguous feature axis, cut into chunks whose slabs are
 *                            added in a fixed order: no floating-point atomics, the same input gives the same bytes)
 *     K = U diag(sigma^2) U^T   the eigenvectors ARE U (svd_flip looks at exactly this matrix), the trace is the total variance
 *     V^T = Sigma^-1 U^T Xc     one more pass over X
 *
 * two passes over X and an eigenproblem of order n: O(n^2 d) like the crate's gesvd, and n x n instead of d x d workspace.
 *
 * The route is taken when the ctx is not sharded, n < d and d > 2048 (PETAL_OPT_PCA_DUAL = 0, the default); every narrower fit keeps
 * the route, the launches and the bytes it had.  Results contract: petal_pca_fit's, with two disclosed differences.
 *
 *   Undetermined components.  A component whose singular value is at or below the relative threshold of the Gram route (1e-6
 *   float32, 1e-10 float64, times sigma_1) is not determined by the data here: it comes back as a ZERO ROW, its singular value as
 *   computed, and nothing is raised (the crate returns an arbitrary unit vector of the null space).  Centred data of n rows have rank
 *   n - 1 at most, so a centred fit with k = n always ends in one such row; that one is cleared by structure, not by the threshold
 *   (its computed singular value is the rounding of K, about 1e-8 sigma_1).
 *   Accuracy.  The Gram route's statement holds unchanged: singular values and components good to about eps64 (sigma_1 / sigma_j)^2
 *   over the relative gap.  The float64 small-sigma accurate route of the primal fit is NOT taken on this route.
 *
 * Not in this version: sharded wide fits (K needs row pairs across ranks; a sharded ctx keeps the primal route at every shape),
 * FastICA whitening on wide data, SegmentedPca's kernel (its segments stay at d <= 64), and the small-sigma accurate route.
 */
#ifndef PETAL_HIP_WIDE_H
#define PETAL_HIP_WIDE_H

#include "petal_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* petal_ctx_set_option / petal_ctx_get_option.  Numbered apart from petal_hip.h's options (0 .. 15), whose next free number stays an
 * unknown option.
 * PETAL_OPT_PCA_DUAL: 0 = the auto rule above; 1 (any positive value) = the dual route at EVERY shape on a non-sharded ctx (n >= d
 * included: how tests reach the kernel at small d); -1 (any negative value) = never: the primal route as before this header existed. */
#define PETAL_OPT_PCA_DUAL 33
/* non-zero: K and the components are built from the library's other products (widen, rank-one centring, fp64 GEMM) instead of
 * k_row_gram -- a test and A/B aid like PETAL_OPT_IPCA_FALLBACK; no environment variable. */
#define PETAL_OPT_PCA_DUAL_FALLBACK 34

/* Facts of the last petal_pca_fit on this ctx: out4 = { route (0 primal, 1 dual), k_row_gram ran (1) or the other products built K (0;
 * also 0 on the primal route), order of the eigenproblem (d or n; 0 when the fit returned before one), feature chunks of the last
 * row-Gram launch (0 when the kernel did not run) }. */
int petal_pca_last_route(petal_ctx* ctx, int64_t* out4);

/* The row Gram matrix by itself (a test aid in the manner of petal_csr_gemm): out (HOST float64, n x n row-major) =
 * sum_j (x_ij - centre_j)(x_i'j - centre_j).  x: host or device, any strides petal_pca_fit takes; centre: HOST float64, d values, or
 * NULL for no centring.  info2 (nullable) = { k_row_gram ran, feature chunks }.  The device result is formed inside a guard (an odd
 * pitch, one more row, every byte 0xFF beforehand): PETAL_DEVICE_ERROR "row_gram wrote outside the n x n block" if the guard changed.
 * A sharded ctx is PETAL_INVALID_INPUT. */
int petal_row_gram(petal_ctx* ctx, const petal_matrix* x, const double* centre, double* out, int64_t* info2);

#ifdef __cplusplus
}
#endif

#endif /* PETAL_HIP_WIDE_H */
