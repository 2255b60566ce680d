/* petal_hip_segments.h -- segmented Pca: an exact Pca of every row segment of a row-sorted matrix in one call (one model per cluster,
 * window, sensor, group of a sorted table).  An extension beyond the crate, declared beside petal_hip.h, whose
 * set of entry points mirrors the crate's public interface one to one.
 *
 * A segment is a run of consecutive rows: segment b holds rows offsets[b] .. offsets[b + 1] - 1.  Each segment gets what Pca::fit
 * gives on that segment alone (pca.rs:195-231, svd_flip at 815-850).  For d <= 64 the whole batch is ONE launch, a workgroup per
 * segment; wider data and device-op layers without the kernel run the single-matrix code segment by segment, with the same results
 * contract -- no shape the crate accepts is refused.  A segment of any length is legal; a very long one keeps one compute unit busy
 * (correct, not fast: fit it with petal_pca_fit).
 *
 * Accuracy: the kernel is the Gram route, as exact Pca is.  Singular values and components hold to about eps64 (sigma_1 / sigma_j)^2,
 * divided by the relative gap to the neighbouring sigma; float32 data are widened on load, so their results are good to float32
 * rounding of the outputs.  petal_pca_fit switches to its QR + one-sided Jacobi route below 10^-3.5 sigma_1 for float64 data; the
 * segment kernel does not: callers who need such small sigma of a segment to full relative accuracy use petal_pca_fit on it.
 */
#ifndef PETAL_HIP_SEGMENTS_H
#define PETAL_HIP_SEGMENTS_H

#include "petal_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* offsets: HOST, n_segments + 1 values; offsets[0] == 0, non-decreasing, offsets[n_segments] == x.rows -- anything else is
 * PETAL_INVALID_INPUT, the message names the first offending index.
 * A segment with fewer than k rows, or d < k, is PETAL_INVALID_INPUT ("segment b: every dimension should be at least k"), raised
 * before anything is launched.  n_segments == 0, k == 0 and empty segments (only legal when k == 0) are legal; an empty segment's
 * means and total variance are zero.
 * status (nullable): 0 for a good segment, 1 for one that holds a NaN or an infinity (the crate's LinalgError "did not converge"):
 * that segment's components, means, singular values, total variance and rows of y_out are NaN, the other segments are untouched by
 * it, and the call returns PETAL_OK.  With status == NULL such a segment makes the call return PETAL_LINALG_ERROR; the message holds
 * the index of the first one.
 * kernel_segments (nullable): how many segments the segment kernel fitted (n_segments, or 0 when the call looped).
 * Per segment and local: on a sharded ctx every rank fits its own segments and the collective is not touched. */
int petal_pca_fit_segments(petal_ctx* ctx, const petal_matrix* x, const int64_t* offsets, int64_t n_segments,
                           int64_t k, int centering,
                           void* components,      /* HOST n_segments x k x d, dtype of x */
                           void* means,           /* HOST n_segments x d */
                           void* singular,        /* HOST n_segments x k */
                           void* total_variance,  /* HOST n_segments */
                           int32_t* status,       /* HOST n_segments, nullable */
                           const petal_matrix* y_out,      /* nullable: x.rows x k, HOST or DEVICE, any strides */
                           int64_t* kernel_segments);      /* nullable */

/* components / means: HOST, as petal_pca_fit_segments wrote them (means ignored when centering == 0).  Errors as petal_transform /
 * petal_inverse_transform ("# of columns should be d" / "... k"), and the offsets rules above. */
int petal_transform_segments(petal_ctx* ctx, const petal_matrix* x, const int64_t* offsets, int64_t n_segments,
                             const void* components, const void* means, int64_t k, int64_t d, int centering,
                             const petal_matrix* y_out);
int petal_inverse_transform_segments(petal_ctx* ctx, const petal_matrix* y, const int64_t* offsets, int64_t n_segments,
                                     const void* components, const void* means, int64_t k, int64_t d, int centering,
                                     const petal_matrix* x_out);

#ifdef __cplusplus
}
#endif

#endif /* PETAL_HIP_SEGMENTS_H */
