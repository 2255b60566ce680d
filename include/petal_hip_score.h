/* petal_hip_score.h -- row scores against a fitted projection: an extension beyond the crate, declared beside
 * petal_hip.h, whose set of entry points mirrors the crate's public interface one to one.
 *
 * With xc = x - means (when centering) and y = xc . components^T, per row i of x:
 *     q_i        = |xc_i|^2
 *     residual_i = max(q_i - sum_j y_ij^2, 0)      the reconstruction error (Q / SPE statistic) when the components are orthonormal
 *     weighted_i = sum_j weights_j y_ij^2          Hotelling's T^2 with weights_j = 1 / lambda_j
 * from ONE pass over x: both come out of the accumulators of the product kernel; nothing of size n x d or n x k is written
 * unless y_out is asked for.
 *
 * The residual is a DIFFERENCE formed in the accumulation precision (fp32 for PETAL_F32 data): its absolute error is a few
 * epsilon q_i, so a residual below about 1e-5 q_i is rounding noise in fp32.  Callers who need smaller residuals pass
 * PETAL_F64 data (floor: about 1e-14 q_i).
 */
#ifndef PETAL_HIP_SCORE_H
#define PETAL_HIP_SCORE_H

#include "petal_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* components: HOST, k x d row-major, dtype of x (any rows; orthonormal for the PCA models).  means: HOST, d values (ignored when
 * centering == 0).  weights: HOST, k values in the dtype of x, or NULL for all ones (then residual + weighted = q); a non-finite
 * weight is PETAL_INVALID_INPUT.
 * out: n x 2 = [residual, weighted] (dtype of x, HOST or DEVICE, any strides).
 * y_out (nullable): n x k projections, exactly what petal_transform writes -- stored by the same launch.
 * Errors as petal_transform ("# of columns should be d"); a wrong shape or dtype of out / y_out is PETAL_INVALID_INPUT.
 * n == 0 and k == 0 are legal (k == 0: residual = q, weighted = 0; that call runs on the any-shape kernel, one wave per row with fp64
 * accumulation -- correct, not fast: ask for q as residual + weighted of a call you make anyway).  Per-row and local: on a sharded ctx every rank scores its own
 * rows and the collective is not touched. */
int petal_score_rows(petal_ctx* ctx, const petal_matrix* x, const void* components, const void* means,
                     int64_t k, int64_t d, int centering, const void* weights,
                     const petal_matrix* out, const petal_matrix* y_out);

#ifdef __cplusplus
}
#endif

#endif /* PETAL_HIP_SCORE_H */
