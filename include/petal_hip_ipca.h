/* petal_hip_ipca.h -- IncrementalPca: the exact Pca fitted batch by batch, on data that never exists as one array (event tables that
 * arrive in chunks, matrices larger than one card, fits that are checkpointed or combined across processes).  An extension beyond the
 * crate, declared beside petal_hip.h, whose set of entry points mirrors the crate's public interface one to one.
 *
 * Exact Pca is the Gram route: the d x d float64 matrix (X - mu)^T (X - mu), the means and the row count are a sufficient statistic.
 * A handle keeps that statistic -- mean (d) and M2 = sum (x - mean)(x - mean)^T (d x d, symmetric, stored in full), both float64 in
 * device memory, padded to a multiple of 16; the row count on the host -- and petal_ipca_partial_fit folds one batch into it:
 *
 *     c  = the running mean (the first non-empty batch: the mean of its first min(m, 64) rows; centering == 0: zero)
 *     s  = sum (x - c),   G = sum (x - c)(x - c)^T      one pass over the batch; x is WIDENED to float64 before c is subtracted, every
 *                                                        product and sum is float64
 *     n' = n + m,   mean' = c + s / n',   M2' = M2 + G - s s^T / n'
 *
 * petal_ipca_finalize solves the eigenproblem of a COPY of M2 with the solvers of petal_pca_fit and returns what petal_pca_fit returns
 * on the concatenation of the batches, with two disclosed differences:
 *
 *   Signs.  The crate's svd_flip decides from U, which a streaming fit never holds.  Here the entry of largest magnitude of every
 *   component is positive (ties: the lowest index) -- scikit-learn's rule for its IncrementalPCA.  Components equal petal_pca_fit's up
 *   to sign.
 *   Accuracy.  There is no X at finalize, hence no accurate small-sigma route: the Gram route alone, singular values and components
 *   good to about eps64 (sigma_1 / sigma_j)^2 over the relative gap (the disclosure of petal_pca_fit_segments).
 *
 * Cancellation.  G - s s^T / n' subtracts two terms of size m |s / m|^2: it loses digits, relative to the within-batch variances
 * sigma_j^2, in proportion to |s / m|^2 / sigma_j^2 when a batch lies many standard deviations from everything seen before (sorted or
 * drifting streams).  Measured on eight float64 batches of 500 x 16, each 40 sigma beyond the last: M2 off by 1.4 eps64 of its largest
 * diagonal entry -- which then holds the squared drift -- and by 1.5e4 eps64 n sigma_i sigma_j of the within-batch spread; per-batch
 * handles merged give 1.1 and 1.2e4.  Callers with such streams shuffle, or fit chunks into separate handles and
 * petal_ipca_merge them: the merge is the pairwise, cancellation-free form  M2 = M2_a + M2_b + (n_a n_b / n) dd^T,  d = mean_b - mean_a.
 *
 * No floating-point atomics anywhere: the same batches in the same order give the same bytes on every run.
 *
 * Not in this version: sharded contexts, incremental RandomizedPca or FastIca, sparse batches, forgetting factors and row weights, the
 * small-sigma accurate route, and overlapping the library's own host upload of batch i + 1 with batch i (a caller can do that already
 * with device tensors and a stream).
 */
#ifndef PETAL_HIP_IPCA_H
#define PETAL_HIP_IPCA_H

#include "petal_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PETAL_IPCA_KERNEL_MAX_D 1024   /* wider batches take the two-pass path built from the library's other products */
/* petal_ctx_set_option: non-zero sends every partial_fit and merge of this ctx through the two-pass path (a test aid, like
 * PETAL_OPT_STEERING_HOOK; no environment variable).  Numbered apart from petal_hip.h's options (0 .. 15), whose next free number
 * stays an unknown option. */
#define PETAL_OPT_IPCA_FALLBACK 32

typedef struct petal_ipca petal_ipca;   /* opaque: the statistic, resident with its ctx; destroy it before that ctx */

/* d >= 0 columns, dtype PETAL_F32 / PETAL_F64 (the type of every batch and of finalize's outputs), centering as petal_pca_fit's.
 * A sharded ctx (world size > 1) is PETAL_INVALID_INPUT in this version (and in every entry below). */
int petal_ipca_create(petal_ctx* ctx, int64_t d, int32_t dtype, int centering, petal_ipca** out);
void petal_ipca_destroy(petal_ipca* h);
/* back to the state of a fresh handle: no rows seen, a poisoned statistic cleared, counters zero */
int petal_ipca_reset(petal_ipca* h);

/* x: host or device, any strides petal_pca_fit takes.  x.dtype must be the handle's (PETAL_INVALID_INPUT), x.cols must be d
 * ("# of columns should be d").  0 rows: a legal no-op.  Nothing is read back and, for device input, nothing waits for the device:
 * values are not inspected -- a NaN or an infinity poisons the statistic and surfaces in petal_ipca_finalize as PETAL_LINALG_ERROR
 * "did not converge"; petal_ipca_reset clears it. */
int petal_ipca_partial_fit(petal_ctx* ctx, petal_ipca* h, const petal_matrix* x);

/* into += other (same ctx, d, dtype and centering: PETAL_INVALID_INPUT otherwise).  An empty `other` changes no byte of `into`;
 * `other` itself is never changed. */
int petal_ipca_merge(petal_ctx* ctx, petal_ipca* into, const petal_ipca* other);

/* The model of the rows seen so far: components (k x d), means (d), singular (k), total_variance (1 = trace of M2), all in the handle's
 * dtype and laid out as petal_pca_fit's.  The state is not modified: call it any number of times, with any k, between batches.
 * Errors: "every dimension should be at least k" (rows seen or d below k), "no rows have been seen" (PETAL_INVALID_INPUT),
 * "did not converge" (PETAL_LINALG_ERROR: a non-finite statistic). */
int petal_ipca_finalize(petal_ctx* ctx, const petal_ipca* h, int64_t k, void* components, void* means, void* singular,
                        void* total_variance);

/* out8 = { d, dtype, centering, rows seen, batches (non-empty partial_fit calls), batches the streaming kernel took, merges, 0 } */
int petal_ipca_info(const petal_ipca* h, int64_t* out8);

/* The unpadded statistic to and from HOST float64 (checkpoints, serialisation, combining the work of several processes or GPUs by
 * hand): n rows seen, mean_d (d), m2_dxd (d x d row-major).  Every pointer of get_state is nullable.  set_state: n >= 0 and integral
 * (PETAL_INVALID_INPUT otherwise); n == 0 resets the handle and ignores the arrays. */
int petal_ipca_get_state(petal_ctx* ctx, const petal_ipca* h, double* n, double* mean_d, double* m2_dxd);
int petal_ipca_set_state(petal_ctx* ctx, petal_ipca* h, double n, const double* mean_d, const double* m2_dxd);

#ifdef __cplusplus
}
#endif

#endif /* PETAL_HIP_IPCA_H */
