/* petal_hip_nmf_kl_dense.h -- Nmf with the generalised Kullback-Leibler loss on DENSE data: scikit-learn's NMF(solver="mu",
 * beta_loss="kullback-leibler") on magnitude spectrograms, spectra, images and dense count tables.  An extension beyond the crate's
 * interface (DESIGN.md sections 4 and 7), declared beside petal_hip_nmf.h (the model handle, petal_nmf_spec, the stopping rule, the
 * initialisation, the penalty mapping) and petal_hip_nmf_kl.h (the same loss on a resident CSR handle).  Every existing signature, message
 * and refusal stays: petal_nmf_transform still refuses a Kullback-Leibler model and petal_nmf_spec is unchanged.
 *
 * The statement is petal_hip_nmf_kl.h's on every entry of X.  eps = 2^-23, everything is float64 inside, the padding is Nmf's.  One
 * iteration:
 *
 *     WH = W H ;  WH[WH < eps] = eps ;  Q = X / WH                                   (X == 0 gives Q == 0)
 *     den = rowsum(H) + l1_w + l2_w W ;  den[den == 0] = eps ;  W <- W o ((Q H^T) / den)
 *     WH' = W H with the NEW W, clamped ;  Q' = X / WH'
 *     den = colsum(W) + l1_h + l2_h H ;  den[den == 0] = eps ;  H <- H o ((W^T Q') / den)
 *
 * Loss: sqrt(2 max(0, term + <colsum W, rowsum H> - sum[x > eps] x)) with term = sum [x > eps] x log(x / max(WH, eps)), read at the
 * initial point, at every 10th iteration when tol > 0, and once after the last iteration if that one was not a check.  The stopping
 * rule, the random initialisation, the penalty mapping and the order "new W, then H with the new W" are Nmf's, unchanged.
 * transform: W starts at the constant sqrt(mean(Xq) / k) and takes exactly max_iter updates with H fixed; no tolerance stop.
 *
 * Results contract (Nmf's, unchanged).  X is widened to float64 on load; W, H and every product, quotient and sum are float64; the
 * rule is w * (num / den) in that order, without a reciprocal; there are no floating-point atomics and the order of every sum is
 * a function of the shape alone (tiles of 16 rows, at most 256 persistent workgroups whose slabs are added in workgroup order): the
 * same arrays give the same bytes on every run; outputs are rounded once to the data's type.  The sums run in another order than the CSR
 * sweep's, so the two routes agree to rounding, not to the byte.
 *
 * Where it runs.  k_nmf_kl_pass (fit_kernel / transform_kernel 1) inside k_nmf_pass's envelope: 16, 32 or 64 padded components (k <= 32
 * or 49 <= k <= 64), at most 512 padded columns, rows that allow 16-byte loads.  In a fit the pass reads X from memory once per
 * iteration; in transform once, whatever max_iter is (the 16 rows of a tile stay in registers over the updates).  One exception, because
 * the one-launch form does not fit in 512 registers without spilling: with 64 padded components and more than 256 padded columns a
 * fit's iteration is three launches (the W update, then the H side over the two halves of the feature axis) and reads X twice; the sums
 * and their order are the same.  Everything else -- a
 * device-op layer without the kernels (the host simulation of the tests), PETAL_OPT_NMF_FALLBACK (a test and A/B aid), k = 33 .. 48,
 * k > 64, more than 512 padded columns -- takes the composed path (0): the same statement from op_cvt_to_f64, op_dgemm and element-wise
 * steps on the host, X in row blocks of bounded size, blocks added in block order.  The composed path has no cap on k: "at most 64
 * components" stays the CSR entries' error alone.  petal_nmf_get's info6[4] and info6[5] report kernel (1) or composed path (0).
 *
 * The handle is an ordinary petal_nmf with loss = PETAL_NMF_LOSS_KL: petal_nmf_transform_csr works on it, and a model fitted on CSR
 * transforms dense rows through petal_nmf_transform_loss.  petal_nmf_inverse_transform, petal_nmf_get and petal_nmf_get_loss work unchanged.
 *
 * Measured: see README.md (Nmf with the Kullback-Leibler loss on dense data) and EXPERIMENTS.md; every figure not measured on the device
 * is marked "unmeasured".
 *
 * Not in this version: sharded fits, other beta (Itakura-Saito), float32 or split-bf16 products, a tolerance stop in transform, a kernel
 * for 48 padded components or more than 512 padded columns, a loss term fused into the update pass (a check costs one more pass), a
 * change of the Python facade's default route for dense input (it stays the compressed CSR route).
 */
#ifndef PETAL_HIP_NMF_KL_DENSE_H
#define PETAL_HIP_NMF_KL_DENSE_H

#include "petal_hip_nmf_kl.h"

#ifdef __cplusplus
extern "C" {
#endif

/* petal_nmf_fit with a loss.  PETAL_NMF_LOSS_FROBENIUS is petal_nmf_fit bit for bit; PETAL_NMF_LOSS_KL is the dense Kullback-Leibler
 * fit; any other value is PETAL_INVALID_INPUT "unknown loss".  Arguments, outputs, errors and messages are petal_nmf_fit's. */
int petal_nmf_fit_loss(petal_ctx* ctx, const petal_matrix* x, int64_t k, const petal_nmf_spec* spec, int64_t loss, const petal_matrix* w0,
                       const petal_matrix* h0, int64_t seed, petal_nmf** out, const petal_matrix* w_out);

/* petal_nmf_transform that dispatches on the model's loss: a Frobenius model gives petal_nmf_transform's bytes, a Kullback-Leibler model
 * (fitted here or on CSR) takes max_iter updates of the W rule above.  Errors and messages are petal_nmf_transform's. */
int petal_nmf_transform_loss(petal_ctx* ctx, petal_nmf* h, const petal_matrix* x, const petal_matrix* w_out);

/* test aid: the pass by itself on HOST float64 w_in (n x k) and h (k x d); spec's l1_w, l2_w are the penalties; rowsum(H) is formed by
 * the call.  w_out (n x k) = W after inner_iters updates (inner_iters == 0: w_in); a_out (k x d, nullable) = W^T (X / max(W H, eps)),
 * colsum_out (k, nullable) = colsum(W), both with the W written; term_out (1, nullable) is accepted with inner_iters == 0 only;
 * info1 = { k_nmf_kl_pass ran }.  The device W is formed inside a guard (a row in front and a row behind, every byte 0xFF beforehand):
 * PETAL_DEVICE_ERROR "nmf_kl_pass wrote outside the n x k block" if a guard row or a padding column changed. */
int petal_nmf_kl_pass(petal_ctx* ctx, const petal_matrix* x, int64_t k, const double* w_in, const double* h, const petal_nmf_spec* spec,
                      int64_t inner_iters, double* w_out, double* a_out, double* colsum_out, double* term_out, int64_t* info1);

#ifdef __cplusplus
}
#endif

#endif /* PETAL_HIP_NMF_KL_DENSE_H */
