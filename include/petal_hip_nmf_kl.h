/* petal_hip_nmf_kl.h -- Nmf with the generalised Kullback-Leibler loss on sparse data: scikit-learn's NMF(solver="mu",
 * beta_loss="kullback-leibler"), the loss of PLSA and topic models, for the data petal_hip_nmf_sparse.h names (term-document counts,
 * expression tables, click matrices).  An extension beyond the crate's interface (DESIGN.md sections 4 and 7), declared beside
 * petal_hip_nmf.h (the model handle, the stopping rule, the initialisation, the penalty mapping) and petal_hip_nmf_sparse.h (the sweeps on
 * a resident CSR handle).  petal_nmf_spec and every existing signature stay as they are.
 *
 * On sparse X the updates touch X only at its stored entries: the numerator is (X / (W H)) H^T and X / (W H) is zero wherever X is, the
 * denominator is a k-vector of column sums, and sum(W H) in the loss is an inner product of two k-vectors.  An iteration is two SWEEPS of
 * one kernel; an n x d quotient matrix is never formed.  eps = 2^-23, as in Nmf.  "KL sweep" of an image M (R x C, M = X or X^T) with
 * G (R x k, updated), F (C x k, gathered), c = the column sums of F (a k-vector), penalties l1 and l2, and inner >= 0.  For row r,
 * `inner` times:
 *
 *     for every stored entry t of row r:   wh_t = <g_r, F[idx_t, :]> ;  wh_t < eps -> eps ;  q_t = val_t / wh_t
 *     num = sum_t q_t F[idx_t, :]
 *     den = c + l1 + l2 g_r ;  den[den == 0] = eps ;  g_r <- g_r o (num / den)
 *
 * Outputs: the new G; colsum(G_new) (a k-vector); only for inner == 0:
 *     term = sum_r sum_t [val_t > eps] val_t log(val_t / max(<g_r, F[idx_t]>, eps)).
 * One fit iteration: the row sweep on X with G = W, F = H^T, c = the row sums of H, (l1_w, l2_w); then the column sweep on the
 * transposed image with G = H^T, F = the NEW W, c = colsum(W), (l1_h, l2_h).
 * Loss: sqrt(2 max(0, term + <colsum W, rowsum H> - sum[val > eps] val)), evaluated by a sweep with inner = 0 at the initial point, at
 * every 10th iteration when tol > 0, and once after the last iteration if that one was not a check.  The stopping rule, the random
 * initialisation, the penalty mapping and the order "new W, then H with the new W" are Nmf's, unchanged.
 * transform: G starts at the constant sqrt(mean(Xq) / k) and the sweep runs exactly max_iter updates with H fixed; no tolerance stop.
 * An explicit zero contributes nothing; an empty row gives a zero row.
 *
 * Results contract (Nmf's, unchanged).  Values are widened to float64 on load; F, G, c and every product, quotient and sum are float64;
 * the factors are padded to 16 / 32 / 64 columns with zeros; there are no floating-point atomics and the order of every sum is a function
 * of the handle's work items and the padding alone: the same arrays give the same bytes on every run and on a second handle built from
 * them; outputs are rounded once to the data's type.
 *
 * Where it runs.  On a resident handle: k_nmf_kl_sweep (kernel_path 1).  On a handle that is not resident (a device-op layer without the
 * kernels: the host simulation of the tests), or with PETAL_OPT_NMF_FALLBACK set on a resident handle (the images are copied back: a test
 * and A/B aid): the same driver over a plain host loop of the statement in position order (kernel_path 0).  There is no densifying path
 * for this loss.  k > 64 is PETAL_INVALID_INPUT "kullback-leibler takes at most 64 components".  petal_nmf_get's info6[4] and info6[5]
 * report the same as kernel_path.  Dense input takes the same path once compressed to the CSR of its non-zero entries (the Python facade
 * does that on the host); the dense C entry petal_nmf_transform refuses a Kullback-Leibler model (PETAL_INVALID_INPUT naming the loss).
 * petal_nmf_inverse_transform and petal_nmf_get work unchanged.
 *
 * Disclosed, beside petal_hip_nmf_sparse.h's duplicate disclosure.  Stored values are checked one by one (a duplicate pair (+3, -1) is
 * refused).  In the updates duplicates act as their sum (sum_t val_t / wh with the same wh); in the loss each stored value enters
 * v log v by itself, so with duplicates present the reported loss differs from the loss of the summed matrix (W and H do not).
 *
 * Measured: see README.md (Nmf with the Kullback-Leibler loss) and EXPERIMENTS.md; every figure not measured on the device is marked
 * "unmeasured".
 *
 * Not in this version: sharded fits, k > 64, a fused dense Kullback-Leibler kernel (dense input is compressed on the host; the dense
 * kernel now lives beside this header, in petal_hip_nmf_kl_dense.h, with entries of its own), other beta,
 * a loss term fused into the column sweep (a check costs one more sweep), one-launch multi-update transform on images with split rows
 * (such an image takes one launch pair per update), a tolerance stop in transform, device-resident CSR arrays.
 */
#ifndef PETAL_HIP_NMF_KL_H
#define PETAL_HIP_NMF_KL_H

#include "petal_hip_nmf_sparse.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PETAL_NMF_LOSS_FROBENIUS 0
#define PETAL_NMF_LOSS_KL 1

/* petal_nmf_fit_csr with a loss.  PETAL_NMF_LOSS_FROBENIUS is petal_nmf_fit_csr bit for bit; any other value than 0 or 1 is
 * PETAL_INVALID_INPUT.  Arguments, outputs, errors and messages are petal_nmf_fit_csr's, plus "kullback-leibler takes at most 64
 * components".  The handle returned is an ordinary petal_nmf that remembers its loss: petal_nmf_transform_csr dispatches on it. */
int petal_nmf_fit_csr_loss(petal_ctx* ctx, const petal_csr* x, int64_t k, const petal_nmf_spec* spec, int64_t loss, const petal_matrix* w0,
                           const petal_matrix* h0, int64_t seed, petal_nmf** out, const petal_matrix* w_out, int64_t* kernel_path);

/* loss[0] = the loss the model was fitted with (a model of petal_nmf_fit or petal_nmf_fit_csr: PETAL_NMF_LOSS_FROBENIUS). */
int petal_nmf_get_loss(const petal_nmf* h, int64_t* loss);

/* test aid: HOST float64 g_in (R x k), f (C x k); transposed selects the image; spec's l1_w, l2_w are THE penalties of the sweep; c is
 * formed by the call; g_out (R x k), colsum_out (k, nullable), term_out (1, nullable; accepted with inner_iters == 0 only, when g_out is
 * g_in); info1 = { k_nmf_kl_sweep ran }.  The device G is formed inside a guard (one row more, every byte 0xFF beforehand):
 * PETAL_DEVICE_ERROR "nmf_kl_sweep wrote outside the R x k block" if the guard or a padding column changed.  On a handle that is not
 * resident: the plain host loop of the same statement in position order.  k > 64 on a resident handle: PETAL_INVALID_INPUT. */
int petal_nmf_kl_sweep_csr(petal_ctx* ctx, const petal_csr* x, int transposed, int64_t k, const double* g_in, const double* f,
                           const petal_nmf_spec* spec, int64_t inner_iters, double* g_out, double* colsum_out, double* term_out, int64_t* info1);

#ifdef __cplusplus
}
#endif

#endif /* PETAL_HIP_NMF_KL_H */
