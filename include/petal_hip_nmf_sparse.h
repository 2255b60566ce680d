/* petal_hip_nmf_sparse.h -- Nmf on sparse data in CSR form: fit and transform without densifying (term-document counts, expression
 * tables, click matrices).  An extension beyond the crate's interface (DESIGN.md sections 4 and 7), declared beside petal_hip_nmf.h
 * (the model, the statement of an iteration, the loss, the stopping rule, the initialisation) and petal_hip_sparse.h (the resident
 * handle: checked, transposed once on the host, cut into work items of at most PETAL_CSR_ITEM_NNZ stored entries).
 *
 * On sparse X an iteration is two SWEEPS of the same shape: one over the rows of X updates W, one over the rows of X^T (the transposed
 * image the handle already holds) updates H.  In both a row gathers the rows of the OTHER factor at its stored entries, applies the
 * multiplicative rule in registers and stores its own factor row; A = W^T X (k x d) is never formed.  "Sweep" of an image M (R x C,
 * M = X or X^T) with G (R x k, updated), F (C x k, gathered), S = F^T F (k x k), penalties l1 and l2, and inner >= 0:
 *
 *     z_r = sum over the stored entries t of row r of val[t] * F[idx[t], :]
 *     inner times:  D = g_r S + l1 + l2 g_r ;  D[D == 0] = 2^-23 ;  g_r <- g_r o (z_r / D)
 *     outputs:  G (new),  Gram = G^T G (new G),  dot = sum_r <z_r, g_r>  (new G)
 *
 * One fit iteration: the row sweep on the matrix with G = W, F = H^T (d x k), S = H H^T, (l1_w, l2_w), inner = 1 gives W and
 * B = W^T W; the column sweep on the transposed image with G = H^T, F = W, S = B, (l1_h, l2_h), inner = 1 gives H, H H^T and
 * <W^T X, H>; the loss is sqrt(max(0, |X|^2 - 2 <W^T X, H> + <B, H H^T>)).  This is petal_hip_nmf.h's statement term for term: the same
 * eps, the same order "new W, then H with the new W", the same loss, the same stopping rule (every 10th iteration) and the same random
 * initialisation (avg = sqrt(sum(X) / (n d) / k), W0 then H0 row-major from Pcg(seed)).  The initial loss comes from Gram(W0) and a
 * column sweep with inner = 0.  transform is ONE row sweep started from the constant sqrt(mean(Xq) / k) with inner = max_iter, H fixed
 * and no Gram: one pass over Xq whatever max_iter is.  inverse_transform is petal_nmf_inverse_transform (dense W in, dense out).
 *
 * Results contract (Nmf's).  Values are widened to float64 on load; F, G, S and every product and sum are float64; the summation order
 * is a function of the handle alone (its work items) -- no floating-point atomics: the same arrays give the same bytes on every run and
 * on another handle built from them; outputs are rounded once to the data's type.
 *
 * Fall-back: densify, then the dense entry -- bit for bit petal_nmf_fit / petal_nmf_transform on the densified matrix (duplicates added
 * in position order in the data's type).  It is taken for a handle that is not resident (a device-op layer without the kernels: the
 * host simulation of the tests), with PETAL_OPT_NMF_FALLBACK set, and for k > 64 (the sparse kernel takes at most 64 components).  A
 * resident handle is densified on the device; rows x cols x the element size beyond 2^32 bytes is PETAL_INVALID_INPUT
 * "too large to densify".  kernel_path: 1 when the sweep ran, 0 when the call densified; petal_nmf_get's info6[4] and info6[5] report the same.
 *
 * Disclosed differences from the dense fit.  Stored values are checked one by one: a duplicate pair (+3, -1) is refused ("negative
 * values in data") although its sum is legal.  |X|^2 and sum(X) come from one scan of the stored values: with duplicates present |X|^2
 * is the sum of the squares of the stored values, not of the summed entries, and the reported losses differ from the dense fit's by
 * the cross terms (W and H do not).  Explicit zeros, empty rows and columns, unsorted indices and duplicates are legal; an all-zero
 * matrix behaves as the dense fit does on it.
 *
 * Measured: see README.md (Nmf on sparse data) and EXPERIMENTS.md; every figure not measured on the device is marked "unmeasured".
 *
 * Not in this version: sharded fits, device-resident CSR arrays, other beta-losses, a tolerance stop in transform, k > 64 on the sweep
 * (it densifies), CSR output of inverse_transform.  (The Kullback-Leibler loss has since been added beside this header:
 * petal_hip_nmf_kl.h.)
 */
#ifndef PETAL_HIP_NMF_SPARSE_H
#define PETAL_HIP_NMF_SPARSE_H

#include "petal_hip_nmf.h"
#include "petal_hip_sparse.h"

#ifdef __cplusplus
extern "C" {
#endif

/* petal_nmf_fit on a sparse matrix: arguments, outputs and errors as petal_nmf_fit, with the same messages (w0, h0, w_out: dense
 * matrices in the handle's dtype), plus PETAL_INVALID_INPUT for a handle of another ctx, a sharded ctx ("sharded"), w0 / h0 / w_out of
 * another dtype than the handle's and a negative stored value ("negative values in data"); PETAL_LINALG_ERROR "did not converge" for a
 * NaN or an infinity among the stored values.  The handle returned is an ordinary petal_nmf: petal_nmf_transform,
 * petal_nmf_inverse_transform, petal_nmf_get and petal_nmf_destroy work on it.  kernel_path: nullable. */
int petal_nmf_fit_csr(petal_ctx* ctx, const petal_csr* x, int64_t k, const petal_nmf_spec* spec, const petal_matrix* w0, const petal_matrix* h0,
                      int64_t seed, petal_nmf** out, const petal_matrix* w_out, int64_t* kernel_path);

/* w_out (rows of x, k; the fit's dtype) = transform(x) for a model fitted on dense or on sparse data.  Another width: "# of columns
 * should be d"; a handle of another dtype than the model's: "dtype". */
int petal_nmf_transform_csr(petal_ctx* ctx, petal_nmf* h, const petal_csr* x, const petal_matrix* w_out, int64_t* kernel_path);

/* test aid: HOST float64 g_in (R x k), f (C x k); transposed selects the image; spec's l1_w, l2_w are THE penalties of the sweep;
 * g_out (R x k), gram_out (k x k, nullable), dot_out (1, nullable; with gram_out or not at all); info1 = { k_nmf_sweep ran }.
 * S = f^T f is formed by the call.  The device G is formed inside a guard (one row more, every byte 0xFF beforehand):
 * PETAL_DEVICE_ERROR "nmf_sweep wrote outside the R x k block" if the guard or a padding column changed.  On a handle that is not
 * resident: a plain host loop of the same statement in position order.  k > 64 on a resident handle: PETAL_INVALID_INPUT. */
int petal_nmf_sweep_csr(petal_ctx* ctx, const petal_csr* x, int transposed, int64_t k, const double* g_in, const double* f,
                        const petal_nmf_spec* spec, int64_t inner_iters, double* g_out, double* gram_out, double* dot_out, int64_t* info1);

#ifdef __cplusplus
}
#endif

#endif /* PETAL_HIP_NMF_SPARSE_H */
