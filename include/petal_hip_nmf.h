/* petal_hip_nmf.h -- Nmf: non-negative matrix factorisation X ~ W H by multiplicative updates for the Frobenius loss.  An extension
 * beyond the crate's interface (DESIGN.md sections 4 and 7), declared beside petal_hip.h.  The model is scikit-learn's
 * NMF(solver="mu", beta_loss=2).
 *
 * X is n x d with X >= 0, W is n x k, H is k x d.  eps = 2^-23 (float32's machine epsilon) for both data types.  One iteration:
 *
 *     D = W (H H^T) + l1_w + l2_w W ;  D[D == 0] = eps ;  W <- W o (X H^T) / D
 *     E = (W^T W) H + l1_h + l2_h H ;  E[E == 0] = eps ;  H <- H o (W^T X) / E          (the NEW W)
 *
 * Loss.  err = sqrt(max(0, |X|^2 - 2 <W^T X, H> + <W^T W, H H^T>)), with W^T X and W^T W as the iteration formed them and the H just
 * updated: no extra pass over X.
 * Stopping.  tol > 0: after every 10th iteration, stop if (err_prev - err) / err_init < tol; err_init is the loss at the initial
 * (W, H), err_prev the loss at the previous check (at the first check: err_init).  tol = 0 runs exactly max_iter iterations.
 * transform(Xq), H fixed: W0 = sqrt(mean(Xq) / k) in every entry, then exactly max_iter W-updates with the fit's l1_w, l2_w -- ONE pass
 * over Xq whatever max_iter is (X H^T does not change between the updates).  No tolerance stop in transform.
 * inverse_transform(W) = W H.
 * Initialisation.  w0 and h0 given ("custom"), or both null ("random"): avg = sqrt(mean(X) / k), W0 = |avg N(0,1)| (n x k, drawn
 * first), then H0 (k x d), both filled in row-major order from the Pcg stream (Mcg128Xsl64 + Ziggurat, petal_decomposition.hpp's Pcg)
 * whose state is `seed` (its 64 bits, unsigned).
 * scikit-learn's alpha_W, alpha_H, l1_ratio map as l1_w = d alpha_W rho, l2_w = d alpha_W (1 - rho), l1_h = n alpha_H rho,
 * l2_h = n alpha_H (1 - rho).
 *
 * An iteration is ONE fused pass over X (k_nmf_pass: X H^T, the W rule in registers, W^T X and W^T W with the new W) and k x d work on
 * H.  X comes from memory once per iteration; there is no n x k or n x d intermediate but W itself.
 *
 * Results contract.  Everything is float64 inside: X is widened on load, W and H live in float64 on the device during a fit whatever
 * the data's type, every product and sum is float64 in an order the shape alone fixes, outputs are rounded once to the data's type.
 * No floating-point atomics: the same input gives the same bytes.
 *
 * Not in this version: other beta-losses, the coordinate-descent solver, NNDSVD initialisation, CSR input, sharded fits, float32 /
 * split-bf16 products, a tolerance stop in transform.  CSR input and sharded fits are the natural follow-ups: the W rule is row-local
 * and W^T X, W^T W are sums over rows.  (CSR input has since been added beside this header: petal_hip_nmf_sparse.h; the
 * Kullback-Leibler loss on CSR input: petal_hip_nmf_kl.h; the
 * coordinate-descent solver on dense input: petal_hip_nmf_cd.h.)
 */
#ifndef PETAL_HIP_NMF_H
#define PETAL_HIP_NMF_H

#include "petal_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* petal_ctx_set_option: non-zero = the pass, the scan and the H update are built from the library's other products (widen, fp64 GEMM)
 * and an element-wise step on the host, walking X in row blocks of bounded size, instead of k_nmf_pass / k_nmf_scan / k_nmf_hrule -- a
 * test and A/B aid like PETAL_OPT_KPCA_FALLBACK; no environment variable.  The same path is taken where the device-op layer lacks the
 * kernels, the shape is outside their envelope (k > 64, more than 512 padded columns) or a matrix does not allow their 16-byte loads.
 * (38: tests hold 35 and 37 to "unknown option".) */
#define PETAL_OPT_NMF_FALLBACK 38

typedef struct petal_nmf_spec {
    int64_t max_iter;                  /* >= 1 */
    double tol, l1_w, l2_w, l1_h, l2_h; /* >= 0 */
} petal_nmf_spec;

typedef struct petal_nmf petal_nmf;

/* Fits on x (n x d; float32 or float64, host or device, any strides petal_pca_fit takes) and returns a handle that lives with the ctx.
 * w0 (n x k) and h0 (k x d): matrices in x's dtype, both given or both null (random, from `seed`).  w_out (nullable, n x k in x's
 * dtype): fit_transform's W.  Errors, PETAL_INVALID_INPUT: k < 1, k > min(n, d) "every dimension should be at least k", n = 0, d = 0,
 * negative penalties or tol, max_iter < 1, a negative entry in x, w0 or h0 "negative values in data", one of w0 / h0 alone, a wrong
 * shape, a sharded ctx; PETAL_LINALG_ERROR "did not converge": NaN or infinity in x, w0 or h0. */
int petal_nmf_fit(petal_ctx* ctx, const petal_matrix* x, int64_t k, const petal_nmf_spec* spec, const petal_matrix* w0, const petal_matrix* h0,
                  int64_t seed, petal_nmf** out, const petal_matrix* w_out);
void petal_nmf_destroy(petal_nmf* h);

/* w_out (m x k, the fit's dtype) = transform(x), x: m x d in the fit's dtype.  Another width: "# of columns should be d"; a negative
 * entry: "negative values in data". */
int petal_nmf_transform(petal_ctx* ctx, petal_nmf* h, const petal_matrix* x, const petal_matrix* w_out);
/* x_out (m x d) = w (m x k) H, rounded once. */
int petal_nmf_inverse_transform(petal_ctx* ctx, petal_nmf* h, const petal_matrix* w, const petal_matrix* x_out);

/* components (nullable): HOST float64, k x d row-major: H.  info6 (nullable) = { n, d, k, n_iter, the kernel ran in the fit (1) or the
 * composed path did (0), the kernel ran in the last transform (1 / 0; -1 before the first) }.  err2 (nullable) = { reconstruction_err,
 * err_init }. */
int petal_nmf_get(const petal_nmf* h, double* components, int64_t* info6, double* err2);

/* The pass by itself (a test aid in the manner of petal_kernel_apply), HOST float64 operands and results: with w_in (n x k) and
 * h (k x d), Z = x h^T once, then inner_iters times the W rule with spec's l1_w, l2_w (inner_iters = 0: none); w_out (n x k) = the
 * result, a_out (k x d, nullable) = w_out^T x, b_out (k x k, nullable; with a_out or not at all) = w_out^T w_out.  spec's other fields
 * are not read.  The device W is formed inside a guard (a row more, every byte 0xFF beforehand): PETAL_DEVICE_ERROR "nmf_pass wrote
 * outside the n x k block" if the guard changed.  info1 (nullable) = { k_nmf_pass ran }.  A sharded ctx is PETAL_INVALID_INPUT. */
int petal_nmf_pass(petal_ctx* ctx, const petal_matrix* x, int64_t k, const double* w_in, const double* h, const petal_nmf_spec* spec, int64_t inner_iters,
                   double* w_out, double* a_out, double* b_out, int64_t* info1);

#ifdef __cplusplus
}
#endif

#endif /* PETAL_HIP_NMF_H */
