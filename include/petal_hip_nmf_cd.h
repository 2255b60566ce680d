/* petal_hip_nmf_cd.h -- Nmf with the coordinate-descent solver on DENSE data under the Frobenius loss: scikit-learn's
 * NMF(solver="cd"), its default solver, with its default shuffle=False.  An extension beyond the crate's interface (DESIGN.md sections 4
 * and 7), declared beside petal_hip_nmf.h (the model handle, petal_nmf_spec, the initialisation, the penalty mapping, the loss) and
 * petal_hip_nmf_kl_dense.h.  Every existing signature, message and refusal stays; petal_nmf_spec is unchanged.
 *
 * The statement.  eps is not used.  X is n x d with X >= 0, W is n x k, H is k x d.  With S = H H^T + l2 I (l2 on the first k diagonal
 * entries) and z = (X H^T)[i, :] - l1, one sweep of a row w of W runs t = 0 .. k - 1 in order:
 *
 *     grad = -z[t] + sum_r S[t][r] w[r]            (the CURRENT w: coordinates < t are already new)
 *     pg   = (w[t] == 0) ? min(0, grad) : grad ;   violation += |pg|
 *     if S[t][t] != 0:  w[t] = max(w[t] - grad / S[t][t], 0)
 *
 * The H side is the same sweep on the rows of H^T (one per feature j) with z = (W^T X)[:, j] - l1_h and S = W^T W + l2_h I, using the
 * NEW W.  No shuffling.  One iteration is the W sweep, then the H sweep; its violation is the sum of both.
 * Stopping.  tol > 0: after EVERY iteration, with violation_init the violation of iteration 1, stop if violation_init == 0 or
 * violation / violation_init <= tol -- scikit-learn's rule, so the same n_iter.  tol = 0 runs exactly max_iter iterations (this
 * project's convention; scikit-learn would stop at a fixed point, where further iterations change nothing, so only n_iter can differ).
 * transform(Xq), H fixed: W starts at ZERO (scikit-learn's start for this solver, not sqrt(mean / k)), then exactly max_iter sweeps on
 * the fixed X H^T with the fit's l1_w, l2_w -- ONE pass over Xq whatever max_iter is.  No tolerance stop in transform.
 * The loss (reconstruction_err, err_init), the initialisation ("custom" or the Pcg draw, bit for bit) and the penalty mapping are
 * petal_hip_nmf.h's: err = sqrt(max(0, |X|^2 - 2 <W^T X, H> + <W^T W, H H^T>)) from the iteration's own products and the H just updated.
 * Padded components stay zero and add nothing to the violation (z = -l1, w = 0: grad >= 0, pg = 0; S[t][t] = 0 skips the update: l2
 * stays off the padded diagonal).
 *
 * Results contract (Nmf's).  Everything is float64 inside: X is widened on load, W, H, every product, sum and quotient are float64;
 * there are no floating-point atomics and the order of every sum is a function of the shape alone (tiles of 16 rows, at most 256
 * persistent workgroups whose slabs and violations are added in workgroup order): the same input gives the same bytes; outputs are
 * rounded once to the data's type.  Inside the kernel a lane keeps g = S w - z for its coordinates and adds (w_new[t] - w[t]) S[t][:]
 * after every step; g is formed afresh from w at the start of every sweep, so the sweeps of a transform do not accumulate drift.  The
 * kernel and the composed path therefore agree to rounding, not to the byte.
 *
 * Where it runs.  k_nmf_cd_pass (fit_kernel / transform_kernel 1) inside k_nmf_pass's envelope: 16, 32 or 64 padded components (k <= 32
 * or 49 <= k <= 64), at most 512 padded columns, rows that allow 16-byte loads.  An iteration reads X from memory once, has no n x k
 * intermediate but W, and transform reads Xq once whatever max_iter is.  Everything else -- a device-op layer without the kernels (the
 * host simulation of the tests), PETAL_OPT_NMF_FALLBACK, k = 33 .. 48, k > 64, more than 512 padded columns -- takes the composed path
 * (0): op_cvt_to_f64 and op_dgemm for X H^T, W^T X and W^T W in row blocks of bounded size, the sweep on the host over read-back
 * copies, blocks added in block order.  With tol > 0 a fit reads two doubles back after every iteration; with tol = 0 the whole fit is
 * queued without a host round trip.  What that read-back costs is unmeasured.
 *
 * Measured: see README.md (Nmf with the coordinate-descent solver) and EXPERIMENTS.md; every figure not measured on the device is
 * marked "unmeasured".
 *
 * Not in this version: coordinate descent with the Kullback-Leibler loss (scikit-learn refuses it too), coordinate descent on CSR input
 * (a k_nmf_sweep variant is the natural follow-up), sharded fits, shuffle=True, a tolerance stop in transform, a kernel for 48 padded
 * components or more than 512 padded columns.  (Coordinate descent on CSR input has since been added beside this header:
 * petal_hip_nmf_cd_sparse.h.)
 */
#ifndef PETAL_HIP_NMF_CD_H
#define PETAL_HIP_NMF_CD_H

#include "petal_hip_nmf_kl_dense.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PETAL_NMF_SOLVER_MU 0
#define PETAL_NMF_SOLVER_CD 1

/* petal_nmf_fit with a solver.  PETAL_NMF_SOLVER_MU is petal_nmf_fit bit for bit; PETAL_NMF_SOLVER_CD is the coordinate-descent fit
 * above; any other value is PETAL_INVALID_INPUT "unknown solver".  Arguments, outputs, errors and messages are petal_nmf_fit's.
 * petal_nmf_transform and petal_nmf_transform_loss on a handle fitted with PETAL_NMF_SOLVER_CD run the coordinate-descent transform;
 * petal_nmf_transform_csr refuses such a handle. */
int petal_nmf_fit_solver(petal_ctx* ctx, const petal_matrix* x, int64_t k, const petal_nmf_spec* spec, int64_t solver, const petal_matrix* w0,
                         const petal_matrix* h0, int64_t seed, petal_nmf** out, const petal_matrix* w_out);
int petal_nmf_get_solver(const petal_nmf* h, int64_t* solver);

/* test aid: the pass by itself on HOST float64 w_in (n x k) and h (k x d); Z = x h^T once, then inner_iters sweeps of every row with
 * spec's l1_w, l2_w (from_zero != 0: W starts as zeros instead of w_in; inner_iters == 0: w_in comes back).  w_out (n x k) = the
 * result; a_out (k x d, nullable) = w_out^T x, b_out (k x k, nullable; with a_out or not at all) = w_out^T w_out; violation_out
 * (nullable): inner_iters doubles, one per sweep; info1 = { k_nmf_cd_pass ran }.  The device W is formed inside a guard (a row in
 * front and a row behind, every byte 0xFF beforehand): PETAL_DEVICE_ERROR "nmf_cd_pass wrote outside the n x k block" if a guard row
 * or a padding column changed.  A sharded ctx is PETAL_INVALID_INPUT. */
int petal_nmf_cd_pass(petal_ctx* ctx, const petal_matrix* x, int64_t k, const double* w_in, const double* h, const petal_nmf_spec* spec,
                      int64_t inner_iters, int from_zero, double* w_out, double* a_out, double* b_out, double* violation_out, int64_t* info1);

/* test aid: the H side by itself on HOST float64 a (k x d), b (k x k) and h_in (k x d): one sweep of every row of h_in^T with spec's
 * l1_h, l2_h; h_out (k x d) = the result, violation_out (nullable, 1 double), info1 = { k_nmf_cd_hrule ran }. */
int petal_nmf_cd_hupdate(petal_ctx* ctx, int64_t k, int64_t d, const double* a, const double* b, const double* h_in, const petal_nmf_spec* spec,
                         double* h_out, double* violation_out, int64_t* info1);

#ifdef __cplusplus
}
#endif

#endif /* PETAL_HIP_NMF_CD_H */
