/* petal_hip_nmf_cd_sparse.h -- Nmf with the coordinate-descent solver on sparse data in CSR form: scikit-learn's NMF(solver="cd"), its
 * default solver, on tf-idf, count and click matrices without densifying.  An extension beyond the crate's interface (DESIGN.md sections 4
 * and 7), declared beside petal_hip_nmf_cd.h (the sweep over the coordinates, the stopping rule, the transform from zero) and
 * petal_hip_nmf_sparse.h (the gather over the stored entries, the resident handle, the fall-back, the disclosures).  Every existing
 * signature, message and refusal stays; neither of those statements changes; petal_nmf_spec is unchanged.
 *
 * The statement.  A "cd sweep" of an image M (R x C; M = X or the transposed image the handle already holds) with G (R x k, updated),
 * F (C x k, gathered), S = F^T F + l2 I (l2 on the first k diagonal entries only), the penalty l1 and inner >= 0 does for each row r:
 *
 *     z_r = sum over the stored entries t of row r of val[t] * F[idx[t], :]            (petal_hip_nmf_sparse.h's gather)
 *     inner times, coordinates t = 0 .. k - 1 in order, on the CURRENT g_r:             (petal_hip_nmf_cd.h's sweep, with z = z_r - l1)
 *         grad = -(z_r[t] - l1) + sum_j S[t][j] g_r[j]
 *         pg   = (g_r[t] == 0) ? min(0, grad) : grad ;   violation += |pg|
 *         if S[t][t] != 0:  g_r[t] = max(g_r[t] - grad / S[t][t], 0)
 *     outputs:  G (new),  Gram = G^T G (new G),  dot = sum_r <z_r, g_r>  (the raw z_r, the new g_r),  one violation per sweep
 *
 * A row with no stored entries is still swept, with z = -l1.  Padded components stay zero and add no violation.  from_zero starts G at
 * zero (scikit-learn's start for transform under this solver).
 * One fit iteration is two sweeps: the row sweep with G = W, F = H^T, S = H H^T + l2_w I and l1_w gives W, B = W^T W and the W
 * violation; the column sweep on the transposed image with G = H^T, F = the NEW W, S = B + l2_h I and l1_h gives H, H H^T, <W^T X, H>
 * and the H violation.  No shuffling.  Everything else is petal_hip_nmf_cd.h's and petal_hip_nmf_sparse.h's, term for term: the loss
 * sqrt(max(0, |X|^2 - 2 <W^T X, H> + <B, H H^T>)) from the iteration's own products; the stopping rule (tol > 0: after EVERY iteration
 * stop if violation_init == 0 or violation / violation_init <= tol; tol = 0 runs exactly max_iter iterations); the initialisation of
 * petal_nmf_fit_csr ("custom" W and H, or the Pcg draw bit for bit with avg = sqrt(sum(X) / (n d) / k)); the initial loss from
 * Gram(W0) and a column sweep with inner = 0.  transform is ONE row sweep with from_zero and inner = max_iter: one pass over the query
 * matrix whatever max_iter is, no tolerance stop.
 *
 * Results contract (Nmf's).  Values are widened to float64 on load; F, G, S and every product, sum and quotient are float64; there are
 * no floating-point atomics and the order of every sum -- the sum of the violations among them -- is a function of the handle (its
 * work items) and the padded k alone: the same arrays give the same bytes on every run and on a second handle built from them; outputs
 * are rounded once to the data's type.  The sweep kernel and the dense coordinate-descent paths sum z in different orders: they agree
 * to rounding, not to the byte.
 *
 * Where it runs.  k_nmf_cd_sweep on a resident handle with k <= 64 (16, 32 or 64 padded components): a wave gathers four work items
 * in turn and then sweeps four rows at once, one per 16-lane group.  Fall-back: densify, then the dense entry -- bit for bit
 * petal_nmf_fit_solver(..., PETAL_NMF_SOLVER_CD, ...) / petal_nmf_transform on the densified matrix (duplicates added in position order
 * in the data's type).  It is taken for a handle that is not resident (a device-op layer without the kernels: the host simulation of
 * the tests), with PETAL_OPT_NMF_FALLBACK set, and for k > 64; rows x cols x the element size beyond 2^32 bytes is PETAL_INVALID_INPUT
 * "too large to densify".  kernel_path: 1 when the sweep ran, 0 when the call densified.  With tol > 0 a fit reads two doubles back
 * after every iteration; with tol = 0 the whole fit is queued without a host round trip.
 *
 * Disclosed differences from the dense fit: those of petal_hip_nmf_sparse.h.  Stored values are checked one by one (a duplicate pair
 * (+3, -1) is refused, "negative values in data", although its sum is legal); |X|^2 and sum(X) come from one scan of the stored values,
 * so with duplicates present the reported losses differ from the dense fit's by the cross terms (W and H do not).
 *
 * Measured: see README.md (Nmf with the coordinate-descent solver on sparse data) and EXPERIMENTS.md; every figure not measured on the
 * device is marked "unmeasured".
 *
 * Not in this version: sharded fits, shuffle=True, a tolerance stop in transform, k > 64 on the sweep (it densifies), coordinate
 * descent with the Kullback-Leibler loss.
 */
#ifndef PETAL_HIP_NMF_CD_SPARSE_H
#define PETAL_HIP_NMF_CD_SPARSE_H

#include "petal_hip_nmf_cd.h"
#include "petal_hip_nmf_sparse.h"

#ifdef __cplusplus
extern "C" {
#endif

/* petal_nmf_fit_csr with a solver.  PETAL_NMF_SOLVER_MU is petal_nmf_fit_csr bit for bit; PETAL_NMF_SOLVER_CD is the fit above; any
 * other value is PETAL_INVALID_INPUT "unknown solver".  Arguments, outputs, errors and messages are petal_nmf_fit_csr's.  The handle
 * returned is an ordinary petal_nmf (petal_nmf_get_solver: PETAL_NMF_SOLVER_CD): the dense petal_nmf_transform,
 * petal_nmf_inverse_transform and petal_nmf_get work on it. */
int petal_nmf_fit_csr_solver(petal_ctx* ctx, const petal_csr* x, int64_t k, const petal_nmf_spec* spec, int64_t solver, const petal_matrix* w0,
                             const petal_matrix* h0, int64_t seed, petal_nmf** out, const petal_matrix* w_out, int64_t* kernel_path);

/* petal_nmf_transform_csr for every solver: on a handle fitted with PETAL_NMF_SOLVER_MU, of either loss, it is petal_nmf_transform_csr
 * bit for bit; on a handle fitted with PETAL_NMF_SOLVER_CD, on dense or on sparse data, it runs the transform above.
 * (petal_nmf_transform_csr itself still refuses such a handle.) */
int petal_nmf_transform_csr_solver(petal_ctx* ctx, petal_nmf* h, const petal_csr* x, const petal_matrix* w_out, int64_t* kernel_path);

/* test aid: one cd sweep by itself on HOST float64 g_in (R x k) and f (C x k); transposed selects the image; spec's l1_w, l2_w are THE
 * penalties of the sweep; S = f^T f is formed by the call.  from_zero != 0 with inner_iters > 0: G starts as zeros instead of g_in;
 * inner_iters == 0: g_in comes back; at most 1024 sweeps.  g_out (R x k), gram_out (k x k, nullable), dot_out (1, nullable; with
 * gram_out or not at all), violation_out (nullable): inner_iters doubles, one per sweep; info1 = { k_nmf_cd_sweep ran }.  The device G
 * is formed inside a guard (one row more, every byte 0xFF beforehand): PETAL_DEVICE_ERROR "nmf_cd_sweep wrote outside the R x k block"
 * if the guard or a padding column changed.  On a handle that is not resident: a plain host loop of the same statement in position
 * order.  k > 64 on a resident handle and a sharded ctx: PETAL_INVALID_INPUT. */
int petal_nmf_cd_sweep_csr(petal_ctx* ctx, const petal_csr* x, int transposed, int64_t k, const double* g_in, const double* f,
                           const petal_nmf_spec* spec, int64_t inner_iters, int from_zero, double* g_out, double* gram_out, double* dot_out,
                           double* violation_out, int64_t* info1);

#ifdef __cplusplus
}
#endif

#endif /* PETAL_HIP_NMF_CD_SPARSE_H */
