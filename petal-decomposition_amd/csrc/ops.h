// ops.h -- the device-operation layer the host algorithms (algo.cpp) are written against.
//
// The product library links exactly one implementation: hip_ops.hip (hand-written gfx950 kernels).
// tests/ additionally build a host-memory simulation of the same functions from oracle/cpu_ops.cpp
// (TEST INFRASTRUCTURE, never linked into the product) so that the host algorithms and the
// sample-sharded collective path can be exercised without a GPU (world_size-2 gloo test).
//
// All matrices are row-major.  "f64 small" matrices live in device memory as doubles: everything
// that is O(l^2), O(d l) or O(nc^2) is kept in fp64 so that only the O(n) streams are fp32.
#pragma once
#include <cstddef>
#include <cstdint>

namespace petal {

enum DType : int { F32 = 0, F64 = 1 };
inline size_t dtype_size(int dt) { return dt == F64 ? 8 : 4; }

struct Dev;  // opaque: stream, allocator cache, event pool (hip) / nothing much (cpu sim)

// hot-kernel tags: launches issued while a tag is set are bracketed with events when profiling is on
// (TAG_STREAM: the other kernels of a fit whose time falls with the rows a rank holds -- the means pass, U = Z (T Uh) -- so that
// fit time minus every tagged kernel is the REPLICATED small-matrix chain, the part of a sharded fit that does not shrink with N)
enum Tag : int { TAG_NONE = 0, TAG_XP = 1, TAG_ATB = 2, TAG_ICA = 3, TAG_COMM = 4, TAG_POW = 5, TAG_STREAM = 6, TAG_COUNT = 7 };
struct KernelTiming {
    double ms[TAG_COUNT] = {0, 0, 0, 0, 0, 0, 0};
    int64_t launches[TAG_COUNT] = {0, 0, 0, 0, 0, 0, 0};
};

// ---- lifetime / memory ---------------------------------------------------------------------
Dev*  dev_create(int device, void* stream, char* err, size_t errlen);  // nullptr on failure
void  dev_destroy(Dev*);
void* dev_stream(Dev*);
void* dev_alloc(Dev*, size_t bytes);      // cached; never returns nullptr (throws std::runtime_error)
void  dev_free(Dev*, void*);
bool  dev_live(Dev*, int64_t* blocks, int64_t* bytes);   // the blocks handed out and not yet returned; false: this layer keeps no count (algo.cpp's weak default)
void  dev_memset(Dev*, void* p, int v, size_t bytes);
void  dev_h2d(Dev*, void* dst, const void* src, size_t bytes);
void  dev_h2d_async(Dev*, void* dst, const void* src, size_t bytes);  // src is consumed before the call returns; no host wait
void  dev_d2h(Dev*, void* dst, const void* src, size_t bytes);  // dst is valid after the next dev_sync
void  dev_d2h_multi(Dev*, int nseg, void* const* dst, const void* const* src, const size_t* bytes);   // several dev_d2h in one launch (nseg <= 8)
const void* dev_h2d_view(Dev*, const void* src, size_t bytes);   // host bytes staged in the pinned ring; returns its device-visible address (nullptr: too large), valid until the next dev_sync
const void* dev_d2h_view(Dev*, const void* src, size_t bytes);   // the result where the copy lands (pinned ring): readable after the next dev_sync, until the next copy is queued
size_t dev_view_limit(Dev*);                                     // the largest dev_d2h_view / dev_h2d_view (one ring slot); dev_d2h_view THROWS above it
void  dev_d2d(Dev*, void* dst, const void* src, size_t bytes);
// pitched copies (bytes); kind: 0 h2d, 1 d2h, 2 d2d
void  dev_copy2d(Dev*, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height, int kind);
void  dev_sync(Dev*);
void  dev_set_profiling(Dev*, int level);   // 0 off, 1 one sampled launch per tag and fit, 2 every tagged launch
// Options of a device context: every switch that selects WHICH arithmetic or kernel form a fit runs.  The defaults come from the
// environment ONCE, at dev_create (the variable named with each); afterwards only dev_set_option (petal_ctx_set_option) changes
// them -- no kernel launcher reads the environment.  The values equal include/petal_hip.h's PETAL_OPT_*.
enum PetalOpt {
    OPT_TWO_PLANE = 0,         // (1) optimistic first run of an fp32 RandomizedPca fit: sketch matrix and re-based iterates on two bf16 planes,
                               //     behind the spectrum verdict; 0 = three planes throughout                       env PETAL_NO_P2=1 -> 0
    OPT_TWO_PLANE_OMEGA = 1,   // (1) ... the sketch matrix alone                                                     env PETAL_NO_P2_OMEGA=1 -> 0
    OPT_TWO_PLANE_ITERATE = 2, // (1) ... the re-based iterates alone                                                 env PETAL_NO_P2_ITERATE=1 -> 0
    OPT_STEERING = 3,          // (1) the passes before the last one round Xc and z to two planes as well             env PETAL_NO_POW3_FAST=1 -> 0
    OPT_FUSED_PASS = 4,        // (1) the fused power-iteration pass where the kernel exists                          env PETAL_NO_POW3=1 -> 0
    OPT_FUSED_PASS_MIN_ROWS = 5, // (8192) fewer rows: K1 + K2                                                        env PETAL_POW3_MIN_ROWS
    OPT_VERDICT_THRESHOLD = 6, // (4e-6) the two-plane verdict redoes a fit whose estimated component error exceeds it  env PETAL_P2_VERDICT_THR
    OPT_MEANS_FOLD_ROWS = 7,   // (200000) single-rank fp32 fits gather the means inside the first pass from this many rows on; < 0: never
                               //                                                      env PETAL_MEANS_FOLD_ROWS, PETAL_NO_MEANS_FOLD=1 -> -1
    OPT_GRAM_SPLIT = 8,        // (1) FastICA whitening: the optimistic split-product covariance (k_gram5); 0 = fp64 products   env PETAL_NO_GRAM3=1 -> 0
    OPT_GRAM_SPLIT_HOOK = 9,   // (0) test hook: petal_gemm_atb sends Gram products to the split-product Gram kernel  env PETAL_GRAM_SPLIT=1
    OPT_D2H_KERNEL = 10,       // (1) small results leave through a copy kernel into the pinned ring; 0 = hipMemcpyAsync  env PETAL_D2H_MEMCPY=1 -> 0
    OPT_ROW_PAD = 11,          // (1) copied inputs land with 128 B of row padding when the natural pitch is a multiple of 1 KiB  env PETAL_NO_ROW_PAD=1 -> 0
    OPT_EIGH_JACOBI = 12,      // (0) symmetric eigenproblems go straight to the Jacobi solvers                        env PETAL_EIGH_JACOBI=1
    OPT_POISON = 13,           // (0) every workspace block is filled with NaN patterns when handed out (tests)         env PETAL_POISON=1
    // (14 is PETAL_OPT_FORCE_COLLECTIVE: it lives in the ctx, not in the device layer)
    OPT_STEERING_HOOK = 15,    // (0) test hook: petal_gemm_xp / petal_gemm_atb / petal_power_pass (without z) ask for the steering forms   no env
    OPT_COUNT = 16
};
void   dev_set_option(Dev*, int opt, double value);
double dev_option(const Dev*, int opt);
void  dev_set_gemm_mode(Dev*, int mode);    // 0 = split-product (bf16x3) GEMM kernels for fp32 data, 1 = fp32-MFMA kernels
int   dev_gemm_mode(const Dev*);
void  dev_make_current(Dev*);               // hipSetDevice(the ctx's device) on the calling thread
int   dev_push_current(Dev*);               // the same, returning the thread's previous device (-1: none) ...
void  dev_pop_current(Dev*, int prev);      // ... which this restores: every ABI entry point brackets its work with the pair
void  dev_abort(Dev*);                     // error path: wait for the stream, drop queued device-to-host hand-overs
void  dev_reset_timing(Dev*);
void  dev_set_tag(Dev*, int tag);
// side stream for work that does not depend on the main chain: launches between dev_fork and dev_fork_end go to it (behind
// everything queued so far; at once with after_main = false), dev_join makes the main stream wait for it; dev_fork_abort is the
// error path
void  dev_fork(Dev*, bool after_main = true);
void  dev_fork_end(Dev*);
void  dev_join(Dev*);
void  dev_fork_abort(Dev*);
KernelTiming dev_timing(Dev*);            // resolves pending events (call after dev_sync)
// Brackets stream work that is not one of this file's kernels (the collective) with the same event machinery as the tagged
// kernels: begin returns a token (nullptr when this launch is not sampled), end records the closing event.
void* dev_span_begin(Dev*, int tag);
void  dev_span_end(Dev*, void* token);

// ---- O(n) streaming ops --------------------------------------------------------------------
// dst[i*ld_dst + j] = src[i*rs + j*cs] for j < d, 0 for d <= j < d_pad   (device -> device gather)
void op_pack_strided(Dev*, int dtype, const void* src, int64_t n, int64_t d, int64_t rs, int64_t cs,
                     void* dst, int64_t ld_dst, int64_t d_pad);
// dst[i*rs + j*cs] = src[i*ld_src + j] (device -> device scatter), j < d
void op_unpack_strided(Dev*, int dtype, const void* src, int64_t n, int64_t d, int64_t ld_src,
                       void* dst, int64_t rs, int64_t cs, const double* scale = nullptr);   // scale (device, d doubles): dst = src * scale[j]
// out[j] = sum_i X[i][j]  (fp64, deterministic order)
// with_sq: out has 2 d entries, [column sums | column sums of squares]
void op_colsum(Dev*, int dtype, const void* X, int64_t n, int64_t d, int64_t ldx, double* out, bool with_sq = false);
// single-rank column means in one go: mu64[j] = (sum_i X_ij) / n_total, mu64[d + j] = sum_i X_ij^2 (with_sq), muT = the means in dtype
void op_colmean(Dev*, int dtype, const void* X, int64_t n, int64_t d, int64_t ldx, double n_total, double* mu64, void* muT, bool with_sq);
// Z[n x N] = (X[n x K] - mu) . P[K x N] * 1 + bias        (mu, bias nullable; mu/bias in dtype)
// P is an f64 small matrix (ldp).  sumsq (nullable, fp64 scalar): += sum_ij (X_ij - mu_j)^2.
// colscale (nullable, f64[N]): Z[:, j] *= colscale[j].
// p_planes = 2: the caller accepts P rounded to the sum of its two leading bf16 pieces (a random sketch matrix: any matrix
// serves) -- the split-product kernel then forms five piece products instead of six; other paths ignore it.
void op_gemm_xp(Dev*, int dtype, const void* X, int64_t n, int64_t K, int64_t ldx, const void* mu,
                const double* P, int64_t N, int64_t ldp, const void* bias,
                void* Z, int64_t ldz, double* sumsq, int p_planes = 3, bool steering = false);
// steering (op_gemm_xp, op_rebase_xp with p_planes = 2; op_gemm_atb): the product only STEERS a power iteration -- the split-product
// kernels may round the LARGE operands (Xc; Xc and Z) to two bf16 planes as well: four piece products per tile (the forms for more than
// 80 columns; see op_power_pass).
// op_gemm_xp with P = A . T formed on the fly (A: K x M, lda; T: M x N, ldt; both fp64 small matrices): the re-basing
// product Y = Yp T of the power iteration goes straight into the GEMM kernel's operand planes instead of through a GEMM
// launch of its own.  P_out (nullable, K x N fp64, ldpo) also receives the product.
void op_gemm_xp_prod(Dev*, int dtype, const void* X, int64_t n, int64_t K, int64_t ldx, const void* mu,
                     const double* A, int64_t M, int64_t lda, const double* T, int64_t N, int64_t ldt,
                     double* P_out, int64_t ldpo, void* Z, int64_t ldz);
// op_gemm_xp_prod followed by op_col_absmax over the N columns of the product Z (svd_flip's scan, pca.rs:826-839), the scan taken
// from the product kernel's accumulators where that kernel runs (no second pass over Z).
void op_gemm_xp_prod_absmax(Dev*, int dtype, const void* X, int64_t n, int64_t K, int64_t ldx, const void* mu,
                            const double* A, int64_t M, int64_t lda, const double* T, int64_t N, int64_t ldt,
                            double* P_out, int64_t ldpo, void* Z, int64_t ldz,
                            int64_t row_offset, double* absmax, double* idx, double* sign, bool store_product = true, bool a_rt = false);
// (a_rt: A is not a matrix to multiply with but an upper-triangular R in RT form, as op_chol_rt left it -- P = R^-1 T by blocked back
//  substitution; only after op_chol_rt returned true)
// (store_product = false: Z may be left unwritten where the scan comes out of the product kernel's accumulators)
// op_gemm_xp with the same scan (absmax / idx / sign: N doubles each, as op_col_absmax delivers them over the leading N columns)
void op_gemm_xp_absmax(Dev*, int dtype, const void* X, int64_t n, int64_t K, int64_t ldx, const void* mu, const double* P, int64_t N,
                       int64_t ldp, void* Z, int64_t ldz, int64_t row_offset, double* absmax, double* idx, double* sign,
                       bool store_product = true);
// Row scores of the projection Y = (X - mu) . P, from the product kernel's accumulators in its one pass over X (an extension beyond the
// crate; a device-op layer may lack it -- algo.cpp holds a weak default that refuses):
//   st[i][0] = max(|xc_i|^2 - sum_j Y_ij^2, 0),  st[i][1] = sum_j wts[j] Y_ij^2      (st: device, n x 2 in dtype, leading dimension ldst)
// wts (nullable = all ones): device, N values in dtype.  Z (nullable, ldz): also receives Y, bit for bit op_gemm_xp's.  N == 0 is legal (q only; it takes the
// any-shape kernel, one wave per row: the slow path).
void op_gemm_xp_scores(Dev*, int dtype, const void* X, int64_t n, int64_t K, int64_t ldx, const void* mu, const double* P, int64_t N,
                       int64_t ldp, const void* wts, void* Z, int64_t ldz, void* st, int64_t ldst);
// Segmented Pca (include/petal_hip_segments.h; an extension beyond the crate): an exact Pca of every row segment [offsets[b], offsets[b + 1])
// of X (row-major, unit column stride, ldx) in ONE launch, a workgroup per segment.  offsets: HOST, nseg + 1 values, validated by the
// caller.  Results to DEVICE buffers in dtype: comp nseg x k x d (svd_flip's sign applied), means nseg x d, sing nseg x k, tv nseg;
// status nseg int32 (1: the segment holds a non-finite value -- its results and its rows of Y are NaN); Y (nullable): rows x k, leading
// dimension k, = Xc V_k^T signed.  Each returns "this layer did the work": false, NOTHING done, where the layer has no kernel for the
// shape (d > 64) or lacks the op altogether -- algo.cpp's weak defaults return false, and the caller then loops over the segments with
// the single-matrix code.  op_transform_segments / op_inverse_transform_segments: comp and means (nullable: no centring) are DEVICE
// arrays in dtype as above; Y / X out: rows x k / rows x d with leading dimension k / d.
bool op_pca_segments(Dev*, int dtype, const void* X, int64_t ldx, int64_t d, const int64_t* offsets, int64_t nseg, int64_t k, bool centering,
                     void* comp, void* means, void* sing, void* tv, int32_t* status, void* Y);
bool op_transform_segments(Dev*, int dtype, const void* X, int64_t ldx, const int64_t* offsets, int64_t nseg, const void* comp,
                           const void* means, int64_t k, int64_t d, void* Y);
bool op_inverse_transform_segments(Dev*, int dtype, const void* Y, int64_t ldy, const int64_t* offsets, int64_t nseg, const void* comp,
                                   const void* means, int64_t k, int64_t d, void* X);
// Sparse products (include/petal_hip_sparse.h; an extension beyond the crate).  One image of a CSR matrix as algo.cpp's csr_create lays
// it out in DEVICE memory: positions [first, first + count) of idx / val belong to image row `row`; a whole row is ONE item with
// slot < 0 (an empty row too: count == 0), a row of more than PETAL_CSR_ITEM_NNZ nonzeros is several consecutive items with consecutive
// slots >= 0, and `splits` names each such row with its first slot and its number of items.
struct CsrItem { int64_t first; int32_t row, count, slot, pad; };
struct CsrSplit { int32_t row, first_slot, count, pad; };
struct CsrImage {
    int64_t rows = 0, nnz = 0;             // rows of THIS image (the columns of the other one)
    const int32_t* idx = nullptr;          // nnz: the row of the dense operand each nonzero multiplies
    const void* val = nullptr;             // nnz values in the handle's dtype
    const CsrItem* items = nullptr;
    int64_t n_items = 0;
    const CsrSplit* splits = nullptr;
    int64_t n_splits = 0, n_slots = 0;
};
// Does this layer have the sparse product?  algo.cpp's weak defaults say no (and the two ops below return false, nothing done): the
// handle then keeps its host arrays and the entries densify.
bool op_csr_supported(Dev*);
// out[r, :] (img.rows x N in dtype, ldo) = sum over the nonzeros t of image row r, in position order, of val[t] * P[idx[t], :]
// (P: dtype, ldp), minus a[r] * s[:] when s != nullptr (a, s: DEVICE fp64; a == nullptr: a[r] = 1) -- the implicit centring.  N, ldp,
// ldo: multiples of 16 (the iterates' padding), P and out 16-byte aligned.  Every product and sum in fp64, no atomics: a split row's
// partial sums are added in item order by a second launch.
bool op_csr_gemm(Dev*, int dtype, const CsrImage& img, const void* P, int64_t N, int64_t ldp, const double* a, const double* s,
                 void* out, int64_t ldo);
// stats[r] = { sum_t val[t], sum_t val[t]^2 } over the nonzeros of image row r (fp64, DEVICE, 2 img.rows doubles): on the transposed
// image the column sums and column sums of squares of the matrix.
bool op_csr_colstats(Dev*, int dtype, const CsrImage& img, double* stats);
// out (rows x N in dtype, ldo) = M (rows x K in dtype, ldm) . S (K x N fp64, lds): the dense products of the sparse fit (re-basing
// M R^-1, U = Q Uh) with every product and sum in fp64 -- ONE form, independent of the ctx's GEMM mode and options (op_gemm_xp would
// send float32 data through the split-product or the fp32-MFMA kernel as the mode says).
bool op_tall_times_small(Dev*, int dtype, const void* M, int64_t rows, int64_t K, int64_t ldm, const double* S, int64_t N, int64_t lds,
                         void* out, int64_t ldo);
// IncrementalPca (include/petal_hip_ipca.h; an extension beyond the crate).  The statistic lives in DEVICE memory as fp64: M2 (dp x dp,
// symmetric, both triangles) and mean (dp); dp a multiple of 16, the padding zero.  Each returns "this layer did the work": false,
// NOTHING done, where it has no kernel for the shape (dp > 1024) or lacks the op -- algo.cpp's weak defaults return false and the
// caller then takes two passes with op_colmean / op_gemm_atb(precise) and merges pairwise.
// One batch X (m rows x dp in dtype, ldx; m > 0) in one pass about `centre` (DEVICE fp64, dp; nullable = centring off):
//     s = sum (x - centre),  G = sum (x - centre)(x - centre)^T     x widened to fp64 BEFORE the subtraction, all products and sums fp64
//     M2 += G - s s^T / (n_seen + m),   mean = centre + s / (n_seen + m)     (centre may be mean itself; centring off: M2 += G only)
// No atomics, no host round trip between the two launches.
bool op_ipca_accumulate(Dev*, int dtype, const void* X, int64_t m, int64_t dp, int64_t ldx, const double* centre, double n_seen, double* M2,
                        double* mean);
// The pairwise merge: M2_a += M2_b + (n_a n_b / n) dd^T, mean_out = mean_a + (n_b / n) d, d = mean_b - mean_a, n = n_a + n_b.
// mean_out must not be mean_a, and M2_a not M2_b.
bool op_ipca_merge(Dev*, int64_t dp, double n_a, double* M2_a, const double* mean_a, double* mean_out, double n_b, const double* M2_b,
                   const double* mean_b);
// Exact Pca's dual route on wide data (include/petal_hip_wide.h; an extension beyond the crate).  The ROW Gram matrix
//     K[i][i'] (n x n fp64, ldk; both triangles written, nothing outside the leading n x n block) = sum_j (x_ij - c_j)(x_i'j - c_j)
// of X (n rows x dp columns in dtype, ldx; dp a multiple of 16 whose padding columns hold zeros, as ingest leaves them) about `centre`
// (DEVICE fp64, dp values, zero in the padding; nullable = centring off).  x is widened to fp64 BEFORE the subtraction, every product
// and sum is fp64.  The feature axis is cut into *chunks (nullable) pieces whose slabs a second launch adds in a fixed order: no
// atomics, the same input gives the same bytes.  Returns "this layer did the work": false, NOTHING done, where X does not allow
// 16-byte loads along its rows or the layer lacks the op -- algo.cpp's weak default returns false and the caller builds K from
// op_cvt_to_f64 and op_dgemm.
bool op_row_gram(Dev*, int dtype, const void* X, int64_t n, int64_t dp, int64_t ldx, const double* centre, double* K, int64_t ldk,
                 int64_t* chunks);
// KernelPca (include/petal_hip_kpca.h; an extension beyond the crate).  kernel = PETAL_KERNEL_* with (gamma, coef0, degree) already
// resolved.  Each returns "this layer did the work": false, NOTHING done, where a matrix does not allow 16-byte loads along its rows or
// the layer lacks the op -- algo.cpp's weak defaults return false and the caller builds the same statement from op_cvt_to_f64, op_dgemm
// and a phi loop on the host.
// The fit's map: the leading n x n block of K (ldk; nothing outside it is written) holds the row Gram matrix G on entry and
//     K~_ij = phi(G_ij, diag_i, diag_j) - rbar_i - rbar_j + tbar
// on return; diag (n, DEVICE) = the diagonal of G set aside by the caller, rbar (n) / tbar (1) receive the column means and the grand
// mean of K.  The row sums are formed in a fixed order: no atomics.
bool op_kpca_map(Dev*, int kernel, double gamma, double coef0, int degree, double* K, int64_t n, int64_t ldk, const double* diag,
                 double* rbar, double* tbar);
// The fused pass: out (m x cols fp64, ldo; nothing outside that block is written) = phi((Xq - c)(Xt - c)^T) A.  Xt: n x dp, ldt; Xq:
// m x dp, ldq; both in dtype, dp a multiple of 16 whose padding columns hold zeros.  centre: DEVICE fp64, dp values (zeros: no centring;
// never null).  nt (nullable: formed here): DEVICE fp64, n values |xt_i - c|^2, read by rbf and cosine.  A: DEVICE fp64 with
// round_up(n, 32) readable rows and lda >= round_up(cols, 64), ZERO outside the leading n x cols block.  The m x n matrix in between
// never touches memory; every product and sum is fp64, in an order the shape alone fixes.
bool op_kernel_apply(Dev*, int dtype, const void* Xt, int64_t n, int64_t ldt, const void* Xq, int64_t m, int64_t ldq, int64_t dp,
                     const double* centre, const double* nt, int kernel, double gamma, double coef0, int degree, const double* A, int64_t lda,
                     int64_t cols, double* out, int64_t ldo);
// transform's epilogue: Y (m x k in dtype, ldy) = O_ij - ra_j - (O_ik / n - *tbar) oa_j from the fused pass's output O (m x >= k + 1
// fp64, ldo; column k = the row sums of Kq); ra, oa, tbar: DEVICE fp64.  Rounded once to dtype.
bool op_kpca_finish(Dev*, int dtype, const double* O, int64_t ldo, int64_t m, int64_t k, const double* ra, const double* oa, double n,
                    const double* tbar, void* Y, int64_t ldy);
// Nmf (include/petal_hip_nmf.h; an extension beyond the crate): multiplicative updates for the Frobenius loss.  Device layouts, all
// fp64: W n x kp, H and A kp x dp (leading dimension dp), H H^T and B kp x kp, kp = nmf_padded_k(k), ZERO in every padding row and
// column.  Each returns "this layer did the work": false, NOTHING done, where the shape is outside the kernel's envelope (k > 64,
// kp = 48, dp > 512), X does not allow 16-byte loads along its rows or the layer lacks the op -- algo.cpp's weak defaults return false and the
// caller builds the same statement from op_cvt_to_f64, op_dgemm and an element-wise step on the host.
inline int64_t nmf_padded_k(int64_t k) { return k <= 16 ? 16 : (k <= 32 ? 32 : (k + 15) / 16 * 16); }
// out4 (DEVICE) = { sum x, sum x^2, min(x, 0), 1 if a NaN or an infinity was seen else 0 } over X (n x dp in dtype, ldx), fp64, a fixed order.
bool op_nmf_scan(Dev*, int dtype, const void* X, int64_t n, int64_t dp, int64_t ldx, double* out4);
// The fused pass: Z = X H^T once, then `inner` times  D = W HHt + l1 + l2 W, D[D == 0] = 2^-23, W <- W o Z / D  (W in place;
// from_const: W starts as wconst in its k leading columns instead of its contents), then, where A and B are given (both or neither),
// A = W^T X and B = W^T W with the W just written.  inner == 0: W is left alone.  X is read once from memory; no n x kp or n x dp
// intermediate but W; every product and sum fp64 in an order the shape alone fixes; no atomics.
bool op_nmf_pass(Dev*, int dtype, const void* X, int64_t n, int64_t dp, int64_t ldx, const double* H, const double* HHt, int64_t k, int64_t kp,
                 double* W, bool from_const, double wconst, double l1, double l2, int64_t inner, double* A, double* B);
// The H side of an iteration: E = B H + l1 + l2 H, E[E == 0] = 2^-23, H <- H o A / E, HHt = H H^T, dots2 (DEVICE) = { <A, H>, <B, HHt> }
// with the new H (the two inner products of the loss).
bool op_nmf_hupdate(Dev*, int64_t kp, int64_t dp, const double* A, const double* B, double* H, double* HHt, double l1, double l2, double* dots2);
// Nmf on sparse CSR data (include/petal_hip_nmf_sparse.h; an extension beyond the crate).  The sweep's own padding: 16, 32 or 64 columns
// (nmf_padded_k gives 48, which does not fill whole lanes of a gathered row).  Each returns "this layer did the work": false, NOTHING
// done, where the shape is outside the kernel's envelope (k > 64) or the layer lacks the op -- algo.cpp's weak defaults return false.
inline int64_t nmf_csr_padded_k(int64_t k) { return k <= 16 ? 16 : (k <= 32 ? 32 : 64); }
// One sweep of an image (img.rows = R, its column count = C): G (R x kp, DEVICE fp64, in place; from_const: starts as gconst in its k
// leading columns), F (C x kp), S = F^T F (kp x kp), all ZERO in the padding:
//     z_r = sum over the stored entries t of row r, in the items' fixed order, of val[t] F[idx[t], :]
//     inner times:  D = g_r S + l1 + l2 g_r,  D[D == 0] = 2^-23,  g_r <- g_r o (z_r / D)        (inner == 0 without from_const: G is left alone)
// gram_dot (nullable, DEVICE, kp kp + 1 doubles): G^T G with the G just written, then sum_r <z_r, g_r>.  No atomics.
bool op_nmf_sweep_csr(Dev*, int dtype, const CsrImage& img, int64_t k, int64_t kp, const double* F, double* G, const double* S, bool from_const,
                      double gconst, double l1, double l2, int64_t inner, double* gram_dot);
// gram_dot (DEVICE, kp kp + 1 doubles) = { G^T G, sum of dots (nullable: 0) } over G (rows x kp fp64), a fixed order.
bool op_nmf_gram(Dev*, const double* G, int64_t rows, int64_t kp, const double* dots, double* gram_dot);
// out4 (DEVICE) = { sum v, sum v^2, min(v, 0), 1 if a NaN or an infinity was seen else 0 } over nnz stored values in dtype.
bool op_nmf_valscan(Dev*, int dtype, const void* val, int64_t nnz, double* out4);
// Nmf with the Kullback-Leibler loss on sparse CSR data (include/petal_hip_nmf_kl.h).  One sweep of an image: G (R x kp, DEVICE fp64, in
// place; from_const: starts as gconst in its k leading columns), F (C x kp), csum = colsum(F) (kp), all ZERO in the padding; `inner` times
//     wh_t = <g_r, F[idx_t, :]>, wh_t < 2^-23 -> 2^-23, num = sum_t (val_t / wh_t) F[idx_t, :] in the items' fixed order,
//     den = (csum + l1) + l2 g_r,  den[den == 0] = 2^-23,  g_r <- g_r o (num / den)
// colsum_term (nullable, DEVICE, kp + 1 doubles): colsum(G) with the G just written, then 0.  inner == 0 (needs colsum_term, no
// from_const): G is left alone and colsum_term[kp] = sum_r sum_t [val_t > 2^-23] val_t log(val_t / wh_t).  No atomics.
bool op_nmf_kl_sweep_csr(Dev*, int dtype, const CsrImage& img, int64_t k, int64_t kp, const double* F, double* G, const double* csum,
                         bool from_const, double gconst, double l1, double l2, int64_t inner, double* colsum_term);
// colsum_term (DEVICE, kp + 1 doubles) = { colsum(G), sum of terms (nullable: 0) } over G (rows x kp fp64), a fixed order.
bool op_nmf_kl_colsum(Dev*, const double* G, int64_t rows, int64_t kp, const double* terms, double* colsum_term);
// out1 (DEVICE) = sum over nnz stored values in dtype of [v > 2^-23] v, a fixed order.
bool op_nmf_kl_vsum(Dev*, int dtype, const void* val, int64_t nnz, double* out1);
// Nmf with the Kullback-Leibler loss on dense data (include/petal_hip_nmf_kl_dense.h).  Device layouts are op_nmf_pass's; rsum (DEVICE,
// kp doubles) = the row sums of H.  The fused pass: `inner` times  WH = W H, WH[WH < 2^-23] = 2^-23, Q = X / WH, den = rsum + l1 + l2 W,
// den[den == 0] = 2^-23, W <- W o ((Q H^T) / den)  (W in place; from_const as op_nmf_pass), then, where A and cts are given (both or
// neither), A = W^T (X / max(W H, 2^-23)) with the W just written and cts (DEVICE, kp + 2 doubles) = { colsum(W), term, sum x }: the
// last two for inner == 0 only (which needs A and leaves W alone), term = sum [x > 2^-23] x log(x / max(W H, 2^-23)) and sum x over the
// same entries, else zeros.  X is read once from memory however large `inner` is (with the H side at 64 padded components and more than
// 256 padded columns: three launches, X read twice -- k_nmf_kl_dense.inc); no n x dp intermediate; no atomics.  false, NOTHING done:
// outside op_nmf_pass's envelope.
bool op_nmf_kl_pass(Dev*, int dtype, const void* X, int64_t n, int64_t dp, int64_t ldx, const double* H, const double* rsum, int64_t k, int64_t kp,
                    double* W, bool from_const, double wconst, double l1, double l2, int64_t inner, double* A, double* cts);
// den = colsum[row] + l1 + l2 H, den[den == 0] = 2^-23, H <- H o (A / den) on kp x dp (ld dp).
bool op_nmf_kl_hrule(Dev*, int64_t kp, int64_t dp, const double* A, const double* colsum, double* H, double l1, double l2);
// out (DEVICE, kp doubles) = the row sums of H (kp x dp, ld dp), a fixed order.
bool op_nmf_kl_rowsum(Dev*, int64_t kp, int64_t dp, const double* H, double* out);
// Nmf by coordinate descent (include/petal_hip_nmf_cd.h).  Device layouts are op_nmf_pass's.  The fused pass: Z = X H^T once, then
// `inner` Gauss-Seidel sweeps of every row of W over its coordinates with S = HHt + l2 I (the first k diagonal entries) and
// z = Z[i, :] - l1 (W in place; from_zero: W starts as zeros; inner = 0 leaves W alone), then, where A and B are given (both or neither),
// A = W^T X and B = W^T W with the W just written.  viol (nullable, DEVICE, `inner` doubles): the violation sum |pg| of every sweep, the
// workgroups' parts added in workgroup order.  X is read once from memory; no atomics.  false, NOTHING done: outside op_nmf_pass's envelope.
bool op_nmf_cd_pass(Dev*, int dtype, const void* X, int64_t n, int64_t dp, int64_t ldx, const double* H, const double* HHt, int64_t k, int64_t kp,
                    double* W, bool from_zero, double l1, double l2, int64_t inner, double* A, double* B, double* viol);
// The H side: one sweep of the dp rows of H^T with S = B + l2 I (the first k diagonal entries) and z = A[:, f] - l1, H in place; then
// HHt = H H^T, dots2 (DEVICE) = { <A, H>, <B, HHt> } and viol1 (DEVICE) = the sweep's violation.  false, NOTHING done: kp not 16, 32 or 64.
bool op_nmf_cd_hupdate(Dev*, int64_t k, int64_t kp, int64_t dp, const double* A, const double* B, double* H, double* HHt, double l1, double l2,
                       double* dots2, double* viol1);
// Nmf by coordinate descent on sparse CSR data (include/petal_hip_nmf_cd_sparse.h).  One cd sweep of an image: G (R x kp, DEVICE fp64,
// in place; from_zero: starts as zeros, needs inner >= 1), F (C x kp), S (kp x kp; the kernel adds l2 on its first k diagonal entries),
// all ZERO in the padding, kp = nmf_csr_padded_k(k):
//     z_r = op_nmf_sweep_csr's;  inner Gauss-Seidel sweeps of g_r over its coordinates with z = z_r - l1  (inner == 0: G is left alone)
// gram_dot_viol (nullable, DEVICE, kp kp + 1 + inner doubles; then inner <= 1024): G^T G with the G just written, sum_r <z_r, g_r> (the raw
// z_r), then the violation of every sweep.  No atomics; every order is fixed by the image's items and kp.  false, NOTHING done: k > 64 or
// the layer lacks the op.
bool op_nmf_cd_sweep_csr(Dev*, int dtype, const CsrImage& img, int64_t k, int64_t kp, const double* F, double* G, const double* S, bool from_zero,
                         double l1, double l2, int64_t inner, double* gram_dot_viol);
// out (img.rows x cols in dtype, ldo; DEVICE) = the dense image: zeros, then every stored entry added in position order.
bool op_csr_densify(Dev*, int dtype, const CsrImage& img, void* out, int64_t cols, int64_t ldo);
// One re-basing step of the power iteration: G (L x L, ldg) = R^T R, P_out (K x M fp64, ldpo) = A R^-1 (A: K x M, lda; columns
// L .. M of the result are zero), Z = (X - mu) . P_out.  Same results contract as op_chol_inv(G -> T, Lz = M) followed by
// op_gemm_xp_prod(A, T); T (M x M, ldt) is SCRATCH here -- it may hold R^-1 or a factored form of it, callers must not read it.
// p_planes = 2 (fp32 data, split-product mode): where the factor is applied in RT form (L <= 140, M a multiple of 16 <= 144) P_out IS
// ROUNDED to the sum of its two leading bf16 pieces -- both rounded from the fp64 value: |P_out - A R^-1| <= 2^-17 |A R^-1| -- in P_out
// itself and in the product's operand, which saves a piece product; where the explicit inverse is formed (larger L or M) it is NOT
// rounded and the product reads float32(P_out) on three planes.  3, fp64 data, the fp32-MFMA mode: the iterate to fp64 accuracy.
void op_rebase_xp(Dev*, int dtype, const void* X, int64_t n, int64_t K, int64_t ldx, const void* mu, const double* G, int64_t L,
                  int64_t ldg, double rel_tol, int* ndead, const double* A, int64_t M, int64_t lda, double* T, int64_t ldt,
                  double* P_out, int64_t ldpo, void* Z, int64_t ldz, int p_planes = 2, bool steering = false);
// One FUSED power-iteration pass, the two products of pca.rs:711 + 714 in ONE pass over X:
//     Y (K x N fp64, ldy) = (X - mu)^T ((X - mu) P),     Z (nullable, n x N, ldz) = (X - mu) P
// with P rounded to the sum of its two leading bf16 pieces (a caller that needs P to fp32 accuracy uses op_gemm_xp + op_gemm_atb).
// Returns false, NOTHING done, where no fused kernel exists for the shape / mode (op_power_pass_applies says so up front).
bool op_power_pass_applies(Dev*, int dtype, const void* X, int64_t n, int64_t K, int64_t ldx, const void* mu, int64_t N);
// steering: the pass only STEERS a power iteration (its Y feeds the next re-basing, nothing else; Z == NULL): the kernel may then also
// round Xc and z to two bf16 planes -- four piece products per tile in both products, two barriers per stage (k_pow3f).  The caller
// owns the consequences: rpca_fit runs such passes on its optimistic path only, under the spectral verdict.
bool op_power_pass(Dev*, int dtype, const void* X, int64_t n, int64_t K, int64_t ldx, const void* mu, const double* P, int64_t N, int64_t ldp,
                   void* Z, int64_t ldz, double* Y, int64_t ldy, bool steering = false);
// The FIRST fused pass of a fit with the means pass folded in (single rank, fp32, centring; L < N: a padding column is free):
// mu64 / muT come back as the column means of X (d real columns of K), *tv as sum (X - mean)^2, and Y = Xc^T (Xc P) about that
// mean -- X is read once, not twice: the kernel centres about the means mu0 of a row SAMPLE (every (n / 4096)-th row, 4096 of them),
// gathers the column sums and the sum of squares about that provisional centre in the same pass, and a one-workgroup kernel moves Y,
// the means and the variance to the true centre (a rank-one correction of relative size (delta / sigma)^2).
// THE CONTRACT of the folded sums (tests/rebase_cases.py, table C, holds the device and the host simulation to it): they are the sums of
// the operand product 2 reads, accumulated in fp32 inside a workgroup's slab and in fp64 across slabs.  In the steering form (k_pow3f,
// PETAL_OPT_STEERING on: the default) that operand is fl32(x - mu0) ROUNDED TO TWO bf16 PLANES, so with a_f = mean_i |x_if - mu0_f|
//     |mu64_f - mean_f| <= 2^-17 a_f + 2^-24 (rows per workgroup) a_f
// and on columns of few distinct values (binary, counts) the first term is a BIAS that does not shrink with n: equal values round
// alike.  With PETAL_OPT_STEERING off (k_pow3<.., MEANS>: three planes re-add to fl32(x - mu0)) the first term is absent.  Neither
// is "exact"; both are far below the 1e-5 of a column's spread a fit is held to.  *tv = sum fl32(x - mu0)^2 - n |delta|^2 with the
// squares taken BEFORE the rounding and added per lane in fp32 over all stages of a workgroup: its error grows with the rows per
// workgroup (DESIGN.md section 4 has the bound and the measured figures).  ssq_scratch: one device double.  False: nothing done.
bool op_power_pass_means(Dev*, int dtype, const void* X, int64_t n, int64_t K, int64_t d, int64_t ldx, double n_total, const double* P,
                         int64_t N, int64_t ldp, int64_t L, double* Y, int64_t ldy, double* mu64, void* muT, double* ssq_scratch, double* tv);
// the same behind one re-basing step (arguments as op_rebase_xp, p_planes = 2): P_out = A R^-1 rounded, then the fused pass with it
bool op_rebase_power_pass(Dev*, int dtype, const void* X, int64_t n, int64_t K, int64_t ldx, const void* mu, const double* G, int64_t L,
                          int64_t ldg, double rel_tol, int* ndead, const double* A, int64_t M, int64_t lda, double* T, int64_t ldt,
                          double* P_out, int64_t ldpo, void* Z, int64_t ldz, double* Y, int64_t ldy, bool steering = false);
// Was a 16-bit (two-plane) rounding of the sketch matrix and of the re-based iterates harmless for the spectrum this fit found?
// A rounding E of the basis P (|E_ij| <= eps2 |P_ij|) reaches the next iterate as C E, C = Xc^T Xc: directions the block already
// spans are harmless, the part from BEYOND the block -- sum_{i > L} sigma_i^2 v_i (v_i^T E), of size eps2 T with
// T^2 = sum_{i > L} sigma_i^4 / d <= lam_{L-1} (tv - sum_j lam_j) / d -- tilts wanted direction j by eps2 T / lam_j, and the
// component that comes out by that over the relative gap to its neighbours.  lam (L, descending): the eigenvalues of B B^T (squared
// singular values); mu_sq ([means | sums of squares], 2 dp; nullable): the total variance is sum_j (sq_j - n_total mu_j^2), else *tv.
// Sets flag2[1] = 1 when that estimate exceeds thr for one of the k wanted components (flag2[0] is not touched).
void op_tail_verdict(Dev*, const double* lam, int64_t L, int64_t k, const double* mu_sq, int64_t dp, int64_t d, double n_total,
                     const double* tv, double eps2, double thr, int* flag2);
// C[M x N] (f64, ldc) = (A - muA)^T . (B - muB),  A: n x M (lda), B: n x N (ldb), reduction over n rows.
// precise: every product and the whole accumulation in fp64 (needed where the result's small eigenvalues
// matter: exact Pca, FastICA whitening); otherwise fp32 MFMA chunks combined in fp64.
void op_gemm_atb(Dev*, int dtype, const void* A, int64_t lda, int64_t M, const void* muA,
                 const void* B, int64_t ldb, int64_t N, const void* muB, int64_t n,
                 double* C, int64_t ldc, bool precise = false, bool steering = false);
// C (dp x dp fp64, ldc; only the leading d x d block is non-zero) = (X - mu)^T (X - mu) for fp32 X by EXACT bf16-piece products with
// fp32 accumulation over row chunks (fp64 across them): good to ~1e-6 of C's largest entries -- enough for a whitening whose wanted
// eigenvalues lie within two decades (the caller checks), not for an exact Pca.  False, nothing done: shape / mode not covered.
// mu64_fold != NULL: the column means are formed by the same call (mu: provisional centre in, true means out; mu64_fold: true means, fp64)
bool op_gram_split(Dev*, const void* X, int64_t n, int64_t d, int64_t dp, int64_t ldx, const void* mu, double* C, int64_t ldc,
                   double* mu64_fold = nullptr, double n_total = 0.0);
// per column j < L of U (n x L): absmax[j] = max_i |U_ij|, idx[j] = row_offset + first such i,
// sign[j] = U_ij >= 0 ? +1 : -1 (sign of -0.0 / 0.0 follows f64::signum: +1 for +0, -1 for -0).
// n == 0: absmax = -1, idx = +inf, sign = +1.
void op_col_absmax(Dev*, int dtype, const void* U, int64_t n, int64_t L, int64_t ldu, int64_t row_offset,
                   double* absmax, double* idx, double* sign);
// svd_flip across ranks, fp32 data: key[j] = the fp64 image of absmax[j] with (2^28 - 1 - row[j], sign[j] < 0) packed into
// the 29 low mantissa bits an fp32 magnitude leaves zero (absmax < 0, an empty shard, gives key 0); `triple` is
// op_col_absmax's [absmax | row | sign] (3 L).  A MAX all-reduce of the keys elects the first element of maximal magnitude.
// flag != nullptr (three ints): key[L] = verdict_code(flag) -- a replicated decision word riding the same MAX all-reduce, so that
// every rank branches on the agreed value
void op_flip_key(Dev*, const double* triple, double* key, int64_t L, const int* flag = nullptr);
// The redo verdict of an optimistic RandomizedPca run (algo.cpp's attempt loop) from its three verdict words: [0] pivot breakdowns,
// [1] a heavy tail behind the block, [2] eigenvalues among the wanted ones too close for the two-stage eigen-solver's vectors.  The one
// definition of the code for the host algorithms, the device's op_flip_key and the host simulation's: a sharded fp32 fit and a
// single-rank fit must branch alike.  (Words read lazily, in this order.)
constexpr double VERDICT_TAIL = 1.0, VERDICT_EIG = 2.0, VERDICT_PIVOT = 3.0;
constexpr double verdict_code(const int* w) {
    return w[0] != 0 ? VERDICT_PIVOT : (w[1] != 0 ? VERDICT_TAIL : (w[2] != 0 ? VERDICT_EIG : 0.0));
}
// A[i][j] *= s[j] (dtype matrix, f64 scale vector), i < n, j < L
void op_scale_cols(Dev*, int dtype, void* A, int64_t n, int64_t L, int64_t lda, const double* s);
// G = tanh(X) elementwise (n x c), gp[j]... logcosh KAT helper: rows are components:
// G[i][j] = tanh(X[i][j]); gp[i] = sum_j (1 - G_ij^2)   (f64 out, un-normalised)
void op_logcosh_rows(Dev*, int dtype, const void* X, int64_t r, int64_t c, int64_t ldx, void* G, int64_t ldg, double* gp);

// ---- FastICA fused step (ica.rs:332-333) -----------------------------------------------------
// X1T: n x nc (ld) whitened samples (sample-major).  W: nc x nc f64.
// GX[i][j] = sum_s tanh(w_i . x_s) x_s[j];  gp[i] = sum_s (1 - tanh(w_i . x_s)^2)     (f64 out)
// state[0] != 0 (converged) -> no-op.
// Call once in front of a fixed-point loop over X1T (and again whenever X1T's CONTENTS change): lets the implementation prepare what
// is constant over the loop's iterations (the device library: the bf16 planes of X1).  op_ica_step works without it.
void op_ica_prepare(Dev*, int dtype, const void* X1T, int64_t n, int64_t nc, int64_t ld);
void op_ica_step(Dev*, int dtype, const void* X1T, int64_t n, int64_t nc, int64_t ld,
                 const double* W, double* GX_gp /* nc*nc + nc contiguous */, const int* state);
// The same step with another contrast function g in tanh's place: GX[i][j] = sum_s g(w_i . x_s) x_s[j];  gp[i] = sum_s g'(w_i . x_s).
// contrast = PETAL_ICA_CONTRAST_* >> 4:  1  g(u) = u exp(-u^2/2)   2  g(u) = u^3   (0: what op_ica_step computes).
// An extension beyond the crate: a device-op layer that does not define it gets algo.cpp's weak default,
// which refuses the contrast (PETAL_INVALID_INPUT) -- never a silent tanh fit.
void op_ica_step_g(Dev*, int dtype, const void* X1T, int64_t n, int64_t nc, int64_t ld,
                   const double* W, double* GX_gp /* nc*nc + nc contiguous */, const int* state, int contrast);
// ica.rs:334-358 on one workgroup: D = GX/n_total - gp/n_total (.) W; W1 = symdecorr(D); lim; update.
// state = {done, n_iter}; iter is the 0-based index of this iteration.  W is replaced by W1 unless done.
// progress (nullable): dev_host_progress()'s array; the kernel publishes {n_iter if converged else 0, iter + 1} there when it
// finishes, so the host can follow the loop without a synchronisation.
void op_ica_tail(Dev*, int64_t nc, double n_total, double* W, const double* GX_gp, int mode, double tol,
                 int* state, int iter, int* progress = nullptr);
// four ints of pinned host memory that kernels can store to (system-scope stores over PCIe); the host reads them directly
volatile int* dev_host_progress(Dev*);
// Wout = symmetric_decorrelation(Win) (ica.rs:363-381)
void op_symdecorr(Dev*, int64_t nc, const double* Win, double* Wout, int mode, int* zero2 = nullptr);  // zero2 (nullable): two device ints to clear

// ---- f64 small-matrix ops ----------------------------------------------------------------------
// colscale (nullable, N values): column j of alpha op(A) op(B) is multiplied by colscale[j] (beta must be 0)
void op_dgemm(Dev*, bool ta, bool tb, int64_t M, int64_t N, int64_t K, double alpha,
              const double* A, int64_t lda, const double* B, int64_t ldb, double beta, double* C, int64_t ldc,
              const double* colscale = nullptr);
// sig[i] = sqrt(max(lam[i], 0)); inv[i] = sig[i] > thr * sig[0] ? 1 / sig[i] : 0   (the two op_dvec steps of an SVD from
// eigenvalues, in one launch)
void op_sigma_inv(Dev*, const double* lam, double* sig, double* inv, int64_t count, double thr);
// P (rows x rp row-major) = [ V[:, :r] diag(inv) | 0 ]  (V: ldv)
void op_scale_pad_cols(Dev*, const double* V, int64_t ldv, const double* inv, int64_t rows, int64_t r, int64_t rp, double* P);
// comp (k x d row-major, dtype) = V[:d, :k]^T
void op_transpose_out(Dev*, int dtype, const double* V, int64_t ldv, int64_t d, int64_t k, void* comp);
// comp[j][i] (k x d row-major, the input dtype) = (Bt u_j)[i] / sigma_j: rows of V^T from Bt (d x L, ldb), the eigenvectors Uh
// (columns, ldu) and eigenvalues lam of B B^T; sigma_j = sqrt(max(lam_j, 0)), 1 / sigma_j = 0 at or below thr * sigma_0.
void op_components_out(Dev*, int dtype, const double* Bt, int64_t ldb, const double* Uh, int64_t ldu, const double* lam, double thr,
                       int64_t d, int64_t L, int64_t k, void* comp);
// G (L x L, SPD up to rounding) = R^T R;  T = R^{-1} (upper triangular, L x L, ldt).
// A pivot with r_jj^2 <= rel_tol * G_jj (or G_jj <= 0) marks column j as dependent: T[:, j] = 0.
// Only the upper triangle of G is read.  ndead (nullable, device int): *ndead = max(*ndead, number of dependent columns).
// Lz > L: T is additionally zero-filled out to Lz x Lz (the padded extent of the caller's buffers).
// ndead_cols > 0: only dependent columns j < ndead_cols count towards *ndead (orders the one-workgroup kernel takes; larger
// orders count them all).
// The factorisation of op_chol_inv WITHOUT the explicit inverse where the device has the kernels for it (fp32 data in the split-product
// mode, L <= 140, Lz a multiple of 16 <= 144, 64 <= n < 2^31 rows in the product that follows): returns true and leaves T in "RT form"
// -- diagonal 16 x 16 blocks T_JJ = R_JJ^-1, the blocks above them R itself, zeros below -- which only op_trsm_right and
// op_gemm_xp_prod_absmax(a_rt = true) understand; otherwise it IS op_chol_inv and returns false.  (Round 6: the last factorisation of
// a RandomizedPca fit on the register-resident kernel of the power iterations, 15 instead of 40 us at l = 74.)
bool op_chol_rt(Dev*, int dtype, int64_t n, const double* G, int64_t L, int64_t ldg, double* T, int64_t ldt, double rel_tol, int* ndead,
                int64_t Lz, int64_t ndead_cols);
// out (rows x M fp64, ldo) = A (rows x M, lda) . R^-1 for R in RT form (M x M, ldt); rows a multiple of 16
void op_trsm_right(Dev*, const double* A, int64_t rows, int64_t lda, const double* RT, int64_t M, int64_t ldt, double* out, int64_t ldo);
void op_chol_inv(Dev*, const double* G, int64_t L, int64_t ldg, double* T, int64_t ldt, double rel_tol, int* ndead = nullptr,
                 int64_t Lz = 0, int64_t ndead_cols = 0);
// symmetric PSD A (L x L) -> eigenvalues w (descending) and eigenvectors in the COLUMNS of V.  A may be destroyed.
// tol_rel: off-diagonal elements are annihilated down to |a_pq| <= tol_rel sqrt(a_pp a_qq) (graded matrices keep the
// relative accuracy of their small eigenvalues) or to the 1e-16 ||diag|| rounding floor; 1e-15 for fp64 data, 1e-8 is
// ample when the matrix was formed from fp32 data.  (Behind the floor the Jacobi solvers go on while the first criterion
// still makes quadratic progress: a graded matrix keeps its eigenvalues BELOW 1e-16 ||A|| too, rounding noise ends as before.)
// The two-stage solver computes each eigenvector on its own: v_i . v_j carries up to 2 eps ||A|| / |lam_i - lam_j|.
// clustered = true: the caller expects eigenvalues closer than the two-stage solver's gap tolerance (the Ritz values of a
// subspace iteration: a block of noise-level eigenvalues) -- go to the Jacobi solver directly instead of paying for both
// Lz > L: V is an Lz x Lz matrix (leading dimension ldv) whose rows / columns L .. Lz - 1 must come out zero (padding for the
// GEMM kernels); the solver's first kernel writes those zeros itself, which saves the caller a memset launch.
// ncheck > 0: only the leading ncheck eigenpairs are delivered to full accuracy -- the two-stage solver's closeness verdict
// looks at those alone (a cluster further down, e.g. the noise-level Ritz values of a subspace iteration, gets vectors that
// are accurate to eps ||A|| / gap only and need not be mutually orthogonal; it no longer sends the whole problem to Jacobi).
// verdict (nullable, device int): instead of running the Jacobi fallback behind a flagged two-stage solve, OR a non-zero value into
// *verdict and deliver the two-stage result as it is (orders the register-resident kernels take; other orders ignore it).
void op_eigh(Dev*, double* A, int64_t L, int64_t lda, double* V, int64_t ldv, double* w, double tol_rel = 1e-15,
             bool clustered = false, int64_t Lz = 0, int64_t ncheck = 0, int* verdict = nullptr, bool verdict_fresh = false,
             double gap_tol_override = 0.0);
// (gap_tol_override > 0: the closeness threshold of the two-stage solver, relative to ||A||, instead of the one tol_rel implies --
// a caller whose matrix came from fp32 data can accept eigenvectors to eps / 1e-8 while still asking the fallback for 1e-15)
// (verdict_fresh: *verdict is cleared first instead of accumulated into; orders that ignore the verdict leave it 0)
// Residual verdict of a Rayleigh-Ritz step without a host round trip: with the Ritz vectors Vr (rows x >= nc, ldv), their
// images CV = C Vr (ldc) and the Ritz values theta,  out[0] = max_{j < nc} ||CV[:, j] - theta_j Vr[:, j]||_2^2,  out[1] = theta[0],
// out[2] = 1 if one of those nc squared norms is NOT BELOW 1e300 (NaN and inf included: a residual of 1e150 theta_0 is no residual, and
// the comparison costs nothing where an isfinite() would; such a column does not enter out[0]) or *flag / *flag2 (nullable device ints: op_eigh's verdict; the pivots the
// orthonormalisations of the iteration dropped) is non-zero.  One launch, no clear needed; the caller reads `out` with its other results.
void op_ritz_residual(Dev*, const double* CV, int64_t ldc, const double* Vr, int64_t ldv, int64_t rows, int64_t nc, const double* theta,
                      const int* flag, double* out3, double* w_out = nullptr, const int* flag2 = nullptr);   // w_out (nullable): receives theta[0 .. nc)
// FastICA whitening matrix from the eigenpairs of the covariance (ica.rs:190-208) in one launch:
//   KT[i][j]  = s_j U[i][j] / sigma_j,  sigma_j = sqrt(max(lam_j, 0)) (0 where sigma_j == 0),  j < nc;  0 for nc <= j < ncp
//   s_j = +-1 normalises the eigenvector's sign: its first component of largest magnitude becomes positive (an eigen-solver's
//   own sign is arbitrary and may flip under a last-bit perturbation; the whitening rows must not)
//   KTs[i][j] = KT[i][j] * scale          (scale = sqrt(n): X1 = K X sqrt(n))
// U: rows x >= nc (ldu), KT / KTs: rows x ncp.
void op_whiten_k(Dev*, const double* U, int64_t ldu, const double* lam, int64_t rows, int64_t nc, int64_t ncp, double scale,
                 double* KT, double* KTs);
// Singular value decomposition of a small square matrix A (L x L fp64, lda) by ONE-SIDED (Hestenes) Jacobi on its rows --
// the route that keeps the relative accuracy of small singular values (eps kappa of the row-scaled matrix, not eps kappa^2
// like an eigen-decomposition of A A^T): rows p, q are rotated until all are mutually orthogonal, G A = W, so A = G^T W and
// the rows of G are the LEFT singular vectors, the row norms of W the singular values.
//   U (L x L, ldu): column j = the left singular vector of the j-th singular value in ASCENDING order,
//   s_inv (L):      1 / (that singular value)  (descending; 0 where the singular value is 0).
// (This is the order its one caller wants: A = R^-1 of a thin QR X = Q R, whose left singular vectors are the right
// singular vectors of X and whose inverse singular values are X's, largest first.)  A is destroyed.
// nonconv (nullable, device int): set to 1 when 40 sweeps did not orthogonalise the rows (never cleared here).
void op_jacobi_svd_rows(Dev*, double* A, int64_t L, int64_t lda, double* U, int64_t ldu, double* s_inv, int* nonconv = nullptr);
// Every column j < cols of Y (rows x cols, ldy) that is exactly zero is replaced by column j of Src (lds): the robust re-basing
// of RandomizedPca refills the directions its dependence test dropped with fresh (random) ones instead of shrinking the block.
void op_refill_zero_cols(Dev*, double* Y, int64_t rows, int64_t cols, int64_t ldy, const double* Src, int64_t lds);
// x[i] *= alpha
void op_dscal(Dev*, double* x, int64_t count, double alpha);
// y[i] += alpha * x[i]
void op_daxpy(Dev*, int64_t count, double alpha, const double* x, double* y);
// elementwise helpers on f64 vectors:  mode 0: y = sqrt(max(x,0)); mode 1: y = x > thr*x[0] ? 1/x : 0; mode 2: y = x^2
void op_dvec(Dev*, int mode, const double* x, double* y, int64_t count, double thr);
// A[i][j] *= s[j]  (f64 matrix M x N)
void op_dscale_cols(Dev*, double* A, int64_t M, int64_t N, int64_t lda, const double* s);
void op_cvt_from_f64(Dev*, int dtype, void* dst, const double* src, int64_t count);
void op_cvt_to_f64(Dev*, int dtype, double* dst, const void* src, int64_t count);
// dst (rows_p x cols_p fp64, zero padded) <- the leading rows x cols block of the row-major device matrix src (ld lds)
// (zero_ptr, zero_count: a small fp64 range the same launch clears -- the caller's accumulators -- instead of a memset of its own)
void op_pad_to_f64(Dev*, int dtype, double* dst, int64_t rows_p, int64_t cols_p, const void* src, int64_t rows, int64_t cols, int64_t lds,
                   double* zero_ptr = nullptr, int64_t zero_count = 0);

}  // namespace petal
