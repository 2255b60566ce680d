/* petal_hip_sparse.h -- RandomizedPca on sparse data in CSR form: fit and transform without densifying (term-document counts, expression
 * tables, click matrices).  An extension beyond the crate, declared beside petal_hip.h, whose set of entry points
 * mirrors the crate's public interface one to one.
 *
 * The randomized range finder (pca.rs:689-718) never needs X itself, only X . P and X^T . Z against tall-skinny dense blocks, and the
 * centring is never applied to X:  Xc . P = X . P - 1 (mu^T P),  Xc^T . Z = X^T . Z - mu (1^T Z).  petal_csr_create builds, on the
 * host, the transposed image (a STABLE counting sort: rows stay ascending inside every column) and for both images a list of work
 * items (row, first, last) of at most PETAL_CSR_ITEM_NNZ nonzeros each -- a longer row becomes several consecutive items -- and uploads
 * both; they stay in device memory until petal_csr_destroy.  One kernel serves both products (X^T . Z is the same kernel on the
 * transposed image).  No floating-point atomics anywhere: the partial results of a split row are summed in item order by a second
 * launch, so the same handle, or another handle made from the same arrays, gives the same bits on every run.
 *
 * Accuracy: the dense operand and the result of a product are kept in the data's type (float32 for float32 data), every product and
 * every sum inside it is float64.  Against the float64 reference with the same Omega and n_iter the components and singular values hold
 * 1e-5 (float32) / 1e-9 (float64) relative on the project's parity inputs.  The centring is implicit: X . P and mu^T P are each of size
 * |mu| sqrt(nonzeros per row) and their difference is formed in float64 -- float64 data whose means are far larger than their spread
 * lose digits in that proportion (a mean 1e6 times the spread costs six of the sixteen).
 *
 * The GEMM mode and the two-plane / steering / fused-pass options of the ctx select dense kernels; they do not apply to a sparse fit or
 * transform: its products with X are the sparse kernel, its other products (Gram matrices, re-basing, U) are formed in float64 by
 * kernels that have one form, and the same input gives the same bytes under every mode and option.
 *
 * Not in this version: CSR arrays that already live in device memory (the deterministic transposition is then a segmented sort on the
 * device), sharded sparse fits, exact Pca and FastICA on sparse input, row scores on sparse input, 64-bit column indices, CSC or COO
 * as input formats (convert on the host).
 */
#ifndef PETAL_HIP_SPARSE_H
#define PETAL_HIP_SPARSE_H

#include "petal_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PETAL_CSR_ITEM_NNZ 256   /* most nonzeros one work item (one wave of the product kernel) covers */

typedef struct petal_csr petal_csr;   /* opaque: a sparse matrix resident with its ctx; destroy it before that ctx */

/* indptr: HOST rows + 1 values; indices: HOST nnz column indices; values: HOST nnz values of `dtype` (PETAL_F32 / PETAL_F64).  The
 * arrays are copied: the caller may release them when the call returns.
 * Checked before anything is uploaded, every violation PETAL_INVALID_INPUT with a message that names the first offending position:
 * indptr[0] == 0, indptr non-decreasing, indptr[rows] == nnz, every index in [0, cols).  cols < 2^31.
 * Indices inside a row need not be sorted; duplicates are legal and act as their sum; explicit zeros, empty rows and empty columns are
 * legal.  Values are not inspected: a NaN or an infinity surfaces in the fit (PETAL_LINALG_ERROR "did not converge") -- and so does a
 * float64 column whose sum of squares overflows (|x| beyond about 1e154), whose total variance is not representable either. */
int petal_csr_create(petal_ctx* ctx, int64_t rows, int64_t cols, int64_t nnz, const int64_t* indptr, const int32_t* indices,
                     const void* values, int32_t dtype, petal_csr** out);
void petal_csr_destroy(petal_csr* x);

/* out8 = { rows, cols, nnz, dtype, resident, items of the image, items of the transposed image, PETAL_CSR_ITEM_NNZ }.
 * resident: 1 when both images live in device memory and the product kernel serves this handle; 0 where the device-op layer has no
 * sparse product (the host simulation of the tests) -- the handle then keeps its host arrays and the entries below densify. */
int petal_csr_info(const petal_csr* x, int64_t* out8);

/* Debug accessor of a handle that is NOT resident (PETAL_INVALID_INPUT otherwise): copies one image as petal_csr_create built it.
 * transposed == 0: the matrix itself (rows + 1 / nnz / nnz); != 0: the transposed image (cols + 1 / nnz / nnz; `indices` are then row
 * numbers).  items: 3 values per work item -- the image row it belongs to, its first position, one past its last position -- in launch
 * order; an empty row has one item with first == last.  Every pointer is nullable. */
int petal_csr_image(const petal_csr* x, int transposed, int64_t* indptr, int32_t* indices, void* values, int64_t* items);

/* RandomizedPca::fit / fit_transform on a resident sparse matrix: arguments, outputs and errors exactly as petal_rpca_fit
 * ("every dimension should be at least k"; l = min(k + n_oversample, rows, cols); all-zero input is legal; non-finite values:
 * PETAL_LINALG_ERROR "did not converge").  A sharded ctx (world size > 1) is PETAL_INVALID_INPUT in this version.
 * kernel_path (nullable): 1 when the sparse product kernel did the work, 0 when the call densified X on the host and ran
 * petal_rpca_fit (a handle that is not resident: same results contract, bit for bit petal_rpca_fit's on the densified matrix). */
int petal_rpca_fit_csr(petal_ctx* ctx, const petal_csr* x, int64_t k, int64_t n_oversample, int64_t n_iter, int centering,
                       const void* omega, void* components, void* means, void* singular, void* total_variance,
                       const petal_matrix* y_out, int64_t* kernel_path);

/* y = (x - means) . components^T, as petal_transform ("# of columns should be d"). */
int petal_transform_csr(petal_ctx* ctx, const petal_csr* x, const void* components, const void* means, int64_t k, int64_t d,
                        int centering, const petal_matrix* y_out, int64_t* kernel_path);

/* Test aid, like the probe entries: out = X . P (transposed == 0: rows x N) or X^T . P (cols x N), minus a[r] * s[:] when s != NULL
 * (a == NULL means a[r] = 1).  P, a, s, out: HOST float64; P and out row-major without padding.  On a float32 handle P is rounded to
 * float32 and the result comes back through float32, as inside a fit. */
int petal_csr_gemm(petal_ctx* ctx, const petal_csr* x, int transposed, const double* P, int64_t N, const double* a, const double* s,
                   double* out);

/* Test aid of the ctx, declared here because only the sparse handle keeps device memory between calls: the device blocks the ctx's
 * caching allocator has handed out and not got back (a resident sparse matrix holds up to eight;
 * between calls nothing else does), and their bytes.  Both -1 where the device-op layer keeps no count (the host simulation). */
int petal_ctx_workspace_in_use(petal_ctx* ctx, int64_t* blocks, int64_t* bytes);

#ifdef __cplusplus
}
#endif

#endif /* PETAL_HIP_SPARSE_H */
