//! Raw binding of include/petal_hip_sparse.h: RandomizedPca on sparse CSR data, never densified (an extension beyond the crate).
use crate::ffi::{PetalCtx, PetalMatrix};
use std::os::raw::{c_int, c_void};

/// Opaque: a sparse matrix and its transposed image, resident with the ctx that created it.
#[repr(C)]
pub struct PetalCsr {
    _private: [u8; 0],
}

/// Most nonzeros one work item of the product kernel covers (PETAL_CSR_ITEM_NNZ).
pub const PETAL_CSR_ITEM_NNZ: i64 = 256;

extern "C" {
    /// indptr: rows + 1 values from 0 to nnz, non-decreasing; indices: nnz column indices in [0, cols), unsorted and duplicated ones
    /// are legal; values: nnz values of `dtype` (host arrays, copied)
    pub fn petal_csr_create(
        ctx: *mut PetalCtx, rows: i64, cols: i64, nnz: i64, indptr: *const i64, indices: *const i32, values: *const c_void,
        dtype: i32, out: *mut *mut PetalCsr,
    ) -> c_int;
    pub fn petal_csr_destroy(x: *mut PetalCsr);
    /// out8 = { rows, cols, nnz, dtype, resident, items, items of the transposed image, PETAL_CSR_ITEM_NNZ }
    pub fn petal_csr_info(x: *const PetalCsr, out8: *mut i64) -> c_int;
    pub fn petal_csr_image(
        x: *const PetalCsr, transposed: c_int, indptr: *mut i64, indices: *mut i32, values: *mut c_void, items: *mut i64,
    ) -> c_int;
    /// outputs as petal_rpca_fit; kernel_path (nullable): 1 the sparse product kernel, 0 the densifying fall-back
    pub fn petal_rpca_fit_csr(
        ctx: *mut PetalCtx, x: *const PetalCsr, k: i64, n_oversample: i64, n_iter: i64, centering: c_int, omega: *const c_void,
        components: *mut c_void, means: *mut c_void, singular: *mut c_void, total_variance: *mut c_void,
        y_out: *const PetalMatrix, kernel_path: *mut i64,
    ) -> c_int;
    pub fn petal_transform_csr(
        ctx: *mut PetalCtx, x: *const PetalCsr, components: *const c_void, means: *const c_void, k: i64, d: i64,
        centering: c_int, y_out: *const PetalMatrix, kernel_path: *mut i64,
    ) -> c_int;
    /// test aid: out = X . P or X^T . P minus a s^T (host float64, row-major)
    pub fn petal_csr_gemm(
        ctx: *mut PetalCtx, x: *const PetalCsr, transposed: c_int, p: *const f64, n: i64, a: *const f64, s: *const f64,
        out: *mut f64,
    ) -> c_int;
    /// test aid: blocks and bytes the ctx's allocator has handed out and not got back (-1: no count kept)
    pub fn petal_ctx_workspace_in_use(ctx: *mut PetalCtx, blocks: *mut i64, bytes: *mut i64) -> c_int;
}
