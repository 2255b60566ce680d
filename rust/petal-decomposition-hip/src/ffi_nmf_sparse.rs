//! Raw binding of include/petal_hip_nmf_sparse.h: Nmf on sparse CSR data and its sweep by itself (an extension beyond the crate).
use crate::ffi::{PetalCtx, PetalMatrix};
use crate::ffi_nmf::{PetalNmf, PetalNmfSpec};
use crate::ffi_sparse::PetalCsr;
use std::os::raw::c_int;

extern "C" {
    /// petal_nmf_fit on a sparse matrix; kernel_path (nullable): 1 the sweep kernel ran, 0 the call densified and ran the dense fit
    pub fn petal_nmf_fit_csr(ctx: *mut PetalCtx, x: *const PetalCsr, k: i64, spec: *const PetalNmfSpec, w0: *const PetalMatrix, h0: *const PetalMatrix,
                             seed: i64, out: *mut *mut PetalNmf, w_out: *const PetalMatrix, kernel_path: *mut i64) -> c_int;
    /// w_out (rows of x, k) = transform(x) for a model fitted on dense or on sparse data
    pub fn petal_nmf_transform_csr(ctx: *mut PetalCtx, h: *mut PetalNmf, x: *const PetalCsr, w_out: *const PetalMatrix, kernel_path: *mut i64) -> c_int;
    /// one sweep by itself on host f64 operands: g_out (R x k), gram_out (k x k), dot_out (1); info1 = { k_nmf_sweep ran }
    pub fn petal_nmf_sweep_csr(ctx: *mut PetalCtx, x: *const PetalCsr, transposed: c_int, k: i64, g_in: *const f64, f: *const f64,
                               spec: *const PetalNmfSpec, inner_iters: i64, g_out: *mut f64, gram_out: *mut f64, dot_out: *mut f64,
                               info1: *mut i64) -> c_int;
}
