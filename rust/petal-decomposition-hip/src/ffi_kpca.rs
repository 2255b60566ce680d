//! Raw binding of include/petal_hip_kpca.h: KernelPca and its fused pass by itself (an extension beyond the crate).
use crate::ffi::{PetalCtx, PetalMatrix};
use std::os::raw::c_int;

pub const PETAL_KERNEL_LINEAR: i32 = 0;
pub const PETAL_KERNEL_POLY: i32 = 1;
pub const PETAL_KERNEL_RBF: i32 = 2;
pub const PETAL_KERNEL_SIGMOID: i32 = 3;
pub const PETAL_KERNEL_COSINE: i32 = 4;
/// petal_ctx_set_option: non-zero builds K~ and transform's phi(Xq Xt^T) A' from the library's other products (a test and A/B aid).
pub const PETAL_OPT_KPCA_FALLBACK: c_int = 36;

/// gamma <= 0 or NaN: 1 / d.
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct PetalKernelSpec {
    pub kernel: i32,
    pub degree: i32,
    pub gamma: f64,
    pub coef0: f64,
}

#[repr(C)]
pub struct PetalKpca {
    _private: [u8; 0],
}

extern "C" {
    /// fits on x (n x d) and returns a handle that lives with the ctx; y_out (nullable, n x k): fit_transform
    pub fn petal_kpca_fit(ctx: *mut PetalCtx, x: *const PetalMatrix, k: i64, spec: *const PetalKernelSpec, out: *mut *mut PetalKpca,
                          y_out: *const PetalMatrix) -> c_int;
    pub fn petal_kpca_destroy(h: *mut PetalKpca);
    /// y_out (m x k) = transform(x)
    pub fn petal_kpca_transform(ctx: *mut PetalCtx, h: *mut PetalKpca, x: *const PetalMatrix, y_out: *const PetalMatrix) -> c_int;
    /// eigenvalues: host f64 (k); scaled_vectors: host f64 (n x k); info8 = { n, d, k, fit kernel, transform kernel, order, kernel, top-k eigen-solver delivered }
    pub fn petal_kpca_get(h: *const PetalKpca, eigenvalues: *mut f64, scaled_vectors: *mut f64, info8: *mut i64) -> c_int;
    /// out (host f64, m x cols) = phi((xq - centre)(xt - centre)^T) a; a: host f64 (n x cols); centre: host f64 (d) or null
    pub fn petal_kernel_apply(ctx: *mut PetalCtx, xq: *const PetalMatrix, xt: *const PetalMatrix, spec: *const PetalKernelSpec, a: *const f64,
                              cols: i64, centre: *const f64, out: *mut f64, info1: *mut i64) -> c_int;
}
