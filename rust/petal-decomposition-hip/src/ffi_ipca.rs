//! Raw binding of include/petal_hip_ipca.h: IncrementalPca, the exact Pca fitted batch by batch (an extension beyond the crate).
use crate::ffi::{PetalCtx, PetalMatrix};
use std::os::raw::{c_int, c_void};

/// Opaque: the running statistic (rows seen, mean, M2), resident with the ctx that created it.
#[repr(C)]
pub struct PetalIpca {
    _private: [u8; 0],
}

/// Widest batch the streaming kernel takes (PETAL_IPCA_KERNEL_MAX_D); wider ones take the two-pass path.
pub const PETAL_IPCA_KERNEL_MAX_D: i64 = 1024;
/// petal_ctx_set_option: non-zero sends every batch and merge through the two-pass path (a test aid).
pub const PETAL_OPT_IPCA_FALLBACK: c_int = 32;

extern "C" {
    pub fn petal_ipca_create(ctx: *mut PetalCtx, d: i64, dtype: i32, centering: c_int, out: *mut *mut PetalIpca) -> c_int;
    pub fn petal_ipca_destroy(h: *mut PetalIpca);
    pub fn petal_ipca_reset(h: *mut PetalIpca) -> c_int;
    /// x.dtype must be the handle's, x.cols must be d; 0 rows: a no-op; values are not inspected
    pub fn petal_ipca_partial_fit(ctx: *mut PetalCtx, h: *mut PetalIpca, x: *const PetalMatrix) -> c_int;
    /// into += other (same ctx, d, dtype, centering); `other` is unchanged
    pub fn petal_ipca_merge(ctx: *mut PetalCtx, into: *mut PetalIpca, other: *const PetalIpca) -> c_int;
    /// outputs in the handle's dtype, laid out as petal_pca_fit's; the state is not modified
    pub fn petal_ipca_finalize(
        ctx: *mut PetalCtx, h: *const PetalIpca, k: i64, components: *mut c_void, means: *mut c_void, singular: *mut c_void,
        total_variance: *mut c_void,
    ) -> c_int;
    /// out8 = { d, dtype, centering, rows seen, batches, kernel batches, merges, 0 }
    pub fn petal_ipca_info(h: *const PetalIpca, out8: *mut i64) -> c_int;
    pub fn petal_ipca_get_state(ctx: *mut PetalCtx, h: *const PetalIpca, n: *mut f64, mean_d: *mut f64, m2_dxd: *mut f64) -> c_int;
    pub fn petal_ipca_set_state(ctx: *mut PetalCtx, h: *mut PetalIpca, n: f64, mean_d: *const f64, m2_dxd: *const f64) -> c_int;
}
