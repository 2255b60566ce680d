//! Raw binding of include/petal_hip_wide.h: exact Pca on wide data through the n x n row Gram matrix (an extension beyond the crate).
use crate::ffi::{PetalCtx, PetalMatrix};
use std::os::raw::c_int;

/// petal_ctx_set_option: 0 = the auto rule (not sharded, n < d and d > 2048), positive = the dual route at every shape, negative = never.
pub const PETAL_OPT_PCA_DUAL: c_int = 33;
/// petal_ctx_set_option: non-zero builds K and the components from the library's other products (a test and A/B aid).
pub const PETAL_OPT_PCA_DUAL_FALLBACK: c_int = 34;

extern "C" {
    /// out4 = { route (0 primal, 1 dual), k_row_gram ran, order of the eigenproblem, feature chunks } of the last petal_pca_fit
    pub fn petal_pca_last_route(ctx: *mut PetalCtx, out4: *mut i64) -> c_int;
    /// out (host f64, n x n) = (x - centre)(x - centre)^T; centre: host f64 (d) or null; info2 = { kernel ran, feature chunks }
    pub fn petal_row_gram(ctx: *mut PetalCtx, x: *const PetalMatrix, centre: *const f64, out: *mut f64, info2: *mut i64) -> c_int;
}
