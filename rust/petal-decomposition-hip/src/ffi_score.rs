//! Raw binding of include/petal_hip_score.h: row scores against a fitted projection (an extension beyond the crate).
use crate::ffi::{PetalCtx, PetalMatrix};
use std::os::raw::{c_int, c_void};

extern "C" {
    /// out: n x 2 = [residual, weighted]; weights: k values or null (all ones); y_out: nullable n x k projections
    pub fn petal_score_rows(
        ctx: *mut PetalCtx, x: *const PetalMatrix, components: *const c_void, means: *const c_void, k: i64,
        d: i64, centering: c_int, weights: *const c_void, out: *const PetalMatrix, y_out: *const PetalMatrix,
    ) -> c_int;
}
