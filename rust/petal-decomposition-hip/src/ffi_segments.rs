//! Raw binding of include/petal_hip_segments.h: one exact Pca per row segment of a row-sorted matrix (an extension beyond the crate).
use crate::ffi::{PetalCtx, PetalMatrix};
use std::os::raw::{c_int, c_void};

extern "C" {
    /// offsets: n_segments + 1 values from 0 to x.rows; components n_segments x k x d, means n_segments x d, singular n_segments x k,
    /// total_variance n_segments (host); status (nullable): 1 for a segment that holds a non-finite value; y_out: nullable rows x k
    pub fn petal_pca_fit_segments(
        ctx: *mut PetalCtx, x: *const PetalMatrix, offsets: *const i64, n_segments: i64, k: i64, centering: c_int,
        components: *mut c_void, means: *mut c_void, singular: *mut c_void, total_variance: *mut c_void, status: *mut i32,
        y_out: *const PetalMatrix, kernel_segments: *mut i64,
    ) -> c_int;
    pub fn petal_transform_segments(
        ctx: *mut PetalCtx, x: *const PetalMatrix, offsets: *const i64, n_segments: i64, components: *const c_void,
        means: *const c_void, k: i64, d: i64, centering: c_int, y_out: *const PetalMatrix,
    ) -> c_int;
    pub fn petal_inverse_transform_segments(
        ctx: *mut PetalCtx, y: *const PetalMatrix, offsets: *const i64, n_segments: i64, components: *const c_void,
        means: *const c_void, k: i64, d: i64, centering: c_int, x_out: *const PetalMatrix,
    ) -> c_int;
}
