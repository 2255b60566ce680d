//! Raw binding of include/petal_hip_nmf.h: Nmf and its fused pass by itself (an extension beyond the crate).
use crate::ffi::{PetalCtx, PetalMatrix};
use std::os::raw::c_int;

/// petal_ctx_set_option: non-zero builds the pass, the scan and the H update from the library's other products (a test and A/B aid).
pub const PETAL_OPT_NMF_FALLBACK: c_int = 38;

/// max_iter >= 1; tol and the four penalties >= 0.
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct PetalNmfSpec {
    pub max_iter: i64,
    pub tol: f64,
    pub l1_w: f64,
    pub l2_w: f64,
    pub l1_h: f64,
    pub l2_h: f64,
}

#[repr(C)]
pub struct PetalNmf {
    _private: [u8; 0],
}

extern "C" {
    /// fits on x (n x d) and returns a handle that lives with the ctx; w0 / h0: both given or both null (random, from seed); w_out (nullable, n x k): fit_transform
    pub fn petal_nmf_fit(ctx: *mut PetalCtx, x: *const PetalMatrix, k: i64, spec: *const PetalNmfSpec, w0: *const PetalMatrix, h0: *const PetalMatrix,
                         seed: i64, out: *mut *mut PetalNmf, w_out: *const PetalMatrix) -> c_int;
    pub fn petal_nmf_destroy(h: *mut PetalNmf);
    /// w_out (m x k) = transform(x): max_iter W-updates from sqrt(mean(x) / k), one pass over x
    pub fn petal_nmf_transform(ctx: *mut PetalCtx, h: *mut PetalNmf, x: *const PetalMatrix, w_out: *const PetalMatrix) -> c_int;
    /// x_out (m x d) = w H
    pub fn petal_nmf_inverse_transform(ctx: *mut PetalCtx, h: *mut PetalNmf, w: *const PetalMatrix, x_out: *const PetalMatrix) -> c_int;
    /// components: host f64 (k x d); info6 = { n, d, k, n_iter, fit kernel, transform kernel }; err2 = { reconstruction_err, err_init }
    pub fn petal_nmf_get(h: *const PetalNmf, components: *mut f64, info6: *mut i64, err2: *mut f64) -> c_int;
    /// the pass by itself on host f64 operands: w_out (n x k), a_out (k x d) = w_out^T x, b_out (k x k) = w_out^T w_out
    pub fn petal_nmf_pass(ctx: *mut PetalCtx, x: *const PetalMatrix, k: i64, w_in: *const f64, h: *const f64, spec: *const PetalNmfSpec, inner_iters: i64,
                          w_out: *mut f64, a_out: *mut f64, b_out: *mut f64, info1: *mut i64) -> c_int;
}
