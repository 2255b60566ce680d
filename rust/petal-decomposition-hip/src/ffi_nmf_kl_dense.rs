//! Raw binding of include/petal_hip_nmf_kl_dense.h: Nmf with the Kullback-Leibler loss on dense data and its fused pass by itself (an
//! extension beyond the crate).
use crate::ffi::{PetalCtx, PetalMatrix};
use crate::ffi_nmf::{PetalNmf, PetalNmfSpec};
use std::os::raw::c_int;

extern "C" {
    /// petal_nmf_fit with a loss: 0 is petal_nmf_fit bit for bit, 1 the dense Kullback-Leibler fit, anything else InvalidInput
    pub fn petal_nmf_fit_loss(ctx: *mut PetalCtx, x: *const PetalMatrix, k: i64, spec: *const PetalNmfSpec, loss: i64, w0: *const PetalMatrix,
                              h0: *const PetalMatrix, seed: i64, out: *mut *mut PetalNmf, w_out: *const PetalMatrix) -> c_int;
    /// petal_nmf_transform that dispatches on the model's loss
    pub fn petal_nmf_transform_loss(ctx: *mut PetalCtx, h: *mut PetalNmf, x: *const PetalMatrix, w_out: *const PetalMatrix) -> c_int;
    /// the fused dense Kullback-Leibler pass by itself on host f64 operands: w_out (n x k), a_out (k x d), colsum_out (k), term_out (1,
    /// with inner_iters == 0 only); info1 = { k_nmf_kl_pass ran }
    pub fn petal_nmf_kl_pass(ctx: *mut PetalCtx, x: *const PetalMatrix, k: i64, w_in: *const f64, h: *const f64, spec: *const PetalNmfSpec,
                             inner_iters: i64, w_out: *mut f64, a_out: *mut f64, colsum_out: *mut f64, term_out: *mut f64,
                             info1: *mut i64) -> c_int;
}
