//! Raw binding of include/petal_hip_nmf_kl.h: Nmf with the Kullback-Leibler loss on sparse CSR data and its sweep by itself (an
//! extension beyond the crate).
use crate::ffi::{PetalCtx, PetalMatrix};
use crate::ffi_nmf::{PetalNmf, PetalNmfSpec};
use crate::ffi_sparse::PetalCsr;
use std::os::raw::c_int;

pub const PETAL_NMF_LOSS_FROBENIUS: i64 = 0;
pub const PETAL_NMF_LOSS_KL: i64 = 1;

extern "C" {
    /// petal_nmf_fit_csr with a loss: 0 is petal_nmf_fit_csr bit for bit, 1 the Kullback-Leibler loss, anything else InvalidInput
    pub fn petal_nmf_fit_csr_loss(ctx: *mut PetalCtx, x: *const PetalCsr, k: i64, spec: *const PetalNmfSpec, loss: i64, w0: *const PetalMatrix,
                                  h0: *const PetalMatrix, seed: i64, out: *mut *mut PetalNmf, w_out: *const PetalMatrix, kernel_path: *mut i64) -> c_int;
    /// loss[0] = the loss the model was fitted with
    pub fn petal_nmf_get_loss(h: *const PetalNmf, loss: *mut i64) -> c_int;
    /// one Kullback-Leibler sweep by itself on host f64 operands: g_out (R x k), colsum_out (k), term_out (1, with inner_iters == 0
    /// only); info1 = { k_nmf_kl_sweep ran }
    pub fn petal_nmf_kl_sweep_csr(ctx: *mut PetalCtx, x: *const PetalCsr, transposed: c_int, k: i64, g_in: *const f64, f: *const f64,
                                  spec: *const PetalNmfSpec, inner_iters: i64, g_out: *mut f64, colsum_out: *mut f64, term_out: *mut f64,
                                  info1: *mut i64) -> c_int;
}
