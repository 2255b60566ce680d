//! Raw binding of include/petal_hip_nmf_cd_sparse.h: Nmf with the coordinate-descent solver on sparse CSR data and its sweep by itself
//! (an extension beyond the crate).
use crate::ffi::{PetalCtx, PetalMatrix};
use crate::ffi_nmf::{PetalNmf, PetalNmfSpec};
use crate::ffi_sparse::PetalCsr;
use std::os::raw::c_int;

extern "C" {
    /// petal_nmf_fit_csr with a solver: 0 is petal_nmf_fit_csr bit for bit, 1 the coordinate-descent fit on the sweeps, anything else
    /// InvalidInput; kernel_path: 1 the sweep ran, 0 the call densified
    pub fn petal_nmf_fit_csr_solver(ctx: *mut PetalCtx, x: *const PetalCsr, k: i64, spec: *const PetalNmfSpec, solver: i64, w0: *const PetalMatrix,
                                    h0: *const PetalMatrix, seed: i64, out: *mut *mut PetalNmf, w_out: *const PetalMatrix, kernel_path: *mut i64) -> c_int;
    /// petal_nmf_transform_csr for every solver: a solver-0 handle gives its bytes, a solver-1 handle the transform from zero
    pub fn petal_nmf_transform_csr_solver(ctx: *mut PetalCtx, h: *mut PetalNmf, x: *const PetalCsr, w_out: *const PetalMatrix, kernel_path: *mut i64) -> c_int;
    /// one coordinate-descent sweep by itself on host f64 operands: g_out (R x k), gram_out (k x k), dot_out (1), violation_out
    /// (inner_iters doubles, one per sweep); info1 = { k_nmf_cd_sweep ran }
    pub fn petal_nmf_cd_sweep_csr(ctx: *mut PetalCtx, x: *const PetalCsr, transposed: c_int, k: i64, g_in: *const f64, f: *const f64,
                                  spec: *const PetalNmfSpec, inner_iters: i64, from_zero: c_int, g_out: *mut f64, gram_out: *mut f64,
                                  dot_out: *mut f64, violation_out: *mut f64, info1: *mut i64) -> c_int;
}
