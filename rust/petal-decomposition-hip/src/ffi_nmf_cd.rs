//! Raw binding of include/petal_hip_nmf_cd.h: Nmf with the coordinate-descent solver, its fused pass and its H side by themselves (an
//! extension beyond the crate).
use crate::ffi::{PetalCtx, PetalMatrix};
use crate::ffi_nmf::{PetalNmf, PetalNmfSpec};
use std::os::raw::c_int;

pub const PETAL_NMF_SOLVER_MU: i64 = 0;
pub const PETAL_NMF_SOLVER_CD: i64 = 1;

extern "C" {
    /// petal_nmf_fit with a solver: 0 is petal_nmf_fit bit for bit, 1 the coordinate-descent fit, anything else InvalidInput
    pub fn petal_nmf_fit_solver(ctx: *mut PetalCtx, x: *const PetalMatrix, k: i64, spec: *const PetalNmfSpec, solver: i64, w0: *const PetalMatrix,
                                h0: *const PetalMatrix, seed: i64, out: *mut *mut PetalNmf, w_out: *const PetalMatrix) -> c_int;
    /// the solver the model was fitted with
    pub fn petal_nmf_get_solver(h: *const PetalNmf, solver: *mut i64) -> c_int;
    /// the fused coordinate-descent pass by itself on host f64 operands: w_out (n x k), a_out (k x d), b_out (k x k), violation_out
    /// (inner_iters doubles, one per sweep); info1 = { k_nmf_cd_pass ran }
    pub fn petal_nmf_cd_pass(ctx: *mut PetalCtx, x: *const PetalMatrix, k: i64, w_in: *const f64, h: *const f64, spec: *const PetalNmfSpec,
                             inner_iters: i64, from_zero: c_int, w_out: *mut f64, a_out: *mut f64, b_out: *mut f64, violation_out: *mut f64,
                             info1: *mut i64) -> c_int;
    /// the H side by itself on host f64 operands: h_out (k x d), violation_out (1); info1 = { k_nmf_cd_hrule ran }
    pub fn petal_nmf_cd_hupdate(ctx: *mut PetalCtx, k: i64, d: i64, a: *const f64, b: *const f64, h_in: *const f64, spec: *const PetalNmfSpec,
                                h_out: *mut f64, violation_out: *mut f64, info1: *mut i64) -> c_int;
}
