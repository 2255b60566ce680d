//! `Nmf` over the C ABI (include/petal_hip_nmf.h; an extension beyond the crate): scikit-learn's `NMF(solver="mu",
//! beta_loss="frobenius")`.  An iteration is one fused pass over the data; `transform` is one pass whatever `max_iter` is.  Everything
//! is float64 inside; outputs are rounded once to `A`.
use crate::ffi_nmf::{self, PetalNmf, PetalNmfSpec};
use crate::ffi_nmf_kl;
use crate::ffi_nmf_cd;
use crate::ffi_nmf_cd_sparse;
use crate::ffi_nmf_kl_dense;
use crate::ffi_nmf_sparse;
use crate::pca::CsrMatrix;
use crate::{view, with_ctx, DecompositionError, HipScalar};
use ndarray::{Array2, ArrayBase, Data, Ix2};
use std::marker::PhantomData;

/// The loss of a fit on sparse CSR input (include/petal_hip_nmf_kl.h; source only, unverified like the rest of this crate).
/// `KullbackLeibler` is scikit-learn's `beta_loss="kullback-leibler"`; dense input is refused under it.
#[derive(Debug, Clone, Copy, PartialEq, Eq, Default)]
pub enum NmfLoss {
    #[default]
    Frobenius,
    KullbackLeibler,
}

impl NmfLoss {
    fn code(self) -> i64 {
        match self {
            NmfLoss::Frobenius => ffi_nmf_kl::PETAL_NMF_LOSS_FROBENIUS,
            NmfLoss::KullbackLeibler => ffi_nmf_kl::PETAL_NMF_LOSS_KL,
        }
    }
}

/// What the dense entries do under the Kullback-Leibler loss (include/petal_hip_nmf_kl_dense.h; source only, unverified like the rest
/// of this crate).  `Compress` (the default) keeps them refusing; `Fused` sends the array to the fused dense pass `k_nmf_kl_pass` (the
/// composed path outside its envelope).  Under the Frobenius loss it changes nothing.
#[derive(Debug, Clone, Copy, PartialEq, Eq, Default)]
pub enum NmfDensePath {
    #[default]
    Compress,
    Fused,
}

/// The solver of a dense fit (include/petal_hip_nmf_cd.h; source only, unverified like the rest of this crate).
/// `CoordinateDescent` is scikit-learn's `solver="cd"` (its default, `shuffle=False`) under the Frobenius loss: the stopping rule runs
/// after every iteration and `transform` starts from W = 0.  It is refused with the Kullback-Leibler loss and with a `CsrMatrix`.
#[derive(Debug, Clone, Copy, PartialEq, Eq, Default)]
pub enum NmfSolver {
    #[default]
    MultiplicativeUpdate,
    CoordinateDescent,
}

impl NmfSolver {
    fn code(self) -> i64 {
        match self {
            NmfSolver::MultiplicativeUpdate => ffi_nmf_cd::PETAL_NMF_SOLVER_MU,
            NmfSolver::CoordinateDescent => ffi_nmf_cd::PETAL_NMF_SOLVER_CD,
        }
    }
}

/// What `fit_csr` / `transform_csr` do under `NmfSolver::CoordinateDescent` (include/petal_hip_nmf_cd_sparse.h; source only, unverified
/// like the rest of this crate).  `Refuse` (the default) returns InvalidInput; `Sweep` sends the matrix to the coordinate-descent sweeps
/// `k_nmf_cd_sweep` (at most 64 components on the kernel, otherwise the library densifies).  Under `MultiplicativeUpdate` it changes
/// nothing.
#[derive(Debug, Clone, Copy, PartialEq, Eq, Default)]
pub enum NmfSparsePath {
    #[default]
    Refuse,
    Sweep,
}

/// The parameters of a fit; `alpha_h: None` means the same as `alpha_w` (scikit-learn's "same").  `loss` is read by `fit_csr` and its
/// siblings; `transform_csr` follows the loss the model was fitted with.
#[derive(Debug, Clone, Copy, PartialEq)]
pub struct NmfParams {
    pub max_iter: usize,
    pub tol: f64,
    pub seed: u64,
    pub alpha_w: f64,
    pub alpha_h: Option<f64>,
    pub l1_ratio: f64,
    pub loss: NmfLoss,
    pub dense_path: NmfDensePath,
    pub solver: NmfSolver,
    pub sparse_path: NmfSparsePath,
}

impl Default for NmfParams {
    fn default() -> Self { Self { max_iter: 200, tol: 1e-4, seed: 0, alpha_w: 0.0, alpha_h: None, l1_ratio: 0.0, loss: NmfLoss::Frobenius, dense_path: NmfDensePath::Compress, solver: NmfSolver::MultiplicativeUpdate, sparse_path: NmfSparsePath::Refuse } }
}

/// { n, d, k, iterations run, k_nmf_pass ran in the fit, k_nmf_pass ran in the last transform (-1 before the first) }
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub struct NmfInfo {
    pub n: i64,
    pub d: i64,
    pub k: i64,
    pub n_iter: i64,
    pub fit_kernel: bool,
    pub transform_kernel: i64,
}

/// The fitted model lives on the device with the process's ctx.
pub struct Nmf<A: HipScalar> {
    raw: *mut PetalNmf,
    k: usize,
    params: NmfParams,
    kernel_path: i64,
    _a: PhantomData<A>,
}
unsafe impl<A: HipScalar> Send for Nmf<A> {}

impl<A: HipScalar> Nmf<A> {
    pub fn new(n_components: usize, params: NmfParams) -> Self { Self { raw: std::ptr::null_mut(), k: n_components, params, kernel_path: 0, _a: PhantomData } }
    pub fn n_components(&self) -> usize { self.k }

    /// Random initialisation from `Pcg(seed)`.
    pub fn fit<S: Data<Elem = A>>(&mut self, input: &ArrayBase<S, Ix2>) -> Result<(), DecompositionError> { self.inner_fit(input, None, None) }
    pub fn fit_transform<S: Data<Elem = A>>(&mut self, input: &ArrayBase<S, Ix2>) -> Result<Array2<A>, DecompositionError> {
        let mut w = Array2::<A>::default((input.nrows(), self.k));
        self.inner_fit(input, None, Some(&mut w))?;
        Ok(w)
    }
    /// Custom initialisation: `w0` (n x k) and `h0` (k x d).
    pub fn fit_transform_from<S: Data<Elem = A>>(&mut self, input: &ArrayBase<S, Ix2>, w0: &Array2<A>, h0: &Array2<A>) -> Result<Array2<A>, DecompositionError> {
        let mut w = Array2::<A>::default((input.nrows(), self.k));
        self.inner_fit(input, Some((w0, h0)), Some(&mut w))?;
        Ok(w)
    }
    pub fn transform<S: Data<Elem = A>>(&mut self, input: &ArrayBase<S, Ix2>) -> Result<Array2<A>, DecompositionError> {
        let raw = self.handle()?;
        let mut w = Array2::<A>::default((input.nrows(), self.k));
        let (x, wv) = (view(input), view(&w.view_mut()));
        if self.params.dense_path == NmfDensePath::Fused {
            // dispatches on the model's loss; a Frobenius model: petal_nmf_transform's bytes
            with_ctx(|ctx| unsafe { ffi_nmf_kl_dense::petal_nmf_transform_loss(ctx, raw, &x, &wv) }, || ())?;
            if self.model_loss()? == NmfLoss::KullbackLeibler && input.nrows() > 0 {
                self.kernel_path = self.info()?.transform_kernel;
            }
        } else {
            with_ctx(|ctx| unsafe { ffi_nmf::petal_nmf_transform(ctx, raw, &x, &wv) }, || ())?;
        }
        Ok(w)
    }
    pub fn inverse_transform<S: Data<Elem = A>>(&mut self, w: &ArrayBase<S, Ix2>) -> Result<Array2<A>, DecompositionError> {
        let raw = self.handle()?;
        let d = self.info()?.d as usize;
        let mut x = Array2::<A>::default((w.nrows(), d));
        let (wv, xv) = (view(w), view(&x.view_mut()));
        with_ctx(|ctx| unsafe { ffi_nmf::petal_nmf_inverse_transform(ctx, raw, &wv, &xv) }, || ())?;
        Ok(x)
    }
    /// H, k x d, float64.
    pub fn components(&self) -> Result<Array2<f64>, DecompositionError> {
        let raw = self.handle()?;
        let d = self.info()?.d as usize;
        let mut h = Array2::<f64>::zeros((self.k, d));
        with_ctx(|_| unsafe { ffi_nmf::petal_nmf_get(raw, h.as_mut_ptr(), std::ptr::null_mut(), std::ptr::null_mut()) }, || ())?;
        Ok(h)
    }
    pub fn reconstruction_err(&self) -> Result<f64, DecompositionError> {
        let raw = self.handle()?;
        let mut e = [0f64; 2];
        with_ctx(|_| unsafe { ffi_nmf::petal_nmf_get(raw, std::ptr::null_mut(), std::ptr::null_mut(), e.as_mut_ptr()) }, || ())?;
        Ok(e[0])
    }
    pub fn info(&self) -> Result<NmfInfo, DecompositionError> {
        let raw = self.handle()?;
        let mut v = [0i64; 6];
        with_ctx(|_| unsafe { ffi_nmf::petal_nmf_get(raw, std::ptr::null_mut(), v.as_mut_ptr(), std::ptr::null_mut()) }, || ())?;
        Ok(NmfInfo { n: v[0], d: v[1], k: v[2], n_iter: v[3], fit_kernel: v[4] != 0, transform_kernel: v[5] })
    }

    /// Sparse CSR input (include/petal_hip_nmf_sparse.h; source only, unverified like the rest of this crate): never densified where
    /// the sweep kernel runs (at most 64 components, a resident handle); `kernel_path` says which path the last sparse call took.
    pub fn fit_csr(&mut self, input: &CsrMatrix<A>) -> Result<(), DecompositionError> { self.inner_fit_csr(input, None, None) }
    pub fn fit_transform_csr(&mut self, input: &CsrMatrix<A>) -> Result<Array2<A>, DecompositionError> {
        let mut w = Array2::<A>::default((input.nrows(), self.k));
        self.inner_fit_csr(input, None, Some(&mut w))?;
        Ok(w)
    }
    pub fn fit_transform_csr_from(&mut self, input: &CsrMatrix<A>, w0: &Array2<A>, h0: &Array2<A>) -> Result<Array2<A>, DecompositionError> {
        let mut w = Array2::<A>::default((input.nrows(), self.k));
        self.inner_fit_csr(input, Some((w0, h0)), Some(&mut w))?;
        Ok(w)
    }
    pub fn transform_csr(&mut self, input: &CsrMatrix<A>) -> Result<Array2<A>, DecompositionError> {
        let raw = self.handle()?;
        let mut w = Array2::<A>::default((input.nrows(), self.k));
        let wv = view(&w.view_mut());
        let mut path = 0i64;
        if self.params.sparse_path == NmfSparsePath::Sweep {
            // dispatches on the model's solver; a multiplicative model: petal_nmf_transform_csr's bytes
            with_ctx(|ctx| unsafe { ffi_nmf_cd_sparse::petal_nmf_transform_csr_solver(ctx, raw, input.raw(), &wv, &mut path) }, || ())?;
        } else {
            with_ctx(|ctx| unsafe { ffi_nmf_sparse::petal_nmf_transform_csr(ctx, raw, input.raw(), &wv, &mut path) }, || ())?;
        }
        self.kernel_path = path;
        Ok(w)
    }
    /// The loss the fitted model remembers.
    pub fn model_loss(&self) -> Result<NmfLoss, DecompositionError> {
        let raw = self.handle()?;
        let mut v = 0i64;
        with_ctx(|_| unsafe { ffi_nmf_kl::petal_nmf_get_loss(raw, &mut v) }, || ())?;
        Ok(if v == ffi_nmf_kl::PETAL_NMF_LOSS_KL { NmfLoss::KullbackLeibler } else { NmfLoss::Frobenius })
    }
    /// 1: the sweep kernel ran in the last sparse call; 0: the call densified (Frobenius) or ran the host loop (Kullback-Leibler).
    pub fn kernel_path(&self) -> i64 { self.kernel_path }

    fn spec(&self, n: f64, d: f64) -> PetalNmfSpec {
        let p = self.params;
        let (aw, ah, rho) = (p.alpha_w, p.alpha_h.unwrap_or(p.alpha_w), p.l1_ratio);
        PetalNmfSpec { max_iter: p.max_iter as i64, tol: p.tol, l1_w: d * aw * rho, l2_w: d * aw * (1.0 - rho), l1_h: n * ah * rho, l2_h: n * ah * (1.0 - rho) }
    }
    fn inner_fit_csr(&mut self, input: &CsrMatrix<A>, init: Option<(&Array2<A>, &Array2<A>)>, w: Option<&mut Array2<A>>)
        -> Result<(), DecompositionError> {
        let solver = self.params.solver;
        let cd = solver == NmfSolver::CoordinateDescent;
        if cd && self.params.sparse_path != NmfSparsePath::Sweep {
            return Err(DecompositionError::InvalidInput("Nmf: the coordinate-descent solver does not take a CsrMatrix in this version".into()));
        }
        if cd && self.params.loss != NmfLoss::Frobenius {
            return Err(DecompositionError::InvalidInput("Nmf: the coordinate-descent solver does not take the kullback-leibler loss".into()));
        }
        let wv = w.map(|w| view(&w.view_mut()));
        let iv = init.map(|(w0, h0)| (view(w0), view(h0)));
        let spec = self.spec(input.nrows() as f64, input.ncols() as f64);
        let mut raw = std::ptr::null_mut();
        let mut path = 0i64;
        let (k, seed, loss) = (self.k as i64, self.params.seed as i64, self.params.loss);
        with_ctx(
            |ctx| unsafe {
                let (w0, h0) = (iv.as_ref().map_or(std::ptr::null(), |m| &m.0 as *const _), iv.as_ref().map_or(std::ptr::null(), |m| &m.1 as *const _));
                let wo = wv.as_ref().map_or(std::ptr::null(), |m| m as *const _);
                if cd {
                    ffi_nmf_cd_sparse::petal_nmf_fit_csr_solver(ctx, input.raw(), k, &spec, solver.code(), w0, h0, seed, &mut raw, wo, &mut path)
                } else if loss == NmfLoss::Frobenius {
                    ffi_nmf_sparse::petal_nmf_fit_csr(ctx, input.raw(), k, &spec, w0, h0, seed, &mut raw, wo, &mut path)
                } else {
                    ffi_nmf_kl::petal_nmf_fit_csr_loss(ctx, input.raw(), k, &spec, loss.code(), w0, h0, seed, &mut raw, wo, &mut path)
                }
            },
            || (),
        )?;
        unsafe { ffi_nmf::petal_nmf_destroy(self.raw) };
        self.raw = raw;
        self.kernel_path = path;
        Ok(())
    }
    /// The solver the fitted model remembers.
    pub fn model_solver(&self) -> Result<NmfSolver, DecompositionError> {
        let raw = self.handle()?;
        let mut v: i64 = 0;
        if unsafe { ffi_nmf_cd::petal_nmf_get_solver(raw, &mut v) } != 0 {
            return Err(DecompositionError::InvalidInput("petal_nmf_get_solver failed".into()));
        }
        Ok(if v == ffi_nmf_cd::PETAL_NMF_SOLVER_CD { NmfSolver::CoordinateDescent } else { NmfSolver::MultiplicativeUpdate })
    }
    fn handle(&self) -> Result<*mut PetalNmf, DecompositionError> {
        if self.raw.is_null() {
            return Err(DecompositionError::InvalidInput("the model has not been fitted".into()));
        }
        Ok(self.raw)
    }
    fn inner_fit<S: Data<Elem = A>>(&mut self, input: &ArrayBase<S, Ix2>, init: Option<(&Array2<A>, &Array2<A>)>, w: Option<&mut Array2<A>>)
        -> Result<(), DecompositionError> {
        let solver = self.params.solver;
        let cd = solver == NmfSolver::CoordinateDescent;
        if cd && self.params.loss != NmfLoss::Frobenius {
            return Err(DecompositionError::InvalidInput("Nmf: the coordinate-descent solver does not take the kullback-leibler loss".into()));
        }
        let fused = self.params.loss == NmfLoss::KullbackLeibler && self.params.dense_path == NmfDensePath::Fused;
        if self.params.loss == NmfLoss::KullbackLeibler && !fused {
            return Err(DecompositionError::InvalidInput("Nmf: the kullback-leibler loss takes a CsrMatrix".into()));
        }
        let x = view(input);
        let wv = w.map(|w| view(&w.view_mut()));
        let iv = init.map(|(w0, h0)| (view(w0), view(h0)));
        let spec = self.spec(input.nrows() as f64, input.ncols() as f64);
        let mut raw = std::ptr::null_mut();
        let (k, seed, loss) = (self.k as i64, self.params.seed as i64, self.params.loss);
        with_ctx(
            |ctx| unsafe {
                let (w0, h0) = (iv.as_ref().map_or(std::ptr::null(), |m| &m.0 as *const _), iv.as_ref().map_or(std::ptr::null(), |m| &m.1 as *const _));
                let wo = wv.as_ref().map_or(std::ptr::null(), |m| m as *const _);
                if cd {
                    ffi_nmf_cd::petal_nmf_fit_solver(ctx, &x, k, &spec, solver.code(), w0, h0, seed, &mut raw, wo)
                } else if fused {
                    ffi_nmf_kl_dense::petal_nmf_fit_loss(ctx, &x, k, &spec, loss.code(), w0, h0, seed, &mut raw, wo)
                } else {
                    ffi_nmf::petal_nmf_fit(ctx, &x, k, &spec, w0, h0, seed, &mut raw, wo)
                }
            },
            || (),
        )?;
        unsafe { ffi_nmf::petal_nmf_destroy(self.raw) };
        self.raw = raw;
        if fused {
            self.kernel_path = if self.info()?.fit_kernel { 1 } else { 0 };
        }
        Ok(())
    }
}

impl<A: HipScalar> Drop for Nmf<A> {
    fn drop(&mut self) { unsafe { ffi_nmf::petal_nmf_destroy(self.raw) } }
}
