//! `KernelPca` over the C ABI (include/petal_hip_kpca.h; an extension beyond the crate): scikit-learn's KernelPCA with the kernels
//! linear, poly, rbf, sigmoid and cosine.  `fit_transform` = V sqrt(lambda); `transform` is one fused pass over the query rows whose
//! m x n kernel matrix never touches memory.  Everything is float64 inside; outputs are rounded once to `A`.
use crate::ffi_kpca::{self, PetalKernelSpec, PetalKpca};
use crate::{view, with_ctx, DecompositionError, HipScalar};
use ndarray::{Array1, Array2, ArrayBase, Data, Ix2};
use std::marker::PhantomData;

/// The kernel function; `gamma: None` means 1 / d.
#[derive(Debug, Clone, Copy, PartialEq)]
pub enum Kernel {
    Linear,
    Poly { gamma: Option<f64>, coef0: f64, degree: u32 },
    Rbf { gamma: Option<f64> },
    Sigmoid { gamma: Option<f64>, coef0: f64 },
    Cosine,
}

impl Kernel {
    fn spec(self) -> PetalKernelSpec {
        let (kernel, gamma, coef0, degree) = match self {
            Kernel::Linear => (ffi_kpca::PETAL_KERNEL_LINEAR, None, 1.0, 3),
            Kernel::Poly { gamma, coef0, degree } => (ffi_kpca::PETAL_KERNEL_POLY, gamma, coef0, degree as i32),
            Kernel::Rbf { gamma } => (ffi_kpca::PETAL_KERNEL_RBF, gamma, 1.0, 3),
            Kernel::Sigmoid { gamma, coef0 } => (ffi_kpca::PETAL_KERNEL_SIGMOID, gamma, coef0, 3),
            Kernel::Cosine => (ffi_kpca::PETAL_KERNEL_COSINE, None, 1.0, 3),
        };
        PetalKernelSpec { kernel, degree, gamma: gamma.unwrap_or(0.0), coef0 }
    }
}

/// { n, d, k, k_kmap ran on the fit's map, k_kapply ran on the last transform (-1 before the first), order of the eigenproblem, which
/// eigen-solver delivered }
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub struct KernelPcaInfo {
    pub n: i64,
    pub d: i64,
    pub k: i64,
    pub fit_kernel: bool,
    pub transform_kernel: i64,
    pub order: i64,
    /// the top-k subspace iteration delivered the eigenpairs (false: the full eigen-solver of order n ran)
    pub topk_solver: bool,
}

/// A component at or below the relative threshold (1e-6 f32, 1e-10 f64, on sqrt(lambda)) is a zero column of both outputs.  The fitted
/// model lives on the device with the process's ctx and keeps its own copy of the training rows.
pub struct KernelPca<A: HipScalar> {
    raw: *mut PetalKpca,
    k: usize,
    kernel: Kernel,
    _a: PhantomData<A>,
}
unsafe impl<A: HipScalar> Send for KernelPca<A> {}

impl<A: HipScalar> KernelPca<A> {
    pub fn new(n_components: usize, kernel: Kernel) -> Self { Self { raw: std::ptr::null_mut(), k: n_components, kernel, _a: PhantomData } }
    pub fn n_components(&self) -> usize { self.k }

    pub fn fit<S: Data<Elem = A>>(&mut self, input: &ArrayBase<S, Ix2>) -> Result<(), DecompositionError> { self.inner_fit(input, None) }
    pub fn fit_transform<S: Data<Elem = A>>(&mut self, input: &ArrayBase<S, Ix2>) -> Result<Array2<A>, DecompositionError> {
        let mut y = Array2::<A>::default((input.nrows(), self.k));
        self.inner_fit(input, Some(&mut y))?;
        Ok(y)
    }
    pub fn transform<S: Data<Elem = A>>(&mut self, input: &ArrayBase<S, Ix2>) -> Result<Array2<A>, DecompositionError> {
        let raw = self.handle()?;
        let mut y = Array2::<A>::default((input.nrows(), self.k));
        let (x, yv) = (view(input), view(&y.view_mut()));
        with_ctx(|ctx| unsafe { ffi_kpca::petal_kpca_transform(ctx, raw, &x, &yv) }, || ())?;
        Ok(y)
    }
    /// The k leading eigenvalues of the centred kernel matrix, as computed (descending).
    pub fn eigenvalues(&self) -> Result<Array1<f64>, DecompositionError> {
        let raw = self.handle()?;
        let mut lam = Array1::<f64>::zeros(self.k);
        with_ctx(|_| unsafe { ffi_kpca::petal_kpca_get(raw, lam.as_mut_ptr(), std::ptr::null_mut(), std::ptr::null_mut()) }, || ())?;
        Ok(lam)
    }
    pub fn info(&self) -> Result<KernelPcaInfo, DecompositionError> {
        let raw = self.handle()?;
        let mut v = [0i64; 8];
        with_ctx(|_| unsafe { ffi_kpca::petal_kpca_get(raw, std::ptr::null_mut(), std::ptr::null_mut(), v.as_mut_ptr()) }, || ())?;
        Ok(KernelPcaInfo { n: v[0], d: v[1], k: v[2], fit_kernel: v[3] != 0, transform_kernel: v[4], order: v[5], topk_solver: v[7] != 0 })
    }

    fn handle(&self) -> Result<*mut PetalKpca, DecompositionError> {
        if self.raw.is_null() {
            return Err(DecompositionError::InvalidInput("the model has not been fitted".into()));
        }
        Ok(self.raw)
    }
    fn inner_fit<S: Data<Elem = A>>(&mut self, input: &ArrayBase<S, Ix2>, y: Option<&mut Array2<A>>) -> Result<(), DecompositionError> {
        let x = view(input);
        let yv = y.map(|y| view(&y.view_mut()));
        let spec = self.kernel.spec();
        let mut raw = std::ptr::null_mut();
        let k = self.k as i64;
        with_ctx(
            |ctx| unsafe {
                ffi_kpca::petal_kpca_fit(ctx, &x, k, &spec, &mut raw, yv.as_ref().map_or(std::ptr::null(), |m| m as *const _))
            },
            || (),
        )?;
        unsafe { ffi_kpca::petal_kpca_destroy(self.raw) };
        self.raw = raw;
        Ok(())
    }
}

impl<A: HipScalar> Drop for KernelPca<A> {
    fn drop(&mut self) { unsafe { ffi_kpca::petal_kpca_destroy(self.raw) } }
}
