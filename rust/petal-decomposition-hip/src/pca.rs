//! `Pca` (`src/pca.rs:41-231` of the reference) and `RandomizedPca` (`src/pca.rs:317-663`) over the C ABI.
use crate::{ffi, ffi_ipca, ffi_score, ffi_segments, ffi_sparse, ffi_wide, view, with_ctx, DecompositionError, HipScalar};
use ndarray::{Array1, Array2, Array3, ArrayBase, Data, Ix2};
use rand::Rng;
use rand_distr::StandardNormal;
use rand_pcg::Mcg128Xsl64 as Pcg;
use std::os::raw::c_void;

const N_OVERSAMPLE: usize = 10; // src/pca.rs:679
const N_ITER: i64 = 7; // src/pca.rs:680

/// Facts of the last exact `Pca` fit of this process (include/petal_hip_wide.h): `dual` = the n x n row-Gram route of wide data
/// (n < d, d > 2048) was taken, `kernel` = k_row_gram ran, `order` of the eigenproblem, feature `chunks` of the row-Gram launch.
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub struct PcaRoute {
    pub dual: bool,
    pub kernel: bool,
    pub order: i64,
    pub chunks: i64,
}

/// Exact PCA.  Field names follow the reference so serialized models interchange.
#[cfg_attr(feature = "serde", derive(serde::Serialize, serde::Deserialize))]
#[derive(Debug, Clone)]
pub struct Pca<A: HipScalar> {
    components: Array2<A>,
    n_samples: usize,
    means: Array1<A>,
    total_variance: A,
    singular: Array1<A>,
    centering: bool,
}

impl<A: HipScalar> Pca<A> {
    pub fn new(n_components: usize) -> Self { PcaBuilder::new(n_components).build() }
    pub fn components(&self) -> &Array2<A> { &self.components }
    pub fn mean(&self) -> &Array1<A> { &self.means }
    pub fn n_components(&self) -> usize { self.components.nrows() }
    pub fn singular_values(&self) -> &Array1<A> { &self.singular }
    /// sigma^2 / total_variance (src/pca.rs:101-105).
    pub fn explained_variance_ratio(&self) -> Array1<A> {
        let tv = self.total_variance.to_f64();
        self.singular.mapv(|s| A::from_f64(s.to_f64() * s.to_f64() / tv))
    }

    pub fn fit<S: Data<Elem = A>>(&mut self, input: &ArrayBase<S, Ix2>) -> Result<(), DecompositionError> {
        self.inner_fit(input, None)
    }
    pub fn fit_transform<S: Data<Elem = A>>(&mut self, input: &ArrayBase<S, Ix2>) -> Result<Array2<A>, DecompositionError> {
        let mut y = Array2::<A>::default((input.nrows(), self.n_components()));
        self.inner_fit(input, Some(&mut y))?;
        Ok(y)
    }
    pub fn transform<S: Data<Elem = A>>(&self, input: &ArrayBase<S, Ix2>) -> Result<Array2<A>, DecompositionError> {
        transform(input, &self.components, &self.means, self.centering)
    }
    pub fn inverse_transform<S: Data<Elem = A>>(&self, input: &ArrayBase<S, Ix2>) -> Result<Array2<A>, DecompositionError> {
        inverse_transform(input, &self.components, &self.means, self.centering)
    }

    /// Which route the last exact fit took (include/petal_hip_wide.h; an extension beyond the crate).
    pub fn last_route() -> Result<PcaRoute, DecompositionError> {
        let mut v = [0i64; 4];
        with_ctx(|ctx| unsafe { ffi_wide::petal_pca_last_route(ctx, v.as_mut_ptr()) }, || ())?;
        Ok(PcaRoute { dual: v[0] != 0, kernel: v[1] != 0, order: v[2], chunks: v[3] })
    }

    // ---- scores of rows against the fitted model: an extension beyond the crate (include/petal_hip_score.h) ----
    /// lambda_j = sigma_j^2 / (n_samples - 1).
    pub fn explained_variance(&self) -> Array1<A> { explained_variance(&self.singular, self.n_samples) }
    /// Mean variance of the min(n_samples, d) - k discarded directions, as scikit-learn defines it.
    pub fn noise_variance(&self) -> A { noise_variance(&self.singular, self.total_variance, self.n_samples, self.means.len()) }
    /// |xc|^2 - |xc V^T|^2 per row from one pass over the input (rounding noise below about 1e-5 |xc|^2 for f32).
    pub fn reconstruction_error<S: Data<Elem = A>>(&self, input: &ArrayBase<S, Ix2>) -> Result<Array1<A>, DecompositionError> {
        Ok(score_rows(input, &self.components, &self.means, self.centering, None)?.column(0).to_owned())
    }
    /// Hotelling's T^2: sum_j y_j^2 / lambda_j per row.
    pub fn hotelling_t2<S: Data<Elem = A>>(&self, input: &ArrayBase<S, Ix2>) -> Result<Array1<A>, DecompositionError> {
        let w = inverse_variances(&self.explained_variance())?;
        Ok(score_rows(input, &self.components, &self.means, self.centering, Some(&w))?.column(1).to_owned())
    }
    /// Log-likelihood of each row under the probabilistic-PCA model (scikit-learn's `score_samples`).
    pub fn score_samples<S: Data<Elem = A>>(&self, input: &ArrayBase<S, Ix2>) -> Result<Array1<A>, DecompositionError> {
        score_samples(input, &self.components, &self.means, self.centering, &self.explained_variance(), self.noise_variance())
    }

    fn inner_fit<S: Data<Elem = A>>(&mut self, input: &ArrayBase<S, Ix2>, y: Option<&mut Array2<A>>) -> Result<(), DecompositionError> {
        let (k, d) = (self.n_components(), input.ncols());
        let mut comps = Array2::<A>::default((k, d));
        let mut means = Array1::<A>::default(d);
        let mut sing = Array1::<A>::default(k);
        let mut tv = A::default();
        let x = view(input);
        let yv = y.as_ref().map(|y| view(&**y));
        with_ctx(
            |ctx| unsafe {
                ffi::petal_pca_fit(ctx, &x, k as i64, self.centering as i32, comps.as_mut_ptr() as *mut c_void,
                    means.as_mut_ptr() as *mut c_void, sing.as_mut_ptr() as *mut c_void,
                    &mut tv as *mut A as *mut c_void, yv.as_ref().map_or(std::ptr::null(), |v| v as *const _))
            },
            || (),
        )?;
        if input.nrows() == 0 && self.centering {
            return Ok(()); // mean_axis -> None: Ok, model untouched (src/pca.rs:207-211)
        }
        self.components = comps;
        self.means = means;
        self.singular = sing;
        self.total_variance = tv;
        self.n_samples = input.nrows();
        Ok(())
    }
}

pub struct PcaBuilder {
    n_components: usize,
    centering: bool,
}
impl PcaBuilder {
    pub fn new(n_components: usize) -> Self { Self { n_components, centering: true } }
    pub fn centering(mut self, centering: bool) -> Self { self.centering = centering; self }
    pub fn build<A: HipScalar>(self) -> Pca<A> {
        Pca {
            components: Array2::default((self.n_components, 0)),
            n_samples: 0,
            means: Array1::default(0),
            total_variance: A::default(),
            singular: Array1::default(0),
            centering: self.centering,
        }
    }
}

/// Randomized truncated SVD (Halko range finder with power iterations, src/pca.rs:668-718).
#[cfg_attr(feature = "serde", derive(serde::Serialize, serde::Deserialize))]
#[derive(Debug, Clone)]
pub struct RandomizedPca<A: HipScalar, R = Pcg> {
    rng: R,
    components: Array2<A>,
    n_samples: usize,
    means: Array1<A>,
    total_variance: A,
    singular: Array1<A>,
    centering: bool,
}

impl<A: HipScalar> RandomizedPca<A, Pcg> {
    pub fn new(n_components: usize) -> Self { RandomizedPcaBuilder::new(n_components).build() }
    pub fn with_seed(n_components: usize, seed: u128) -> Self { RandomizedPcaBuilder::new(n_components).seed(seed).build() }
}
impl<A: HipScalar, R: Rng> RandomizedPca<A, R> {
    pub fn with_rng(n_components: usize, rng: R) -> Self { RandomizedPcaBuilder::with_rng(rng, n_components).build() }
    pub fn components(&self) -> &Array2<A> { &self.components }
    pub fn mean(&self) -> &Array1<A> { &self.means }
    pub fn n_components(&self) -> usize { self.components.nrows() }
    pub fn singular_values(&self) -> &Array1<A> { &self.singular }
    pub fn explained_variance_ratio(&self) -> Array1<A> {
        let tv = self.total_variance.to_f64();
        self.singular.mapv(|s| A::from_f64(s.to_f64() * s.to_f64() / tv))
    }

    pub fn fit<S: Data<Elem = A>>(&mut self, input: &ArrayBase<S, Ix2>) -> Result<(), DecompositionError> {
        self.inner_fit(input, None)
    }
    pub fn fit_transform<S: Data<Elem = A>>(&mut self, input: &ArrayBase<S, Ix2>) -> Result<Array2<A>, DecompositionError> {
        let mut y = Array2::<A>::default((input.nrows(), self.n_components()));
        self.inner_fit(input, Some(&mut y))?;
        Ok(y)
    }
    pub fn transform<S: Data<Elem = A>>(&self, input: &ArrayBase<S, Ix2>) -> Result<Array2<A>, DecompositionError> {
        transform(input, &self.components, &self.means, self.centering)
    }
    pub fn inverse_transform<S: Data<Elem = A>>(&self, input: &ArrayBase<S, Ix2>) -> Result<Array2<A>, DecompositionError> {
        inverse_transform(input, &self.components, &self.means, self.centering)
    }

    // ---- scores of rows against the fitted model: an extension beyond the crate (include/petal_hip_score.h) ----
    /// lambda_j = sigma_j^2 / (n_samples - 1).
    pub fn explained_variance(&self) -> Array1<A> { explained_variance(&self.singular, self.n_samples) }
    /// Mean variance of the min(n_samples, d) - k discarded directions, as scikit-learn defines it.
    pub fn noise_variance(&self) -> A { noise_variance(&self.singular, self.total_variance, self.n_samples, self.means.len()) }
    /// |xc|^2 - |xc V^T|^2 per row from one pass over the input (rounding noise below about 1e-5 |xc|^2 for f32).
    pub fn reconstruction_error<S: Data<Elem = A>>(&self, input: &ArrayBase<S, Ix2>) -> Result<Array1<A>, DecompositionError> {
        Ok(score_rows(input, &self.components, &self.means, self.centering, None)?.column(0).to_owned())
    }
    /// Hotelling's T^2: sum_j y_j^2 / lambda_j per row.
    pub fn hotelling_t2<S: Data<Elem = A>>(&self, input: &ArrayBase<S, Ix2>) -> Result<Array1<A>, DecompositionError> {
        let w = inverse_variances(&self.explained_variance())?;
        Ok(score_rows(input, &self.components, &self.means, self.centering, Some(&w))?.column(1).to_owned())
    }
    /// Log-likelihood of each row under the probabilistic-PCA model (scikit-learn's `score_samples`).
    pub fn score_samples<S: Data<Elem = A>>(&self, input: &ArrayBase<S, Ix2>) -> Result<Array1<A>, DecompositionError> {
        score_samples(input, &self.components, &self.means, self.centering, &self.explained_variance(), self.noise_variance())
    }

    // ---- sparse CSR input, never densified: an extension beyond the crate (include/petal_hip_sparse.h) ----
    pub fn fit_csr(&mut self, input: &CsrMatrix<A>) -> Result<(), DecompositionError> {
        self.inner_fit_csr(input, None)
    }
    pub fn fit_transform_csr(&mut self, input: &CsrMatrix<A>) -> Result<Array2<A>, DecompositionError> {
        let mut y = Array2::<A>::default((input.nrows(), self.n_components()));
        self.inner_fit_csr(input, Some(&mut y))?;
        Ok(y)
    }
    pub fn transform_csr(&self, input: &CsrMatrix<A>) -> Result<Array2<A>, DecompositionError> {
        let (k, d) = (self.n_components(), self.means.len());
        if input.ncols() != d {
            return Err(DecompositionError::InvalidInput(format!("# of columns should be {d}")));
        }
        let y = Array2::<A>::default((input.nrows(), k));
        let yv = view(&y);   // (the library writes through the view's pointer, as transform() above)
        with_ctx(
            |ctx| unsafe {
                ffi_sparse::petal_transform_csr(ctx, input.raw, self.components.as_ptr() as *const c_void, self.means.as_ptr() as *const c_void,
                    k as i64, d as i64, self.centering as i32, &yv, std::ptr::null_mut())
            },
            || (),
        )?;
        Ok(y)
    }
    fn inner_fit_csr(&mut self, input: &CsrMatrix<A>, y: Option<&mut Array2<A>>) -> Result<(), DecompositionError> {
        let (k, d) = (self.n_components(), input.ncols());
        if input.nrows() < k || d < k {
            return Err(DecompositionError::InvalidInput(format!("every dimension should be at least {k}")));
        }
        if input.nrows() == 0 && self.centering {
            return Ok(());
        }
        let l = k + N_OVERSAMPLE;
        let omega = Array2::<A>::from_shape_fn((d, l), |_| A::from_f64(self.rng.sample::<f64, _>(StandardNormal)));
        let mut comps = Array2::<A>::default((k, d));
        let mut means = Array1::<A>::default(d);
        let mut sing = Array1::<A>::default(k);
        let mut tv = A::default();
        let yv = y.as_ref().map(|y| view(&**y));
        with_ctx(
            |ctx| unsafe {
                ffi_sparse::petal_rpca_fit_csr(ctx, input.raw, k as i64, N_OVERSAMPLE as i64, N_ITER, self.centering as i32,
                    omega.as_ptr() as *const c_void, comps.as_mut_ptr() as *mut c_void, means.as_mut_ptr() as *mut c_void,
                    sing.as_mut_ptr() as *mut c_void, &mut tv as *mut A as *mut c_void,
                    yv.as_ref().map_or(std::ptr::null(), |v| v as *const _), std::ptr::null_mut())
            },
            || (),
        )?;
        self.components = comps;
        self.means = means;
        self.singular = sing;
        self.total_variance = tv;
        self.n_samples = input.nrows();
        Ok(())
    }

    fn inner_fit<S: Data<Elem = A>>(&mut self, input: &ArrayBase<S, Ix2>, y: Option<&mut Array2<A>>) -> Result<(), DecompositionError> {
        let (k, d) = (self.n_components(), input.ncols());
        if input.nrows() < k || d < k {
            return Err(DecompositionError::InvalidInput(format!("every dimension should be at least {k}")));
        }
        if input.nrows() == 0 && self.centering {
            return Ok(());
        }
        // Omega exactly as the reference draws it (src/pca.rs:701-705): d x (k + 10), row-major fill order, one f64
        // StandardNormal draw per entry cast to the element type; the model's RNG advances once per fit.
        let l = k + N_OVERSAMPLE;
        let omega = Array2::<A>::from_shape_fn((d, l), |_| A::from_f64(self.rng.sample::<f64, _>(StandardNormal)));
        let mut comps = Array2::<A>::default((k, d));
        let mut means = Array1::<A>::default(d);
        let mut sing = Array1::<A>::default(k);
        let mut tv = A::default();
        let x = view(input);
        let yv = y.as_ref().map(|y| view(&**y));
        with_ctx(
            |ctx| unsafe {
                ffi::petal_rpca_fit(ctx, &x, k as i64, N_OVERSAMPLE as i64, N_ITER, self.centering as i32,
                    omega.as_ptr() as *const c_void, comps.as_mut_ptr() as *mut c_void, means.as_mut_ptr() as *mut c_void,
                    sing.as_mut_ptr() as *mut c_void, &mut tv as *mut A as *mut c_void,
                    yv.as_ref().map_or(std::ptr::null(), |v| v as *const _))
            },
            || (),
        )?;
        self.components = comps;
        self.means = means;
        self.singular = sing;
        self.total_variance = tv;
        self.n_samples = input.nrows();
        Ok(())
    }
}

pub struct RandomizedPcaBuilder<R> {
    rng: R,
    n_components: usize,
    centering: bool,
}
impl RandomizedPcaBuilder<Pcg> {
    /// Randomly seeded PCG, like the reference (src/pca.rs:578-585).
    pub fn new(n_components: usize) -> Self {
        use rand::SeedableRng;
        let seed: u128 = rand::rng().random();
        Self { rng: Pcg::from_seed(seed.to_be_bytes()), n_components, centering: true }
    }
    /// `Pcg::from_seed(seed.to_be_bytes())` as in src/pca.rs:599-602.
    pub fn seed(mut self, seed: u128) -> Self {
        use rand::SeedableRng;
        self.rng = Pcg::from_seed(seed.to_be_bytes());
        self
    }
}
impl<R: Rng> RandomizedPcaBuilder<R> {
    pub fn with_rng(rng: R, n_components: usize) -> Self { Self { rng, n_components, centering: true } }
    pub fn centering(mut self, centering: bool) -> Self { self.centering = centering; self }
    pub fn build<A: HipScalar>(self) -> RandomizedPca<A, R> {
        RandomizedPca {
            rng: self.rng,
            components: Array2::default((self.n_components, 0)),
            n_samples: 0,
            means: Array1::default(0),
            total_variance: A::default(),
            singular: Array1::default(0),
            centering: self.centering,
        }
    }
}

/// (input - mean) . components^T  (src/pca.rs:726-750)
pub(crate) fn transform<A: HipScalar, S: Data<Elem = A>>(
    input: &ArrayBase<S, Ix2>, components: &Array2<A>, means: &Array1<A>, centering: bool,
) -> Result<Array2<A>, DecompositionError> {
    let (k, d) = components.dim();
    let mut y = Array2::<A>::default((input.nrows(), k));
    let (x, yv) = (view(input), view(&y));
    with_ctx(
        |ctx| unsafe {
            ffi::petal_transform(ctx, &x, components.as_ptr() as *const c_void, means.as_ptr() as *const c_void, k as i64,
                d as i64, centering as i32, &yv)
        },
        || (),
    )?;
    let _ = &mut y; // written through yv
    Ok(y)
}

/// input . components + mean  (src/pca.rs:788-811)
pub(crate) fn inverse_transform<A: HipScalar, S: Data<Elem = A>>(
    input: &ArrayBase<S, Ix2>, components: &Array2<A>, means: &Array1<A>, centering: bool,
) -> Result<Array2<A>, DecompositionError> {
    let (k, d) = components.dim();
    let mut x_out = Array2::<A>::default((input.nrows(), d));
    let (yv, xv) = (view(input), view(&x_out));
    with_ctx(
        |ctx| unsafe {
            ffi::petal_inverse_transform(ctx, &yv, components.as_ptr() as *const c_void, means.as_ptr() as *const c_void,
                k as i64, d as i64, centering as i32, &xv)
        },
        || (),
    )?;
    let _ = &mut x_out;
    Ok(x_out)
}

fn explained_variance<A: HipScalar>(singular: &Array1<A>, n_samples: usize) -> Array1<A> {
    let nm1 = n_samples as f64 - 1.0;
    singular.mapv(|s| A::from_f64(s.to_f64() * s.to_f64() / nm1))
}

fn noise_variance<A: HipScalar>(singular: &Array1<A>, total_variance: A, n_samples: usize, d: usize) -> A {
    let rest = n_samples.min(d) as i64 - singular.len() as i64;
    if rest <= 0 {
        return A::from_f64(0.0);
    }
    let kept: f64 = singular.iter().map(|s| s.to_f64() * s.to_f64()).sum();
    A::from_f64((total_variance.to_f64() - kept) / (n_samples as f64 - 1.0) / rest as f64)
}

fn inverse_variances<A: HipScalar>(lambda: &Array1<A>) -> Result<Array1<A>, DecompositionError> {
    if lambda.iter().any(|l| !(l.to_f64() > 0.0)) {
        return Err(DecompositionError::InvalidInput("a kept component has zero variance".into()));
    }
    Ok(lambda.mapv(|l| A::from_f64(1.0 / l.to_f64())))
}

/// n x 2 = [residual, weighted] (include/petal_hip_score.h)
pub(crate) fn score_rows<A: HipScalar, S: Data<Elem = A>>(
    input: &ArrayBase<S, Ix2>, components: &Array2<A>, means: &Array1<A>, centering: bool, weights: Option<&Array1<A>>,
) -> Result<Array2<A>, DecompositionError> {
    let (k, d) = components.dim();
    let mut out = Array2::<A>::default((input.nrows(), 2));
    let (x, ov) = (view(input), view(&out));
    with_ctx(
        |ctx| unsafe {
            ffi_score::petal_score_rows(ctx, &x, components.as_ptr() as *const c_void, means.as_ptr() as *const c_void,
                k as i64, d as i64, centering as i32, weights.map_or(std::ptr::null(), |w| w.as_ptr() as *const c_void), &ov,
                std::ptr::null())
        },
        || (),
    )?;
    let _ = &mut out; // written through ov
    Ok(out)
}

fn score_samples<A: HipScalar, S: Data<Elem = A>>(
    input: &ArrayBase<S, Ix2>, components: &Array2<A>, means: &Array1<A>, centering: bool, lambda: &Array1<A>, noise: A,
) -> Result<Array1<A>, DecompositionError> {
    let s2 = noise.to_f64();
    if !(s2 > 0.0) {
        return Err(DecompositionError::InvalidInput(
            "the noise variance is not positive (no discarded direction, or an exactly low-rank fit)".into(),
        ));
    }
    let w = inverse_variances(lambda)?;
    let (k, d) = components.dim();
    let c = d as f64 * (2.0 * std::f64::consts::PI).ln()
        + lambda.iter().map(|l| l.to_f64().ln()).sum::<f64>()
        + (d - k) as f64 * s2.ln();
    let sc = score_rows(input, components, means, centering, Some(&w))?;
    Ok(Array1::from_iter(sc.rows().into_iter().map(|r| A::from_f64(-0.5 * (c + r[0].to_f64() / s2 + r[1].to_f64())))))
}

/// One exact `Pca` per row segment of a row-sorted matrix, in one call (include/petal_hip_segments.h: an extension beyond the crate).
/// Segment `b` is rows `offsets[b] .. offsets[b + 1]` and gets what `Pca::fit` gives on those rows alone; for d <= 64 the batch is one
/// launch, a workgroup per segment (a very long segment is correct and not fast: fit it with `Pca`).
pub struct SegmentedPca<A: HipScalar> {
    n_components: usize,
    centering: bool,
    components: Array3<A>,
    means: Array2<A>,
    singular: Array2<A>,
    total_variance: Array1<A>,
    status: Vec<i32>,
    kernel_segments: i64,
}

impl<A: HipScalar> SegmentedPca<A> {
    pub fn new(n_components: usize) -> Self { Self::with_centering(n_components, true) }
    pub fn with_centering(n_components: usize, centering: bool) -> Self {
        SegmentedPca {
            n_components, centering, components: Array3::default((0, n_components, 0)), means: Array2::default((0, 0)),
            singular: Array2::default((0, n_components)), total_variance: Array1::default(0), status: Vec::new(), kernel_segments: 0,
        }
    }
    /// (B, k, d), svd_flip's sign applied
    pub fn components(&self) -> &Array3<A> { &self.components }
    pub fn mean(&self) -> &Array2<A> { &self.means }
    pub fn n_components(&self) -> usize { self.n_components }
    pub fn singular_values(&self) -> &Array2<A> { &self.singular }
    /// 0: fitted; 1: the segment held a NaN or an infinity and its results are NaN
    pub fn status(&self) -> &[i32] { &self.status }
    /// how many segments of the last fit the segment kernel fitted (0: the call looped over `Pca`'s code)
    pub fn kernel_segments(&self) -> i64 { self.kernel_segments }
    pub fn explained_variance_ratio(&self) -> Array2<A> {
        let mut r = self.singular.clone();
        for (b, mut row) in r.rows_mut().into_iter().enumerate() {
            let tv = self.total_variance[b].to_f64();
            row.mapv_inplace(|s| A::from_f64(s.to_f64() * s.to_f64() / tv));
        }
        r
    }

    pub fn fit<S: Data<Elem = A>>(&mut self, input: &ArrayBase<S, Ix2>, offsets: &[i64]) -> Result<(), DecompositionError> {
        self.inner_fit(input, offsets, None)
    }
    pub fn fit_transform<S: Data<Elem = A>>(&mut self, input: &ArrayBase<S, Ix2>, offsets: &[i64]) -> Result<Array2<A>, DecompositionError> {
        let mut y = Array2::<A>::default((input.nrows(), self.n_components));
        self.inner_fit(input, offsets, Some(&mut y))?;
        Ok(y)
    }
    pub fn transform<S: Data<Elem = A>>(&self, input: &ArrayBase<S, Ix2>, offsets: &[i64]) -> Result<Array2<A>, DecompositionError> {
        let (nseg, d) = self.means.dim();
        check_offsets_len(offsets, nseg)?;
        let mut y = Array2::<A>::default((input.nrows(), self.n_components));
        let (x, yv) = (view(input), view(&y));
        with_ctx(
            |ctx| unsafe {
                ffi_segments::petal_transform_segments(ctx, &x, offsets.as_ptr(), nseg as i64, self.components.as_ptr() as *const c_void,
                    self.means.as_ptr() as *const c_void, self.n_components as i64, d as i64, self.centering as i32, &yv)
            },
            || (),
        )?;
        let _ = &mut y; // written through yv
        Ok(y)
    }
    pub fn inverse_transform<S: Data<Elem = A>>(&self, input: &ArrayBase<S, Ix2>, offsets: &[i64]) -> Result<Array2<A>, DecompositionError> {
        let (nseg, d) = self.means.dim();
        check_offsets_len(offsets, nseg)?;
        let mut x_out = Array2::<A>::default((input.nrows(), d));
        let (yv, xv) = (view(input), view(&x_out));
        with_ctx(
            |ctx| unsafe {
                ffi_segments::petal_inverse_transform_segments(ctx, &yv, offsets.as_ptr(), nseg as i64,
                    self.components.as_ptr() as *const c_void, self.means.as_ptr() as *const c_void, self.n_components as i64, d as i64,
                    self.centering as i32, &xv)
            },
            || (),
        )?;
        let _ = &mut x_out;
        Ok(x_out)
    }

    fn inner_fit<S: Data<Elem = A>>(&mut self, input: &ArrayBase<S, Ix2>, offsets: &[i64], y: Option<&mut Array2<A>>) -> Result<(), DecompositionError> {
        if offsets.is_empty() {
            return Err(DecompositionError::InvalidInput("offsets needs n_segments + 1 values".into()));
        }
        let (nseg, k, d) = (offsets.len() - 1, self.n_components, input.ncols());
        let mut comps = Array3::<A>::default((nseg, k, d));
        let mut means = Array2::<A>::default((nseg, d));
        let mut sing = Array2::<A>::default((nseg, k));
        let mut tv = Array1::<A>::default(nseg);
        let mut status = vec![0i32; nseg];
        let mut ks = 0i64;
        let x = view(input);
        let yv = y.as_ref().map(|y| view(&**y));
        with_ctx(
            |ctx| unsafe {
                ffi_segments::petal_pca_fit_segments(ctx, &x, offsets.as_ptr(), nseg as i64, k as i64, self.centering as i32,
                    comps.as_mut_ptr() as *mut c_void, means.as_mut_ptr() as *mut c_void, sing.as_mut_ptr() as *mut c_void,
                    tv.as_mut_ptr() as *mut c_void, status.as_mut_ptr(), yv.as_ref().map_or(std::ptr::null(), |v| v as *const _), &mut ks)
            },
            || (),
        )?;
        self.components = comps;
        self.means = means;
        self.singular = sing;
        self.total_variance = tv;
        self.status = status;
        self.kernel_segments = ks;
        Ok(())
    }
}

fn check_offsets_len(offsets: &[i64], nseg: usize) -> Result<(), DecompositionError> {
    if offsets.len() != nseg + 1 {
        return Err(DecompositionError::InvalidInput(format!("the model holds {} segments, offsets describe {}", nseg, offsets.len() as i64 - 1)));
    }
    Ok(())
}

/// A sparse matrix in CSR form, resident on the device with the process's context (include/petal_hip_sparse.h: an extension beyond the
/// crate).  The arrays are checked and copied; the transposed image and the work items are built on the host and uploaded once.
/// Indices inside a row need not be sorted, duplicates act as their sum, explicit zeros and empty rows / columns are legal.
pub struct CsrMatrix<A: HipScalar> {
    raw: *mut ffi_sparse::PetalCsr,
    rows: usize,
    cols: usize,
    nnz: usize,
    _elem: std::marker::PhantomData<A>,
}
unsafe impl<A: HipScalar> Send for CsrMatrix<A> {}

impl<A: HipScalar> CsrMatrix<A> {
    pub fn new(rows: usize, cols: usize, indptr: &[i64], indices: &[i32], values: &[A]) -> Result<Self, DecompositionError> {
        if indptr.len() != rows + 1 {
            return Err(DecompositionError::InvalidInput(format!("indptr should have {} entries (it has {})", rows + 1, indptr.len())));
        }
        if indices.len() != values.len() {
            return Err(DecompositionError::InvalidInput("indices and values differ in length".into()));
        }
        let mut raw = std::ptr::null_mut();
        with_ctx(
            |ctx| unsafe {
                ffi_sparse::petal_csr_create(ctx, rows as i64, cols as i64, values.len() as i64, indptr.as_ptr(), indices.as_ptr(),
                    values.as_ptr() as *const c_void, A::DTYPE, &mut raw)
            },
            || (),
        )?;
        Ok(Self { raw, rows, cols, nnz: values.len(), _elem: std::marker::PhantomData })
    }
    pub fn nrows(&self) -> usize { self.rows }
    pub fn ncols(&self) -> usize { self.cols }
    pub fn nnz(&self) -> usize { self.nnz }
    pub(crate) fn raw(&self) -> *const ffi_sparse::PetalCsr { self.raw }
    /// false where the device-op layer has no sparse product: the fit and the transform then densify on the host
    pub fn resident(&self) -> bool {
        let mut v = [0i64; 8];
        unsafe { ffi_sparse::petal_csr_info(self.raw, v.as_mut_ptr()) };
        v[4] != 0
    }
}
impl<A: HipScalar> Drop for CsrMatrix<A> {
    fn drop(&mut self) { unsafe { ffi_sparse::petal_csr_destroy(self.raw) } }
}

/// The exact `Pca` fitted batch by batch (include/petal_hip_ipca.h: an extension beyond the crate).  `partial_fit` folds a batch into
/// the float64 statistic (rows seen, mean, M2) resident on the device; `model` is what `Pca::fit` returns on the concatenation of the
/// batches, up to the SIGN of each component: its entry of largest magnitude is positive (scikit-learn's rule), because a streaming
/// fit never holds U.  Gram route only: about eps64 (sigma_1 / sigma_j)^2 over the relative gap.
pub struct IncrementalPca<A: HipScalar> {
    raw: *mut ffi_ipca::PetalIpca,
    model: Pca<A>,
    dirty: bool,
}
unsafe impl<A: HipScalar> Send for IncrementalPca<A> {}

impl<A: HipScalar> IncrementalPca<A> {
    pub fn new(n_components: usize) -> Self { Self::with_centering(n_components, true) }
    pub fn with_centering(n_components: usize, centering: bool) -> Self {
        Self { raw: std::ptr::null_mut(), model: PcaBuilder::new(n_components).centering(centering).build(), dirty: false }
    }
    pub fn n_components(&self) -> usize { self.model.n_components() }
    /// { d, dtype, centering, rows seen, batches, batches the streaming kernel took, merges, 0 }
    pub fn info(&self) -> [i64; 8] {
        let mut v = [0i64; 8];
        if !self.raw.is_null() {
            unsafe { ffi_ipca::petal_ipca_info(self.raw, v.as_mut_ptr()) };
        }
        v
    }
    pub fn n_samples_seen(&self) -> usize { self.info()[3] as usize }

    fn open(&mut self, d: usize) -> Result<(), DecompositionError> {
        if !self.raw.is_null() {
            return Ok(());
        }
        let mut raw = std::ptr::null_mut();
        with_ctx(|ctx| unsafe { ffi_ipca::petal_ipca_create(ctx, d as i64, A::DTYPE, self.model.centering as i32, &mut raw) }, || ())?;
        self.raw = raw;
        Ok(())
    }
    /// Folds one batch into the statistic; the first batch fixes d.
    pub fn partial_fit<S: Data<Elem = A>>(&mut self, batch: &ArrayBase<S, Ix2>) -> Result<(), DecompositionError> {
        self.open(batch.ncols())?;
        let x = view(batch);
        let raw = self.raw;
        with_ctx(|ctx| unsafe { ffi_ipca::petal_ipca_partial_fit(ctx, raw, &x) }, || ())?;
        self.dirty = true;
        Ok(())
    }
    /// Adds the statistic of `other` (same d and centering), exactly: the pairwise form.  `other` is unchanged.
    pub fn merge(&mut self, other: &IncrementalPca<A>) -> Result<(), DecompositionError> {
        if other.raw.is_null() {
            return Ok(());
        }
        self.open(other.info()[0] as usize)?;
        let (raw, theirs) = (self.raw, other.raw);
        with_ctx(|ctx| unsafe { ffi_ipca::petal_ipca_merge(ctx, raw, theirs) }, || ())?;
        self.dirty = true;
        Ok(())
    }
    pub fn reset(&mut self) -> Result<(), DecompositionError> {
        let raw = self.raw;
        if !raw.is_null() {
            with_ctx(|_| unsafe { ffi_ipca::petal_ipca_reset(raw) }, || ())?;
        }
        self.model = PcaBuilder::new(self.model.n_components()).centering(self.model.centering).build();
        self.dirty = false;
        Ok(())
    }
    /// The statistic as host float64: (rows seen, mean, M2).
    pub fn state(&self) -> Result<(f64, Array1<f64>, Array2<f64>), DecompositionError> {
        if self.raw.is_null() {
            return Err(DecompositionError::InvalidInput("no batch has been seen yet".into()));
        }
        let d = self.info()[0] as usize;
        let (mut n, mut mean, mut m2) = (0f64, Array1::<f64>::default(d), Array2::<f64>::default((d, d)));
        let raw = self.raw;
        with_ctx(|ctx| unsafe { ffi_ipca::petal_ipca_get_state(ctx, raw, &mut n, mean.as_mut_ptr(), m2.as_mut_ptr()) }, || ())?;
        Ok((n, mean, m2))
    }
    pub fn set_state(&mut self, n: f64, mean: &Array1<f64>, m2: &Array2<f64>) -> Result<(), DecompositionError> {
        if m2.dim() != (mean.len(), mean.len()) || !m2.is_standard_layout() {
            return Err(DecompositionError::InvalidInput("m2 should be d x d in row-major order".into()));
        }
        self.open(mean.len())?;
        let raw = self.raw;
        with_ctx(|ctx| unsafe { ffi_ipca::petal_ipca_set_state(ctx, raw, n, mean.as_ptr(), m2.as_ptr()) }, || ())?;
        self.dirty = true;
        Ok(())
    }
    /// The model of the rows seen so far (solved once after each batch, on the first call): every accessor, `transform`,
    /// `inverse_transform` and row score of `Pca`.  Nothing seen yet: the empty model of an unfitted `Pca`.
    pub fn model(&mut self) -> Result<&Pca<A>, DecompositionError> {
        if self.dirty && !self.raw.is_null() && self.n_samples_seen() > 0 {
            let (k, d) = (self.model.n_components(), self.info()[0] as usize);
            let mut comps = Array2::<A>::default((k, d));
            let mut means = Array1::<A>::default(d);
            let mut sing = Array1::<A>::default(k);
            let mut tv = A::default();
            let raw = self.raw;
            with_ctx(
                |ctx| unsafe {
                    ffi_ipca::petal_ipca_finalize(ctx, raw, k as i64, comps.as_mut_ptr() as *mut c_void, means.as_mut_ptr() as *mut c_void,
                        sing.as_mut_ptr() as *mut c_void, &mut tv as *mut A as *mut c_void)
                },
                || (),
            )?;
            self.model.components = comps;
            self.model.means = means;
            self.model.singular = sing;
            self.model.total_variance = tv;
            self.model.n_samples = self.n_samples_seen();
            self.dirty = false;
        }
        Ok(&self.model)
    }
}
impl<A: HipScalar> Drop for IncrementalPca<A> {
    fn drop(&mut self) { unsafe { ffi_ipca::petal_ipca_destroy(self.raw) } }
}
