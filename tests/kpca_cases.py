"""KernelPca (include/petal_hip_kpca.h): the generators, the references, the case tables with their bounds, and the checks the GPU suite
(tests/test_gpu_kpca.py, expect_kernel=True) and the host suite (tests/test_kpca_host.py, expect_kernel=False) share.

A. petal_kernel_apply on exact integers, bit for bit against numpy int64, over the seams of the fused pass (16-row MFMA tiles, the
   32-row wave tile, the 128-row query block of a workgroup, the 32- and 64-column panels of A') and every input form.
B. petal_kernel_apply on real data against numpy.longdouble, expressed over the error of the MODEL -- the same statement in float64
   numpy, centring included -- with a floor:

       ratio = max |out - ref| / max(max |model - ref|, FLOOR_EPS eps64 max_i sum_j |K_ij A_jc|)

   MULTIPLIER is, per path, twice the largest ratio measured on the device and on the host simulation (profiles/kpca_errors.txt; the
   convention of tests/wide_cases.py), and the bound itself -- multiplier x max(model, floor) -- must stay below CAP = 1e-12 of that
   scale, so that it cannot hide a lost precision.
C. fit / fit_transform / transform against the numpy model: K in long double, the double centring, numpy.linalg.eigh in float64.

Run as a script on a machine with the GPU it writes profiles/kpca_errors.txt: the device's rows and the host simulation's."""
import functools
import os
import sys
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import petal_decomposition_amd as petal  # noqa: E402
from parity_cases import decided_signs, rowwise_rel  # noqa: E402
from wide_cases import as_form, np_dt  # noqa: E402

EPS64 = float(np.finfo(np.float64).eps)
FLOOR_EPS = 4.0
CAP = 1e-12
QUERY_BLOCK = 128        # query rows of a k_kapply workgroup (four waves of 32)
COLUMN_PANEL = 64        # the widest column panel of A' (the narrow one is 32)
FORMS = ("host", "device", "device-odd-pitch", "host-fortran")

Spec = namedtuple("Spec", "kernel gamma coef0 degree", defaults=(None, 1.0, 3))


def spec_kwargs(s):
    return {"kernel": s.kernel, "gamma": s.gamma, "coef0": s.coef0, "degree": s.degree}


def spec_name(s):
    return s.kernel + ("" if s.gamma is None else f"-g{s.gamma:.3g}") + (f"-c{s.coef0:g}-p{s.degree}" if s.kernel == "poly" else "")


# ------------------------------------------------------------------------------------------- A. exact integers
INT_M = (1, 15, 16, 17, 33, QUERY_BLOCK - 1, QUERY_BLOCK, QUERY_BLOCK + 1)
INT_N = (1, 15, 16, 17, 33, 257)
INT_D = (1, 3, 16, 19, 67, 1000)
INT_COLS = (1, 15, 16, 17, 33, COLUMN_PANEL + 1)
INT_SPECS = (Spec("linear"),) + tuple(Spec("poly", 1.0, float(c0), p) for c0 in (0, 1) for p in (2, 3))
# the full product of m and n at two widths and two d; the full lists of d and cols at two (m, n)
INT_SHAPES = tuple((m, n, d, cols) for m in INT_M for n in INT_N for (d, cols) in ((3, 1), (19, 17))) + \
    tuple((m, n, d, cols) for (m, n) in ((17, 33), (QUERY_BLOCK + 1, 257)) for d in INT_D for cols in INT_COLS)


@functools.lru_cache(maxsize=None)
def int_inputs(m, n, d, cols, dt):
    """(xq, xt, a, centre) with integers in [-3, 3], [-3, 3], [-4, 4] and [-3, 3]"""
    rng = np.random.default_rng(104729 * m + 7919 * n + 31 * d + cols)
    xq = rng.integers(-3, 4, size=(m, d)).astype(np_dt(dt))
    xt = rng.integers(-3, 4, size=(n, d)).astype(np_dt(dt))
    a = rng.integers(-4, 5, size=(n, cols)).astype(np.float64)
    c = rng.integers(-3, 4, size=d).astype(np.float64)
    for v in (xq, xt, a, c):
        v.setflags(write=False)
    return xq, xt, a, c


def int_reference(xq, xt, a, c, s):
    """the statement in int64; every intermediate is asserted below 2^53, so float64 holds it exactly"""
    ci = np.zeros(xt.shape[1], dtype=np.int64) if c is None else c.astype(np.int64)
    g = (xq.astype(np.int64) - ci) @ (xt.astype(np.int64) - ci).T
    k = g
    if s.kernel == "poly":
        b = int(s.gamma) * g + int(s.coef0)
        k = b.copy()
        for _ in range(s.degree - 1):
            assert np.abs(k).max(initial=0) * max(np.abs(b).max(initial=0), 1) < 2 ** 53
            k = k * b
    ai = a.astype(np.int64)
    assert (np.abs(k) @ np.abs(ai)).max(initial=0) < 2 ** 53
    return (k @ ai).astype(np.float64)


def check_integers_exact(ctx, shape, dt, form, expect_kernel):
    """kernel_apply equals numpy's int64 statement bit for bit for linear and the four poly kernels, with a centre (and, for linear,
    without); what lies outside the m x cols block of the device buffer stays untouched (petal_kernel_apply forms the result inside a
    guard and raises if it changed)"""
    m, n, d, cols = shape
    xq, xt, a, c = int_inputs(m, n, d, cols, dt)
    fq, ft = as_form(xq, form), as_form(xt, form)
    for s in INT_SPECS:
        for centre in ((c, None) if s.kernel == "linear" else (c,)):
            out, info = petal.kernel_apply(fq, ft, a, centre=centre, ctx=ctx, want_info=True, **spec_kwargs(s))
            want = int_reference(xq, xt, a, centre, s)
            assert out.tobytes() == want.tobytes(), (shape, dt, form, s, centre is not None, np.abs(out - want).max())
            assert info["kernel"] == (1 if expect_kernel else 0), info


def check_rbf_diagonal_is_one(ctx, n, d, dt, form, expect_kernel):
    """rbf with an integer centre and xq = xt: every diagonal entry of kernel_apply(.., A = I) is exactly 1.0 -- a squared distance of
    exactly zero: norms and cross terms are formed from the same values"""
    _, xt, _, c = int_inputs(n, n, d, 1, dt)
    f = as_form(xt, form)
    out, info = petal.kernel_apply(f, f, np.eye(n), kernel="rbf", gamma=0.37, centre=c, ctx=ctx, want_info=True)
    assert info["kernel"] == (1 if expect_kernel else 0), info
    assert np.all(np.diag(out) == 1.0), np.diag(out)
    assert np.array_equal(out, out.T) and np.all(out <= 1.0) and np.all(out >= 0.0)


# ------------------------------------------------------------------------------------------- the data of B and C
def planted(n, d, seed, offset=0.0):
    """x = z diag(3 0.75^i, i < 6) Q^T + 0.05 noise + 5 (a sign per column) [+ offset]: z n x 6 standard normal, Q d x 6 orthonormal"""
    rng = np.random.default_rng(seed)
    r = min(6, d)
    z = rng.standard_normal((n, r))
    q, _ = np.linalg.qr(rng.standard_normal((d, r)))
    x = (z * (3.0 * 0.75 ** np.arange(r))) @ q.T + 0.05 * rng.standard_normal((n, d)) + 5.0 * np.sign(rng.standard_normal(d))
    return x + offset


def specs_for(d):
    """the kernels of B and C with their parameters (gamma None = 1 / d)"""
    return (Spec("linear"), Spec("poly", 1.0 / d, 1.0, 3), Spec("rbf"), Spec("rbf", 0.02), Spec("sigmoid", 0.02 / d, 0.0), Spec("cosine"))


def resolved(s, d):
    return s._replace(gamma=1.0 / d if (s.gamma is None or s.gamma <= 0) else s.gamma)


def phi(s, g, na, nb):
    """phi on arrays of any float type: g = <x, y>, na / nb = |x|^2 (column) / |y|^2 (row)"""
    if s.kernel == "linear":
        return g
    if s.kernel == "poly":
        b = s.gamma * g + s.coef0
        k = b.copy()
        for _ in range(s.degree - 1):
            k = k * b
        return k
    if s.kernel == "rbf":
        return np.exp(-s.gamma * np.maximum(na + nb - 2 * g, 0))
    if s.kernel == "sigmoid":
        return np.tanh(s.gamma * g + s.coef0)
    den = np.sqrt(na) * np.sqrt(nb)
    return np.where(den > 0, g / np.where(den > 0, den, 1), 0)


def kernel_matrix(s, xq, xt, centre, ft):
    """phi((xq - c)(xt - c)^T) with every step in the float type ft (numpy.longdouble: the reference; numpy.float64: the model); s
    resolved"""
    c = np.zeros(xt.shape[1], dtype=ft) if centre is None else centre.astype(ft)
    q, t = xq.astype(ft) - c, xt.astype(ft) - c
    g = np.empty((q.shape[0], t.shape[0]), dtype=ft)
    for i in range(q.shape[0]):   # (row by row: a longdouble matmul holds m x n x d temporaries in some numpy builds)
        g[i] = (t * q[i]).sum(axis=1)
    return phi(s, g, (q * q).sum(axis=1)[:, None], (t * t).sum(axis=1)[None, :])


# ------------------------------------------------------------------------------------------- B. real data against long double
ApplyCase = namedtuple("ApplyCase", "name m n d dt spec")
APPLY_SHAPES = ((17, 33, 19), (50, 100, 67), (129, 257, 130))
APPLY_COLS = 5
APPLY_CASES = [ApplyCase(f"{dt}-{m}x{n}x{d}-{spec_name(s)}", m, n, d, dt, s)
               for (m, n, d) in APPLY_SHAPES for dt in ("f32", "f64") for s in specs_for(d)]
# twice the largest measured ratio per path (profiles/kpca_errors.txt: k_kapply 5.059, the host simulation's fallback 3.921; both at rbf,
# whose squared distance adds the rounding of two norms to the cross term's)
MULTIPLIER = {"device": 10.12, "hostsim": 7.85}


@functools.lru_cache(maxsize=None)
def apply_inputs(m, n, d, dt):
    """(xq, xt, a, mean): the planted generator with +40 added to every column; a: n x 5 standard normal; mean: the float64 column mean
    of xt -- the centre an rbf fit passes"""
    xt = planted(n, d, n + d, offset=40.0).astype(np_dt(dt))
    xq = planted(m, d, 1000 + m + d, offset=40.0).astype(np_dt(dt))
    a = np.random.default_rng(m + n + d).standard_normal((n, APPLY_COLS))
    mean = xt.astype(np.float64).mean(axis=0)
    for v in (xq, xt, a, mean):
        v.setflags(write=False)
    return xq, xt, a, mean


@functools.lru_cache(maxsize=None)
def apply_reference(c):
    """(ref, model error, scale): phi(..) A in long double, max |model - ref| of the float64 numpy statement, max_i sum_j |K_ij A_jc|"""
    xq, xt, a, mean = apply_inputs(c.m, c.n, c.d, c.dt)
    s = resolved(c.spec, c.d)
    centre = mean if s.kernel == "rbf" else None
    kl = kernel_matrix(s, xq, xt, centre, np.longdouble)
    ref = kl @ a.astype(np.longdouble)
    scale = float((np.abs(kl) @ np.abs(a).astype(np.longdouble)).max())
    model = kernel_matrix(s, xq, xt, centre, np.float64) @ a
    return ref, float(np.abs(model.astype(np.longdouble) - ref).max()), scale


def apply_call(ctx, c):
    xq, xt, a, mean = apply_inputs(c.m, c.n, c.d, c.dt)
    return petal.kernel_apply(xq, xt, a, centre=mean if c.spec.kernel == "rbf" else None, ctx=ctx, want_info=True, **spec_kwargs(c.spec))


def apply_ratio(c, out):
    ref, model, scale = apply_reference(c)
    err = float(np.abs(out.astype(np.longdouble) - ref).max())
    floor = FLOOR_EPS * EPS64 * scale
    return err / max(model, floor), err, model, floor, scale


def check_apply_against_long_double(ctx, c, expect_kernel):
    out, info = apply_call(ctx, c)
    assert info["kernel"] == (1 if expect_kernel else 0), info
    ratio, err, model, floor, scale = apply_ratio(c, out)
    bound = MULTIPLIER["device" if expect_kernel else "hostsim"] * max(model, floor)
    print(f"{c.name}: error {err / scale:.3e}, model {model / scale:.3e}, floor {floor / scale:.3e} of the scale; ratio {ratio:.3f}, "
          f"bound {bound / scale:.3e} (cap {CAP:.0e})")
    assert bound <= CAP * scale, (bound / scale, CAP)
    assert err <= bound, (c.name, ratio)
    return ratio


def check_same_bytes_twice(ctx, c):
    a, _ = apply_call(ctx, c)
    b, _ = apply_call(ctx, c)
    assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------- C. fits against the numpy model
FitCase = namedtuple("FitCase", "name n d dt spec")
FIT_SHAPES = ((33, 19), (100, 67), (257, 130))
FIT_K = 4
FIT_CASES = [FitCase(f"{dt}-{n}x{d}-{spec_name(s)}", n, d, dt, s) for (n, d) in FIT_SHAPES for dt in ("f32", "f64") for s in specs_for(d)]
NEW_ROWS = (1, 50, 129)


def tol_of(dt):
    """the project's parity bar"""
    return 1e-5 if dt == "f32" else 1e-9


def thr_of(dt):
    return 1e-6 if dt == "f32" else 1e-10


@functools.lru_cache(maxsize=None)
def fit_inputs(n, d, dt):
    x = planted(n, d, n + d).astype(np_dt(dt))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def new_rows(m, d, dt):
    x = planted(m, d, 5000 + m + d).astype(np_dt(dt))
    x.setflags(write=False)
    return x


Model = namedtuple("Model", "spec centre lam v rbar tbar")


def model_fit_of(x, spec):
    """K in long double, the double centring, numpy.linalg.eigh in float64; V with svd_flip's signs (the entry of largest magnitude of
    each column positive)"""
    n, d = x.shape
    s = resolved(spec, d)
    centre = x.astype(np.float64).mean(axis=0) if s.kernel == "rbf" else None
    k = kernel_matrix(s, x, x, centre, np.longdouble)
    rbar = k.mean(axis=0)
    tbar = rbar.mean()
    kc = (k - rbar[None, :] - rbar[:, None] + tbar).astype(np.float64)
    lam, v = np.linalg.eigh((kc + kc.T) / 2)
    lam, v = lam[::-1].copy(), v[:, ::-1].copy()
    idx = np.argmax(np.abs(v), axis=0)
    v *= np.where(v[idx, np.arange(n)] < 0, -1.0, 1.0)
    return Model(s, centre, lam, v, rbar.astype(np.float64), float(tbar))


@functools.lru_cache(maxsize=None)
def model_fit(c):
    return model_fit_of(fit_inputs(c.n, c.d, c.dt), c.spec)


def model_transform(mo, xt, xq, k):
    kq = kernel_matrix(mo.spec, xq, xt, mo.centre, np.longdouble).astype(np.float64)
    kqc = kq - mo.rbar[None, :] - kq.mean(axis=1)[:, None] + mo.tbar
    return kqc @ (mo.v[:, :k] / np.sqrt(mo.lam[:k]))


def scores_rel(y, ref, lam, n):
    """per column: max |y - ref| over max(max |ref|, sqrt(lambda_j / n)) -- the rms of the training scores of the column is the scale a
    score is held to (a single new row's score may lie near zero by chance)"""
    y, ref = np.asarray(y, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    scale = np.maximum(np.abs(ref).max(axis=0), np.sqrt(np.maximum(lam[:ref.shape[1]], 0) / n))
    return np.abs(y - ref).max(axis=0) / scale


def to_numpy(y):
    return y.cpu().numpy() if hasattr(y, "cpu") else np.asarray(y)


def check_model_is_well_posed(c):
    """what the parity bar rests on: the first five eigenvalues of the model are separated and none of the k wanted ones lies under the
    threshold"""
    mo = model_fit(c)
    gaps = np.abs(np.diff(mo.lam[:FIT_K + 1])) / mo.lam[0]
    assert gaps.min() > 1e-3, (c.name, gaps)
    assert np.sqrt(mo.lam[FIT_K - 1] / mo.lam[0]) > 10 * thr_of("f32"), (c.name, mo.lam[:FIT_K])


def check_fit_against_model(ctx, c, expect_kernel, form="host"):
    """eigenvalues relative to lambda_1, fit_transform's columns with their signs, transform(X_train) = fit_transform, info"""
    x = fit_inputs(c.n, c.d, c.dt)
    mo, tol, k = model_fit(c), tol_of(c.dt), FIT_K
    m = petal.KernelPca(k, ctx=ctx, **spec_kwargs(c.spec))
    y = to_numpy(m.fit_transform(as_form(x, form))).astype(np.float64)
    info = m.info()
    want = 1 if expect_kernel else 0
    assert (info["n"], info["d"], info["k"], info["order"], info["fit_kernel"], info["transform_kernel"]) == (c.n, c.d, k, c.n, want, -1), info
    assert info["topk_solver"] in (0, 1) and info["kernel"] == petal.KERNELS[c.spec.kernel]
    lam = m.eigenvalues()
    assert np.abs(lam - mo.lam[:k]).max() <= tol * mo.lam[0], (c.name, lam, mo.lam[:k])
    yo = mo.v[:, :k] * np.sqrt(mo.lam[:k])
    rel = rowwise_rel(y.T, yo.T)
    assert rel.max() <= tol, (c.name, rel)
    dec = decided_signs(mo.v, k, margin=min(0.5, max(1e-3, 100 * tol)))
    sgn = np.sign(np.sum(y * yo, axis=0))
    assert np.all(sgn[dec] == 1), (c.name, sgn, dec)
    y2 = to_numpy(m.transform(as_form(x, form))).astype(np.float64)
    assert m.info()["transform_kernel"] == want
    assert rowwise_rel(y2.T, y.T).max() <= tol, (c.name, rowwise_rel(y2.T, y.T))
    assert np.all(sgn == np.sign(np.sum(y2 * yo, axis=0)))
    vec = m.scaled_eigenvectors()
    assert np.abs(vec * lam - y).max() <= 10 * tol * np.abs(y).max()    # V lambda^(-1/2) lambda = V sqrt(lambda)
    return m


def check_transform_new_rows(ctx, c, expect_kernel):
    x = fit_inputs(c.n, c.d, c.dt)
    mo, tol, k = model_fit(c), tol_of(c.dt), FIT_K
    m = petal.KernelPca(k, ctx=ctx, **spec_kwargs(c.spec)).fit(x)
    for rows in NEW_ROWS:
        xq = new_rows(rows, c.d, c.dt)
        y = np.asarray(m.transform(xq), dtype=np.float64)
        assert y.shape == (rows, k) and m.info()["transform_kernel"] == (1 if expect_kernel else 0)
        yo = model_transform(mo, x, xq, k)
        s = np.sign(np.sum(np.asarray(m.transform(x), dtype=np.float64) * (mo.v[:, :k] * np.sqrt(mo.lam[:k])), axis=0))
        rel = scores_rel(y * s, yo, mo.lam, c.n)
        assert rel.max() <= tol, (c.name, rows, rel)


def check_linear_equals_pca(ctx, n, d, dt):
    """the linear kernel IS Pca: lambda = sigma^2, the scores equal up to the bar"""
    x, k, tol = fit_inputs(n, d, dt), FIT_K, tol_of(dt)
    p = petal.Pca(k, ctx=ctx)
    yp = np.asarray(p.fit_transform(x), dtype=np.float64)
    m = petal.KernelPca(k, "linear", ctx=ctx)
    y = np.asarray(m.fit_transform(x), dtype=np.float64)
    sig = np.asarray(p.singular_values(), dtype=np.float64)
    assert np.abs(m.eigenvalues() - sig * sig).max() <= tol * sig[0] ** 2
    assert rowwise_rel(y.T, yp.T).max() <= tol
    yt = np.asarray(m.transform(x), dtype=np.float64)
    assert rowwise_rel(yt.T, np.asarray(p.transform(x), dtype=np.float64).T).max() <= tol


def check_k_equals_n(ctx, dt="f64"):
    """k = n on a centred K: the n-th component is a zero column of both outputs, its eigenvalue as computed, nothing raised"""
    n, d = 17, 19
    x = fit_inputs(n, d, dt)
    m = petal.KernelPca(n, "rbf", ctx=ctx)
    y = np.asarray(m.fit_transform(x), dtype=np.float64)
    yt = np.asarray(m.transform(x), dtype=np.float64)
    lam = m.eigenvalues()
    assert np.isfinite(y).all() and np.isfinite(yt).all() and np.isfinite(lam).all()
    assert not y[:, n - 1].any() and not yt[:, n - 1].any()
    assert abs(lam[n - 1]) <= 1e-9 * lam[0]
    mo = model_fit_of(x, Spec("rbf"))
    live = np.sqrt(np.maximum(mo.lam[:n - 1], 0) / mo.lam[0]) > 100 * thr_of(dt)
    assert live.sum() >= 8
    assert np.abs(lam[:n - 1] - mo.lam[:n - 1]).max() <= tol_of(dt) * mo.lam[0]
    assert y[:, :n - 1][:, live].any(axis=0).all()


def check_fallback_against_kernel(ctx, c, expect_kernel):
    """PETAL_OPT_KPCA_FALLBACK against the default path within the bar, info() telling them apart"""
    x, k, tol = fit_inputs(c.n, c.d, c.dt), FIT_K, tol_of(c.dt)
    xq = new_rows(50, c.d, c.dt)
    m1 = petal.KernelPca(k, ctx=ctx, **spec_kwargs(c.spec))
    y1 = np.asarray(m1.fit_transform(x), dtype=np.float64)
    t1 = np.asarray(m1.transform(xq), dtype=np.float64)
    i1 = m1.info()
    ctx.set_option("kpca_fallback", 1)
    try:
        assert ctx.get_option("kpca_fallback") == 1.0
        m0 = petal.KernelPca(k, ctx=ctx, **spec_kwargs(c.spec))
        y0 = np.asarray(m0.fit_transform(x), dtype=np.float64)
        t0 = np.asarray(m0.transform(xq), dtype=np.float64)
        i0 = m0.info()
    finally:
        ctx.set_option("kpca_fallback", 0)
    want = 1 if expect_kernel else 0
    assert (i1["fit_kernel"], i1["transform_kernel"], i0["fit_kernel"], i0["transform_kernel"]) == (want, want, 0, 0), (i1, i0)
    lam = m1.eigenvalues()
    assert np.abs(lam - m0.eigenvalues()).max() <= tol * lam[0]
    assert rowwise_rel(y0.T, y1.T).max() <= tol
    assert scores_rel(t0, t1, lam, c.n).max() <= tol


def check_errors(ctx, make_sharded_ctx):
    """every error of the header; a second fit on the same ctx after an error works"""
    x = np.array(fit_inputs(33, 19, "f64"))
    with pytest_raises(petal.InvalidInput, "every dimension should be at least 34"):
        petal.KernelPca(34, ctx=ctx).fit(x)
    m = petal.KernelPca(25, "rbf", ctx=ctx).fit(x)                       # d = 19 < k = 25 is legal here
    assert m.eigenvalues().shape == (25,)
    with pytest_raises(petal.InvalidInput, "# of columns should be 19"):
        m.transform(x[:, :18])
    with pytest_raises(petal.InvalidInput, "dtype"):
        m.transform(x.astype(np.float32))
    with pytest_raises(petal.InvalidInput, "unknown kernel"):
        petal.KernelPca(2, "laplacian", ctx=ctx).fit(x)
    with pytest_raises(petal.InvalidInput, "degree"):
        petal.KernelPca(2, "poly", degree=0, ctx=ctx).fit(x)
    with pytest_raises(petal.InvalidInput, ""):
        petal.KernelPca(2, ctx=ctx).fit(np.zeros((0, 5)))
    with pytest_raises(petal.InvalidInput, "not been fitted"):
        petal.KernelPca(2, ctx=ctx).transform(x)
    for call in ("eigenvalues", "info", "scaled_eigenvectors"):        # an unfitted model without a ctx: the same error, no ctx made
        with pytest_raises(petal.InvalidInput, "not been fitted"):
            getattr(petal.KernelPca(2), call)()
    with pytest_raises(petal.InvalidInput, "too many rows"):
        petal.KernelPca(2, ctx=ctx).fit(np.zeros((32769, 1), dtype=np.float32))
    m.transform(x[:0])                                                  # no rows: the stats record is closed all the same
    assert ctx.stats()["fit_ms"] > 0
    spec = petal.petal_kernel_spec(7, 3, 0.0, 1.0)                        # an unknown kernel number straight through the ABI
    import ctypes as C
    h, mx = C.c_void_p(), petal.describe(x, [])
    assert ctx.lib.petal_kpca_fit(ctx._h, C.byref(mx), 2, C.byref(spec), C.byref(h), None) == petal.PETAL_INVALID_INPUT and not h
    for bad in (np.nan, np.inf):
        for kern in ("linear", "rbf", "sigmoid"):
            xb = x.copy()
            xb[7, 13] = bad
            with pytest_raises(petal.LinalgError, "did not converge"):
                petal.KernelPca(3, kern, ctx=ctx).fit(xb)
            assert np.isfinite(np.asarray(petal.KernelPca(3, kern, ctx=ctx).fit_transform(x))).all()   # the ctx is usable afterwards
    sh = make_sharded_ctx()
    try:
        with pytest_raises(petal.InvalidInput, "sharded"):
            petal.KernelPca(2, ctx=sh).fit(x)
        with pytest_raises(petal.InvalidInput, "sharded"):
            petal.kernel_apply(x, x, np.ones((33, 1)), ctx=sh)
    finally:
        sh.close()


class pytest_raises:
    """pytest.raises with a substring of the message (this module is also run as a script, without pytest)"""

    def __init__(self, exc, text):
        self.exc, self.text = exc, text

    def __enter__(self):
        return self

    def __exit__(self, et, ev, tb):
        assert et is not None and issubclass(et, self.exc), f"expected {self.exc.__name__}, got {et}"
        assert self.text in str(ev), str(ev)
        return True


# ------------------------------------------------------------------------------------------- the measured ratios
def measure(ctx, label, lines):
    worst = 0.0
    for c in APPLY_CASES:
        out, info = apply_call(ctx, c)
        ratio, err, model, floor, scale = apply_ratio(c, out)
        worst = max(worst, ratio)
        lines.append(f"{label:8s} {c.name:40s} kernel {info['kernel']}  error {err / scale:.3e}  model {model / scale:.3e}  "
                     f"floor {floor / scale:.3e}  ratio {ratio:.3f}")
    lines.append(f"{label:8s} largest ratio {worst:.3f}")
    return worst


if __name__ == "__main__":
    import hostsim
    out = ["# petal_kernel_apply against numpy.longdouble: errors over the scale max_i sum_j |K_ij A_jc|; ratio = error / max(model, "
           "floor).  tests/kpca_cases.py MULTIPLIER = twice each path's largest ratio."]
    if len(sys.argv) < 2 or sys.argv[1] != "--host-only":
        dev = petal.Context(0)
        measure(dev, "device", out)
        dev.close()
    host = hostsim.context()
    measure(host, "hostsim", out)
    host.close()
    out.append("tests/kpca_cases.py MULTIPLIER (twice each path's largest ratio): " + ", ".join(f"{k} {v}" for k, v in MULTIPLIER.items()))
    dst = os.path.join(ROOT, sys.argv[2] if len(sys.argv) > 2 else os.path.join("profiles", "kpca_errors.txt"))
    with open(dst, "w") as f:
        f.write("\n".join(out) + "\n")
    print("\n".join(out))
