"""Nmf (include/petal_hip_nmf.h): the numpy model of the statement, the generators, the case tables with their bounds, and the checks the
GPU suite (tests/test_gpu_nmf.py, expect_kernel=True) and the host suite (tests/test_nmf_host.py, expect_kernel=False) share.

The model is the header's statement in float64 numpy, in scikit-learn's order of operations (tests/test_nmf_host.py checks it against
``sklearn.decomposition.NMF(init="custom", solver="mu")`` where scikit-learn is installed).  It is the reference of every test here.

A. petal_nmf_pass on exact operands, bit for bit: H rows are disjoint 0/1 indicators with 2^s ones each (H H^T = 2^s I), W entries are
   powers of two or zero, X holds small integers -- every quotient of the W rule is exact, so W_new, A = W_new^T X and
   B = W_new^T W_new are exact in float64 whatever the order of the sums.
B. petal_nmf_pass on real data against numpy.longdouble, expressed over the error of the model with a floor:

       ratio = max over W_new, A, B of  max |out - ref| / max(max |model - ref|, FLOOR_EPS eps64 scale)

   scale = the largest sum of absolute terms of the quantity.  MULTIPLIER is, per path, twice the largest ratio measured on the device
   and on the host simulation, rounded up (profiles/nmf_errors.txt), and the bound -- multiplier x max(model, floor) -- must stay
   below CAP = 1e-12 of the scale, so that it cannot hide a lost precision.
C. fit / fit_transform / transform / inverse_transform against the model at the project's parity bar, relative to the largest entry:
   1e-5 for float32 data, 1e-9 for float64.

Run as a script on a machine with the GPU it writes profiles/nmf_errors.txt: the device's rows and the host simulation's."""
import functools
import os
import sys
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import petal_decomposition_amd as petal  # noqa: E402
from wide_cases import as_form, np_dt  # noqa: E402

EPS = 2.0 ** -23          # the statement's epsilon, for both data types
EPS64 = float(np.finfo(np.float64).eps)
FLOOR_EPS = 4.0
CAP = 1e-12
ROW_TILE = 16             # rows of a k_nmf_pass tile
MAX_WORKGROUPS = 256      # persistent workgroups of k_nmf_pass: tile t goes to workgroup t mod 256


# ------------------------------------------------------------------------------------------- the model
def penalties(n, d, alpha_w=0.0, alpha_h="same", l1_ratio=0.0):
    """scikit-learn's alpha_W, alpha_H, l1_ratio as (l1_w, l2_w, l1_h, l2_h)"""
    a_h = alpha_w if alpha_h == "same" else alpha_h
    return (d * alpha_w * l1_ratio, d * alpha_w * (1.0 - l1_ratio), n * a_h * l1_ratio, n * a_h * (1.0 - l1_ratio))


def model_w_rule(w, z, hht, l1, l2, ft=np.float64):
    den = w @ hht
    if l1 > 0:
        den += ft(l1)
    if l2 > 0:
        den = den + ft(l2) * w
    den[den == 0] = ft(EPS)
    return w * (z / den)


def model_h_rule(h, a, b, l1, l2, ft=np.float64):
    den = b @ h
    if l1 > 0:
        den += ft(l1)
    if l2 > 0:
        den = den + ft(l2) * h
    den[den == 0] = ft(EPS)
    return h * (a / den)


def model_pass(x, w, h, l1=0.0, l2=0.0, inner=1, ft=np.float64):
    """(W_new, A, B) of the header's pass in the float type ft"""
    x, w, h = x.astype(ft), w.astype(ft), h.astype(ft)
    z, hht = x @ h.T, h @ h.T
    for _ in range(inner):
        w = model_w_rule(w, z, hht, l1, l2, ft)
    return w, w.T @ x, w.T @ w


def model_loss(nx2, a, b, h):
    return float(np.sqrt(max(0.0, nx2 - 2.0 * float((a * h).sum()) + float((b * (h @ h.T)).sum()))))


Fit = namedtuple("Fit", "w h n_iter err err_init checks")


def model_fit(x, w0, h0, max_iter, tol=0.0, pen=(0.0, 0.0, 0.0, 0.0)):
    """the header's fit; checks = the deciding quantity (err_prev - err) / err_init at every check"""
    x, w, h = x.astype(np.float64), np.array(w0, dtype=np.float64), np.array(h0, dtype=np.float64)
    l1w, l2w, l1h, l2h = pen
    nx2 = float((x * x).sum())
    a, b = w.T @ x, w.T @ w
    err_init = model_loss(nx2, a, b, h)
    prev, checks, n_iter = err_init, [], max_iter
    for it in range(1, max_iter + 1):
        w = model_w_rule(w, x @ h.T, h @ h.T, l1w, l2w)
        a, b = w.T @ x, w.T @ w
        h = model_h_rule(h, a, b, l1h, l2h)
        if tol > 0 and it % 10 == 0:
            err = model_loss(nx2, a, b, h)
            checks.append((prev - err) / err_init)
            if checks[-1] < tol:
                n_iter = it
                break
            prev = err
    return Fit(w, h, n_iter, model_loss(nx2, a, b, h), err_init, checks)


def model_transform(xq, h, k, max_iter, pen=(0.0, 0.0, 0.0, 0.0)):
    xq = xq.astype(np.float64)
    w = np.full((xq.shape[0], k), np.sqrt(xq.mean() / k))
    z, hht = xq @ h.T, h @ h.T
    for _ in range(max_iter):
        w = model_w_rule(w, z, hht, pen[0], pen[1])
    return w


def to_numpy(y):
    return y.detach().cpu().numpy() if hasattr(y, "detach") else np.asarray(y)


def tol_of(dt):
    """the project's parity bar"""
    return 1e-5 if dt == "f32" else 1e-9


def rel_max(got, want):
    """max |got - want| over the largest entry of want"""
    got, want = np.asarray(to_numpy(got), dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())


# ------------------------------------------------------------------------------------------- A. exact operands
INT_N = (1, 15, 16, 17, 33, 2 * ROW_TILE + 5)                 # the last one: three workgroups, the third on a partial tile
INT_K = (1, 3, 16, 17, 64)
INT_D = (16, 24, 80, 256, 272, 512)
# more tiles than workgroups: workgroups 0 and 1 take a second tile, the last tile is partial
INT_N_PERSISTENT = ROW_TILE * (MAX_WORKGROUPS + 1) + 3
INT_SHAPES = tuple((n, k, d) for n in INT_N for k in INT_K for d in INT_D if k <= d)
INT_SHAPES_PERSISTENT = tuple((INT_N_PERSISTENT, k, d) for (k, d) in ((3, 24), (17, 272), (64, 512)))


@functools.lru_cache(maxsize=None)
def int_inputs(n, k, d, dt):
    """(x, w, h, s): x integers in [0, 7]; w in {0, 1/4, 1/2, 1, 2, 4}; row c of h is the indicator of 2^s columns taken from a
    random permutation, so the rows are disjoint and h h^T = 2^s I"""
    rng = np.random.default_rng(104729 * n + 7919 * k + d)
    s = min(3, int(np.floor(np.log2(d // k))))
    x = rng.integers(0, 8, size=(n, d)).astype(np_dt(dt))
    w = rng.choice(np.array([0.0, 0.25, 0.5, 1.0, 2.0, 4.0]), size=(n, k))
    perm = rng.permutation(d)
    h = np.zeros((k, d))
    for c in range(k):
        h[c, perm[c * 2 ** s:(c + 1) * 2 ** s]] = 1.0
    assert k * 2 ** s <= d and np.array_equal(h @ h.T, 2.0 ** s * np.eye(k))
    for v in (x, w, h):
        v.setflags(write=False)
    return x, w, h, s


def check_integers_exact(ctx, shape, dt, inner, expect_kernel, form="host"):
    """W_new, A and B equal the model's bit for bit without a penalty and with l2_w = 2^s (D = 2^(s+1) W: still a power of two times W);
    petal_nmf_pass forms W inside a guard and raises if anything outside the n x k block changed"""
    n, k, d = shape
    x, w, h, s = int_inputs(n, k, d, dt)
    fx = as_form(x, form)
    for l2 in (0.0, 2.0 ** s):
        (wn, a, b), info = petal.nmf_pass(fx, w, h, l2_w=l2, inner_iters=inner, ctx=ctx, want_info=True)
        mw, ma, mb = model_pass(x, w, h, 0.0, l2, inner)
        assert info["kernel"] == (1 if expect_kernel else 0), (shape, info)
        for got, want, name in ((wn, mw, "W"), (a, ma, "A"), (b, mb, "B")):
            assert got.tobytes() == want.tobytes(), (shape, dt, inner, l2, form, name, np.abs(got - want).max())
    if inner == 1:   # without A and B, and the pass that leaves W alone
        wn = petal.nmf_pass(fx, w, h, inner_iters=1, want_ab=False, ctx=ctx)
        assert wn.tobytes() == model_pass(x, w, h)[0].tobytes(), shape
        wn, a, b = petal.nmf_pass(fx, w, h, inner_iters=0, ctx=ctx)
        assert wn.tobytes() == w.tobytes() and a.tobytes() == (w.T @ x.astype(np.float64)).tobytes() and b.tobytes() == (w.T @ w).tobytes(), shape


# ------------------------------------------------------------------------------------------- B. real data against long double
PassCase = namedtuple("PassCase", "name n d k dt inner l1 l2")
PASS_CASES = [PassCase(f"{dt}-83x200-k17-inner{inner}" + ("-reg" if l1 else ""), 83, 200, 17, dt, inner, l1, l2)
              for dt in ("f32", "f64") for (inner, l1, l2) in ((1, 0.0, 0.0), (3, 0.25, 0.5))]
# twice the largest measured ratio, rounded up (profiles/nmf_errors.txt: 0.789 on the device, 1.142 on the host simulation)
MULTIPLIER = {"device": 2.0, "hostsim": 3.0}


def planted(n, d, r, seed, noise=0.01):
    """a non-negative rank-r product plus `noise` of its mean in |N(0,1)| noise"""
    rng = np.random.default_rng(seed)
    x = rng.random((n, r)) @ (rng.random((r, d)) * rng.random((r, 1)) * 3.0)
    return x + noise * x.mean() * np.abs(rng.standard_normal((n, d)))


@functools.lru_cache(maxsize=None)
def pass_inputs(n, d, k, dt):
    rng = np.random.default_rng(31 * n + 7 * d + k)
    x = planted(n, d, k + 2, n + d + k).astype(np_dt(dt))
    w, h = rng.random((n, k)) + 0.05, rng.random((k, d)) + 0.05
    for v in (x, w, h):
        v.setflags(write=False)
    return x, w, h


@functools.lru_cache(maxsize=None)
def pass_reference(c):
    """per quantity (W_new, A, B): (ref in long double, max |model - ref|, scale)"""
    x, w, h = pass_inputs(c.n, c.d, c.k, c.dt)
    ld = np.longdouble
    ref = model_pass(x, w, h, c.l1, c.l2, c.inner, ld)
    mod = model_pass(x, w, h, c.l1, c.l2, c.inner, np.float64)
    wl, xl = np.abs(ref[0]), np.abs(x.astype(ld))
    scales = (float(wl.max()), float((wl.T @ xl).max()), float((wl.T @ wl).max()))
    return tuple((r, float(np.abs(m.astype(ld) - r).max()), sc) for r, m, sc in zip(ref, mod, scales))


def pass_call(ctx, c):
    x, w, h = pass_inputs(c.n, c.d, c.k, c.dt)
    return petal.nmf_pass(x, w, h, l1_w=c.l1, l2_w=c.l2, inner_iters=c.inner, ctx=ctx, want_info=True)


def pass_ratio(c, outs):
    """(largest ratio, rows of (name, error / scale, model / scale, floor / scale, ratio))"""
    rows, worst = [], 0.0
    for name, out, (ref, model, scale) in zip("WAB", outs, pass_reference(c)):
        err = float(np.abs(out.astype(np.longdouble) - ref).max())
        floor = FLOOR_EPS * EPS64 * scale
        ratio = err / max(model, floor)
        worst = max(worst, ratio)
        rows.append((name, err / scale, model / scale, floor / scale, ratio))
    return worst, rows


def check_pass_against_long_double(ctx, c, expect_kernel):
    outs, info = pass_call(ctx, c)
    assert info["kernel"] == (1 if expect_kernel else 0), info
    mult = MULTIPLIER["device" if expect_kernel else "hostsim"]
    worst, rows = pass_ratio(c, outs)
    for name, err, model, floor, ratio in rows:
        bound = mult * max(model, floor)
        print(f"{c.name} {name}: error {err:.3e}, model {model:.3e}, floor {floor:.3e} of the scale; ratio {ratio:.3f}, bound {bound:.3e} "
              f"(cap {CAP:.0e})")
        assert bound <= CAP, (c.name, name, bound)
        assert err <= bound, (c.name, name, ratio)
    return worst


# ------------------------------------------------------------------------------------------- C. fits against the model
FitCase = namedtuple("FitCase", "name n d k dt max_iter alpha_w alpha_h l1_ratio")
FIT_SHAPES = ((200, 48, 5), (300, 64, 8))
FIT_CASES = [FitCase(f"{dt}-{n}x{d}-k{k}-it{it}", n, d, k, dt, it, 0.0, "same", 0.0)
             for (n, d, k) in FIT_SHAPES for dt in ("f32", "f64") for it in (1, 3, 10)] + \
            [FitCase(f"{dt}-{n}x{d}-k{k}-it10-reg", n, d, k, dt, 10, 0.01, 0.02, 0.3) for (n, d, k) in FIT_SHAPES[:1] for dt in ("f32", "f64")]
QUERY_ROWS = 37


@functools.lru_cache(maxsize=None)
def fit_inputs(n, d, k, dt):
    """(x, w0, h0, xq), all in the data's type: the planted generator of rank k + 2 with 1 % noise; xq: QUERY_ROWS fresh rows"""
    rng = np.random.default_rng(1000 * n + d + k)
    full = planted(n + QUERY_ROWS, d, k + 2, 7 * n + d)
    x, xq = full[:n].astype(np_dt(dt)), full[n:].astype(np_dt(dt))
    avg = np.sqrt(x.mean() / k)
    w0 = (avg * np.abs(rng.standard_normal((n, k)))).astype(np_dt(dt))
    h0 = (avg * np.abs(rng.standard_normal((k, d)))).astype(np_dt(dt))
    for v in (x, xq, w0, h0):
        v.setflags(write=False)
    return x, w0, h0, xq


def case_penalties(c):
    return penalties(c.n, c.d, c.alpha_w, c.alpha_h, c.l1_ratio)


@functools.lru_cache(maxsize=None)
def fit_model(c, tol=0.0):
    x, w0, h0, _ = fit_inputs(c.n, c.d, c.k, c.dt)
    return model_fit(x, w0, h0, c.max_iter, tol, case_penalties(c))


def make(ctx, c, tol=0.0, **kw):
    return petal.Nmf(c.k, max_iter=c.max_iter, tol=tol, init="custom", alpha_W=c.alpha_w, alpha_H=c.alpha_h, l1_ratio=c.l1_ratio, ctx=ctx, **kw)


def check_fit_against_model(ctx, c, expect_kernel, form="host"):
    """W, H and reconstruction_err at the bar; n_iter; info(); fit_transform's W is the fit's W"""
    x, w0, h0, _ = fit_inputs(c.n, c.d, c.k, c.dt)
    mo = fit_model(c)
    m = make(ctx, c)
    w = m.fit_transform(as_form(x, form), W=as_form(w0, form), H=as_form(h0, form))
    info = m.info()
    assert (info["n"], info["d"], info["k"], info["n_iter"]) == (c.n, c.d, c.k, c.max_iter) and m.n_iter == mo.n_iter
    assert info["fit_kernel"] == (1 if expect_kernel else 0) and info["transform_kernel"] == -1, info
    tol = tol_of(c.dt)
    got = (rel_max(w, mo.w), rel_max(m.components, mo.h), abs(m.reconstruction_err - mo.err) / mo.err, abs(m.err_init - mo.err_init) / mo.err_init)
    print(f"{c.name} {form}: W {got[0]:.2e}, H {got[1]:.2e}, err {got[2]:.2e}, err_init {got[3]:.2e} (bar {tol:.0e})")
    assert to_numpy(w).dtype == np_dt(c.dt) and max(got) <= tol, (c.name, got)
    return m


def check_transform(ctx, c, expect_kernel, form="host"):
    """transform of fresh rows, inverse_transform = W H, at the bar"""
    x, w0, h0, xq = fit_inputs(c.n, c.d, c.k, c.dt)
    mo = fit_model(c)
    m = make(ctx, c).fit(x, W=w0, H=h0)
    wq = m.transform(as_form(xq, form))
    info = m.info()
    assert info["transform_kernel"] == (1 if expect_kernel else 0), info
    want = model_transform(xq, mo.h, c.k, c.max_iter, case_penalties(c))
    tol = tol_of(c.dt)
    back = m.inverse_transform(wq)
    wq64 = to_numpy(wq).astype(np.float64)
    got = (rel_max(wq, want), rel_max(back, wq64 @ m.components))
    print(f"{c.name} {form}: transform {got[0]:.2e}, inverse_transform {got[1]:.2e} (bar {tol:.0e})")
    assert to_numpy(wq).shape == (QUERY_ROWS, c.k) and to_numpy(back).shape == (QUERY_ROWS, c.d) and max(got) <= tol, (c.name, got)


# ------------------------------------------------------------------------------------------- the stopping rule
# One case per dtype whose model stops at a check between iteration 20 and 60, with the deciding quantity a factor of 2 or more away
# from tol at the stopping check and at the check before it (check_stop_case_is_decided verifies that on the model).
StopCase = namedtuple("StopCase", "name n d k dt seed tol")
STOP_CASES = [StopCase("f32-100x24-k2-seed58", 100, 24, 2, "f32", 58, 5.5e-3), StopCase("f64-100x24-k2-seed33", 100, 24, 2, "f64", 33, 4.6e-3)]
STOP_MAX_ITER = 200


@functools.lru_cache(maxsize=None)
def stop_inputs(c):
    rng = np.random.default_rng(c.seed)
    x = planted(c.n, c.d, c.k + 2, c.seed + 100).astype(np_dt(c.dt))
    avg = np.sqrt(x.mean() / c.k)
    w0 = (avg * np.abs(rng.standard_normal((c.n, c.k)))).astype(np_dt(c.dt))
    h0 = (avg * np.abs(rng.standard_normal((c.k, c.d)))).astype(np_dt(c.dt))
    for v in (x, w0, h0):
        v.setflags(write=False)
    return x, w0, h0


@functools.lru_cache(maxsize=None)
def check_stop_case_is_decided(c):
    mo = model_fit(*stop_inputs(c), STOP_MAX_ITER, c.tol)
    assert 20 <= mo.n_iter <= 60 and len(mo.checks) == mo.n_iter // 10, (mo.n_iter, mo.checks)
    assert mo.checks[-1] <= c.tol / 2 and mo.checks[-2] >= 2 * c.tol and min(mo.checks[:-1]) >= 2 * c.tol, (c.tol, mo.checks)
    return mo


def check_stopping_rule(ctx, c, expect_kernel):
    mo = check_stop_case_is_decided(c)
    x, w0, h0 = stop_inputs(c)
    m = petal.Nmf(c.k, max_iter=STOP_MAX_ITER, tol=c.tol, init="custom", ctx=ctx).fit(x, W=w0, H=h0)
    print(f"{c.name}: n_iter {m.n_iter} (model {mo.n_iter}), checks {['%.2e' % v for v in mo.checks]}, tol {c.tol:g}")
    assert m.n_iter == mo.n_iter and m.info()["fit_kernel"] == (1 if expect_kernel else 0)
    assert abs(m.reconstruction_err - mo.err) <= tol_of(c.dt) * mo.err and rel_max(m.components, mo.h) <= tol_of(c.dt)


# ------------------------------------------------------------------------------------------- random initialisation
def random_init(x, k, seed):
    """W0 (n x k) drawn first, then H0 (k x d), |avg N(0,1)| in row-major order from petal.Pcg(seed)"""
    n, d = x.shape
    rng = petal.Pcg(seed)
    avg = np.sqrt(x.astype(np.float64).mean() / k)
    return np.abs(avg * rng.standard_normal((n, k))), np.abs(avg * rng.standard_normal((k, d)))


def check_random_init(ctx, dt, expect_kernel):
    n, d, k = 60, 24, 4
    x = fit_inputs(n, d, k, dt)[0]
    w0, h0 = random_init(x, k, 12345)
    mo = model_fit(x, w0, h0, 1)
    fits = []
    for seed in (12345, 12345, 54321):
        m = petal.Nmf(k, max_iter=1, tol=0.0, init="random", seed=seed, ctx=ctx)
        w = to_numpy(m.fit_transform(x))
        fits.append((w.tobytes(), m.components.tobytes()))
        assert m.info()["fit_kernel"] == (1 if expect_kernel else 0)
        if seed == 12345:
            assert max(rel_max(w, mo.w), rel_max(m.components, mo.h), abs(m.err_init - mo.err_init) / mo.err_init) <= tol_of(dt)
    assert fits[0] == fits[1] and fits[0] != fits[2]


def check_same_bytes_twice(ctx, c):
    x, w0, h0, xq = fit_inputs(c.n, c.d, c.k, c.dt)
    runs = []
    for _ in range(2):
        m = make(ctx, c)
        w = to_numpy(m.fit_transform(x, W=w0, H=h0))
        runs.append((w.tobytes(), m.components.tobytes(), m.reconstruction_err, to_numpy(m.transform(xq)).tobytes()))
    assert runs[0] == runs[1]


# ------------------------------------------------------------------------------------------- paths
def check_fallback_against_kernel(ctx, c, expect_kernel):
    """nmf_fallback = 1: the composed path, within the bar of the default path, info() reports 0"""
    x, w0, h0, xq = fit_inputs(c.n, c.d, c.k, c.dt)
    m = make(ctx, c)
    w = to_numpy(m.fit_transform(x, W=w0, H=h0))
    wq = to_numpy(m.transform(xq))
    assert m.info()["fit_kernel"] == m.info()["transform_kernel"] == (1 if expect_kernel else 0)
    ctx.set_option("nmf_fallback", 1)
    try:
        f = make(ctx, c)
        wf = to_numpy(f.fit_transform(x, W=w0, H=h0))
        wqf = to_numpy(f.transform(xq))
        assert f.info()["fit_kernel"] == 0 and f.info()["transform_kernel"] == 0
    finally:
        ctx.set_option("nmf_fallback", 0)
    tol = tol_of(c.dt)
    assert max(rel_max(wf, w), rel_max(f.components, m.components), rel_max(wqf, wq)) <= tol
    assert abs(f.reconstruction_err - m.reconstruction_err) <= tol * m.reconstruction_err


OUTSIDE_SHAPES = ((70, 80, 65), (40, 520, 6))    # k = 65 > 64; 528 padded columns > 512


def check_outside_envelope(ctx, shape, dt):
    """a shape the kernel does not take fits through the composed path, correctly"""
    n, d, k = shape
    c = FitCase(f"{dt}-{n}x{d}-k{k}", n, d, k, dt, 3, 0.0, "same", 0.0)
    x, w0, h0, xq = fit_inputs(n, d, k, dt)
    mo = fit_model(c)
    m = make(ctx, c)
    w = m.fit_transform(x, W=w0, H=h0)
    wq = m.transform(xq)
    assert m.info()["fit_kernel"] == 0 and m.info()["transform_kernel"] == 0
    tol = tol_of(dt)
    assert max(rel_max(w, mo.w), rel_max(m.components, mo.h), rel_max(wq, model_transform(xq, mo.h, k, 3))) <= tol
    assert abs(m.reconstruction_err - mo.err) <= tol * mo.err


# ------------------------------------------------------------------------------------------- errors
class raises_with:
    def __init__(self, exc, text):
        self.exc, self.text = exc, text

    def __enter__(self):
        return self

    def __exit__(self, et, ev, tb):
        assert et is not None and issubclass(et, self.exc), f"expected {self.exc.__name__}, got {et}"
        assert self.text in str(ev), str(ev)
        return True


def check_errors(ctx, make_sharded_ctx):
    n, d, k = 30, 12, 3
    x, w0, h0, xq = (np.array(v) for v in fit_inputs(n, d, k, "f64"))
    inv, lin = petal.InvalidInput, petal.LinalgError

    def fit(xx=x, kk=k, w=w0, h=h0, **kw):
        args = dict(max_iter=2, tol=0.0, init="custom", ctx=ctx)
        args.update(kw)
        return petal.Nmf(kk, **args).fit(xx, W=w, H=h)
    with raises_with(inv, "at least 1"):
        fit(kk=0, w=w0[:, :0], h=h0[:0])
    with raises_with(inv, "every dimension should be at least 13"):
        fit(kk=13, w=np.ones((n, 13)), h=np.ones((13, d)))
    with raises_with(inv, "every dimension should be at least 3"):
        fit(xx=x[:2], w=w0[:2])
    with raises_with(inv, "no rows or no columns"):
        fit(xx=x[:0], w=w0[:0])
    with raises_with(inv, "no rows or no columns"):
        fit(xx=x[:, :0], h=h0[:, :0])
    for kw in ({"alpha_W": -0.1}, {"alpha_W": 0.1, "l1_ratio": -0.5}, {"alpha_H": -1.0}, {"tol": -1.0}):
        with raises_with(inv, "not negative"):
            fit(**kw)
    with raises_with(inv, "max_iter should be at least 1"):
        fit(max_iter=0)
    for which in range(3):
        bad = [x.copy(), w0.copy(), h0.copy()]
        bad[which][1, 2] = -1e-3
        with raises_with(inv, "negative values in data"):
            fit(xx=bad[0], w=bad[1], h=bad[2])
        for v in (np.nan, np.inf):
            bad[which][1, 2] = v
            with raises_with(lin, "did not converge"):
                fit(xx=bad[0], w=bad[1], h=bad[2])
    with raises_with(inv, "# of columns should be 12"):
        fit(h=np.ones((k, d + 1)))
    with raises_with(inv, "w0 should be n x k"):
        fit(w=np.ones((n + 1, k)))
    with raises_with(inv, "needs W and H"):
        petal.Nmf(k, init="custom", ctx=ctx).fit(x)
    with raises_with(inv, "custom"):
        petal.Nmf(k, init="random", ctx=ctx).fit(x, W=w0, H=h0)
    with raises_with(inv, "unknown init"):
        petal.Nmf(k, init="nndsvd", ctx=ctx)
    with raises_with(inv, "not been fitted"):
        petal.Nmf(k, ctx=ctx).transform(x)
    m = fit()
    with raises_with(inv, "# of columns should be 12"):
        m.transform(x[:, :11])
    with raises_with(inv, "# of columns should be 3"):
        m.inverse_transform(np.ones((4, 4)))
    with raises_with(inv, "dtype"):
        m.transform(xq.astype(np.float32))
    bad = xq.copy()
    bad[0, 0] = -1.0
    with raises_with(inv, "negative values in data"):
        m.transform(bad)
    bad[0, 0] = np.nan
    with raises_with(lin, "did not converge"):
        m.transform(bad)
    assert to_numpy(m.transform(x[:0])).shape == (0, k)
    with raises_with(inv, "negative values in data"):
        petal.nmf_pass(-x, w0, h0, ctx=ctx)
    with raises_with(inv, "w should be"):
        petal.nmf_pass(x, w0[:5], h0, ctx=ctx)
    other = make_sharded_ctx()
    try:
        with raises_with(inv, "sharded"):
            fit(ctx=other)
        with raises_with(inv, "sharded"):
            petal.nmf_pass(x, w0, h0, ctx=other)
    finally:
        other.close()


# ------------------------------------------------------------------------------------------- the measured ratios
def measure(ctx, label, lines):
    worst = 0.0
    for c in PASS_CASES:
        outs, info = pass_call(ctx, c)
        w, rows = pass_ratio(c, outs)
        worst = max(worst, w)
        for name, err, model, floor, ratio in rows:
            lines.append(f"{label:8s} {c.name:28s} {name}  kernel {info['kernel']}  error {err:.3e}  model {model:.3e}  floor {floor:.3e}  "
                         f"ratio {ratio:.3f}")
    lines.append(f"{label:8s} largest ratio {worst:.3f}")
    return worst


if __name__ == "__main__":
    import hostsim
    out = ["# petal_nmf_pass against numpy.longdouble: W_new, A = W_new^T X, B = W_new^T W_new; errors over the scale (the largest sum of "
           "absolute terms); ratio = error / max(model, floor).  tests/nmf_cases.py MULTIPLIER = twice each path's largest ratio, rounded up."]
    if len(sys.argv) < 2 or sys.argv[1] != "--host-only":
        dev = petal.Context(0)
        measure(dev, "device", out)
        dev.close()
    host = hostsim.context()
    measure(host, "hostsim", out)
    host.close()
    out.append("tests/nmf_cases.py MULTIPLIER: " + ", ".join(f"{k} {v}" for k, v in MULTIPLIER.items()))
    dst = os.path.join(ROOT, sys.argv[2] if len(sys.argv) > 2 else os.path.join("profiles", "nmf_errors.txt"))
    with open(dst, "w") as f:
        f.write("\n".join(out) + "\n")
    print("\n".join(out))
