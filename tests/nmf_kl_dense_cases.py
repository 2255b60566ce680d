"""Nmf with the Kullback-Leibler loss on dense data (include/petal_hip_nmf_kl_dense.h): the numpy model of the dense pass, the
generators, the case tables with their bounds, and the checks the GPU suite (tests/test_gpu_nmf_kl_dense.py, expect_kernel=True:
k_nmf_kl_pass) and the host suite (tests/test_nmf_kl_dense_host.py, expect_kernel=False: the composed path) share.

1. petal_nmf_kl_pass on exact operands, bit for bit: W and H hold the integers 1 .. 3, X = C o (W H) with integer C in {0, 1, 2, 3}, so
   every quotient is exactly C and Q H^T, rowsum(H), W^T Q and colsum(W) are sums of small integers: exact in float64 whatever their
   order.  With integer penalties numpy's w * (num / den) rounds the same operands in the same two steps as the library.
2. petal_nmf_kl_pass on real data against numpy.longdouble, in nmf_cases' form: error / max(error of the float64 numpy model, floor),
   bounded by nmf_cases.MULTIPLIER (2 on the device, 3 on the host simulation) with the bound itself capped at 1e-12 of the scale.
3 .. 7. fit, fit_transform and transform against nmf_kl_cases' model (the statement on the CSR of the non-zero entries: the same
   statement, another order of the sums) and against the library's own CSR route, at the project's parity bar (nmf_cases.tol_of).

Run as a script on a machine with the GPU it writes profiles/nmf_kl_dense_errors.txt: the device's rows and the host simulation's."""
import ctypes as C
import functools
import os
import sys
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import petal_decomposition_amd as petal  # noqa: E402
import nmf_cases as nc  # noqa: E402
import nmf_kl_cases as kc  # noqa: E402
from nmf_cases import FitCase, raises_with, rel_max, tol_of, to_numpy  # noqa: E402
from nmf_sparse_cases import csr  # noqa: E402
from sparse_cases import to_csr  # noqa: E402
from wide_cases import np_dt  # noqa: E402

EPS = nc.EPS
EPS64 = nc.EPS64
FLOOR_EPS = nc.FLOOR_EPS
CAP = nc.CAP
MULTIPLIER = nc.MULTIPLIER      # the existing multipliers hold (profiles/nmf_kl_dense_errors.txt: the measured ratios)
KL = kc.KL
FUSED = "fused"


def in_envelope(k, d):
    """k_nmf_kl_pass's envelope (k_nmf_pass's): 16, 32 or 64 padded components, at most 512 padded columns"""
    kp = 16 if k <= 16 else (32 if k <= 32 else (k + 15) // 16 * 16)
    return kp in (16, 32, 64) and (d + 15) // 16 * 16 <= 512


def kernel_flag(expect_kernel, k, d):
    return 1 if expect_kernel and in_envelope(k, d) else 0


# ------------------------------------------------------------------------------------------- the model of the pass
def model_pass(x, w, h, l1=0.0, l2=0.0, inner=1, ft=np.float64):
    """(W_new, A, colsum(W_new), term) of the header's pass in the float type ft; term is None unless inner == 0"""
    x, w, h = x.astype(ft), w.astype(ft), h.astype(ft)
    eps, rs = ft(EPS), h.sum(axis=1)
    for _ in range(inner):
        wh = w @ h
        wh[wh < eps] = eps
        den = (rs + ft(l1)) + ft(l2) * w
        den[den == 0] = eps
        w = w * (((x / wh) @ h.T) / den)
    wh = w @ h
    wh[wh < eps] = eps
    term = None
    if inner == 0:
        m = x > eps
        term = (x[m] * np.log(x[m] / wh[m])).sum()
    return w, w.T @ (x / wh), w.sum(axis=0), term


def pitched(x, expect_kernel, extra=16):
    """the same values as a view whose row pitch is d + extra elements, NaN behind every row: a device tensor where the kernel runs
    (d a multiple of 16 and extra of 4: taken zero-copy with that pitch), else a host view"""
    n, d = x.shape
    if expect_kernel:
        import torch
        buf = torch.full((n, d + extra), float("nan"), dtype=torch.float32 if x.dtype == np.float32 else torch.float64, device="cuda")
        buf[:, :d] = torch.from_numpy(np.array(x)).cuda()
        return buf[:, :d]
    buf = np.full((n, d + extra), np.nan, dtype=x.dtype)
    buf[:, :d] = x
    return buf[:, :d]


# ------------------------------------------------------------------------------------------- 1. exact operands
INT_SHAPES = nc.INT_SHAPES
INT_SHAPES_PERSISTENT = nc.INT_SHAPES_PERSISTENT


@functools.lru_cache(maxsize=None)
def int_inputs(n, k, d, dt):
    """(x, w, h, c): w, h integers in 1 .. 3, c integers in 0 .. 3, x = c o (w h) (at most 3 * 576: exact in float32)"""
    rng = np.random.default_rng(7907 * n + 101 * k + d)
    w = rng.integers(1, 4, size=(n, k)).astype(np.float64)
    h = rng.integers(1, 4, size=(k, d)).astype(np.float64)
    c = rng.integers(0, 4, size=(n, d)).astype(np.float64)
    x = (c * (w @ h)).astype(np_dt(dt))
    assert np.array_equal(x.astype(np.float64), c * (w @ h)) and (c == 0).any()
    for v in (x, w, h, c):
        v.setflags(write=False)
    return x, w, h, c


def check_integers_exact(ctx, shape, dt, expect_kernel, pitch=False):
    """inner = 1: W_new equals numpy's w * (num / den) byte for byte, without a penalty and with integer l1 / l2; inner = 0: A = W^T C
    and colsum(W) equal the integers and W comes back as it went in.  petal_nmf_kl_pass forms W inside a guard and raises if anything
    outside the n x k block changed"""
    n, k, d = shape
    x, w, h, c = int_inputs(n, k, d, dt)
    fx = pitched(x, expect_kernel) if pitch else x
    want_kernel = kernel_flag(expect_kernel, k, d)
    num, rs = c @ h.T, h.sum(axis=1)
    for l1, l2 in ((0.0, 0.0), (2.0, 3.0)):
        (wn, a, cs), info = petal.nmf_kl_pass(fx, w, h, l1_w=l1, l2_w=l2, inner_iters=1, ctx=ctx, want_info=True)
        assert info["kernel"] == want_kernel, (shape, info)
        want = w * (num / ((rs + l1) + l2 * w))
        assert wn.tobytes() == want.tobytes(), (shape, dt, l1, l2, np.abs(wn - want).max())
        mw, ma, mc, _ = model_pass(x, w, h, l1, l2, 1)
        assert mw.tobytes() == want.tobytes()
        # (A and colsum of the NEW W are not exact: sums of n <= 4115 terms over quotients of k <= 64 terms, (n + k) eps64 < 1e-12)
        assert max(rel_max(a, ma), rel_max(cs, mc)) <= 1e-12, (shape, dt, rel_max(a, ma), rel_max(cs, mc))
    wn = petal.nmf_kl_pass(fx, w, h, inner_iters=1, want_a=False, ctx=ctx)          # the pass without the H side
    assert wn.tobytes() == (w * (num / rs)).tobytes(), shape
    (w0, a, cs, term), info = petal.nmf_kl_pass(fx, w, h, inner_iters=0, ctx=ctx, want_info=True)
    assert info["kernel"] == want_kernel, (shape, info)
    assert w0.tobytes() == w.tobytes() and a.tobytes() == (w.T @ c).tobytes() and cs.tobytes() == w.sum(axis=0).tobytes(), shape
    m = c > 0
    xd = x.astype(np.float64)
    tw = float((xd[m] * np.log(c[m])).sum())
    # (a sum of N terms in any order, each with a rounded logarithm: at most (N + 4) eps64 of the sum of the absolute terms)
    assert abs(term - tw) <= (int(m.sum()) + 4) * EPS64 * float(np.abs(xd[m] * np.log(c[m])).sum()) + 1e-300, (shape, term, tw)


# ------------------------------------------------------------------------------------------- 2. real data against long double
PassCase = namedtuple("PassCase", "name n d k dt inner l1 l2")
PASS_CASES = [PassCase(f"{dt}-83x200-k17-inner{inner}" + ("-reg" if l1 else ""), 83, 200, 17, dt, inner, l1, l2)
              for dt in ("f32", "f64") for inner in (0, 1, 3) for (l1, l2) in ((0.0, 0.0), (0.25, 0.5))]


@functools.lru_cache(maxsize=None)
def pass_reference(c):
    """per quantity (W_new, A, colsum, term): (ref in long double, max |model - ref|, scale); term only for inner == 0"""
    x, w, h = nc.pass_inputs(c.n, c.d, c.k, c.dt)
    ld = np.longdouble
    ref = model_pass(x, w, h, c.l1, c.l2, c.inner, ld)
    mod = model_pass(x, w, h, c.l1, c.l2, c.inner, np.float64)
    wl, xl = np.abs(ref[0]), x.astype(ld)
    wh = ref[0] @ h.astype(ld)
    wh[wh < ld(EPS)] = ld(EPS)
    scales = [float(wl.max()), float((wl.T @ (xl / wh)).max()), float(wl.sum(axis=0).max())]
    if c.inner == 0:
        m = xl > ld(EPS)
        scales.append(float(np.abs(xl[m] * np.log(xl[m] / wh[m])).sum()))
    out = []
    for r, mo, sc in zip(ref, mod, scales):
        out.append((r, float(np.abs(np.asarray(mo, dtype=ld) - r).max()), sc))
    return tuple(out)


def pass_call(ctx, c):
    x, w, h = nc.pass_inputs(c.n, c.d, c.k, c.dt)
    outs, info = petal.nmf_kl_pass(x, w, h, l1_w=c.l1, l2_w=c.l2, inner_iters=c.inner, ctx=ctx, want_info=True)
    return outs, info


def pass_ratio(c, outs):
    """(largest ratio, rows of (name, error / scale, model / scale, floor / scale, ratio))"""
    rows, worst = [], 0.0
    for name, out, (ref, model, scale) in zip(("W", "A", "colsum", "term"), outs, pass_reference(c)):
        err = float(np.abs(np.asarray(out, dtype=np.longdouble) - ref).max())
        floor = FLOOR_EPS * EPS64 * scale
        ratio = err / max(model, floor)
        worst = max(worst, ratio)
        rows.append((name, err / scale, model / scale, floor / scale, ratio))
    return worst, rows


def check_pass_against_long_double(ctx, c, expect_kernel):
    outs, info = pass_call(ctx, c)
    assert info["kernel"] == kernel_flag(expect_kernel, c.k, c.d), info
    assert len(outs) == (4 if c.inner == 0 else 3)
    mult = MULTIPLIER["device" if expect_kernel else "hostsim"]
    worst, rows = pass_ratio(c, outs)
    for name, err, model, floor, ratio in rows:
        bound = mult * max(model, floor)
        print(f"{c.name} {name}: error {err:.3e}, model {model:.3e}, floor {floor:.3e} of the scale; ratio {ratio:.3f}, bound {bound:.3e} "
              f"(cap {CAP:.0e})")
        assert bound <= CAP, (c.name, name, bound)
        assert err <= bound, (c.name, name, ratio)
    return worst


# ------------------------------------------------------------------------------------------- 3. fits against the model and the CSR route
K33_SHAPE = (120, 48, 33)        # 48 padded components: no kernel form, the composed path on the device too
FIT_SHAPES = nc.FIT_SHAPES + (K33_SHAPE,)
DenseCase = namedtuple("DenseCase", "name fit zeros")
FIT_CASES = [DenseCase(f"{dt}-{n}x{d}-k{k}-it{it}" + ("-reg" if reg else "") + ("-z70" if zeros else ""),
                       FitCase("", n, d, k, dt, it, 0.01 if reg else 0.0, 0.02 if reg else "same", 0.3 if reg else 0.0), zeros)
             for (n, d, k) in FIT_SHAPES for dt in ("f32", "f64") for (it, reg) in ((1, False), (12, False), (12, True)) for zeros in (False, True)]
QUERY_ROWS = nc.QUERY_ROWS


@functools.lru_cache(maxsize=None)
def fit_inputs(n, d, k, dt, zeros):
    """nmf_cases.fit_inputs; zeros: with about 70 % of the entries of x and xq set to zero"""
    x, w0, h0, xq = nc.fit_inputs(n, d, k, dt)
    if zeros:
        rng = np.random.default_rng(n + 31 * d + 977 * k)
        x, xq = x * (rng.random(x.shape) < 0.3), xq * (rng.random(xq.shape) < 0.3)
        x, xq = x.astype(np_dt(dt)), xq.astype(np_dt(dt))
        assert 0.6 < (x == 0).mean() < 0.8
        x.setflags(write=False)
        xq.setflags(write=False)
    return x, w0, h0, xq


def case_inputs(c):
    f = c.fit
    return fit_inputs(f.n, f.d, f.k, f.dt, c.zeros)


@functools.lru_cache(maxsize=None)
def fit_model(c, tol=0.0):
    x, w0, h0, _ = case_inputs(c)
    return kc.model_fit(x, w0, h0, c.fit.max_iter, tol, nc.case_penalties(c.fit))


def make(ctx, f, tol=0.0, dense_path=FUSED, **kw):
    """dense_path=None: the keyword is not given"""
    if dense_path is not None:
        kw["dense_path"] = dense_path
    return petal.Nmf(f.k, max_iter=f.max_iter, tol=tol, init="custom", alpha_W=f.alpha_w, alpha_H=f.alpha_h, l1_ratio=f.l1_ratio, ctx=ctx,
                     beta_loss=KL, **kw)


def check_fit_against_model(ctx, c, expect_kernel):
    """W, H, reconstruction_err and err_init of the fused fit at the bar against the model and against the library's CSR fit of
    to_csr(x) from the same W0 / H0; n_iter; which path ran; fit_transform's dtype"""
    f = c.fit
    x, w0, h0, _ = case_inputs(c)
    mo = fit_model(c)
    m = make(ctx, f)
    w = m.fit_transform(x, W=w0, H=h0)
    info = m.info()
    want_kernel = kernel_flag(expect_kernel, f.k, f.d)
    assert (info["n"], info["d"], info["k"], info["n_iter"]) == (f.n, f.d, f.k, f.max_iter) and m.n_iter == mo.n_iter
    assert info["fit_kernel"] == m.kernel_path == want_kernel and info["transform_kernel"] == -1, (info, m.kernel_path)
    tol = tol_of(f.dt)
    got = (rel_max(w, mo.w), rel_max(m.components, mo.h), abs(m.reconstruction_err - mo.err) / mo.err, abs(m.err_init - mo.err_init) / mo.err_init)
    print(f"{c.name}: against the model W {got[0]:.2e}, H {got[1]:.2e}, err {got[2]:.2e}, err_init {got[3]:.2e} (bar {tol:.0e})")
    assert to_numpy(w).dtype == np_dt(f.dt) and max(got) <= tol, (c.name, got)
    sx = csr(ctx, *to_csr(x), x.shape)
    try:
        s = make(ctx, f)
        ws = s.fit_transform(sx, W=w0, H=h0)
        gs = (rel_max(w, to_numpy(ws)), rel_max(m.components, s.components), abs(m.reconstruction_err - s.reconstruction_err) / s.reconstruction_err,
              abs(m.err_init - s.err_init) / s.err_init)
        print(f"{c.name}: against the CSR fit W {gs[0]:.2e}, H {gs[1]:.2e}, err {gs[2]:.2e}, err_init {gs[3]:.2e}")
        assert max(gs) <= tol and m.n_iter == s.n_iter, (c.name, gs)
    finally:
        sx.close()
    return m


# ------------------------------------------------------------------------------------------- 4. transform
def check_transform(ctx, c, expect_kernel, updates):
    """`updates` W-updates of fresh rows against the model; a model fitted on CSR transforms dense rows through the new entry and a
    model fitted dense transforms CSR rows: all at the bar of each other; no rows give (0, k)"""
    f = c.fit._replace(max_iter=updates)
    x, w0, h0, xq = case_inputs(c)
    pen = nc.case_penalties(f)
    tol = tol_of(f.dt)
    want_kernel = kernel_flag(expect_kernel, f.k, f.d)
    sx, sq = csr(ctx, *to_csr(x), x.shape), csr(ctx, *to_csr(xq), xq.shape)
    try:
        dense, sparse = make(ctx, f).fit(x, W=w0, H=h0), make(ctx, f).fit(sx, W=w0, H=h0)
        assert rel_max(dense.components, sparse.components) <= tol
        want = kc.model_transform(xq, dense.components, f.k, updates, pen)
        wdd = to_numpy(dense.transform(xq))
        assert dense.info()["transform_kernel"] == dense.kernel_path == want_kernel, dense.info()
        wsd = to_numpy(sparse.transform(xq))            # fitted on CSR, dense rows through petal_nmf_transform_loss
        assert sparse.info()["transform_kernel"] == sparse.kernel_path == want_kernel, sparse.info()
        wds = to_numpy(dense.transform(sq))             # fitted dense, CSR rows
        got = (rel_max(wdd, want), rel_max(wsd, wdd), rel_max(wds, wdd))
        print(f"{c.name} {updates} updates: model {got[0]:.2e}, csr-fitted on dense rows {got[1]:.2e}, dense-fitted on csr rows {got[2]:.2e} (bar {tol:.0e})")
        assert wdd.shape == (QUERY_ROWS, f.k) and wdd.dtype == np_dt(f.dt) and max(got) <= tol, (c.name, got)
        before = dense.kernel_path
        assert to_numpy(dense.transform(xq[:0])).shape == (0, f.k) and dense.kernel_path == before
    finally:
        sx.close()
        sq.close()


# ------------------------------------------------------------------------------------------- 5. stopping rule, initialisation, determinism
def check_stopping_rule(ctx, c, expect_kernel):
    """nmf_kl_cases.STOP_CASES' data as a dense array: the model's n_iter"""
    mo = kc.check_stop_case_is_decided(c)
    x, w0, h0 = kc.stop_inputs(c)
    m = petal.Nmf(c.k, max_iter=kc.STOP_MAX_ITER, tol=c.tol, init="custom", ctx=ctx, beta_loss=KL, dense_path=FUSED).fit(x, W=w0, H=h0)
    print(f"{c.name}: n_iter {m.n_iter} (model {mo.n_iter}), checks {['%.2e' % v for v in mo.checks]}, tol {c.tol:g}")
    assert m.n_iter == mo.n_iter and m.kernel_path == kernel_flag(expect_kernel, c.k, c.d)
    assert abs(m.reconstruction_err - mo.err) <= tol_of(c.dt) * mo.err and rel_max(m.components, mo.h) <= tol_of(c.dt)


def check_random_init(ctx, dt, expect_kernel):
    """init="random" draws nmf_cases.random_init's stream: W0 first, then H0"""
    n, d, k = 60, 24, 4
    x = nc.fit_inputs(n, d, k, dt)[0]
    w0, h0 = nc.random_init(x, k, 12345)
    mo = kc.model_fit(x, w0, h0, 1)
    fits = []
    for seed in (12345, 12345, 54321):
        m = petal.Nmf(k, max_iter=1, tol=0.0, init="random", seed=seed, ctx=ctx, beta_loss=KL, dense_path=FUSED)
        w = to_numpy(m.fit_transform(x))
        fits.append((w.tobytes(), m.components.tobytes()))
        assert m.kernel_path == kernel_flag(expect_kernel, k, d)
        if seed == 12345:
            got = (rel_max(w, mo.w), rel_max(m.components, mo.h), abs(m.err_init - mo.err_init) / mo.err_init)
            assert max(got) <= tol_of(dt), got
    assert fits[0] == fits[1] and fits[0] != fits[2]


def fit_bytes(ctx, c, x_in, xq_in, **kw):
    _, w0, h0, _ = case_inputs(c)
    m = make(ctx, c.fit, **kw)
    w = to_numpy(m.fit_transform(x_in, W=w0, H=h0))
    return m, (w.tobytes(), m.components.tobytes(), m.reconstruction_err, m.err_init, to_numpy(m.transform(xq_in)).tobytes())


def check_same_bytes_twice(ctx, c):
    x, _, _, xq = case_inputs(c)
    assert fit_bytes(ctx, c, x, xq)[1] == fit_bytes(ctx, c, x, xq)[1]


# ------------------------------------------------------------------------------------------- 6. paths
def check_fallback_against_kernel(ctx, c, expect_kernel):
    """nmf_fallback = 1: the composed path (kernel_path 0), within the bar of the default path"""
    f = c.fit
    x, w0, h0, xq = case_inputs(c)
    want_kernel = kernel_flag(expect_kernel, f.k, f.d)
    m = make(ctx, f)
    w = to_numpy(m.fit_transform(x, W=w0, H=h0))
    assert m.kernel_path == want_kernel
    wq = to_numpy(m.transform(xq))
    assert m.kernel_path == want_kernel and m.info()["fit_kernel"] == m.info()["transform_kernel"] == want_kernel
    ctx.set_option("nmf_fallback", 1)
    try:
        g = make(ctx, f)
        wf = to_numpy(g.fit_transform(x, W=w0, H=h0))
        assert g.kernel_path == 0
        wqf = to_numpy(g.transform(xq))
        assert g.kernel_path == 0 and g.info()["fit_kernel"] == 0 and g.info()["transform_kernel"] == 0
    finally:
        ctx.set_option("nmf_fallback", 0)
    tol = tol_of(f.dt)
    assert max(rel_max(wf, w), rel_max(g.components, m.components), rel_max(wqf, wq)) <= tol
    assert abs(g.reconstruction_err - m.reconstruction_err) <= tol * m.reconstruction_err


OUTSIDE_SHAPES = nc.OUTSIDE_SHAPES    # k = 65 > 64 (no cap on this route); 528 padded columns > 512


def check_outside_envelope(ctx, shape, dt):
    """a shape the kernel does not take fits through the composed path, correctly"""
    n, d, k = shape
    f = FitCase(f"{dt}-{n}x{d}-k{k}", n, d, k, dt, 3, 0.0, "same", 0.0)
    x, w0, h0, xq = nc.fit_inputs(n, d, k, dt)
    mo = kc.model_fit(x, w0, h0, 3)
    m = make(ctx, f)
    w = m.fit_transform(x, W=w0, H=h0)
    assert m.kernel_path == 0
    wq = m.transform(xq)
    assert m.kernel_path == 0 and m.info()["fit_kernel"] == 0 and m.info()["transform_kernel"] == 0
    tol = tol_of(dt)
    assert max(rel_max(w, mo.w), rel_max(m.components, mo.h), rel_max(wq, kc.model_transform(xq, mo.h, k, 3))) <= tol
    assert abs(m.reconstruction_err - mo.err) <= tol * mo.err


def check_device_input_stays_on_the_device(ctx, c):
    """a torch.cuda input with dense_path="fused": device tensors back, kernel_path 1, the bytes of the numpy-input fit"""
    import torch
    x, w0, h0, xq = case_inputs(c)
    m = make(ctx, c.fit)
    dev = lambda v: torch.from_numpy(np.array(v)).cuda()       # (the cached inputs are read-only: a copy goes up)
    w = m.fit_transform(dev(x), W=dev(w0), H=dev(h0))
    assert isinstance(w, torch.Tensor) and w.is_cuda and m.kernel_path == 1
    wq = m.transform(dev(xq))
    assert isinstance(wq, torch.Tensor) and wq.is_cuda and m.kernel_path == 1
    ref, want = fit_bytes(ctx, c, x, xq)
    assert (to_numpy(w).tobytes(), m.components.tobytes(), m.reconstruction_err, m.err_init, to_numpy(wq).tobytes()) == want


# ------------------------------------------------------------------------------------------- 7. nothing existing moved
def raw_fit_loss(ctx, x, k, loss, w0, h0, max_iter=3):
    """petal_nmf_fit_loss by itself: (status-checked) handle wrapped in an Nmf of the Frobenius facade, and W"""
    keep = []
    mx, mw, mh = petal.describe(x, keep), petal.describe(w0, keep), petal.describe(h0, keep)
    w = np.empty((x.shape[0], k), dtype=x.dtype)
    mo = petal.describe(w, keep)
    spec = petal.petal_nmf_spec(max_iter, 0.0, 0.0, 0.0, 0.0, 0.0)
    h = C.c_void_p()
    ctx.check(ctx.lib.petal_nmf_fit_loss(ctx._h, C.byref(mx), k, C.byref(spec), C.c_int64(loss), C.byref(mw), C.byref(mh), C.c_int64(0),
                                         C.byref(h), C.byref(mo)))
    m = petal.Nmf(k, max_iter=max_iter, tol=0.0, init="custom", ctx=ctx)
    m._h = h
    ctx._nmf.add(m)
    return m, w


def check_nothing_existing_moved(ctx, c):
    f = c.fit
    x, w0, h0, xq = case_inputs(c)
    # dense_path="compress", given explicitly, is the call without it
    assert fit_bytes(ctx, c, x, xq, dense_path="compress")[1] == fit_bytes(ctx, c, x, xq, dense_path=None)[1]
    # under the Frobenius loss the keyword changes nothing
    frob = []
    for kw in ({}, {"dense_path": FUSED}):
        m = petal.Nmf(f.k, max_iter=3, tol=0.0, init="custom", ctx=ctx, **kw)
        frob.append((to_numpy(m.fit_transform(x, W=w0, H=h0)).tobytes(), m.components.tobytes(), m.reconstruction_err,
                     to_numpy(m.transform(xq)).tobytes()))
    assert frob[0] == frob[1]
    # petal_nmf_fit_loss(..., 0, ...) is petal_nmf_fit; petal_nmf_transform_loss gives petal_nmf_transform's bytes on it
    m, w = raw_fit_loss(ctx, x, f.k, petal.NMF_LOSS_FROBENIUS, w0, h0)
    keep = []
    wq = np.empty((xq.shape[0], f.k), dtype=xq.dtype)
    mq, mo = petal.describe(xq, keep), petal.describe(wq, keep)
    ctx.check(ctx.lib.petal_nmf_transform_loss(ctx._h, m._handle(), C.byref(mq), C.byref(mo)))
    assert (w.tobytes(), m.components.tobytes(), m.reconstruction_err, wq.tobytes()) == frob[0]
    # petal_nmf_transform still refuses the Kullback-Leibler model
    kl = make(ctx, f).fit(x, W=w0, H=h0)
    with raises_with(petal.InvalidInput, "does not take a kullback-leibler model"):
        ctx.check(ctx.lib.petal_nmf_transform(ctx._h, kl._handle(), C.byref(mq), C.byref(mo)))
    assert C.sizeof(petal.petal_nmf_spec) == 48


# ------------------------------------------------------------------------------------------- 8. errors
def check_errors(ctx, make_other_ctx, make_sharded_ctx):
    n, d, k = 30, 12, 3
    x, w0, h0, xq = (np.array(v) for v in nc.fit_inputs(n, d, k, "f64"))
    inv, lin = petal.InvalidInput, petal.LinalgError

    def fit(xx=x, kk=k, w=w0, h=h0, **kw):
        args = dict(max_iter=2, tol=0.0, init="custom", ctx=ctx, beta_loss=KL, dense_path=FUSED)
        args.update(kw)
        return petal.Nmf(kk, **args).fit(xx, W=w, H=h)
    for bad_path in ("dense", "", None, 1):
        with raises_with(inv, "unknown dense_path"):
            petal.Nmf(k, ctx=ctx, beta_loss=KL, dense_path=bad_path)
    with raises_with(inv, "unknown dense_path"):
        petal.Nmf(k, ctx=ctx, dense_path="sparse")                    # read under the Frobenius loss too
    with raises_with(inv, "unknown beta_loss"):
        petal.Nmf(k, ctx=ctx, beta_loss="itakura-saito", dense_path=FUSED)
    for loss in (2, -1):
        with raises_with(inv, "unknown loss"):
            raw_fit_loss(ctx, x, k, loss, w0, h0)
    with raises_with(inv, "term_out comes with inner_iters = 0 only"):
        petal.nmf_kl_pass(x, w0, h0, inner_iters=1, want_term=True, ctx=ctx)
    with raises_with(inv, "negative parameter"):
        petal.nmf_kl_pass(x, w0, h0, inner_iters=-1, ctx=ctx)
    with raises_with(inv, "not negative"):
        petal.nmf_kl_pass(x, w0, h0, l1_w=-1.0, ctx=ctx)
    with raises_with(inv, "negative values in data"):
        petal.nmf_kl_pass(-x, w0, h0, ctx=ctx)
    with raises_with(inv, "w should be"):
        petal.nmf_kl_pass(x, w0[:5], h0, ctx=ctx)
    with raises_with(inv, "at least 1"):
        fit(kk=0, w=w0[:, :0], h=h0[:0])
    with raises_with(inv, "every dimension should be at least 13"):
        fit(kk=13, w=np.ones((n, 13)), h=np.ones((13, d)))
    with raises_with(inv, "no rows or no columns"):
        fit(xx=x[:0], w=w0[:0])
    for kw in ({"alpha_W": -0.1}, {"alpha_H": -1.0}, {"tol": -1.0}):
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
    m = fit()
    with raises_with(inv, "# of columns should be 12"):
        m.transform(x[:, :11])
    with raises_with(inv, "dtype"):
        m.transform(xq.astype(np.float32))
    bad = xq.copy()
    bad[0, 0] = -1.0
    with raises_with(inv, "negative values in data"):
        m.transform(bad)
    bad[0, 0] = np.inf
    with raises_with(lin, "did not converge"):
        m.transform(bad)
    other = make_other_ctx()
    try:
        keep = []
        wq = np.empty((xq.shape[0], k))
        mq, mo = petal.describe(xq, keep), petal.describe(wq, keep)
        with raises_with(inv, "belongs to another ctx"):
            other.check(other.lib.petal_nmf_transform_loss(other._h, m._handle(), C.byref(mq), C.byref(mo)))
    finally:
        other.close()
    shard = make_sharded_ctx()
    try:
        with raises_with(inv, "sharded"):
            fit(ctx=shard)
        with raises_with(inv, "sharded"):
            petal.nmf_kl_pass(x, w0, h0, ctx=shard)
    finally:
        shard.close()


# ------------------------------------------------------------------------------------------- the measured ratios
def measure(ctx, label, lines):
    worst = 0.0
    for c in PASS_CASES:
        outs, info = pass_call(ctx, c)
        w, rows = pass_ratio(c, outs)
        worst = max(worst, w)
        for name, err, model, floor, ratio in rows:
            lines.append(f"{label:8s} {c.name:28s} {name:6s}  kernel {info['kernel']}  error {err:.3e}  model {model:.3e}  floor {floor:.3e}  "
                         f"ratio {ratio:.3f}")
    lines.append(f"{label:8s} largest ratio {worst:.3f}")
    return worst


if __name__ == "__main__":
    import hostsim
    out = ["# petal_nmf_kl_pass against numpy.longdouble: W_new, A = W_new^T (X / (W_new H)), colsum(W_new) and, for inner = 0, the loss's "
           "term; errors over the scale (the largest sum of absolute terms); ratio = error / max(model, floor), model = the error of the "
           "float64 numpy statement.  The bound of the tests is nmf_cases.MULTIPLIER (unchanged) x max(model, floor)."]
    if len(sys.argv) < 2 or sys.argv[1] != "--host-only":
        dev = petal.Context(0)
        measure(dev, "device", out)
        dev.close()
    host = hostsim.context()
    measure(host, "hostsim", out)
    host.close()
    out.append("tests/nmf_cases.py MULTIPLIER: " + ", ".join(f"{k} {v}" for k, v in MULTIPLIER.items()))
    dst = os.path.join(ROOT, sys.argv[2] if len(sys.argv) > 2 else os.path.join("profiles", "nmf_kl_dense_errors.txt"))
    with open(dst, "w") as f:
        f.write("\n".join(out) + "\n")
    print("\n".join(out))
