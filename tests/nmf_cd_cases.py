"""Nmf with the coordinate-descent solver (include/petal_hip_nmf_cd.h): the numpy model of the statement, the generators, the case tables
with their bounds, and the checks the GPU suite (tests/test_gpu_nmf_cd.py, expect_kernel=True) and the host suite
(tests/test_nmf_cd_host.py, expect_kernel=False) share.  The layout is nmf_cases.py's.

The model is the header's statement in float64 numpy: scikit-learn's _update_cdnmf_fast without shuffling, one coordinate at a time over
all rows at once (tests/test_nmf_cd_host.py holds it to ``sklearn.decomposition.NMF(init="custom", solver="cd")`` where scikit-learn is
installed).  It is the reference of every test here.

A. petal_nmf_cd_pass on exact operands, bit for bit: H rows are disjoint 0/1 indicators with 2^s ones each (S = 2^s I), X holds small
   integers, l1 is a small integer and l2 = 0 -- W_new = max(Z - l1, 0) 2^-s, A, B and the violation are exact in float64 whatever the
   order of the sums; the second sweep is a fixed point with violation 0.
B. petal_nmf_cd_pass and petal_nmf_cd_hupdate on real data against numpy.longdouble, nmf_cases.py's section B:

       ratio = max |out - ref| / max(max |model - ref|, FLOOR_EPS eps64 scale)

   MULTIPLIER is, per path, twice the largest ratio measured on the device and on the host simulation, rounded up
   (profiles/nmf_cd_errors.txt), and the bound -- multiplier x max(model, floor) -- must stay below CAP = 1e-12 of the scale.  The
   violation is discontinuous where a coordinate lands exactly on 0, so every case keeps every pre-clamp value w - grad / S_tt of the
   long-double reference at least MARGIN x scale away from 0 (asserted for EVERY case in pass_reference / h_reference).
C. fit / fit_transform / transform / inverse_transform against the model at the project's parity bar.

Run as a script on a machine with the GPU it writes profiles/nmf_cd_errors.txt: the device's rows and the host simulation's."""
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
from nmf_cases import CAP, EPS64, FLOOR_EPS, penalties, raises_with, rel_max, to_numpy, tol_of  # noqa: E402,F401
from wide_cases import np_dt  # noqa: E402

MARGIN = 1e-6


# ------------------------------------------------------------------------------------------- the model
def model_sweep(w, z, s, track=None):
    """one sweep of every row of w (rows x k, in place) with z (rows x k, the l1 penalty taken off) and s (k x k, the l2 penalty on its
    diagonal); returns the violation.  track (a list): the smallest |w - grad / S_tt| met is appended."""
    viol, near = w.dtype.type(0), np.inf
    for t in range(w.shape[1]):
        grad = -z[:, t] + w @ s[t]
        pg = np.where(w[:, t] == 0, np.minimum(0, grad), grad)
        viol += np.abs(pg).sum()
        if s[t, t] != 0:
            pre = w[:, t] - grad / s[t, t]
            near = min(near, float(np.abs(pre).min()))
            w[:, t] = np.maximum(pre, 0)
    if track is not None:
        track.append(near)
    return viol


def model_pass(x, w, h, l1=0.0, l2=0.0, inner=1, from_zero=False, ft=np.float64, track=None):
    """(W_new, A, B, violation per sweep) of the header's pass in the float type ft"""
    x, w, h = x.astype(ft), np.array(w, dtype=ft), h.astype(ft)
    if from_zero and inner > 0:
        w[:] = 0
    z, s = x @ h.T - ft(l1), h @ h.T + ft(l2) * np.eye(h.shape[0], dtype=ft)
    viol = np.array([model_sweep(w, z, s, track) for _ in range(inner)], dtype=ft)
    return w, w.T @ x, w.T @ w, viol


def model_hupdate(a, b, h, l1=0.0, l2=0.0, ft=np.float64, track=None):
    """(H_new, violation): the sweep on the rows of H^T"""
    a, b, ht = a.astype(ft), b.astype(ft), np.array(h.T, dtype=ft)
    viol = model_sweep(ht, a.T - ft(l1), b + ft(l2) * np.eye(b.shape[0], dtype=ft), track)
    return np.ascontiguousarray(ht.T), viol


Fit = namedtuple("Fit", "w h n_iter err err_init ratios")


def model_fit(x, w0, h0, max_iter, tol=0.0, pen=(0.0, 0.0, 0.0, 0.0)):
    """the header's fit; ratios = violation / violation_init after every iteration"""
    x, w, h = x.astype(np.float64), np.array(w0, dtype=np.float64), np.array(h0, dtype=np.float64)
    l1w, l2w, l1h, l2h = pen
    nx2 = float((x * x).sum())
    a, b = w.T @ x, w.T @ w
    err_init = nc.model_loss(nx2, a, b, h)
    ratios, n_iter, v_init = [], max_iter, 0.0
    for it in range(1, max_iter + 1):
        w, a, b, vw = model_pass(x, w, h, l1w, l2w, 1)
        h, vh = model_hupdate(a, b, h, l1h, l2h)
        v = float(vw[0]) + float(vh)
        if it == 1:
            v_init = v
        ratios.append(v / v_init if v_init else 0.0)
        if tol > 0 and (v_init == 0 or v / v_init <= tol):
            n_iter = it
            break
    return Fit(w, h, n_iter, nc.model_loss(nx2, a, b, h), err_init, ratios)


def model_transform(xq, h, max_iter, pen=(0.0, 0.0, 0.0, 0.0)):
    """W from ZERO, exactly max_iter sweeps on the fixed Z"""
    k = h.shape[0]
    return model_pass(xq, np.zeros((xq.shape[0], k)), h, pen[0], pen[1], max_iter, True)[0]


def kernel_takes(k, d):
    """k_nmf_cd_pass's envelope: 16, 32 or 64 padded components (not 48), at most 512 padded columns"""
    return (k <= 32 or 49 <= k <= 64) and (d + 15) // 16 * 16 <= 512


# ------------------------------------------------------------------------------------------- A. exact operands
INT_N = (1, 15, 16, 17, 33, 37)
INT_K = (1, 3, 16, 17, 32, 49, 64, 33, 48)                    # 33 and 48 pad to 48: the composed path
INT_D = (16, 24, 80, 256, 272, 512)
INT_SHAPES = tuple((n, k, d) for n in INT_N for k in INT_K for d in INT_D if k <= d)
INT_N_PERSISTENT = nc.INT_N_PERSISTENT                        # 16 * 257 + 3: workgroups 0 and 1 take a second tile, the last tile is partial
INT_SHAPES_PERSISTENT = tuple((INT_N_PERSISTENT, k, d) for (k, d) in ((3, 24), (17, 272), (64, 512)))


def check_integers_exact(ctx, shape, dt, expect_kernel, pitch=False):
    """W_new, A, B and every sweep's violation equal the model's bit for bit with l1 = 3 2^s (about half of Z - l1 is negative: the
    clamp works); inner 0, 1 and 3 (sweeps 2 and 3 are a fixed point with violation 0), from W and from zero; the guard of
    petal_nmf_cd_pass raises if anything outside the n x k block changed"""
    n, k, d = shape
    x, w, h, s = nc.int_inputs(n, k, d, dt)
    l1 = 3.0 * 2.0 ** s
    fx = x
    if pitch:   # a view with a row pitch above d
        big = np.full((n, d + 16), 5, dtype=x.dtype)
        big[:, :d] = x
        fx = big[:, :d]
    want_kernel = 1 if expect_kernel and kernel_takes(k, d) else 0
    z = x.astype(np.float64) @ h.T - l1
    assert (z < 0).any() or n * k < 4, shape
    for inner, from_zero, ab in ((1, False, True), (3, False, False), (3, True, True), (1, True, False), (0, False, True)):
        out, info = petal.nmf_cd_pass(fx, w, h, l1_w=l1, inner_iters=inner, from_zero=from_zero, want_ab=ab, ctx=ctx, want_info=True)
        mw, ma, mb, mv = model_pass(x, w, h, l1, 0.0, inner, from_zero)
        assert info["kernel"] == want_kernel, (shape, info)
        got = dict(zip(("W", "A", "B", "V") if ab else ("W", "V"), out))
        for name, want in (("W", mw), ("A", ma), ("B", mb), ("V", mv)):
            if name in got:
                assert got[name].tobytes() == want.tobytes(), (shape, dt, inner, from_zero, name, np.abs(got[name] - want).max())
        if inner == 0:
            assert mw.tobytes() == w.tobytes()
        if inner == 3:
            assert mv[1] == 0 and mv[2] == 0 and (from_zero or n * k < 4 or mv[0] > 0)
            assert mw.tobytes() == (np.maximum(z, 0) * 2.0 ** -s).tobytes()


# ------------------------------------------------------------------------------------------- B. real data against long double
PassCase = namedtuple("PassCase", "name n d k dt inner l1 l2 from_zero")
PASS_CASES = [PassCase(f"{dt}-{n}x{d}-k{k}-inner{inner}" + ("-reg" if l1 else "") + ("-zero" if fz else ""), n, d, k, dt, inner, l1, l2, fz)
              for dt in ("f32", "f64")
              for (n, d, k, inner, l1, l2, fz) in ((83, 200, 17, 1, 0.0, 0.0, False), (83, 200, 17, 3, 0.25, 0.5, False),
                                                  (37, 80, 3, 2, 0.0, 0.0, True), (53, 512, 64, 1, 0.125, 0.0, False))]
HCase = namedtuple("HCase", "name n d k l1 l2")
H_CASES = [HCase("83x200-k17", 83, 200, 17, 0.0, 0.0), HCase("83x200-k17-reg", 83, 200, 17, 0.25, 0.5), HCase("37x80-k3", 37, 80, 3, 0.0, 0.0),
           HCase("53x512-k64-reg", 53, 512, 64, 0.125, 0.25)]
# twice the largest measured ratio, rounded up (profiles/nmf_cd_errors.txt: 1.617 on the device, 3.583 on the host simulation, whose
# literal sweep sums each gradient in another order than the vectorised model; its largest ratios are violations measured over the floor)
MULTIPLIER = {"device": 4.0, "hostsim": 8.0}


@functools.lru_cache(maxsize=None)
def pass_reference(c):
    """per quantity (W_new, A, B, violation): (ref in long double, max |model - ref|, scale); asserts the case's margin"""
    x, w, h = nc.pass_inputs(c.n, c.d, c.k, c.dt)
    ld = np.longdouble
    track = []
    ref = model_pass(x, w, h, c.l1, c.l2, c.inner, c.from_zero, ld, track)
    mod = model_pass(x, w, h, c.l1, c.l2, c.inner, c.from_zero, np.float64)
    wl, xl = np.abs(ref[0]), np.abs(x.astype(ld))
    scales = (float(wl.max()), float((wl.T @ xl).max()), float((wl.T @ wl).max()), float(ref[3].max()))
    assert min(track) >= MARGIN * scales[0], (c.name, min(track), scales[0])   # no coordinate lands within the margin of the clamp
    return tuple((r, float(np.abs(m.astype(ld) - r).max()), sc) for r, m, sc in zip(ref, mod, scales))


@functools.lru_cache(maxsize=None)
def h_inputs(c):
    """(a, b, h): A and B as the pass leaves them (the model's, float64), H random"""
    x, w, h = nc.pass_inputs(c.n, c.d, c.k, "f64")
    _, a, b, _ = model_pass(x, w, h, 0.0, 0.0, 1)
    for v in (a, b):
        v.setflags(write=False)
    return a, b, h


@functools.lru_cache(maxsize=None)
def h_reference(c):
    a, b, h = h_inputs(c)
    ld = np.longdouble
    track = []
    ref = model_hupdate(a, b, h, c.l1, c.l2, ld, track)
    mod = model_hupdate(a, b, h, c.l1, c.l2)
    scales = (float(np.abs(ref[0]).max()), float(ref[1]))
    assert min(track) >= MARGIN * scales[0], (c.name, min(track), scales[0])
    return tuple((r, float(np.abs(np.asarray(m, dtype=ld) - r).max()), sc) for r, m, sc in zip(ref, mod, scales))


def pass_call(ctx, c):
    x, w, h = nc.pass_inputs(c.n, c.d, c.k, c.dt)
    return petal.nmf_cd_pass(x, w, h, l1_w=c.l1, l2_w=c.l2, inner_iters=c.inner, from_zero=c.from_zero, ctx=ctx, want_info=True)


def h_call(ctx, c):
    a, b, h = h_inputs(c)
    (hn, v), info = petal.nmf_cd_hupdate(a, b, h, l1_h=c.l1, l2_h=c.l2, ctx=ctx, want_info=True)
    return (hn, np.array(v)), info


def ratios(names, outs, reference):
    """(largest ratio, rows of (name, error / scale, model / scale, floor / scale, ratio))"""
    rows, worst = [], 0.0
    for name, out, (ref, model, scale) in zip(names, outs, reference):
        err = float(np.abs(np.asarray(out, dtype=np.longdouble) - ref).max())
        floor = FLOOR_EPS * EPS64 * scale
        ratio = err / max(model, floor)
        worst = max(worst, ratio)
        rows.append((name, err / scale, model / scale, floor / scale, ratio))
    return worst, rows


def _check_rows(cname, rows, mult):
    for name, err, model, floor, ratio in rows:
        bound = mult * max(model, floor)
        print(f"{cname} {name}: error {err:.3e}, model {model:.3e}, floor {floor:.3e} of the scale; ratio {ratio:.3f}, bound {bound:.3e} "
              f"(cap {CAP:.0e})")
        assert bound <= CAP, (cname, name, bound)
        assert err <= bound, (cname, name, ratio)


def check_pass_against_long_double(ctx, c, expect_kernel):
    outs, info = pass_call(ctx, c)
    assert info["kernel"] == (1 if expect_kernel else 0), info
    worst, rows = ratios(("W", "A", "B", "violation"), outs, pass_reference(c))
    _check_rows(c.name, rows, MULTIPLIER["device" if expect_kernel else "hostsim"])
    return worst


def check_hupdate_against_long_double(ctx, c, expect_kernel):
    outs, info = h_call(ctx, c)
    assert info["kernel"] == (1 if expect_kernel else 0), info
    worst, rows = ratios(("H", "violation"), outs, h_reference(c))
    _check_rows(c.name, rows, MULTIPLIER["device" if expect_kernel else "hostsim"])
    return worst


# ------------------------------------------------------------------------------------------- C. fits against the model
FitCase = nc.FitCase
_PEN = (("", 0.0, "same", 0.0), ("-l1", 0.01, 0.02, 1.0), ("-l2", 0.01, 0.02, 0.0), ("-l1l2", 0.01, 0.02, 0.3))
FIT_CASES = [FitCase(f"{dt}-200x48-k5-it{it}{tag}", 200, 48, 5, dt, it, aw, ah, rho) for dt in ("f32", "f64") for it in (1, 7)
             for (tag, aw, ah, rho) in _PEN] + \
            [FitCase(f"{dt}-{n}x{d}-k{k}-it7", n, d, k, dt, 7, 0.0, "same", 0.0) for dt in ("f32", "f64")
             for (n, d, k) in ((300, 64, 8), (100, 272, 17), (80, 512, 64))]
QUERY_ROWS = nc.QUERY_ROWS
fit_inputs = nc.fit_inputs
case_penalties = nc.case_penalties


@functools.lru_cache(maxsize=None)
def fit_model(c, tol=0.0):
    x, w0, h0, _ = fit_inputs(c.n, c.d, c.k, c.dt)
    return model_fit(x, w0, h0, c.max_iter, tol, case_penalties(c))


def make(ctx, c, tol=0.0, **kw):
    return petal.Nmf(c.k, max_iter=c.max_iter, tol=tol, init="custom", alpha_W=c.alpha_w, alpha_H=c.alpha_h, l1_ratio=c.l1_ratio, ctx=ctx,
                     solver="cd", **kw)


def check_fit_against_model(ctx, c, expect_kernel):
    """W, H, reconstruction_err and err_init at the bar; n_iter; info(); fit_transform's W is the fit's W"""
    x, w0, h0, _ = fit_inputs(c.n, c.d, c.k, c.dt)
    mo = fit_model(c)
    m = make(ctx, c)
    w = m.fit_transform(x, W=w0, H=h0)
    info = m.info()
    assert m.solver == "cd" and (info["n"], info["d"], info["k"], info["n_iter"]) == (c.n, c.d, c.k, c.max_iter) and m.n_iter == mo.n_iter
    assert info["fit_kernel"] == (1 if expect_kernel and kernel_takes(c.k, c.d) else 0) and info["transform_kernel"] == -1, info
    tol = tol_of(c.dt)
    got = (rel_max(w, mo.w), rel_max(m.components, mo.h), abs(m.reconstruction_err - mo.err) / mo.err, abs(m.err_init - mo.err_init) / mo.err_init)
    print(f"{c.name}: W {got[0]:.2e}, H {got[1]:.2e}, err {got[2]:.2e}, err_init {got[3]:.2e} (bar {tol:.0e})")
    assert to_numpy(w).dtype == np_dt(c.dt) and max(got) <= tol, (c.name, got)
    return m


def check_transform(ctx, c, expect_kernel, updates=None):
    """transform of fresh rows (from W = 0, exactly max_iter sweeps), inverse_transform = W H, at the bar"""
    x, w0, h0, xq = fit_inputs(c.n, c.d, c.k, c.dt)
    if updates is not None:
        c = c._replace(max_iter=updates)
    mo = fit_model(c)
    m = make(ctx, c).fit(x, W=w0, H=h0)
    wq = m.transform(xq)
    info = m.info()
    assert info["transform_kernel"] == (1 if expect_kernel and kernel_takes(c.k, c.d) else 0), info
    want = model_transform(np.asarray(xq, dtype=np.float64), mo.h, c.max_iter, case_penalties(c))   # (the fit's l1_w, l2_w)
    tol = tol_of(c.dt)
    back = m.inverse_transform(wq)
    wq64 = to_numpy(wq).astype(np.float64)
    got = (rel_max(wq, want), rel_max(back, wq64 @ m.components))
    print(f"{c.name}: transform {got[0]:.2e}, inverse_transform {got[1]:.2e} (bar {tol:.0e})")
    assert to_numpy(wq).shape == (QUERY_ROWS, c.k) and to_numpy(back).shape == (QUERY_ROWS, c.d) and max(got) <= tol, (c.name, got)


# ------------------------------------------------------------------------------------------- the stopping rule
# Cases whose model stops before STOP_MAX_ITER with the deciding ratio violation / violation_init at least 1 % away from tol at EVERY
# iteration (check_stop_case_is_decided asserts it on the model), and the all-zero-violation case.
StopCase = namedtuple("StopCase", "name n d k dt seed tol")
STOP_CASES = [StopCase("f32-100x24-k2-seed58", 100, 24, 2, "f32", 58, 2e-2), StopCase("f64-100x24-k2-seed33", 100, 24, 2, "f64", 33, 1e-2),
              StopCase("f64-60x40-k5-seed7", 60, 40, 5, "f64", 7, 6e-2)]
STOP_MAX_ITER = 200


@functools.lru_cache(maxsize=None)
def stop_inputs(c):
    return nc.stop_inputs(nc.StopCase(c.name, c.n, c.d, c.k, c.dt, c.seed, c.tol))


@functools.lru_cache(maxsize=None)
def check_stop_case_is_decided(c):
    mo = model_fit(*stop_inputs(c), STOP_MAX_ITER, c.tol)
    assert 3 <= mo.n_iter < STOP_MAX_ITER and len(mo.ratios) == mo.n_iter, (mo.n_iter, mo.ratios)
    assert mo.ratios[-1] <= c.tol and all(abs(r - c.tol) >= 0.01 * c.tol for r in mo.ratios), (c.tol, mo.ratios)
    assert all(r > c.tol for r in mo.ratios[:-1])
    return mo


def check_stopping_rule(ctx, c, expect_kernel):
    mo = check_stop_case_is_decided(c)
    x, w0, h0 = stop_inputs(c)
    m = petal.Nmf(c.k, max_iter=STOP_MAX_ITER, tol=c.tol, init="custom", ctx=ctx, solver="cd").fit(x, W=w0, H=h0)
    print(f"{c.name}: n_iter {m.n_iter} (model {mo.n_iter}), last ratios {['%.3e' % v for v in mo.ratios[-3:]]}, tol {c.tol:g}")
    assert m.n_iter == mo.n_iter and m.info()["fit_kernel"] == (1 if expect_kernel else 0)
    assert abs(m.reconstruction_err - mo.err) <= tol_of(c.dt) * mo.err and rel_max(m.components, mo.h) <= tol_of(c.dt)


def zero_violation_inputs(dt):
    """X = W0 H0 exactly, H0 H0^T and W0^T W0 diagonal (rows of H0 and columns of W0 with disjoint supports, dyadic entries): every
    gradient is exactly zero, violation_init == 0 and the fit stops at iteration 1"""
    n, d, k = 40, 32, 4
    w0, h0 = np.zeros((n, k)), np.zeros((k, d))
    for c in range(k):
        w0[c * 10:(c + 1) * 10, c] = (0.5, 1.0, 2.0, 0.25, 1.0, 4.0, 0.5, 2.0, 1.0, 0.25)
        h0[c, c * 8:(c + 1) * 8] = (1.0, 2.0, 0.5, 1.0, 0.25, 2.0, 1.0, 0.5)
    x = w0 @ h0
    return x.astype(np_dt(dt)), w0.astype(np_dt(dt)), h0.astype(np_dt(dt))


def check_zero_violation_stops_at_once(ctx, dt, expect_kernel):
    x, w0, h0 = zero_violation_inputs(dt)
    mo = model_fit(x, w0, h0, 50, 1e-4)
    assert mo.n_iter == 1 and mo.ratios == [0.0]
    m = petal.Nmf(4, max_iter=50, tol=1e-4, init="custom", ctx=ctx, solver="cd")
    w = to_numpy(m.fit_transform(x, W=w0, H=h0))
    assert m.n_iter == 1 and m.info()["fit_kernel"] == (1 if expect_kernel else 0)
    assert w.tobytes() == w0.tobytes() and m.components.tobytes() == h0.astype(np.float64).tobytes()
    assert m.reconstruction_err <= 1e-6 * np.sqrt(float((x.astype(np.float64) ** 2).sum()))


# ------------------------------------------------------------------------------------------- random initialisation, determinism, paths
def check_random_init(ctx, dt, expect_kernel):
    """the random start is the existing Pcg draw bit for bit: solver="mu" and solver="cd" report the same err_init bytes, and the
    fit equals the model started from nmf_cases.random_init"""
    n, d, k = 60, 24, 4
    x = fit_inputs(n, d, k, dt)[0]
    w0, h0 = nc.random_init(x, k, 12345)
    mo = model_fit(x, w0, h0, 2)
    fits = []
    for seed in (12345, 12345, 54321):
        m = petal.Nmf(k, max_iter=2, tol=0.0, init="random", seed=seed, ctx=ctx, solver="cd")
        w = to_numpy(m.fit_transform(x))
        fits.append((w.tobytes(), m.components.tobytes()))
        assert m.info()["fit_kernel"] == (1 if expect_kernel else 0)
        if seed == 12345:
            assert max(rel_max(w, mo.w), rel_max(m.components, mo.h), abs(m.err_init - mo.err_init) / mo.err_init) <= tol_of(dt)
            mu = petal.Nmf(k, max_iter=1, tol=0.0, init="random", seed=seed, ctx=ctx).fit(x)
            assert abs(mu.err_init - m.err_init) <= 1e-13 * m.err_init
    assert fits[0] == fits[1] and fits[0] != fits[2]


def check_same_bytes_twice(ctx, c):
    x, w0, h0, xq = fit_inputs(c.n, c.d, c.k, c.dt)
    runs = []
    for _ in range(2):
        m = make(ctx, c)
        w = to_numpy(m.fit_transform(x, W=w0, H=h0))
        runs.append((w.tobytes(), m.components.tobytes(), m.reconstruction_err, to_numpy(m.transform(xq)).tobytes()))
    assert runs[0] == runs[1]


def check_fallback_against_kernel(ctx, expect_kernel):
    """nmf_fallback = 1: the composed path; the pass and the H update agree with the default path to the bound of section B"""
    c, hc = PASS_CASES[1], H_CASES[1]
    outs, info = pass_call(ctx, c)
    houts, hinfo = h_call(ctx, hc)
    assert info["kernel"] == hinfo["kernel"] == (1 if expect_kernel else 0)
    ctx.set_option("nmf_fallback", 1)
    try:
        fouts, finfo = pass_call(ctx, c)
        fhouts, fhinfo = h_call(ctx, hc)
        fc = FIT_CASES[3]
        f = make(ctx, fc)
        x, w0, h0, xq = fit_inputs(fc.n, fc.d, fc.k, fc.dt)
        f.fit(x, W=w0, H=h0)
        f.transform(xq)
        assert finfo["kernel"] == fhinfo["kernel"] == 0 and f.info()["fit_kernel"] == 0 and f.info()["transform_kernel"] == 0
    finally:
        ctx.set_option("nmf_fallback", 0)
    mult = MULTIPLIER["device" if expect_kernel else "hostsim"] + MULTIPLIER["hostsim"]   # (each path within its own bound of the reference)
    for names, a, b, reference in ((("W", "A", "B", "violation"), outs, fouts, pass_reference(c)), (("H", "violation"), houts, fhouts, h_reference(hc))):
        for name, u, v, (ref, model, scale) in zip(names, a, b, reference):
            assert float(np.abs(np.asarray(u) - np.asarray(v)).max()) <= mult * max(model, FLOOR_EPS * EPS64 * scale), name


OUTSIDE_SHAPES = ((70, 80, 33), (70, 80, 48), (40, 520, 6))    # 33 and 48 pad to 48; 528 padded columns > 512


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
    assert max(rel_max(w, mo.w), rel_max(m.components, mo.h), rel_max(wq, model_transform(np.asarray(xq, dtype=np.float64), mo.h, 3))) <= tol
    assert abs(m.reconstruction_err - mo.err) <= tol * mo.err


def check_nothing_existing_moved(ctx, c):
    """solver="mu" and petal_nmf_fit_solver(..., 0, ...) give petal_nmf_fit's bytes"""
    x, w0, h0, xq = fit_inputs(c.n, c.d, c.k, c.dt)
    base = nc.make(ctx, c)
    wb = to_numpy(base.fit_transform(x, W=w0, H=h0))
    want = (wb.tobytes(), base.components.tobytes(), base.reconstruction_err, base.err_init, to_numpy(base.transform(xq)).tobytes())
    mu = nc.make(ctx, c, solver="mu")
    wm = to_numpy(mu.fit_transform(x, W=w0, H=h0))
    assert mu.solver == "mu" and base.solver == "mu"
    assert want == (wm.tobytes(), mu.components.tobytes(), mu.reconstruction_err, mu.err_init, to_numpy(mu.transform(xq)).tobytes())
    keep = []
    mx, mw, mh = petal.describe(np.array(x), keep), petal.describe(np.array(w0), keep), petal.describe(np.array(h0), keep)
    wo = np.zeros_like(wb)
    mo = petal.describe(wo, keep)
    spec = base._spec(c.n, c.d)
    h, solver = C.c_void_p(), C.c_int64(-1)
    ctx.check(ctx.lib.petal_nmf_fit_solver(ctx._h, C.byref(mx), c.k, C.byref(spec), petal.NMF_SOLVER_MU, C.byref(mw), C.byref(mh), 0, C.byref(h),
                                           C.byref(mo)))
    try:
        comp, err = np.zeros((c.k, c.d)), np.zeros(2)
        assert ctx.lib.petal_nmf_get(h, comp.ctypes.data_as(petal._D), None, err.ctypes.data_as(petal._D)) == petal.PETAL_OK
        assert ctx.lib.petal_nmf_get_solver(h, C.byref(solver)) == petal.PETAL_OK and solver.value == petal.NMF_SOLVER_MU
        assert (wo.tobytes(), comp.tobytes(), float(err[0]), float(err[1])) == want[:4]
    finally:
        ctx.lib.petal_nmf_destroy(h)
    assert C.sizeof(petal.petal_nmf_spec) == 48


# ------------------------------------------------------------------------------------------- errors
def check_errors(ctx, make_ctx, make_sharded_ctx):
    n, d, k = 30, 12, 3
    x, w0, h0, xq = (np.array(v) for v in fit_inputs(n, d, k, "f64"))
    inv, lin = petal.InvalidInput, petal.LinalgError

    def fit(xx=x, kk=k, w=w0, h=h0, **kw):
        args = dict(max_iter=2, tol=0.0, init="custom", ctx=ctx, solver="cd")
        args.update(kw)
        return petal.Nmf(kk, **args).fit(xx, W=w, H=h)
    for bad in ("CD", "sgd", 1, None):
        with raises_with(inv, "unknown solver"):
            petal.Nmf(k, solver=bad, ctx=ctx)
    keep = []
    mx, mw, mh = petal.describe(x, keep), petal.describe(w0, keep), petal.describe(h0, keep)
    spec, h = petal.petal_nmf_spec(2, 0.0, 0.0, 0.0, 0.0, 0.0), C.c_void_p()
    for bad in (2, -1, 7):
        with raises_with(inv, "unknown solver"):
            ctx.check(ctx.lib.petal_nmf_fit_solver(ctx._h, C.byref(mx), k, C.byref(spec), bad, C.byref(mw), C.byref(mh), 0, C.byref(h), None))
        assert not h.value
    assert ctx.lib.petal_nmf_fit_solver(ctx._h, None, k, C.byref(spec), 1, None, None, 0, C.byref(h), None) == petal.PETAL_INVALID_INPUT
    assert ctx.lib.petal_nmf_get_solver(None, None) == petal.PETAL_INVALID_INPUT
    with raises_with(inv, "kullback-leibler"):
        petal.Nmf(k, solver="cd", beta_loss="kullback-leibler", ctx=ctx)
    with raises_with(inv, "kullback-leibler"):
        petal.Nmf(k, solver="cd", beta_loss=1, dense_path="fused", ctx=ctx)

    class Csr:
        data, indices, indptr, shape = x[x > 0], np.nonzero(x > 0)[1].astype(np.int32), None, x.shape
    Csr.indptr = np.concatenate([[0], np.cumsum((x > 0).sum(axis=1))]).astype(np.int64)
    sx = petal.CsrMatrix.from_scipy_like(Csr, ctx=ctx)
    try:
        with raises_with(inv, "sparse (CSR) input"):
            fit(xx=sx)
        with raises_with(inv, "sparse (CSR) input"):
            fit(xx=Csr)
        with raises_with(inv, "CSR input"):
            fit().transform(sx)
    finally:
        sx.close()
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
        bad[which][1, 2] = np.nan
        with raises_with(lin, "did not converge"):
            fit(xx=bad[0], w=bad[1], h=bad[2])
    m = fit()
    with raises_with(inv, "# of columns should be 12"):
        m.transform(x[:, :11])
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
        petal.nmf_cd_pass(-x, w0, h0, ctx=ctx)
    with raises_with(inv, "w should be"):
        petal.nmf_cd_pass(x, w0[:5], h0, ctx=ctx)
    with raises_with(inv, "k x d"):
        petal.nmf_cd_hupdate(np.ones((3, 5)), np.ones((4, 4)), np.ones((3, 5)), ctx=ctx)
    # (the guard of petal_nmf_cd_pass runs in every call of section A; a correct kernel cannot make it fire, so its message is held to
    #  the header by the plumbing test)  A handle from another ctx is refused:
    other = make_ctx()
    try:
        with raises_with(inv, "another ctx"):
            other.check(other.lib.petal_nmf_transform(other._h, m._h, C.byref(petal.describe(xq, [])), C.byref(petal.describe(np.zeros((QUERY_ROWS, k)), []))))
    finally:
        other.close()
    other = make_sharded_ctx()
    try:
        with raises_with(inv, "sharded"):
            fit(ctx=other)
        with raises_with(inv, "sharded"):
            petal.nmf_cd_pass(x, w0, h0, ctx=other)
        with raises_with(inv, "sharded"):
            petal.nmf_cd_hupdate(np.ones((3, 5)), np.eye(3), np.ones((3, 5)), ctx=other)
    finally:
        other.close()


# ------------------------------------------------------------------------------------------- the measured ratios
def measure(ctx, label, lines):
    worst = 0.0
    for c in PASS_CASES:
        outs, info = pass_call(ctx, c)
        w, rows = ratios(("W", "A", "B", "violation"), outs, pass_reference(c))
        worst = max(worst, w)
        for name, err, model, floor, ratio in rows:
            lines.append(f"{label:8s} pass    {c.name:30s} {name:9s}  kernel {info['kernel']}  error {err:.3e}  model {model:.3e}  floor {floor:.3e}  "
                         f"ratio {ratio:.3f}")
    for c in H_CASES:
        outs, info = h_call(ctx, c)
        w, rows = ratios(("H", "violation"), outs, h_reference(c))
        worst = max(worst, w)
        for name, err, model, floor, ratio in rows:
            lines.append(f"{label:8s} hupdate {c.name:30s} {name:9s}  kernel {info['kernel']}  error {err:.3e}  model {model:.3e}  floor {floor:.3e}  "
                         f"ratio {ratio:.3f}")
    lines.append(f"{label:8s} largest ratio {worst:.3f}")
    return worst


if __name__ == "__main__":
    import hostsim
    out = ["# petal_nmf_cd_pass (W_new, A = W_new^T X, B = W_new^T W_new, the violation of the last sweeps) and petal_nmf_cd_hupdate (H_new, "
           "the violation) against numpy.longdouble; errors over the scale; ratio = error / max(model, floor).  tests/nmf_cd_cases.py "
           "MULTIPLIER = twice each path's largest ratio, rounded up."]
    if len(sys.argv) < 2 or sys.argv[1] != "--host-only":
        dev = petal.Context(0)
        measure(dev, "device", out)
        dev.close()
    host = hostsim.context()
    measure(host, "hostsim", out)
    host.close()
    out.append("tests/nmf_cd_cases.py MULTIPLIER: " + ", ".join(f"{k} {v}" for k, v in MULTIPLIER.items()))
    dst = os.path.join(ROOT, sys.argv[2] if len(sys.argv) > 2 else os.path.join("profiles", "nmf_cd_errors.txt"))
    with open(dst, "w") as f:
        f.write("\n".join(out) + "\n")
    print("\n".join(out))
