"""Nmf with the coordinate-descent solver on sparse CSR data (include/petal_hip_nmf_cd_sparse.h): the case tables with their bounds and
the checks the GPU suite (tests/test_gpu_nmf_cd_sparse.py, expect_kernel=True) and the host suite (tests/test_nmf_cd_sparse_host.py,
expect_kernel=False: every fit densifies, the sweep probe is the plain host loop) share.  The layout is nmf_sparse_cases.py's.  The
reference everywhere is the numpy model of tests/nmf_cd_cases.py (model_sweep / model_fit / model_transform, held to scikit-learn where
that is installed) applied to the densified matrix; numpy only, scipy and scikit-learn are imported nowhere.

1. petal_nmf_cd_sweep_csr on exact operands, bit for bit: nmf_sparse_cases.int_case (-1 .. 3) and tiny matrices of 1, 2, 3, 5 and 17
   rows, int_operands (F^T F = 2^s I), l1 = 3 2^s (about half of z - l1 is negative: the clamp works), l2 in {0, 2^s} -- G_new =
   max(z - l1, 0) / (2^s + l2), Gram, dot and every violation are dyadic and exact in float64 whatever the order of the sums; sweeps 2
   and 3 are fixed points with violation 0.
2. the sweep on real data against numpy.longdouble, over the error of the float64 model with a floor:

       ratio = max over G_new, Gram, dot, violation of  |out - ref| / max(|model - ref|, FLOOR_EPS eps64 scale)

   The multiplier comes from the project, not from this code: per path the larger of nmf_cd_cases.MULTIPLIER and
   nmf_sparse_cases.MULTIPLIER (the new sweep is the gather of one and the rule of the other), and the bound -- multiplier x max(model,
   floor) -- must stay below CAP = 1e-12 of the scale.  The violation is discontinuous where a coordinate lands exactly on 0, so every
   case asserts, on the long-double reference alone, that every pre-clamp value is at least MARGIN x scale away from 0; the cases carry
   their own generator seeds (SWEEP_SEEDS, found by find_sweep_seeds on the reference alone) because nmf_sparse_cases.sweep_inputs does
   not meet that everywhere.  Every row of these matrices has a stored entry (a dense row and a dense column).
3. fit / fit_transform / transform against the model at the project's parity bar, relative to the largest entry: 1e-5 for float32
   data, 1e-9 for float64.

Run as a script on a machine with the GPU it writes profiles/nmf_cd_sparse_errors.txt: the device's rows and the host simulation's."""
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
import nmf_cd_cases as cd  # noqa: E402
import nmf_sparse_cases as sp  # noqa: E402
from nmf_cases import CAP, EPS64, FLOOR_EPS, raises_with, rel_max, to_numpy, tol_of  # noqa: E402,F401
from nmf_sparse_cases import csr, int_case, int_operands  # noqa: E402
from sparse_cases import Duck, densify, to_csr  # noqa: E402
from wide_cases import np_dt  # noqa: E402

MARGIN = cd.MARGIN
MULTIPLIER = {path: max(cd.MULTIPLIER[path], sp.MULTIPLIER[path]) for path in ("device", "hostsim")}
assert MULTIPLIER == {"device": 4.0, "hostsim": 24.0}


def kernel_flag(expect_kernel):
    return 1 if expect_kernel else 0


def model_cd_sweep(xd, g, f, l1=0.0, l2=0.0, inner=1, from_zero=False, ft=np.float64, track=None):
    """(G_new, Gram, dot, violation per sweep) of the header's cd sweep of the dense image xd (R x C) in the float type ft:
    nmf_cd_cases.model_sweep on z = xd f - l1 and S = f^T f + l2 I"""
    xd, g, f = xd.astype(ft), np.array(g, dtype=ft), f.astype(ft)
    if from_zero and inner > 0:
        g[:] = 0
    z, s = xd @ f, f.T @ f + ft(l2) * np.eye(f.shape[1], dtype=ft)
    viol = np.array([cd.model_sweep(g, z - ft(l1), s, track) for _ in range(inner)], dtype=ft)
    return g, g.T @ g, (z * g).sum(), viol


# ------------------------------------------------------------------------------------------- 1. exact operands
INT_WHICH = tuple(range(-1, len(sp.INT_SHAPES)))
INT_K = sp.INT_K                                                # 1, 3, 16, 17, 33, 64
INT_INNER = (0, 1, 3)
TINY_ROWS = (1, 2, 3, 5, 17)                                    # a wave's four row groups and a workgroup's sixteen are partly empty
TINY_COLS = 40


@functools.lru_cache(maxsize=None)
def tiny_case(rows):
    """(data >= 0, indices, indptr, shape, dense float64): rows x 40 small integers at about 30 %, the last row empty where there are two"""
    rng = np.random.default_rng(400 + rows)
    x = rng.integers(1, 9, (rows, TINY_COLS)).astype(np.float64) * (rng.random((rows, TINY_COLS)) < 0.3)
    x[0, 0] = 2.0
    if rows > 1:
        x[-1, :] = 0
    data, indices, indptr = to_csr(x)
    for v in (data, indices, indptr, x):
        v.setflags(write=False)
    return data, indices, indptr, x.shape, x


def check_cd_sweep_exact(ctx, matrix, tag, dt, expect_kernel, ks=INT_K):
    """G_new, Gram, dot and every sweep's violation equal the float64 model's bytes on both images, for l2 in {0, 2^s}, inner 0, 1 and 3,
    from G and from zero; sweeps 2 and 3 are fixed points with violation 0; petal_nmf_cd_sweep_csr forms G inside a guard and raises if
    anything outside the R x k block changed"""
    data, indices, indptr, shape, dense = matrix
    sx = csr(ctx, data, indices, indptr, shape, dt)
    calls = 0
    try:
        for transposed in (False, True):
            xd = dense.T if transposed else dense
            rows, cols = xd.shape
            for k in ks:
                if k > cols:
                    continue                                    # (int_operands needs k disjoint indicator columns)
                g, f, s = int_operands(rows, cols, k, 7000 + 1000 * (tag + 1) + 10 * k + int(transposed))
                l1 = 3.0 * 2.0 ** s
                z = xd @ f - l1
                assert rows * k < 700 or ((z < 0).any() and (z > 0).any()), (tag, k)   # (the clamp works and is not all there is)
                for l2 in (0.0, 2.0 ** s):
                    for inner in INT_INNER:
                        for from_zero in ((False,) if inner == 0 else (False, True)):
                            (gn, gram, dot, viol), info = petal.nmf_cd_sweep(sx, g, f, transposed=transposed, l1=l1, l2=l2, inner_iters=inner,
                                                                              from_zero=from_zero, want_info=True)
                            mg, mgram, mdot, mv = model_cd_sweep(xd, g, f, l1, l2, inner, from_zero)
                            calls += 1
                            assert info["kernel"] == kernel_flag(expect_kernel), (tag, info)
                            what = (tag, dt, transposed, k, inner, l2, from_zero)
                            assert gn.tobytes() == mg.tobytes(), (what, "G", np.abs(gn - mg).max())
                            assert gram.tobytes() == mgram.tobytes(), (what, "Gram", np.abs(gram - mgram).max())
                            assert dot == float(mdot), (what, "dot", dot, mdot)
                            assert viol.tobytes() == mv.tobytes(), (what, "violation", viol, mv)
                            if inner == 0:
                                assert mg.tobytes() == g.tobytes()
                            if inner == 3:
                                assert mv[1] == 0 and mv[2] == 0
                                assert mg.tobytes() == (np.maximum(z, 0) / (2.0 ** s + l2)).tobytes()
                if k == ks[0]:   # without Gram and dot
                    gn, viol = petal.nmf_cd_sweep(sx, g, f, transposed=transposed, l1=l1, inner_iters=1, want_gram=False)
                    mg, _, _, mv = model_cd_sweep(xd, g, f, l1, 0.0, 1)
                    assert gn.tobytes() == mg.tobytes() and viol.tobytes() == mv.tobytes(), (tag, dt, transposed, k)
    finally:
        sx.close()
    assert calls > 0
    return calls


# ------------------------------------------------------------------------------------------- 2. real data against long double
SweepCase = namedtuple("SweepCase", "name n d k dt transposed inner l1 l2 from_zero")
SWEEP_CASES = [SweepCase(f"{dt}-{n}x{d}-k{k}-{'t' if tr else 'n'}-inner{inner}" + ("-reg" if l1 else "") + ("-zero" if fz else ""),
                         n, d, k, dt, tr, inner, l1, l2, fz)
               for (n, d, k) in sp.SWEEP_SHAPES for dt in ("f32", "f64") for tr in (False, True)
               for (inner, l1, l2) in ((1, 0.0, 0.0), (3, 0.25, 0.5)) for fz in (False, True)]
assert len(SWEEP_CASES) == 48
# The generator seed of every case: the smallest s >= 0 at which the LONG-DOUBLE REFERENCE ALONE keeps every pre-clamp value at least
# 1.5 MARGIN x scale away from 0 (find_sweep_seeds; sweep_reference asserts MARGIN itself for every case in both suites).  Cases not named: 0.
_SEEDS = {"150x700-k17-n-inner1-zero": 1, "150x700-k17-t-inner3-reg-zero": 4, "150x700-k64-n-inner3-reg": 1,
          "150x700-k64-n-inner3-reg-zero": 4, "150x700-k64-t-inner1-zero": 13, "150x700-k64-t-inner3-reg-zero": 23,
          "700x150-k5-n-inner1-zero": 3, "700x150-k5-n-inner3-reg-zero": 5, "700x150-k5-t-inner3-reg": 1,
          "700x150-k5-t-inner3-reg-zero": 1}
SWEEP_SEEDS = {f"{dt}-{name}": seed for dt in ("f32", "f64") for name, seed in _SEEDS.items()}   # (both data types at the same seed)


@functools.lru_cache(maxsize=None)
def sweep_inputs(n, d, k, dt, transposed, seed):
    """(csr triple, dense in the data's type, g, f) of a case: nmf_sparse_cases.sweep_inputs's generator with its own seed"""
    density = 0.02 + 0.04 * ((n + d + k) % 5) / 4.0              # 2 - 6 %
    x = sp.masked_planted(n, d, k + 2, n + d + k + 1000 * seed, density).astype(np_dt(dt))
    rows, cols = (d, n) if transposed else (n, d)
    rng = np.random.default_rng(31 * n + 7 * d + k + int(transposed) + 100003 * (seed + 1))
    g, f = rng.random((rows, k)) + 0.05, rng.random((cols, k)) + 0.05
    assert np.count_nonzero(x, axis=1).min() > 0 and np.count_nonzero(x, axis=0).min() > 0      # no image row without a stored entry
    for v in (x, g, f):
        v.setflags(write=False)
    return to_csr(x), x, g, f


def case_inputs(c):
    return sweep_inputs(c.n, c.d, c.k, c.dt, c.transposed, SWEEP_SEEDS.get(c.name, 0))


def reference_margin(c, seed):
    """(smallest |pre-clamp value| over the scale, the reference) of a case at a seed, from the long-double reference alone"""
    _, x, g, f = sweep_inputs(c.n, c.d, c.k, c.dt, c.transposed, seed)
    xd = x.T if c.transposed else x
    track = []
    ref = model_cd_sweep(xd, g, f, c.l1, c.l2, c.inner, c.from_zero, np.longdouble, track)
    return min(track) / float(np.abs(ref[0]).max()), ref


@functools.lru_cache(maxsize=None)
def sweep_reference(c):
    """per quantity (G_new, Gram, dot, violation): (ref in long double, |model - ref| max, scale); asserts the case's margin"""
    _, x, g, f = case_inputs(c)
    xd = x.T if c.transposed else x
    ld = np.longdouble
    margin, ref = reference_margin(c, SWEEP_SEEDS.get(c.name, 0))
    assert margin >= MARGIN, (c.name, margin)                     # no coordinate lands within the margin of the clamp
    mod = model_cd_sweep(xd, g, f, c.l1, c.l2, c.inner, c.from_zero, np.float64)
    gl = np.abs(ref[0])
    scales = (float(gl.max()), float((gl.T @ gl).max()), float(np.abs(ref[2])), float(ref[3].max()))
    return tuple((r, float(np.abs(np.asarray(m, dtype=ld) - r).max()), sc) for r, m, sc in zip(ref, mod, scales))


def find_sweep_seeds(limit=400):
    """the table SWEEP_SEEDS: per case the first seed whose reference keeps 1.5 MARGIN (a search on the reference alone)"""
    out = {}
    for c in SWEEP_CASES:
        for seed in range(limit):
            if reference_margin(c, seed)[0] >= 1.5 * MARGIN:
                break
        else:
            raise AssertionError(c.name)
        if seed:
            out[c.name] = seed
    return out


def sweep_call(ctx, c):
    (data, indices, indptr), x, g, f = case_inputs(c)
    sx = csr(ctx, data, indices, indptr, x.shape)
    try:
        return petal.nmf_cd_sweep(sx, g, f, transposed=c.transposed, l1=c.l1, l2=c.l2, inner_iters=c.inner, from_zero=c.from_zero, want_info=True)
    finally:
        sx.close()


def sweep_ratio(c, outs):
    return cd.ratios(("G", "Gram", "dot", "violation"), outs, sweep_reference(c))


def check_sweep_against_long_double(ctx, c, expect_kernel):
    outs, info = sweep_call(ctx, c)
    assert info["kernel"] == kernel_flag(expect_kernel), info
    worst, rows = sweep_ratio(c, outs)
    cd._check_rows(c.name, rows, MULTIPLIER["device" if expect_kernel else "hostsim"])   # prints every figure, then asserts
    return worst


# ------------------------------------------------------------------------------------------- 3. fits against the model
FitCase = sp.FitCase
FIT_CASES = sp.FIT_CASES                                          # 260 x 300 and 300 x 260, k in {5, 8, 33}, 1 / 3 / 10 iterations, (0.01, 0.02, 0.3)
QUERY_ROWS = sp.QUERY_ROWS
fit_inputs = sp.fit_inputs
case_penalties = sp.case_penalties


@functools.lru_cache(maxsize=None)
def fit_model(c, tol=0.0):
    x, w0, h0, _ = fit_inputs(c.n, c.d, c.k, c.dt)
    return cd.model_fit(x, w0, h0, c.max_iter, tol, case_penalties(c))


def make(ctx, c, tol=0.0, **kw):
    args = dict(max_iter=c.max_iter, tol=tol, init="custom", alpha_W=c.alpha_w, alpha_H=c.alpha_h, l1_ratio=c.l1_ratio, ctx=ctx, solver="cd",
                sparse_path="sweep")
    args.update(kw)
    return petal.Nmf(c.k, **args)


def check_fit_against_model(ctx, c, expect_kernel, duck=False):
    """W, H, reconstruction_err and err_init at the bar; n_iter; info(); kernel_path; fit_transform's W is the fit's W"""
    x, w0, h0, _ = fit_inputs(c.n, c.d, c.k, c.dt)
    mo = fit_model(c)
    data, indices, indptr = to_csr(x)
    sx = Duck(data, indices, indptr, x.shape) if duck else csr(ctx, data, indices, indptr, x.shape)
    try:
        m = make(ctx, c)
        w = m.fit_transform(sx, W=w0, H=h0)
        info = m.info()
        assert m.solver == "cd" and (info["n"], info["d"], info["k"], info["n_iter"]) == (c.n, c.d, c.k, c.max_iter) and m.n_iter == mo.n_iter
        assert info["fit_kernel"] == m.kernel_path == kernel_flag(expect_kernel) and info["transform_kernel"] == -1, (info, m.kernel_path)
        tol = tol_of(c.dt)
        got = (rel_max(w, mo.w), rel_max(m.components, mo.h), abs(m.reconstruction_err - mo.err) / mo.err,
               abs(m.err_init - mo.err_init) / mo.err_init)
        clamped = float((mo.w == 0).mean()), float((mo.h == 0).mean())
        print(f"{c.name}: W {got[0]:.2e}, H {got[1]:.2e}, err {got[2]:.2e}, err_init {got[3]:.2e} (bar {tol:.0e}); on the clamp: "
              f"{clamped[0]:.0%} of W, {clamped[1]:.0%} of H")
        assert w.dtype == np_dt(c.dt) and w.shape == (c.n, c.k) and max(got) <= tol, (c.name, got)
        f = make(ctx, c).fit(sx, W=w0, H=h0)
        assert f.components.tobytes() == m.components.tobytes() and f.reconstruction_err == m.reconstruction_err
    finally:
        if not duck:
            sx.close()
    return m


def check_transform(ctx, c, expect_kernel, updates):
    """transform of fresh sparse rows (row 3 empty) with `updates` sweeps from zero: a model fitted sparse and a model fitted dense with
    solver="cd" transform a CsrMatrix, the sparse-fitted model a dense array; inverse_transform = W H"""
    x, w0, h0, xq = fit_inputs(c.n, c.d, c.k, c.dt)
    pen = case_penalties(c)
    tol_fit = 1e6 if updates > 10 else 0.0                       # (a tolerance no fit misses: the fit stops at iteration 1, transform still runs `updates`)
    mo = cd.model_fit(x, w0, h0, updates, tol_fit, pen)
    want = cd.model_transform(np.asarray(xq, dtype=np.float64), mo.h, updates, pen)
    sx, sq = csr(ctx, *to_csr(x), x.shape), csr(ctx, *to_csr(xq), xq.shape)
    try:
        cu = c._replace(max_iter=updates)
        ms = make(ctx, cu, tol=tol_fit).fit(sx, W=w0, H=h0)
        md = make(ctx, cu, tol=tol_fit).fit(x, W=w0, H=h0)
        assert ms.n_iter == md.n_iter == mo.n_iter
        tol = tol_of(c.dt)
        wq = ms.transform(sq)
        assert ms.kernel_path == ms.info()["transform_kernel"] == kernel_flag(expect_kernel)
        wq_dense_input = ms.transform(xq)                       # the sparse-fitted model on a dense array
        wq_dense_model = md.transform(sq)                       # the dense-fitted model on a CsrMatrix
        assert md.kernel_path == kernel_flag(expect_kernel)
        got = (rel_max(wq, want), rel_max(wq_dense_input, want), rel_max(wq_dense_model, want),
               rel_max(ms.inverse_transform(wq), to_numpy(wq).astype(np.float64) @ ms.components))
        print(f"{c.name} updates {updates}: transform {got[0]:.2e}, dense input {got[1]:.2e}, dense model {got[2]:.2e}, inverse {got[3]:.2e} "
              f"(bar {tol:.0e})")
        assert wq.shape == (QUERY_ROWS, c.k) and wq.dtype == np_dt(c.dt) and max(got) <= tol, (c.name, got)
        assert not to_numpy(wq)[3].any() and not want[3].any()   # the empty row: z = 0, it stays at zero
    finally:
        sx.close()
        sq.close()


# ------------------------------------------------------------------------------------------- 4. the stopping rule
# nmf_sparse_cases.stop_inputs with tolerances of this solver's own: the model decides with every ratio at least 1 % from tol
# (check_stop_case_is_decided: nmf_cd_cases's rule).  On the model: f32 seed 34 stops at iteration 12 (ratios 5.52e-2, then 4.05e-2),
# f64 seed 16 at iteration 12 (5.24e-2, then 4.28e-2).
StopCase = sp.StopCase
STOP_CASES = [StopCase("f32-100x40-k2-seed34", 100, 40, 2, "f32", 34, 4.8e-2), StopCase("f64-100x40-k2-seed16", 100, 40, 2, "f64", 16, 4.75e-2)]
STOP_MAX_ITER = 200
stop_inputs = sp.stop_inputs


@functools.lru_cache(maxsize=None)
def check_stop_case_is_decided(c):
    mo = cd.model_fit(*stop_inputs(c), STOP_MAX_ITER, c.tol)
    assert 3 <= mo.n_iter < STOP_MAX_ITER and len(mo.ratios) == mo.n_iter, (mo.n_iter, mo.ratios)
    assert mo.ratios[-1] <= c.tol and all(abs(r - c.tol) >= 0.01 * c.tol for r in mo.ratios), (c.tol, mo.ratios)
    assert all(r > c.tol for r in mo.ratios[:-1])
    return mo


def check_stopping_rule(ctx, c, expect_kernel):
    mo = check_stop_case_is_decided(c)
    x, w0, h0 = stop_inputs(c)
    sx = csr(ctx, *to_csr(x), x.shape)
    try:
        m = petal.Nmf(c.k, max_iter=STOP_MAX_ITER, tol=c.tol, init="custom", ctx=ctx, solver="cd", sparse_path="sweep").fit(sx, W=w0, H=h0)
        print(f"{c.name}: n_iter {m.n_iter} (model {mo.n_iter}), last ratios {['%.3e' % v for v in mo.ratios[-3:]]}, tol {c.tol:g}")
        assert m.n_iter == mo.n_iter and m.kernel_path == kernel_flag(expect_kernel)
        assert abs(m.reconstruction_err - mo.err) <= tol_of(c.dt) * mo.err and rel_max(m.components, mo.h) <= tol_of(c.dt)
    finally:
        sx.close()


def check_zero_violation_stops_at_once(ctx, dt, expect_kernel):
    """nmf_cd_cases's zero-violation case as a CSR matrix: it stops at iteration 1, W0 and H0 come back byte for byte"""
    x, w0, h0 = cd.zero_violation_inputs(dt)
    mo = cd.model_fit(x, w0, h0, 50, 1e-4)
    assert mo.n_iter == 1 and mo.ratios == [0.0]
    sx = csr(ctx, *to_csr(x), x.shape)
    try:
        m = petal.Nmf(4, max_iter=50, tol=1e-4, init="custom", ctx=ctx, solver="cd", sparse_path="sweep")
        w = to_numpy(m.fit_transform(sx, W=w0, H=h0))
        assert m.n_iter == 1 and m.kernel_path == kernel_flag(expect_kernel)
        assert w.tobytes() == w0.tobytes() and m.components.tobytes() == h0.astype(np.float64).tobytes()
        assert m.reconstruction_err <= 1e-6 * np.sqrt(float((x.astype(np.float64) ** 2).sum()))
    finally:
        sx.close()


# ------------------------------------------------------------------------------------------- 5. random init, determinism, paths
def check_random_init(ctx, dt, expect_kernel):
    """init="random" equals the model started from nmf_cases.random_init; err_init equals the sparse mu fit's (the same draw)"""
    n, d, k = 260, 300, 5
    x = fit_inputs(n, d, k, dt)[0]
    w0, h0 = nc.random_init(x, k, 12345)
    mo = cd.model_fit(x, w0, h0, 2)
    sx = csr(ctx, *to_csr(x), x.shape)
    try:
        fits = []
        for seed in (12345, 12345, 54321):
            m = petal.Nmf(k, max_iter=2, tol=0.0, init="random", seed=seed, ctx=ctx, solver="cd", sparse_path="sweep")
            w = to_numpy(m.fit_transform(sx))
            fits.append((w.tobytes(), m.components.tobytes()))
            assert m.kernel_path == kernel_flag(expect_kernel)
            if seed == 12345:
                got = (rel_max(w, mo.w), rel_max(m.components, mo.h), abs(m.err_init - mo.err_init) / mo.err_init)
                print(f"random init {dt}: W {got[0]:.2e}, H {got[1]:.2e}, err_init {got[2]:.2e}")
                assert max(got) <= tol_of(dt), got
                mu = petal.Nmf(k, max_iter=1, tol=0.0, init="random", seed=seed, ctx=ctx).fit(sx)
                assert abs(mu.err_init - m.err_init) <= 1e-13 * m.err_init
        assert fits[0] == fits[1] and fits[0] != fits[2]
    finally:
        sx.close()


def fit_bytes(ctx, c, sx, xq_handle):
    x, w0, h0, _ = fit_inputs(c.n, c.d, c.k, c.dt)
    m = make(ctx, c)
    w = to_numpy(m.fit_transform(sx, W=w0, H=h0))
    return m, (w.tobytes(), m.components.tobytes(), m.reconstruction_err, m.err_init, to_numpy(m.transform(xq_handle)).tobytes())


def check_same_bytes_twice(ctx, c):
    """the same fit twice, and on a second handle built from the same arrays: W, H, the errors and the transform"""
    x, _, _, xq = fit_inputs(c.n, c.d, c.k, c.dt)
    handles = [csr(ctx, *to_csr(x), x.shape) for _ in range(2)] + [csr(ctx, *to_csr(xq), xq.shape)]
    try:
        runs = [fit_bytes(ctx, c, handles[i], handles[2])[1] for i in (0, 0, 1)]
        assert runs[0] == runs[1] == runs[2]
    finally:
        for h in handles:
            h.close()


def check_fallback_equals_dense(ctx, c):
    """a fit that densifies (the host simulation; nmf_fallback = 1 or k > 64 on a resident handle) is bit for bit Nmf(solver="cd") on
    sparse_cases.densify of the same arrays; the arrays are handed over unsorted inside their rows"""
    x, w0, h0, xq = fit_inputs(c.n, c.d, c.k, c.dt)
    data, indices, indptr = to_csr(x)
    perm = np.concatenate([np.arange(a, b)[::-1] for a, b in zip(indptr[:-1], indptr[1:])])
    sx, sq = csr(ctx, data[perm], indices[perm], indptr, x.shape), csr(ctx, *to_csr(xq), xq.shape)
    try:
        s = make(ctx, c)
        ws = s.fit_transform(sx, W=w0, H=h0)
        assert s.kernel_path == 0
        d = make(ctx, c, sparse_path="refuse")
        wd = d.fit_transform(densify(data[perm], indices[perm], indptr, x.shape), W=w0, H=h0)
        ts, td = s.transform(sq), d.transform(np.array(xq))
        assert s.kernel_path == 0
        for a, b in ((ws, wd), (s.components, d.components), (ts, td)):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
        assert (s.reconstruction_err, s.err_init, s.n_iter) == (d.reconstruction_err, d.err_init, d.n_iter)
    finally:
        sx.close()
        sq.close()
    return s


# ------------------------------------------------------------------------------------------- 6. nothing moved
def _c_fit(ctx, entry, sx, k, spec, w0, h0, extra=()):
    """(W, H, err, err_init, handle) of a C fit entry on a CsrMatrix"""
    keep = []
    mw, mh = petal.describe(np.array(w0), keep), petal.describe(np.array(h0), keep)
    wo = np.zeros((sx.shape[0], k), dtype=np.array(w0).dtype)
    mo = petal.describe(wo, keep)
    h, path = C.c_void_p(), C.c_int64(-1)
    ctx.check(entry(ctx._h, sx._handle(), k, C.byref(spec), *extra, C.byref(mw), C.byref(mh), 0, C.byref(h), C.byref(mo), C.byref(path)))
    comp, err = np.zeros((k, sx.shape[1])), np.zeros(2)
    assert ctx.lib.petal_nmf_get(h, comp.ctypes.data_as(petal._D), None, err.ctypes.data_as(petal._D)) == petal.PETAL_OK
    return (wo.tobytes(), comp.tobytes(), float(err[0]), float(err[1]), path.value), h


def check_nothing_existing_moved(ctx, c):
    """petal_nmf_fit_csr_solver(..., 0, ...) and petal_nmf_transform_csr_solver on a solver-0 handle of either loss give the bytes of
    petal_nmf_fit_csr / petal_nmf_transform_csr; sparse_path="sweep" with solver="mu" gives the mu bytes"""
    x, w0, h0, xq = fit_inputs(c.n, c.d, c.k, c.dt)
    sx, sq = csr(ctx, *to_csr(x), x.shape), csr(ctx, *to_csr(xq), xq.shape)
    try:
        spec = sp.make(ctx, c)._spec(c.n, c.d)
        base, hb = _c_fit(ctx, ctx.lib.petal_nmf_fit_csr, sx, c.k, spec, w0, h0)
        new, hn = _c_fit(ctx, ctx.lib.petal_nmf_fit_csr_solver, sx, c.k, spec, w0, h0, extra=(petal.NMF_SOLVER_MU,))
        try:
            assert base == new
            solver = C.c_int64(-1)
            assert ctx.lib.petal_nmf_get_solver(hn, C.byref(solver)) == petal.PETAL_OK and solver.value == petal.NMF_SOLVER_MU
            outs = []
            for entry in (ctx.lib.petal_nmf_transform_csr, ctx.lib.petal_nmf_transform_csr_solver):
                wq, path = np.zeros((QUERY_ROWS, c.k), dtype=np_dt(c.dt)), C.c_int64(-1)
                ctx.check(entry(ctx._h, hb, sq._handle(), C.byref(petal.describe(wq, [])), C.byref(path)))
                outs.append((wq.tobytes(), path.value))
            assert outs[0] == outs[1]
        finally:
            ctx.lib.petal_nmf_destroy(hb)
            ctx.lib.petal_nmf_destroy(hn)
        for loss in ("frobenius", "kullback-leibler"):
            runs = []
            for kw in ({}, {"sparse_path": "sweep"}, {"sparse_path": "refuse", "solver": "mu"}):
                m = sp.make(ctx, c, beta_loss=loss, **kw)
                w = to_numpy(m.fit_transform(sx, W=w0, H=h0))
                runs.append((w.tobytes(), m.components.tobytes(), m.reconstruction_err, m.err_init, to_numpy(m.transform(sq)).tobytes(), m.kernel_path))
                m.close()
            assert runs[0] == runs[1] == runs[2], loss
        assert C.sizeof(petal.petal_nmf_spec) == 48
    finally:
        sx.close()
        sq.close()


# ------------------------------------------------------------------------------------------- 7. errors
def check_errors(ctx, make_other_ctx, make_sharded_ctx):
    n, d, k = 40, 30, 3
    rng = np.random.default_rng(8)
    x = (nc.planted(n, d, k + 2, 3) * (rng.random((n, d)) < 0.3))
    x[:, 0] = 1.0
    x[0, :] = 1.0
    avg = np.sqrt(x.mean() / k)
    w0, h0 = avg * np.abs(rng.standard_normal((n, k))), avg * np.abs(rng.standard_normal((k, d)))
    data, indices, indptr = to_csr(x)
    sx = csr(ctx, data, indices, indptr, x.shape)
    inv, lin = petal.InvalidInput, petal.LinalgError

    def fit(s=sx, kk=k, w=w0, h=h0, **kw):
        args = dict(max_iter=2, tol=0.0, init="custom", ctx=ctx, solver="cd", sparse_path="sweep")
        args.update(kw)
        return petal.Nmf(kk, **args).fit(s, W=w, H=h)
    try:
        for bad in ("Sweep", "dense", 1, None):
            with raises_with(inv, "unknown sparse_path"):
                petal.Nmf(k, sparse_path=bad, ctx=ctx)
        # the default and "refuse" keep today's refusals
        for kw in ({}, {"sparse_path": "refuse"}):
            with raises_with(inv, "sparse (CSR) input"):
                petal.Nmf(k, max_iter=2, init="custom", solver="cd", ctx=ctx, **kw).fit(sx, W=w0, H=h0)
            with raises_with(inv, "sparse (CSR) input"):
                petal.Nmf(k, max_iter=2, init="custom", solver="cd", ctx=ctx, **kw).fit(Duck(data, indices, indptr, x.shape), W=w0, H=h0)
            with raises_with(inv, "CSR input"):
                petal.Nmf(k, max_iter=2, tol=0.0, init="custom", solver="cd", ctx=ctx, **kw).fit(x, W=w0, H=h0).transform(sx)
        spec = petal.petal_nmf_spec(2, 0.0, 0.0, 0.0, 0.0, 0.0)
        keep = []
        w64, h64 = petal.describe(w0, keep), petal.describe(h0, keep)
        out = C.c_void_p()
        for bad in (2, -1, 7):
            with raises_with(inv, "unknown solver"):
                ctx.check(ctx.lib.petal_nmf_fit_csr_solver(ctx._h, sx._handle(), k, C.byref(spec), bad, C.byref(w64), C.byref(h64), 0, C.byref(out),
                                                           None, None))
            assert not out.value
        assert ctx.lib.petal_nmf_fit_csr_solver(ctx._h, None, k, C.byref(spec), 1, None, None, 0, C.byref(out), None, None) == petal.PETAL_INVALID_INPUT
        with raises_with(inv, "at least 1"):
            fit(kk=0, w=w0[:, :0], h=h0[:0])
        with raises_with(inv, "every dimension should be at least 31"):
            fit(kk=31, w=np.ones((n, 31)), h=np.ones((31, d)))
        for kw in ({"alpha_W": -0.1}, {"alpha_H": -1.0}, {"tol": -1.0}):
            with raises_with(inv, "not negative"):
                fit(**kw)
        with raises_with(inv, "max_iter should be at least 1"):
            fit(max_iter=0)
        for which in range(3):
            bad = [data.copy(), w0.copy(), h0.copy()]
            bad[which].reshape(-1)[5] = -1e-3
            with raises_with(inv, "negative values in data"):
                fit(s=Duck(bad[0], indices, indptr, x.shape), w=bad[1], h=bad[2])
            for v in (np.nan, np.inf):
                bad[which].reshape(-1)[5] = v
                with raises_with(lin, "did not converge"):
                    fit(s=Duck(bad[0], indices, indptr, x.shape), w=bad[1], h=bad[2])
        with raises_with(inv, "# of columns should be 30"):
            fit(h=np.ones((k, d + 1)))
        with raises_with(inv, "w0 should be n x k"):
            fit(w=np.ones((n + 1, k)))
        # w0 / h0 / w_out of another dtype than the handle's (the facade casts: straight to the entry)
        w32, h32 = petal.describe(w0.astype(np.float32), keep), petal.describe(h0.astype(np.float32), keep)
        o32 = petal.describe(np.zeros((n, k), dtype=np.float32), keep)
        for mw, mh, mo in ((w32, h32, None), (w64, h64, o32)):
            rc = ctx.lib.petal_nmf_fit_csr_solver(ctx._h, sx._handle(), k, C.byref(spec), 1, C.byref(mw), C.byref(mh), 0, C.byref(out),
                                                  C.byref(mo) if mo is not None else None, None)
            assert rc == petal.PETAL_INVALID_INPUT and not out.value
            with raises_with(inv, "dtype"):
                ctx.check(rc)
        m = fit()
        with raises_with(inv, "# of columns should be 30"):
            m.transform(Duck(*to_csr(x[:, :-1]), (n, d - 1)))
        with raises_with(inv, "dtype"):
            m.transform(Duck(data.astype(np.float32), indices, indptr, x.shape))
        bad = data.copy()
        bad[0] = -1.0
        with raises_with(inv, "negative values in data"):
            m.transform(Duck(bad, indices, indptr, x.shape))
        bad[0] = np.nan
        with raises_with(lin, "did not converge"):
            m.transform(Duck(bad, indices, indptr, x.shape))
        assert m.transform(Duck(np.zeros(0), np.zeros(0, dtype=np.int32), np.zeros(1, dtype=np.int64), (0, d))).shape == (0, k)
        # the probe's arguments
        with raises_with(inv, "g should be"):
            petal.nmf_cd_sweep(sx, w0[:5], h0.T)
        with raises_with(inv, "g should be"):
            petal.nmf_cd_sweep(sx, h0.T, w0)                    # the operands of the other image
        with raises_with(inv, "not negative"):
            petal.nmf_cd_sweep(sx, w0, h0.T, l1=-1.0)
        with raises_with(inv, "negative parameter"):
            petal.nmf_cd_sweep(sx, w0, h0.T, inner_iters=-1)
        g1 = np.zeros((n, k))
        rc = ctx.lib.petal_nmf_cd_sweep_csr(ctx._h, sx._handle(), 0, k, w0.ctypes.data_as(petal._D), np.ascontiguousarray(h0.T).ctypes.data_as(petal._D),
                                            C.byref(spec), 1, 0, g1.ctypes.data_as(petal._D), None, g1.ctypes.data_as(petal._D), None, None)
        assert rc == petal.PETAL_INVALID_INPUT                  # dot_out without gram_out
        # a handle of another ctx, a sharded ctx
        other = make_other_ctx()
        try:
            with raises_with(inv, "another ctx"):
                fit(ctx=other)
            with raises_with(inv, "another ctx"):
                petal.Nmf(k, max_iter=2, tol=0.0, init="custom", ctx=other, solver="cd", sparse_path="sweep").fit(x, W=w0, H=h0).transform(sx)
        finally:
            other.close()
        sh = make_sharded_ctx()
        try:
            ssx = sh[1](data, indices, indptr, x.shape)
            with raises_with(inv, "sharded"):
                petal.Nmf(k, max_iter=2, tol=0.0, init="custom", ctx=sh[0], solver="cd", sparse_path="sweep").fit(ssx, W=w0, H=h0)
            with raises_with(inv, "sharded"):
                petal.nmf_cd_sweep(ssx, w0, h0.T)
        finally:
            sh[0].close()
        return m
    finally:
        sx.close()


def check_too_large_to_densify(ctx):
    """65536 x 65537 float32 is more than 2^32 bytes: the fall-back refuses it before anything is allocated"""
    rows, cols = 65536, 65537
    indptr = np.zeros(rows + 1, dtype=np.int64)
    indptr[1:] = 3
    sx = petal.CsrMatrix(np.ones(3, dtype=np.float32), np.array([0, 5, 9], dtype=np.int32), indptr, (rows, cols), ctx=ctx)
    try:
        ctx.set_option("nmf_fallback", 1)
        try:
            with raises_with(petal.InvalidInput, "too large to densify"):
                petal.Nmf(2, max_iter=1, init="random", ctx=ctx, solver="cd", sparse_path="sweep").fit(sx)
        finally:
            ctx.set_option("nmf_fallback", 0)
    finally:
        sx.close()


# ------------------------------------------------------------------------------------------- the measured ratios
def measure(ctx, label, lines):
    worst = 0.0
    for c in SWEEP_CASES:
        outs, info = sweep_call(ctx, c)
        w, rows = sweep_ratio(c, outs)
        worst = max(worst, w)
        for name, err, model, floor, ratio in rows:
            lines.append(f"{label:8s} {c.name:40s} {name:9s}  kernel {info['kernel']}  error {err:.3e}  model {model:.3e}  floor {floor:.3e}  "
                         f"ratio {ratio:.3f}")
    lines.append(f"{label:8s} largest ratio {worst:.3f}")
    return worst


if __name__ == "__main__":
    import hostsim
    if len(sys.argv) > 1 and sys.argv[1] == "--find-seeds":
        print(find_sweep_seeds())
        sys.exit(0)
    out = ["# petal_nmf_cd_sweep_csr against numpy.longdouble: G_new, Gram = G_new^T G_new, dot = sum_r <z_r, g_r>, the violation of every "
           "sweep; errors over the scale; ratio = error / max(model, floor).  The bound of tests/nmf_cd_sparse_cases.py is the project's: per "
           "path the larger of nmf_cd_cases.MULTIPLIER and nmf_sparse_cases.MULTIPLIER."]
    if len(sys.argv) < 2 or sys.argv[1] != "--host-only":
        dev = petal.Context(0)
        measure(dev, "device", out)
        dev.close()
    host = hostsim.context()
    measure(host, "hostsim", out)
    host.close()
    out.append("tests/nmf_cd_sparse_cases.py MULTIPLIER: " + ", ".join(f"{k} {v}" for k, v in MULTIPLIER.items()))
    dst = os.path.join(ROOT, sys.argv[2] if len(sys.argv) > 2 else os.path.join("profiles", "nmf_cd_sparse_errors.txt"))
    with open(dst, "w") as f:
        f.write("\n".join(out) + "\n")
    print("\n".join(out))
