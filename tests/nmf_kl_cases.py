"""Nmf with the Kullback-Leibler loss on sparse CSR data (include/petal_hip_nmf_kl.h): a numpy model of the header's statement, the
generators, the case tables with their bounds, and the checks the GPU suite (tests/test_gpu_nmf_kl.py, expect_kernel=True: k_nmf_kl_sweep)
and the host suite (tests/test_nmf_kl_host.py, expect_kernel=False: the same driver over the plain host loop) share.  The reference is
the model here in numpy.longdouble or float64 -- never the library, never scikit-learn; numpy only, scipy is imported nowhere.  The
generators are those of nmf_cases.py, nmf_sparse_cases.py and sparse_cases.py.

1. petal_nmf_kl_sweep_csr on exact operands, bit for bit: X holds small non-negative integers, F has disjoint 0/1 indicator columns with
   2^s ones each (colsum(F) = 2^s), G has entries in {0, 1/4, 1/2, 1, 2, 4}.  Every wh is one entry of g_r or 0 (clamped to 2^-23),
   every quotient a power-of-two scaling, every sum one of small dyadic numbers: G_new and colsum(G_new) are exact in float64 whatever
   the order of the sums (check_sweep_exact asserts float64 == long double on the model before it compares bytes).  inner = 3 is not
   exact (the second quotient is not dyadic): one call with inner = 3 equals three chained calls with inner = 1, bit for bit.
2. the sweep on real data against numpy.longdouble, expressed over the error of the float64 model with a floor:

       ratio = max over G_new, colsum (inner > 0) or term (inner = 0) of  |out - ref| / max(|model - ref|, FLOOR_EPS eps64 scale)

   scale = the largest sum of absolute terms of the quantity.  MULTIPLIER is, per path, twice the largest ratio measured there, rounded
   up (profiles/nmf_kl_errors.txt), and the bound -- multiplier x max(model, floor) -- must stay below CAP = 1e-12 of the scale.
3. fit / fit_transform / transform against model_fit / model_transform at the project's parity bar, relative to the largest entry:
   1e-5 for float32 data, 1e-9 for float64.

Run as a script on a machine with the GPU it writes profiles/nmf_kl_errors.txt: the device's rows and the host simulation's."""
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
import nmf_sparse_cases as ns  # noqa: E402
from nmf_cases import Fit, raises_with, rel_max, tol_of, to_numpy  # noqa: E402
from nmf_sparse_cases import FitCase, SweepCase, csr, fit_inputs, int_case, int_operands, sweep_inputs  # noqa: E402
from sparse_cases import Duck, ITEM_NNZ, to_csr  # noqa: E402
from wide_cases import np_dt  # noqa: E402

EPS = nc.EPS
EPS64 = nc.EPS64
FLOOR_EPS = nc.FLOOR_EPS
CAP = nc.CAP
KL = "kullback-leibler"


# ------------------------------------------------------------------------------------------- the model
def transposed_triple(data, indices, indptr, shape):
    """the CSR triple of the transposed image as the handle builds it: a stable counting sort over the column indices"""
    rows = np.repeat(np.arange(shape[0]), np.diff(indptr))
    order = np.argsort(indices, kind="stable")
    ptr = np.zeros(shape[1] + 1, dtype=np.int64)
    np.cumsum(np.bincount(indices, minlength=shape[1]), out=ptr[1:])
    return data[order], rows[order].astype(np.int32), ptr


def image_of(triple, shape, transposed):
    """(data, indices, indptr, R, C) of the image a sweep runs on"""
    data, indices, indptr = triple
    if transposed:
        return transposed_triple(data, indices, indptr, shape) + (shape[1], shape[0])
    return data, indices, indptr, shape[0], shape[1]


def model_kl_sweep(image, g, f, l1=0.0, l2=0.0, inner=1, ft=np.float64, g_const=None):
    """(G_new, colsum(G_new), term) of the header's sweep in the float type ft; term is None unless inner == 0.  g_const: G starts as
    that constant (transform)."""
    data, indices, indptr, R, _ = image
    data, f = data.astype(ft), f.astype(ft)
    g = np.full((R, f.shape[1]), ft(g_const), dtype=ft) if g_const is not None else g.astype(ft)
    rows = np.repeat(np.arange(R), np.diff(indptr))
    eps, c, fi = ft(EPS), f.sum(axis=0), f[indices]
    term = None
    for _ in range(max(inner, 1)):
        wh = (g[rows] * fi).sum(axis=1)
        wh[wh < eps] = eps
        if inner == 0:
            m = data > eps
            term = (data[m] * np.log(data[m] / wh[m])).sum()
            break
        num = np.zeros_like(g)
        np.add.at(num, rows, (data / wh)[:, None] * fi)
        den = (c + ft(l1)) + ft(l2) * g
        den[den == 0] = eps
        g = g * (num / den)
    return g, g.sum(axis=0), term


def model_loss(term, csw, rsh, xsum):
    return float(np.sqrt(2.0 * max(0.0, float(term) + float(csw @ rsh) - xsum)))


def model_fit(x, w0, h0, max_iter, tol=0.0, pen=(0.0, 0.0, 0.0, 0.0)):
    """the header's fit on the CSR of the non-zero entries of x, float64; checks = the deciding quantity at every check"""
    triple = to_csr(x)
    img0, img1 = image_of(triple, x.shape, False), image_of(triple, x.shape, True)
    w, ht = np.array(w0, dtype=np.float64), np.array(h0, dtype=np.float64).T.copy()
    l1w, l2w, l1h, l2h = pen
    vals = triple[0].astype(np.float64)
    xsum = float(vals[vals > EPS].sum())

    def loss():
        _, csw, term = model_kl_sweep(img0, w, ht, inner=0)
        return model_loss(term, csw, ht.sum(axis=0), xsum)
    err_init = loss()
    prev, checks, n_iter, err, read = err_init, [], max_iter, err_init, False
    for it in range(1, max_iter + 1):
        w = model_kl_sweep(img0, w, ht, l1w, l2w, 1)[0]
        ht = model_kl_sweep(img1, ht, w, l1h, l2h, 1)[0]
        read = False
        if tol > 0 and it % 10 == 0:
            err, read = loss(), True
            checks.append((prev - err) / err_init)
            if checks[-1] < tol:
                n_iter = it
                break
            prev = err
    if not read:
        err = loss()
    return Fit(w, ht.T.copy(), n_iter, err, err_init, checks)


def model_transform(xq, h, k, max_iter, pen=(0.0, 0.0, 0.0, 0.0)):
    img = image_of(to_csr(xq), xq.shape, False)
    w0 = np.sqrt(xq.astype(np.float64).mean() / k)
    return model_kl_sweep(img, None, np.asarray(h, dtype=np.float64).T.copy(), pen[0], pen[1], max_iter, g_const=w0)[0]


# ------------------------------------------------------------------------------------------- 1. exact operands
INT_SHAPES = ns.INT_SHAPES
INT_K = ns.INT_K


def check_sweep_exact(ctx, which, dt, expect_kernel, ks=INT_K):
    """G_new and colsum(G_new) equal the model's bit for bit on both images, with l1 = 0 and l1 = 2^s (den = 2^s or 2^(s+1));
    petal_nmf_kl_sweep_csr forms G inside a guard and raises if anything outside the R x k block changed"""
    data, indices, indptr, shape, _ = int_case(which)
    sx = csr(ctx, data, indices, indptr, shape, dt)
    try:
        for transposed in (False, True):
            image = image_of((data, indices, indptr), shape, transposed)
            rows, cols = image[3], image[4]
            for k in ks:
                g, f, s = int_operands(rows, cols, k, 1000 * (which + 1) + 10 * k + int(transposed))
                for l1 in (0.0, 2.0 ** s):
                    mg, mc, _ = model_kl_sweep(image, g, f, l1, 0.0, 1)
                    lg, lc, _ = model_kl_sweep(image, g, f, l1, 0.0, 1, np.longdouble)
                    # the construction is exact: float64 equals long double (so the order of the sums cannot matter)
                    assert np.array_equal(mg.astype(np.longdouble), lg) and np.array_equal(mc.astype(np.longdouble), lc), (which, k, l1)
                    (gn, cs), info = petal.nmf_kl_sweep(sx, g, f, transposed=transposed, l1=l1, inner_iters=1, want_info=True)
                    assert info["kernel"] == (1 if expect_kernel else 0), (which, info)
                    what = (which, dt, transposed, k, l1)
                    assert gn.tobytes() == mg.tobytes(), (what, "G", np.abs(gn - mg).max())
                    assert cs.tobytes() == mc.tobytes(), (what, "colsum", np.abs(cs - mc).max())
    finally:
        sx.close()


def split_rows(which, transposed):
    """does the image have rows of more than ITEM_NNZ stored entries (rows the handle splits into several work items)?"""
    data, indices, indptr, shape, _ = int_case(which)
    return int(np.diff(image_of((data, indices, indptr), shape, transposed)[2]).max()) > ITEM_NNZ


def check_inner_is_chained_single_updates(ctx, which, dt, expect_kernel, ks=(3, 17, 64), inner=3):
    """one call with inner = 3 equals three chained calls with inner = 1, bit for bit, on both images"""
    data, indices, indptr, shape, _ = int_case(which)
    sx = csr(ctx, data, indices, indptr, shape, dt)
    try:
        for transposed in (False, True):
            image = image_of((data, indices, indptr), shape, transposed)
            for k in ks:
                g, f, s = int_operands(image[3], image[4], k, 77 * (which + 2) + k + int(transposed))
                (g3, c3), info = petal.nmf_kl_sweep(sx, g, f, transposed=transposed, l1=0.5, l2=0.25, inner_iters=inner, want_info=True)
                assert info["kernel"] == (1 if expect_kernel else 0)
                g1 = g
                for _ in range(inner):
                    g1, c1 = petal.nmf_kl_sweep(sx, g1, f, transposed=transposed, l1=0.5, l2=0.25, inner_iters=1)
                assert g3.tobytes() == g1.tobytes() and c3.tobytes() == c1.tobytes(), (which, dt, transposed, k)
                mg = model_kl_sweep(image, g, f, 0.5, 0.25, inner)[0]
                assert rel_max(g3, mg) <= 1e-12, (which, transposed, k)
    finally:
        sx.close()


# ------------------------------------------------------------------------------------------- 2. real data against long double
SWEEP_SHAPES = ns.SWEEP_SHAPES
SWEEP_CASES = [SweepCase(f"{dt}-{n}x{d}-k{k}-{'t' if tr else 'n'}-inner{inner}" + ("-reg" if l1 else ""), n, d, k, dt, tr, inner, l1, l2)
               for (n, d, k) in SWEEP_SHAPES for dt in ("f32", "f64") for tr in (False, True)
               for (inner, l1, l2) in ((1, 0.0, 0.0), (3, 0.25, 0.5), (0, 0.0, 0.0))]
# twice the largest measured ratio, rounded up (profiles/nmf_kl_errors.txt: 0.773 on the device, 2.365 on the host simulation, whose
# loop adds the terms of the loss one after the other)
MULTIPLIER = {"device": 2.0, "hostsim": 5.0}


@functools.lru_cache(maxsize=None)
def sweep_reference(c):
    """per quantity (G_new and colsum, or term): (ref in long double, |model - ref| max, scale)"""
    triple, x, g, f = sweep_inputs(c.n, c.d, c.k, c.dt, c.transposed)
    image = image_of(triple, x.shape, c.transposed)
    ld = np.longdouble
    ref = model_kl_sweep(image, g, f, c.l1, c.l2, c.inner, ld)
    mod = model_kl_sweep(image, g, f, c.l1, c.l2, c.inner, np.float64)
    if c.inner == 0:
        # the scale of the term: the sum of the absolute values of its terms
        data, indices, indptr, R, _ = image
        rows = np.repeat(np.arange(R), np.diff(indptr))
        wh = np.maximum((g[rows].astype(ld) * f[indices].astype(ld)).sum(axis=1), ld(EPS))
        v = data.astype(ld)
        scale = float(np.abs(v * np.log(v / wh))[v > EPS].sum())
        return ((ref[2], float(abs(ld(mod[2]) - ref[2])), scale),)
    scales = (float(np.abs(ref[0]).max()), float(np.abs(ref[1]).max()))       # (every term of a column sum is non-negative)
    return tuple((r, float(np.abs(np.asarray(m, dtype=ld) - r).max()), sc) for r, m, sc in zip(ref[:2], mod[:2], scales))


def sweep_call(ctx, c):
    (data, indices, indptr), x, g, f = sweep_inputs(c.n, c.d, c.k, c.dt, c.transposed)
    sx = csr(ctx, data, indices, indptr, x.shape)
    try:
        out, info = petal.nmf_kl_sweep(sx, g, f, transposed=c.transposed, l1=c.l1, l2=c.l2, inner_iters=c.inner, want_info=True)
        if c.inner == 0:
            assert out[0].tobytes() == np.ascontiguousarray(g).tobytes()           # G is left alone
            return (out[2],), info
        return out, info
    finally:
        sx.close()


def sweep_ratio(c, outs):
    """(largest ratio, rows of (name, error / scale, model / scale, floor / scale, ratio))"""
    rows, worst = [], 0.0
    names = ("term",) if c.inner == 0 else ("G", "colsum")
    for name, out, (ref, model, scale) in zip(names, outs, sweep_reference(c)):
        err = float(np.abs(np.asarray(out, dtype=np.longdouble) - ref).max())
        floor = FLOOR_EPS * EPS64 * scale
        ratio = err / max(model, floor)
        worst = max(worst, ratio)
        rows.append((name, err / scale, model / scale, floor / scale, ratio))
    return worst, rows


def check_sweep_against_long_double(ctx, c, expect_kernel):
    outs, info = sweep_call(ctx, c)
    assert info["kernel"] == (1 if expect_kernel else 0), info
    mult = MULTIPLIER["device" if expect_kernel else "hostsim"]
    worst, rows = sweep_ratio(c, outs)
    for name, err, model, floor, ratio in rows:
        bound = mult * max(model, floor)
        print(f"{c.name} {name}: error {err:.3e}, model {model:.3e}, floor {floor:.3e} of the scale; ratio {ratio:.3f}, bound {bound:.3e} "
              f"(cap {CAP:.0e})")
        assert bound <= CAP, (c.name, name, bound)
        assert err <= bound, (c.name, name, ratio)
    return worst


# ------------------------------------------------------------------------------------------- 3. fits against the model
FIT_SHAPES = ns.FIT_SHAPES
FIT_K = ns.FIT_K
FIT_CASES = list(ns.FIT_CASES)          # 260 x 300 and 300 x 260, k in {5, 8, 33}, both dtypes, 1 / 3 / 10 iterations, one regularised case per dtype
QUERY_ROWS = ns.QUERY_ROWS


def case_penalties(c):
    return nc.penalties(c.n, c.d, c.alpha_w, c.alpha_h, c.l1_ratio)


@functools.lru_cache(maxsize=None)
def fit_model(c, tol=0.0):
    x, w0, h0, _ = fit_inputs(c.n, c.d, c.k, c.dt)
    return model_fit(x, w0, h0, c.max_iter, tol, case_penalties(c))


def make(ctx, c, tol=0.0, **kw):
    return petal.Nmf(c.k, max_iter=c.max_iter, tol=tol, init="custom", alpha_W=c.alpha_w, alpha_H=c.alpha_h, l1_ratio=c.l1_ratio, ctx=ctx,
                     beta_loss=KL, **kw)


def check_fit_against_model(ctx, c, expect_kernel, duck=False):
    """W, H, reconstruction_err and err_init at the bar; n_iter; info(); kernel_path; fit gives fit_transform's bytes"""
    x, w0, h0, _ = fit_inputs(c.n, c.d, c.k, c.dt)
    mo = fit_model(c)
    data, indices, indptr = to_csr(x)
    sx = Duck(data, indices, indptr, x.shape) if duck else csr(ctx, data, indices, indptr, x.shape)
    try:
        m = make(ctx, c)
        w = m.fit_transform(sx, W=w0, H=h0)
        info = m.info()
        assert m.beta_loss == KL and m._model_loss() == petal.NMF_LOSS_KL
        assert (info["n"], info["d"], info["k"], info["n_iter"]) == (c.n, c.d, c.k, c.max_iter) and m.n_iter == mo.n_iter
        assert info["fit_kernel"] == m.kernel_path == (1 if expect_kernel else 0) and info["transform_kernel"] == -1, (info, m.kernel_path)
        tol = tol_of(c.dt)
        got = (rel_max(w, mo.w), rel_max(m.components, mo.h), abs(m.reconstruction_err - mo.err) / mo.err,
               abs(m.err_init - mo.err_init) / mo.err_init)
        print(f"{c.name}: W {got[0]:.2e}, H {got[1]:.2e}, err {got[2]:.2e}, err_init {got[3]:.2e} (bar {tol:.0e})")
        assert w.dtype == np_dt(c.dt) and w.shape == (c.n, c.k) and max(got) <= tol, (c.name, got)
        f = make(ctx, c).fit(sx, W=w0, H=h0)
        assert f.components.tobytes() == m.components.tobytes() and f.reconstruction_err == m.reconstruction_err
    finally:
        if not duck:
            sx.close()
    return m


# ------------------------------------------------------------------------------------------- 4. transform
def check_transform(ctx, c, expect_kernel, updates):
    """transform of QUERY_ROWS fresh sparse rows (row 3 empty: a zero row) with `updates` updates: the fit stops at its first check (a
    tolerance no fit misses), transform still runs max_iter = updates; a dense numpy array goes through the Python compression and gives
    the bytes of the CSR of its non-zero entries; inverse_transform works unchanged"""
    x, w0, h0, xq = fit_inputs(c.n, c.d, c.k, c.dt)
    fit_iter = min(updates, 10)
    pen = case_penalties(c)
    mo = model_fit(x, w0, h0, fit_iter, 0.0, pen)
    want = model_transform(xq, mo.h, c.k, updates, pen)
    sx, sq = csr(ctx, *to_csr(x), x.shape), csr(ctx, *to_csr(xq), xq.shape)
    try:
        m = petal.Nmf(c.k, max_iter=updates, tol=1e6 if updates > 10 else 0.0, init="custom", alpha_W=c.alpha_w, alpha_H=c.alpha_h,
                      l1_ratio=c.l1_ratio, ctx=ctx, beta_loss=KL).fit(sx, W=w0, H=h0)
        assert m.n_iter == fit_iter
        wq = m.transform(sq)
        assert m.kernel_path == m.info()["transform_kernel"] == (1 if expect_kernel else 0)
        wd = m.transform(np.array(xq))
        tol = tol_of(c.dt)
        got = (rel_max(wq, want), rel_max(m.inverse_transform(wq), to_numpy(wq).astype(np.float64) @ m.components))
        print(f"{c.name} updates {updates}: transform {got[0]:.2e}, inverse {got[1]:.2e} (bar {tol:.0e})")
        assert wq.shape == (QUERY_ROWS, c.k) and wq.dtype == np_dt(c.dt) and max(got) <= tol, (c.name, got)
        assert wd.dtype == wq.dtype and wd.tobytes() == wq.tobytes()
        assert not to_numpy(wq)[3].any()                        # the empty row
    finally:
        sx.close()
        sq.close()


# ------------------------------------------------------------------------------------------- 5. the stopping rule
# One case per dtype, found by a seed search with the model: it stops at a check between iteration 20 and 60 with the deciding quantity a
# factor of 2 or more away from tol at the stopping check and at every check before it (check_stop_case_is_decided verifies that).
StopCase = namedtuple("StopCase", "name n d k dt seed tol")
STOP_CASES = [StopCase("f32-100x40-k2-seed0", 100, 40, 2, "f32", 0, 3.8e-3), StopCase("f64-100x40-k2-seed1", 100, 40, 2, "f64", 1, 4.2e-2)]
STOP_MAX_ITER = 200


@functools.lru_cache(maxsize=None)
def stop_inputs(c):
    return ns.stop_inputs(c)


@functools.lru_cache(maxsize=None)
def check_stop_case_is_decided(c):
    """nmf_cases.check_stop_case_is_decided's conditions with this module's model"""
    mo = model_fit(*stop_inputs(c), STOP_MAX_ITER, c.tol)
    assert 20 <= mo.n_iter <= 60 and len(mo.checks) == mo.n_iter // 10, (mo.n_iter, mo.checks)
    assert mo.checks[-1] <= c.tol / 2 and mo.checks[-2] >= 2 * c.tol and min(mo.checks[:-1]) >= 2 * c.tol, (c.tol, mo.checks)
    return mo


def check_stopping_rule(ctx, c, expect_kernel):
    mo = check_stop_case_is_decided(c)
    x, w0, h0 = stop_inputs(c)
    sx = csr(ctx, *to_csr(x), x.shape)
    try:
        m = petal.Nmf(c.k, max_iter=STOP_MAX_ITER, tol=c.tol, init="custom", ctx=ctx, beta_loss=KL).fit(sx, W=w0, H=h0)
        print(f"{c.name}: n_iter {m.n_iter} (model {mo.n_iter}), checks {['%.2e' % v for v in mo.checks]}, tol {c.tol:g}")
        assert m.n_iter == mo.n_iter and m.kernel_path == (1 if expect_kernel else 0)
        assert abs(m.reconstruction_err - mo.err) <= tol_of(c.dt) * mo.err and rel_max(m.components, mo.h) <= tol_of(c.dt)
    finally:
        sx.close()


# ------------------------------------------------------------------------------------------- 6. random initialisation, determinism, dense input
def check_random_init(ctx, dt, expect_kernel):
    """init="random" gives nmf_cases.random_init's W0 / H0 stream"""
    n, d, k = 260, 300, 5
    x = fit_inputs(n, d, k, dt)[0]
    w0, h0 = nc.random_init(x, k, 12345)
    mo = model_fit(x, w0, h0, 1)
    sx = csr(ctx, *to_csr(x), x.shape)
    try:
        fits = []
        for seed in (12345, 12345, 54321):
            m = petal.Nmf(k, max_iter=1, tol=0.0, init="random", seed=seed, ctx=ctx, beta_loss=KL)
            w = to_numpy(m.fit_transform(sx))
            fits.append((w.tobytes(), m.components.tobytes()))
            assert m.kernel_path == (1 if expect_kernel else 0)
            if seed == 12345:
                got = (rel_max(w, mo.w), rel_max(m.components, mo.h), abs(m.err_init - mo.err_init) / mo.err_init)
                print(f"random init {dt}: W {got[0]:.2e}, H {got[1]:.2e}, err_init {got[2]:.2e}")
                assert max(got) <= tol_of(dt), got
        assert fits[0] == fits[1] and fits[0] != fits[2]
    finally:
        sx.close()


def fit_bytes(ctx, c, x_in, xq_in, **kw):
    _, w0, h0, _ = fit_inputs(c.n, c.d, c.k, c.dt)
    m = make(ctx, c, **kw)
    w = to_numpy(m.fit_transform(x_in, W=w0, H=h0))
    return m, (w.tobytes(), m.components.tobytes(), m.reconstruction_err, m.err_init, to_numpy(m.transform(xq_in)).tobytes())


def check_same_bytes_twice(ctx, c):
    """the same fit twice, and on a second handle built from the same arrays"""
    x, _, _, xq = fit_inputs(c.n, c.d, c.k, c.dt)
    handles = [csr(ctx, *to_csr(x), x.shape) for _ in range(2)] + [csr(ctx, *to_csr(xq), xq.shape)]
    try:
        runs = [fit_bytes(ctx, c, handles[i], handles[2])[1] for i in (0, 0, 1)]
        assert runs[0] == runs[1] == runs[2]
    finally:
        for h in handles:
            h.close()


def check_dense_input_is_the_csr_of_its_nonzeros(ctx, c, expect_kernel):
    """dense numpy input with this loss gives the bytes of the CSR fit of to_csr(x) and takes the same path"""
    x, _, _, xq = fit_inputs(c.n, c.d, c.k, c.dt)
    sx, sq = csr(ctx, *to_csr(x), x.shape), csr(ctx, *to_csr(xq), xq.shape)
    try:
        ms, sparse = fit_bytes(ctx, c, sx, sq)
        md, dense = fit_bytes(ctx, c, np.array(x), np.array(xq))
        assert sparse == dense and md.kernel_path == ms.kernel_path == (1 if expect_kernel else 0)
    finally:
        sx.close()
        sq.close()


def check_explicit_frobenius_changes_nothing(ctx, c):
    """beta_loss="frobenius" (and 2) given explicitly: the bytes of the same call without the argument, dense and CSR"""
    x, w0, h0, xq = fit_inputs(c.n, c.d, c.k, c.dt)
    sx = csr(ctx, *to_csr(x), x.shape)
    try:
        for x_in, xq_in in ((np.array(x), np.array(xq)), (sx, Duck(*to_csr(xq), xq.shape))):
            runs = []
            for kw in ({}, {"beta_loss": "frobenius"}, {"beta_loss": 2}):
                m = petal.Nmf(c.k, max_iter=c.max_iter, tol=0.0, init="custom", ctx=ctx, **kw)
                w = to_numpy(m.fit_transform(x_in, W=w0, H=h0))
                assert m.beta_loss == "frobenius" and m._model_loss() == petal.NMF_LOSS_FROBENIUS
                runs.append((w.tobytes(), m.components.tobytes(), m.reconstruction_err, m.err_init, m.n_iter,
                             to_numpy(m.transform(xq_in)).tobytes()))
            assert runs[0] == runs[1] == runs[2]
    finally:
        sx.close()


# ------------------------------------------------------------------------------------------- 8. errors
def check_errors(ctx, make_other_ctx, make_sharded_ctx):
    n, d, k = 80, 70, 3
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
        args = dict(max_iter=2, tol=0.0, init="custom", ctx=ctx, beta_loss=KL)
        args.update(kw)
        return petal.Nmf(kk, **args).fit(s, W=w, H=h)
    try:
        for bad in ("itakura-saito", 0, 0.5, 3, None, True):
            with raises_with(inv, "unknown beta_loss"):
                petal.Nmf(k, beta_loss=bad, ctx=ctx)
        assert petal.Nmf(k, beta_loss=1, ctx=ctx).beta_loss == KL and petal.Nmf(k, ctx=ctx).beta_loss == "frobenius"
        with raises_with(inv, "kullback-leibler takes at most 64 components"):
            fit(kk=65, w=np.ones((n, 65)), h=np.ones((65, d)))
        with raises_with(inv, "every dimension should be at least 71"):
            fit(kk=71, w=np.ones((n, 71)), h=np.ones((71, d)))
        import ctypes as C
        spec = petal.petal_nmf_spec(2, 0.0, 0.0, 0.0, 0.0, 0.0)
        keep = []
        w64, h64 = petal.describe(w0, keep), petal.describe(h0, keep)
        out = C.c_void_p()
        for loss in (2, -1):                                    # any other value than 0 or 1
            rc = ctx.lib.petal_nmf_fit_csr_loss(ctx._h, sx._handle(), k, C.byref(spec), loss, C.byref(w64), C.byref(h64), 0, C.byref(out), None, None)
            assert rc == petal.PETAL_INVALID_INPUT and not out.value
            with raises_with(inv, "unknown loss"):
                ctx.check(rc)
        # term_out with inner_iters > 0
        g1, c1, t1 = np.zeros((n, k)), np.zeros(k), np.zeros(1)
        ft = np.ascontiguousarray(h0.T)
        rc = ctx.lib.petal_nmf_kl_sweep_csr(ctx._h, sx._handle(), 0, k, w0.ctypes.data_as(petal._D), ft.ctypes.data_as(petal._D), C.byref(spec), 1,
                                            g1.ctypes.data_as(petal._D), c1.ctypes.data_as(petal._D), t1.ctypes.data_as(petal._D), None)
        assert rc == petal.PETAL_INVALID_INPUT
        with raises_with(inv, "term_out"):
            ctx.check(rc)
        with raises_with(inv, "term_out"):
            petal.nmf_kl_sweep(sx, w0, ft, inner_iters=2, want_term=True)
        with raises_with(inv, "g should be"):
            petal.nmf_kl_sweep(sx, w0[:5], ft)
        with raises_with(inv, "not negative"):
            petal.nmf_kl_sweep(sx, w0, ft, l1=-1.0)
        with raises_with(inv, "negative parameter"):
            petal.nmf_kl_sweep(sx, w0, ft, inner_iters=-1)
        # the dense C entry on a model of this loss
        m = fit()
        mq = petal.describe(np.array(x), keep)
        mo = petal.describe(np.zeros((n, k)), keep)
        rc = ctx.lib.petal_nmf_transform(ctx._h, m._handle(), C.byref(mq), C.byref(mo))
        assert rc == petal.PETAL_INVALID_INPUT
        with raises_with(inv, "kullback-leibler"):
            ctx.check(rc)
        # stored values: the existing messages
        for which in range(3):
            bad = [data.copy(), w0.copy(), h0.copy()]
            bad[which].reshape(-1)[5] = -1e-3
            with raises_with(inv, "negative values in data"):
                fit(s=Duck(bad[0], indices, indptr, x.shape), w=bad[1], h=bad[2])
            for v in (np.nan, np.inf):
                bad[which].reshape(-1)[5] = v
                with raises_with(lin, "did not converge"):
                    fit(s=Duck(bad[0], indices, indptr, x.shape), w=bad[1], h=bad[2])
        bad = data.copy()
        bad[0] = -1.0
        with raises_with(inv, "negative values in data"):
            m.transform(Duck(bad, indices, indptr, x.shape))
        bad[0] = np.nan
        with raises_with(lin, "did not converge"):
            m.transform(Duck(bad, indices, indptr, x.shape))
        with raises_with(inv, f"# of columns should be {d}"):
            m.transform(Duck(*to_csr(x[:, :-1]), (n, d - 1)))
        assert m.transform(Duck(np.zeros(0), np.zeros(0, dtype=np.int32), np.zeros(1, dtype=np.int64), (0, d))).shape == (0, k)
        # explicit zeros contribute nothing; an all-zero matrix gives zero factors and a zero loss
        zero = Duck(np.zeros(0), np.zeros(0, dtype=np.int32), np.zeros(n + 1, dtype=np.int64), (n, d))
        mz = petal.Nmf(k, max_iter=2, tol=0.0, init="random", ctx=ctx, beta_loss=KL)
        assert not mz.fit_transform(zero).any() and mz.reconstruction_err == 0.0
        withz = Duck(np.concatenate([data, [0.0]]), np.concatenate([indices, [d - 1]]).astype(np.int32),
                     np.concatenate([indptr[:-1], [indptr[-1] + 1]]), x.shape)
        assert x[n - 1, d - 1] == 0.0
        a, b = fit(), fit(s=withz)
        assert a.components.tobytes() == b.components.tobytes() and a.reconstruction_err == b.reconstruction_err
        # a handle of another ctx, a closed one, a sharded ctx
        other = make_other_ctx()
        try:
            with raises_with(inv, "another ctx"):
                fit(ctx=other)
            with raises_with(inv, "another ctx"):
                petal.Nmf(k, max_iter=2, tol=0.0, init="custom", ctx=other, beta_loss=KL).fit(x, W=w0, H=h0).transform(sx)
        finally:
            other.close()
        gone = csr(ctx, data, indices, indptr, x.shape)
        gone.close()
        with raises_with(inv, "was closed"):
            fit(s=gone)
        sh = make_sharded_ctx()
        try:
            with raises_with(inv, "sharded"):
                petal.Nmf(k, max_iter=2, tol=0.0, init="custom", ctx=sh[0], beta_loss=KL).fit(sh[1](data, indices, indptr, x.shape), W=w0, H=h0)
        finally:
            sh[0].close()
        return m
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
            lines.append(f"{label:8s} {c.name:34s} {name:6s}  kernel {info['kernel']}  error {err:.3e}  model {model:.3e}  floor {floor:.3e}  "
                         f"ratio {ratio:.3f}")
    lines.append(f"{label:8s} largest ratio {worst:.3f}")
    return worst


if __name__ == "__main__":
    import hostsim
    out = ["# petal_nmf_kl_sweep_csr against numpy.longdouble: G_new and colsum(G_new) (inner > 0) or the loss's term (inner = 0); errors over "
           "the scale (the largest sum of absolute terms); ratio = error / max(model, floor).  tests/nmf_kl_cases.py MULTIPLIER = twice each "
           "path's largest ratio, rounded up."]
    if len(sys.argv) < 2 or sys.argv[1] != "--host-only":
        dev = petal.Context(0)
        measure(dev, "device", out)
        dev.close()
    host = hostsim.context()
    measure(host, "hostsim", out)
    host.close()
    out.append("tests/nmf_kl_cases.py MULTIPLIER: " + ", ".join(f"{k} {v}" for k, v in MULTIPLIER.items()))
    dst = os.path.join(ROOT, sys.argv[2] if len(sys.argv) > 2 else os.path.join("profiles", "nmf_kl_errors.txt"))
    with open(dst, "w") as f:
        f.write("\n".join(out) + "\n")
    print("\n".join(out))
