"""Exact Pca on wide data (include/petal_hip_wide.h): the generators, the long-double reference of the row Gram matrix, the float64 numpy
model of the dual route, the case tables with their bounds, and the checks the GPU suite and the host suite share.

The row Gram matrix K = (X - c)(X - c)^T is measured against a numpy.longdouble reference (x widened exactly from the stored type, c the
float64 centre the library is given) and expressed over the error of the MODEL -- the same statement in float64 numpy -- with a floor:

    ratio = max |K - ref| / max(max |K_model - ref|, FLOOR_EPS eps64 max diag(ref))

MULTIPLIER is twice the largest ratio measured on the device and on the host simulation (profiles/pca_wide_errors.txt; the convention of
profiles/ipca_errors.txt and profiles/smallmat_errors.txt), and the bound itself -- multiplier x max(model, floor) -- must stay below
CAP = 1e-12 of the largest diagonal entry of K, so that the bound cannot hide a lost precision: a float32 accumulation misses the cap by
decades on the same inputs.

Run as a script on a machine with the GPU it writes profiles/pca_wide_errors.txt: the device's rows and the host simulation's."""
import functools
import os
import sys
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import petal_oracle as po  # noqa: E402
import petal_decomposition_amd as petal  # noqa: E402
from parity_cases import decided_signs, rowwise_rel  # noqa: E402

EPS64 = float(np.finfo(np.float64).eps)
FLOOR_EPS = 4.0          # the floor of the model error: 4 eps64 of the largest diagonal entry of the reference K
CAP = 1e-12              # of the largest diagonal entry: no bound may exceed it
DUAL_MIN_D = 2048        # the auto rule: n < d and d > 2048


# ------------------------------------------------------------------------------------------- 1. exact integers
# n: one row, one short of / exactly / one past a 16-row MFMA tile, a 32-row wave tile plus one, several wave tiles (100: four row
# blocks, ten upper tiles = three workgroups; 257: nine row blocks, the last with one live row)
INT_N = (1, 15, 16, 17, 33, 100, 257)
# d: below one 16-byte load, one 16-feature step, ragged widths (the padding columns), several chunks (4099 -> 4112 padded features:
# 16 chunks of 272, the last one of 32)
INT_D = (1, 3, 16, 19, 67, 1000, 4099)
# one more width per dtype that the launcher cuts into >= 3 chunks with a ragged last one (the chunk count is read from `info`)
INT_D_RAGGED = {"f32": 3001, "f64": 2400}
FORMS = ("host", "device", "device-odd-pitch", "host-fortran")


def np_dt(name):
    return np.float32 if name == "f32" else np.float64


@functools.lru_cache(maxsize=None)
def int_inputs(n, d, dt):
    """(x, centre, K without centre, K with centre): integers in [-8, 8]; every sum is below 2^28, so float64 holds it exactly"""
    rng = np.random.default_rng(7919 * n + d)
    x = rng.integers(-8, 9, size=(n, d))
    c = rng.integers(-8, 9, size=d)
    k0 = x @ x.T
    k1 = (x - c) @ (x - c).T
    assert max(np.abs(k0).max(), np.abs(k1).max()) < 2 ** 28
    x = x.astype(np_dt(dt))
    x.setflags(write=False)
    return x, c.astype(np.float64), k0.astype(np.float64), k1.astype(np.float64)


def as_form(x, form):
    """the same values as a host array, a device tensor, a device view whose row pitch is no multiple of 4 elements, a column-major host
    view"""
    if form == "host":
        return x
    if form == "host-fortran":
        return np.asfortranarray(x)
    import torch
    if form == "device":
        return torch.from_numpy(np.ascontiguousarray(x)).cuda()
    n, d = x.shape
    pitch = d + 1 if (d + 1) % 4 else d + 2
    buf = torch.full((n, pitch), float("nan"), dtype=torch.from_numpy(x[:0]).dtype, device="cuda")
    buf[:, :d] = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    v = buf[:, :d]
    assert v.stride(0) % 4 != 0
    return v


def check_integers_exact(ctx, n, d, dt, form, expect_kernel):
    """K equals numpy's int64 product bit for bit, with and without a centre, and is exactly symmetric; what lies outside the n x n block
    of the device buffer stays untouched (petal_row_gram forms K inside a guard and raises if it changed).  Returns the chunk count."""
    x, c, k0, k1 = int_inputs(n, d, dt)
    xf = as_form(x, form)
    chunks = 0
    for centre, want in ((None, k0), (c, k1)):
        out, info = petal.row_gram(xf, centre, ctx=ctx, want_info=True)
        assert out.tobytes() == want.tobytes(), (n, d, dt, form, centre is not None, np.abs(out - want).max())
        assert np.array_equal(out, out.T)
        assert info["kernel"] == (1 if expect_kernel else 0), info
        assert (info["chunks"] >= 1) == bool(expect_kernel), info
        chunks = info["chunks"]
    return chunks


# ------------------------------------------------------------------------------------------- 2. real data against long double
GramCase = namedtuple("GramCase", "name n d dt seed")
GRAM_CASES = [GramCase(f"{dt}-{n}x{d}", n, d, dt, seed)
              for (n, d, seed) in ((33, 67, 61), (100, 5000, 62), (257, 2500, 63)) for dt in ("f32", "f64")]
# twice the largest measured ratio (profiles/pca_wide_errors.txt: k_row_gram 0.509; the host simulation's fallback, whose op_dgemm adds
# the d products of an element one after the other where numpy's BLAS blocks them, 5.839)
MULTIPLIER = {"device": 1.02, "hostsim": 11.7}


@functools.lru_cache(maxsize=None)
def gram_inputs(c):
    """(x, centre): unit noise times column scales graded over four decades, every row 40 sigma off zero; the centre is the float64
    column mean -- what a fit passes"""
    rng = np.random.default_rng(c.seed)
    scale = 10.0 ** rng.uniform(-2.0, 2.0, size=c.d)
    x = ((rng.standard_normal((c.n, c.d)) + 40.0 * np.sign(rng.standard_normal(c.d))) * scale).astype(np_dt(c.dt))
    x.setflags(write=False)
    centre = x.astype(np.float64).mean(axis=0)
    centre.setflags(write=False)
    return x, centre


@functools.lru_cache(maxsize=None)
def gram_reference(c):
    """K in numpy.longdouble (read-only)"""
    x, centre = gram_inputs(c)
    xc = x.astype(np.longdouble) - centre.astype(np.longdouble)
    ref = np.empty((c.n, c.n), dtype=np.longdouble)
    for i in range(c.n):   # (row by row: a longdouble matmul of the whole matrix holds n x n x d temporaries in some numpy builds)
        ref[i] = (xc * xc[i]).sum(axis=1)
    ref.setflags(write=False)
    return ref


def gram_model(c, accumulate=np.float64):
    """the statement in numpy: widened, centred in float64, products and sums in `accumulate`"""
    x, centre = gram_inputs(c)
    xc = (x.astype(np.float64) - centre).astype(accumulate)
    return (xc @ xc.T).astype(np.float64)


def gram_ratio(c, k):
    ref = gram_reference(c)
    top = float(np.max(np.diag(ref)))
    err = float(np.max(np.abs(k.astype(np.longdouble) - ref)))
    model = float(np.max(np.abs(gram_model(c).astype(np.longdouble) - ref)))
    floor = FLOOR_EPS * EPS64 * top
    return err / max(model, floor), err, model, floor, top


def check_gram_against_long_double(ctx, c, expect_kernel):
    x, centre = gram_inputs(c)
    k, info = petal.row_gram(x, centre, ctx=ctx, want_info=True)
    assert info["kernel"] == (1 if expect_kernel else 0), info
    ratio, err, model, floor, top = gram_ratio(c, k)
    bound = MULTIPLIER["device" if expect_kernel else "hostsim"] * max(model, floor)
    print(f"{c.name}: error {err / top:.3e}, model {model / top:.3e}, floor {floor / top:.3e} of max diag K; ratio {ratio:.3f}, "
          f"bound {bound / top:.3e} (cap {CAP:.0e}), chunks {info['chunks']}")
    assert bound <= CAP * top, (bound / top, CAP)
    assert err <= bound, (c.name, ratio)
    return ratio


def check_same_bytes_twice(ctx, c):
    x, centre = gram_inputs(c)
    a = petal.row_gram(x, centre, ctx=ctx)
    b = petal.row_gram(x, centre, ctx=ctx)
    assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------- fits
FitCase = namedtuple("FitCase", "name n d k dt centering seed")
FIT_CASES = [
    FitCase("f64-40x300-k5", 40, 300, 5, "f64", True, 71),
    FitCase("f32-33x67-k8", 33, 67, 8, "f32", True, 72),
    FitCase("f32-100x5000-k10", 100, 5000, 10, "f32", True, 73),
    FitCase("f64-257x2500-k16", 257, 2500, 16, "f64", True, 74),
    FitCase("f64-40x300-k5-uncentred", 40, 300, 5, "f64", False, 71),
    FitCase("f64-300x40-k5-tall", 300, 40, 5, "f64", True, 75),     # n > d: the forced route is shape-agnostic
]
ROUND_TRIP_CASE = FIT_CASES[2]


def tol_of(c):
    """the existing suite's for the same dtype (tests/test_gpu_parity.py: 1e-8 float64, 2e-5 float32)"""
    return 2e-5 if c.dt == "f32" else 1e-8


@functools.lru_cache(maxsize=None)
def fit_inputs(c):
    x = po.synth_pca(c.n, c.d, c.k, seed=c.seed, dtype=np_dt(c.dt))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def fit_oracle(c):
    """(oracle, U, y) of PcaOracle(k, thin=True) on the float64 image of the data"""
    o = po.PcaOracle(c.k, centering=c.centering, thin=True)
    uo = o._inner_fit(fit_inputs(c).astype(np.float64))
    return o, uo, po.transform_with_u(uo, o.singular, c.k)


def model_dual_fit(x, k, centering, thr):
    """the dual route in float64 numpy: (components, singular, means, total variance, y).  A component at or below thr sigma_1, and
    the n-th one of centred data, is a zero row."""
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    mu = x.mean(axis=0) if centering else np.zeros(d)
    xc = x - mu
    lam, u = np.linalg.eigh(xc @ xc.T)
    lam, u = lam[::-1], u[:, ::-1]
    sig = np.sqrt(np.maximum(lam, 0.0))
    inv = np.where(sig > thr * sig[0], 1.0 / np.where(sig > 0, sig, 1.0), 0.0)
    if centering:
        inv[n - 1] = 0.0
    r = min(n, d)
    idx = np.argmax(np.abs(u[:, :r]), axis=0)                       # svd_flip (pca.rs:826-839) on U itself
    sg = np.where(u[idx, np.arange(r)] < 0, -1.0, 1.0)
    comp = ((u[:, :k] * inv[:k]).T @ xc) * sg[:k, None]
    return comp, sig[:k], mu, float(np.trace(xc @ xc.T)), u[:, :k] * sig[:k] * sg[:k]


def compare_with_oracle(c, comp, sing, means, tv, y, tol):
    """components with their signs as pca_parity compares them, singular values, means, total variance, fit_transform's y"""
    o, uo, yo = fit_oracle(c)
    comp = np.asarray(comp, dtype=np.float64)
    rel = rowwise_rel(comp, o.components)
    assert rel.max() <= tol, (c.name, rel.max())
    dec = decided_signs(uo, c.k, margin=min(0.5, max(1e-3, 100 * tol)))
    sgn = np.sign(np.sum(comp * o.components, axis=1))
    assert np.all(sgn[dec] == 1), f"svd_flip signs differ from the oracle's on decided components {np.nonzero(dec & (sgn != 1))[0]}"
    assert np.allclose(sing, o.singular, rtol=tol)
    assert np.allclose(means, o.means, rtol=tol, atol=tol * np.abs(o.means).max())
    assert np.isclose(float(tv), float(o.total_variance), rtol=10 * tol)
    s = np.sign(np.sum(np.asarray(y, dtype=np.float64) * yo, axis=0))
    assert np.abs(np.asarray(y, dtype=np.float64) * s - yo).max() <= 100 * tol * np.abs(yo).max()


def fit_dual(ctx, c, dual=1, fallback=0):
    """Pca.fit_transform with the route options set for the call; returns (model, y, last_route)"""
    ctx.set_option("pca_dual", dual)
    ctx.set_option("pca_dual_fallback", fallback)
    try:
        m = petal.Pca(c.k, centering=c.centering, ctx=ctx)
        y = m.fit_transform(fit_inputs(c))
        return m, y, m.last_route()
    finally:
        ctx.set_option("pca_dual", 0)
        ctx.set_option("pca_dual_fallback", 0)


def total_variance_of(m):
    return float(np.asarray(m._total_variance).reshape(-1)[0])


def check_fit_parity(ctx, c, expect_kernel):
    m, y, route = fit_dual(ctx, c)
    assert route["route"] == 1 and route["kernel"] == (1 if expect_kernel else 0) and route["order"] == c.n, route
    compare_with_oracle(c, m.components(), m.singular_values(), m.mean(), total_variance_of(m), y, tol_of(c))
    return m


def check_dual_against_primal(ctx, c):
    tol = tol_of(c)
    m1, y1, r1 = fit_dual(ctx, c, dual=1)
    m0, y0, r0 = fit_dual(ctx, c, dual=-1)
    assert r1["route"] == 1 and r0["route"] == 0 and r0["order"] == c.d and r0["kernel"] == 0, (r1, r0)
    for m, y in ((m1, y1), (m0, y0)):
        compare_with_oracle(c, m.components(), m.singular_values(), m.mean(), total_variance_of(m), y, tol)
    assert rowwise_rel(m1.components().astype(np.float64), m0.components().astype(np.float64)).max() <= 2 * tol
    assert np.allclose(m1.singular_values(), m0.singular_values(), rtol=2 * tol)


def check_fallback_equivalence(ctx, c):
    tol = tol_of(c)
    mf, _, rf = fit_dual(ctx, c, fallback=1)
    mk, _, rk = fit_dual(ctx, c, fallback=0)
    assert (rf["route"], rf["kernel"], rk["route"], rk["kernel"]) == (1, 0, 1, 1), (rf, rk)
    assert rf["chunks"] == 0 and rk["chunks"] >= 1
    assert rowwise_rel(mf.components().astype(np.float64), mk.components().astype(np.float64)).max() <= tol
    assert np.allclose(mf.singular_values(), mk.singular_values(), rtol=tol)


AUTO_RULE = (((64, 2064), 1), ((64, 2048), 0), ((3000, 256), 0), ((2100, 2064), 0))


def check_auto_rule(ctx, shape, want_route):
    """pca_dual = 0: the dual route when n < d and d > 2048, the primal one otherwise"""
    n, d = shape
    assert ctx.get_option("pca_dual") == 0.0
    # (planted directions with a gap behind the two wanted ones: the primal route's subspace iteration converges.  Unstructured
    # noise has no such gap and the order-d eigenproblem is then solved in full: a minute and a half on the device at d = 2048)
    x = po.synth_pca(n, d, 2, seed=n + d, dtype=np.float32)
    m = petal.Pca.new(2, ctx).fit(x)
    r = m.last_route()
    assert r["route"] == want_route and r["order"] == (n if want_route else d), (shape, r)


def sharded_rule_input():
    """(64, 2064) float32, planted like the auto rule's cases: the shape the rule sends to the dual route on a ctx that is not sharded"""
    return po.synth_pca(64, 2064, 2, seed=3, dtype=np.float32)


def check_k_equals_n(ctx, expect_kernel):
    """centred data, k = n: the n-th component is not determined by the data -- a zero row, its singular value as computed, nothing
    raised, nothing non-finite; the first n - 1 within tolerance of the oracle and orthonormal.  Also n = 1, k = 1."""
    c = FitCase("f64-17x1000-k17", 17, 1000, 17, "f64", True, 76)
    tol = tol_of(c)
    m, y, route = fit_dual(ctx, c)
    assert route["route"] == 1 and route["kernel"] == (1 if expect_kernel else 0)
    comp, sing = m.components().astype(np.float64), m.singular_values().astype(np.float64)
    assert np.isfinite(comp).all() and np.isfinite(sing).all() and np.isfinite(np.asarray(y)).all() and np.isfinite(total_variance_of(m))
    assert not comp[16].any()
    o, _, _ = fit_oracle(c)
    assert rowwise_rel(comp[:16], o.components[:16]).max() <= tol
    assert np.allclose(sing[:16], o.singular[:16], rtol=tol)
    assert sing[16] <= 1e-6 * sing[0]                               # (the rounding of K: about sqrt(eps64) sigma_1)
    assert np.abs(comp[:16] @ comp[:16].T - np.eye(16)).max() <= 10 * tol
    one = FitCase("f64-1x50-k1", 1, 50, 1, "f64", True, 77)
    m, y, route = fit_dual(ctx, one)
    assert route["route"] == 1 and route["order"] == 1
    assert not m.components().any() and m.singular_values()[0] == 0 and total_variance_of(m) == 0 and not np.asarray(y).any()
    assert np.array_equal(m.mean(), fit_inputs(one)[0])


def check_non_finite_raises(ctx):
    for bad in (np.nan, np.inf):
        x = np.random.default_rng(5).standard_normal((20, 100))
        x[7, 13] = bad
        ctx.set_option("pca_dual", 1)
        try:
            try:
                petal.Pca.new(3, ctx).fit(x)
            except petal.LinalgError as e:
                assert "did not converge" in str(e), str(e)
            else:
                raise AssertionError(f"a fit on data with {bad} did not raise")
        finally:
            ctx.set_option("pca_dual", 0)


def check_round_trip(ctx, expect_kernel):
    """transform / inverse_transform / reconstruction_error of a dual-fitted model against the oracle's"""
    c = ROUND_TRIP_CASE
    tol = tol_of(c)
    m = check_fit_parity(ctx, c, expect_kernel)
    o, _, _ = fit_oracle(c)
    x = fit_inputs(c)
    x64 = x.astype(np.float64)
    yo = o.transform(x64)
    y = np.asarray(m.transform(x), dtype=np.float64)
    s = np.sign(np.sum(y * yo, axis=0))
    assert np.abs(y * s - yo).max() <= 100 * tol * np.abs(yo).max()
    xr, xo = m.inverse_transform(m.transform(x)), o.inverse_transform(yo)
    assert np.abs(xr - xo).max() <= 100 * tol * np.abs(xo).max()
    xc = x64 - o.means
    q = np.sum(xc * xc, axis=1) - np.sum(yo * yo, axis=1)
    got = np.asarray(m.reconstruction_error(x), dtype=np.float64)
    assert np.abs(got - q).max() <= 100 * tol * np.sum(xc * xc, axis=1).max()


# ------------------------------------------------------------------------------------------- the measured ratios
def measure(ctx, label, lines):
    worst = 0.0
    for c in GRAM_CASES:
        x, centre = gram_inputs(c)
        k, info = petal.row_gram(x, centre, ctx=ctx, want_info=True)
        ratio, err, model, floor, top = gram_ratio(c, k)
        worst = max(worst, ratio)
        lines.append(f"{label:8s} {c.name:16s} kernel {info['kernel']} chunks {info['chunks']:3d}  error {err / top:.3e}  model {model / top:.3e}  "
                     f"floor {floor / top:.3e}  ratio {ratio:.3f}")
    lines.append(f"{label:8s} largest ratio {worst:.3f}")
    return worst


if __name__ == "__main__":
    import hostsim
    out = ["# row Gram matrix (petal_row_gram) against numpy.longdouble: errors over the largest diagonal entry of K; ratio = error / "
           "max(model, floor).  tests/wide_cases.py MULTIPLIER = twice the largest ratio."]
    worst = 0.0
    if len(sys.argv) < 2 or sys.argv[1] != "--host-only":
        dev = petal.Context(0)
        worst = max(worst, measure(dev, "device", out))
        dev.close()
    host = hostsim.context()
    worst = max(worst, measure(host, "hostsim", out))
    host.close()
    out.append(f"largest ratio overall {worst:.3f}; tests/wide_cases.py MULTIPLIER (twice each layer's largest ratio): "
               + ", ".join(f"{k} {v}" for k, v in MULTIPLIER.items()))
    dst = os.path.join(ROOT, sys.argv[2] if len(sys.argv) > 2 else os.path.join("profiles", "pca_wide_errors.txt"))
    with open(dst, "w") as f:
        f.write("\n".join(out) + "\n")
    print("\n".join(out))
