"""The FastICA contrast functions beyond the crate's logcosh -- exp, g(u) = u exp(-u^2/2), and cube, g(u) = u^3 (include/petal_hip.h:
PETAL_ICA_CONTRAST_*) -- through the library's own entries, in the manner of tests/kernel_entry_cases.py, whose table, inputs,
long-double polar factor, floors and guard are used as they stand.  Shared by tests/test_gpu_contrast.py (the HIP library, both GEMM
modes) and tests/test_contrast_host.py (references and models against their own bounds, no GPU).

A. `ica_par(x1, tol = 0, max_iter = k, w_init, ICA_TEXTBOOK | ICA_CONTRAST_*)` runs exactly k iterations of
       W_k = polar(g(W X1) X1^T / n - diag(rowmean g'(W X1)) W),   W_0 = polar(w_init)
   against the same statement in numpy.longdouble (polar factor: kernel_entry_cases.polar_ld, certified per call).  The bound is a
   multiple of the error of a MODEL, the same statement in the precision under test and never the library's output:
     float32: every array and operation in numpy float32, polar factor from numpy's float32 SVD      |W - W_ld| <= MULT32 max(e_model, 2^-24)
     float64: numpy float64, polar factor from the oracle's po.symmetric_decorrelation               |W - W_ld| <= MULT64 max(e_model, 2^-52 (nc + sqrt n))
   The multiples START at the project's starting values (kernel_entry_cases.py: 4 for float32 -- another summation order, W on three
   bf16 planes, a hardware exp2 -- and 16 for float64 -- Newton-Schulz / Jacobi against the oracle's eigh) and are tightened to twice
   the largest error / model ratio measured on the MI355X over the table in both GEMM modes (profiles/contrast_entry_errors.txt).
   Every case asserts that its bound stays below GUARD = 1e-4, the loop's stopping rule.  No x20 "saturated" rows: for exp both g and
   g' underflow there, D -> 0 and the reference has no polar factor; cube has nothing to saturate.
B. exp with ONE planted outlier: sample OUTLIER_AT of the 4099 x 17 row is replaced by a vector of norm 1e3, a thousand times the data
   scale.  g and g' of exp vanish there (exp2 underflows to zero, no NaN from 0 * large): the result must be finite and within the
   same bound.  The vector is 1e3 polar(w_init)^T s / sqrt(nc), s = +-1: EVERY component then sees |u| = 1e3 / sqrt(nc) = 243 in the
   first iteration.  A random direction does not do that: among 17 projections of a random vector one is small (0.17 for the first
   vector tried, the others 56 .. 1441), a sum of products of size 1e3 that cancel to three digits, whose float32 rounding error
   eps32 1e3 reaches D as g'(u) du x / n ~ 6e-8 1e3 1e3 / 4099 = 1.5e-5 in ANY float32 evaluation -- the float32 model itself moved
   between 9.5e-7 and 3.1e-5 with the summation order of W x alone.  That is a case about cancellation at scale 1e3, in which no
   single model evaluation bounds another; the case wanted here is about underflow.
C. the layouts of x1 (kernel_entry_cases.ica_layout_check's list) and two identical calls: the SAME BYTES.
D. whole fits FastIca(fun = ...).fit_transform against a float64 numpy loop with the same contrast, started from the library's side
   of the whitening's sign ambiguity (parity_cases.ica_strict_parity's argument): sources within 2e-3 (float32) / 1e-7 (float64)
   of the identity, no permutation, n_iter within +-1 (float32) / equal (float64).

`python tests/contrast_cases.py` runs A-C on petal.Context(0) in both GEMM modes and prints one line per case: the report kept in
profiles/contrast_entry_errors.txt."""
import os
import sys

import numpy as np

if __name__ == "__main__":      # (run as a script: the package and the oracle are found from the repository root)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import petal_decomposition_amd as petal
from oracle import petal_oracle as po
from kernel_entry_cases import GUARD, ICA_ROWS, _polar_svd32, ica_bound, ica_inputs, polar_ld
import kernel_entry_cases as kc

LD = np.longdouble
# started at 4 and 16 (see A above); now twice the largest error / model ratio measured on the MI355X over the table, both GEMM modes
# (profiles/contrast_entry_errors.txt): float32 1.633 (cube, 256 x 16, k = 2, split-product mode), float64 1.155 (cube, 3000 x 5, k = 3)
MULT32 = 3.3
MULT64 = 2.4
FUNS = ("exp", "cube")
_DT = {"f32": np.float32, "f64": np.float64}
_cache = {}


def mode_of(fun):
    return petal.ICA_TEXTBOOK | {"logcosh": petal.ICA_CONTRAST_LOGCOSH, "exp": petal.ICA_CONTRAST_EXP, "cube": petal.ICA_CONTRAST_CUBE}[fun]


def contrast(fun, s):
    """(g(s), g'(s)) in the dtype of s (numpy keeps float32 / float64 / longdouble through these operations)"""
    one, two, three = s.dtype.type(1), s.dtype.type(2), s.dtype.type(3)
    if fun == "exp":
        e = np.exp(-(s * s) / two)
        return s * e, (one - s * s) * e
    if fun == "cube":
        return s * s * s, three * s * s
    if fun == "logcosh":
        g = np.tanh(s)
        return g, one - g * g
    raise KeyError(fun)


# ------------------------------------------------------------------------------------------- the long-double reference and the models
def steps_ld(fun, x1, w_init, kmax):
    """[(W_k, cond_2(D_k), max |S_k|)] for k = 1 .. kmax in long double; x1 (nc x n) and w_init arrive rounded to the dtype under test"""
    x = np.asarray(x1, dtype=LD)
    n = x.shape[1]
    w, _ = polar_ld(w_init)
    out = []
    for _ in range(kmax):
        s = w @ x
        g, gd = contrast(fun, s)
        assert g.dtype == LD and gd.dtype == LD
        d = (g @ x.T) / LD(n) - (gd.sum(axis=1) / LD(n))[:, None] * w
        w, _ = polar_ld(d)
        out.append((w, float(np.linalg.cond(d.astype(np.float64))), float(np.abs(s).max())))
    return out


def steps_model32(fun, x1, w_init, kmax):
    """the same statement with every array and operation in numpy float32, the polar factor from numpy's float32 SVD"""
    x = np.ascontiguousarray(x1, dtype=np.float32)
    n = np.float32(x.shape[1])
    w = _polar_svd32(np.asarray(w_init, dtype=np.float32))
    out = []
    for _ in range(kmax):
        g, gd = contrast(fun, w @ x)
        w = _polar_svd32((g @ x.T) / n - (gd.sum(axis=1, dtype=np.float32) / n)[:, None] * w)
        assert w.dtype == np.float32
        out.append(w)
    return out


def steps_model64(fun, x1, w_init, kmax):
    """numpy float64, the decorrelation by the oracle's restatement of the crate's route (eigh of D D^T)"""
    x = np.ascontiguousarray(x1, dtype=np.float64)
    n = float(x.shape[1])
    w = po.symmetric_decorrelation(np.asarray(w_init, dtype=np.float64))
    out = []
    for _ in range(kmax):
        g, gd = contrast(fun, w @ x)
        w = po.symmetric_decorrelation((g @ x.T) / n - (gd.sum(axis=1) / n)[:, None] * w)
        out.append(w)
    return out


# ------------------------------------------------------------------------------------------- A / B. k iterations of the loop
# beside ICA_ROWS, which is used as it stands: float64 data at 64 components, where k_ica_simple_g keeps g and g' in 64 KB of dynamic LDS
# (the opt-in launch of host_small.inc); same references, models and bound
EXTRA_ROWS = [(3000, 64, "f64", 1, 25)]
OUTLIER_ROW = (4099, 17, "f32", 1, 13)      # (n, nc, dtype, kmax, seed) of ICA_ROWS' ragged k_ica3p<2> row, one iteration
OUTLIER_AT = 2077
OUTLIER_SCALE = 1e3


def inputs(n, nc, dt, seed, outlier=False):
    x1, w0 = ica_inputs(n, nc, dt, seed)
    if not outlier:
        return x1, w0
    key = ("outlier", n, nc, dt, seed)
    if key not in _cache:
        x = x1.copy()
        u, _, vt = np.linalg.svd(w0.astype(np.float64))             # polar(w_init) = u vt: the W of the first iteration
        sg = np.where(np.random.default_rng(seed + 2000).standard_normal(nc) < 0, -1.0, 1.0)
        x[:, OUTLIER_AT] = (OUTLIER_SCALE * ((u @ vt).T @ sg) / np.sqrt(nc)).astype(x.dtype)      # whitened data: unit scale in every component
        _cache[key] = np.ascontiguousarray(x)
    return _cache[key], w0


def reference(fun, n, nc, dt, kmax, seed, outlier=False):
    """(long-double trajectory, model trajectory) of a row: computed once, whatever the GEMM mode and the k asked for"""
    key = ("ref", fun, n, nc, dt, kmax, seed, outlier)
    if key not in _cache:
        x1, w0 = inputs(n, nc, dt, seed, outlier)
        ref = steps_ld(fun, x1, w0, kmax)
        model = (steps_model32 if dt == "f32" else steps_model64)(fun, x1, w0, kmax)
        _cache[key] = (ref, model)
    return _cache[key]


def bound_of(n, nc, dt, e_model, mult32=None, mult64=None):
    """mult x max(e_model, floor) with kernel_entry_cases.ica_bound's floors"""
    if dt == "f32":
        return ica_bound(n, nc, dt, e_model) / kc.MULT32 * (MULT32 if mult32 is None else mult32)
    return ica_bound(n, nc, dt, e_model) / kc.MULT64 * (MULT64 if mult64 is None else mult64)


def model_check(fun, n, nc, dt, kmax, seed, k, outlier=False, mult32=None, mult64=None):
    """no library involved: (model error, bound, cond(D), max |S|) of a case, the bound asserted non-vacuous"""
    ref, model = reference(fun, n, nc, dt, kmax, seed, outlier)
    w_ld, cond_d, smax = ref[k - 1]
    e_model = float(np.abs(model[k - 1].astype(LD) - w_ld).max())
    bound = bound_of(n, nc, dt, e_model, mult32, mult64)
    assert np.isfinite(e_model) and np.all(np.isfinite(w_ld.astype(np.float64)))
    assert bound <= GUARD, f"vacuous bound {bound:.2e} (cond(D) = {cond_d:.0f}): another seed or a smaller k, never another guard"
    return e_model, bound, cond_d, smax


def step_check(ctx, fun, n, nc, dt, kmax, seed, k, outlier=False):
    """k iterations of the loop from the same x1 and w_init, W compared elementwise with the long double"""
    x1, w0 = inputs(n, nc, dt, seed, outlier)
    e_model, bound, cond_d, smax = model_check(fun, n, nc, dt, kmax, seed, k, outlier)
    w_ld = reference(fun, n, nc, dt, kmax, seed, outlier)[0][k - 1][0]
    if outlier:
        assert smax > 100.0, smax           # the planted sample does project far outside the data
    w, ni = petal.ica_par(x1, 0.0, k, w0, mode_of(fun), ctx)
    assert ni == k, (ni, k)
    assert w.dtype == _DT[dt]
    assert np.all(np.isfinite(w)), "non-finite W"
    err = float(np.abs(w.astype(LD) - w_ld).max())
    step_check.last = {"cond_d": cond_d, "smax": smax}
    return err, e_model, bound


# ------------------------------------------------------------------------------------------- C. layouts, repeated calls
LAYOUT_ROWS = [(20011, 64, "f32", 17), (3000, 5, "f64", 22)]


def layout_check(ctx, fun, n, nc, dt, seed, device):
    """kernel_entry_cases.ica_layout_check's layouts with the contrast in the mode word, and the first layout a second time.
    Returns the number of W entries that differ from the first call's, summed over the calls."""
    x1, w0 = ica_inputs(n, nc, dt, seed)
    mode = mode_of(fun)
    first, ni = petal.ica_par(x1, 0.0, 1, w0, mode, ctx)
    assert ni == 1 and np.all(np.isfinite(first))
    others = [x1, np.ascontiguousarray(x1.T).T]
    if device:
        import torch
        others.append(torch.from_numpy(x1).cuda())
        others.append(torch.from_numpy(np.ascontiguousarray(x1.T)).cuda().T)
    diff = 0
    for x in others:
        assert tuple(x.shape) == (nc, n)
        w, _ = petal.ica_par(x, 0.0, 1, w0, mode, ctx)
        diff += int(np.count_nonzero(w.view(np.uint8) != first.view(np.uint8)))
    if device and nc == 64:
        wide = torch.zeros((n, 80), dtype=torch.float32 if dt == "f32" else torch.float64, device="cuda")
        wide[:, :64] = torch.from_numpy(np.ascontiguousarray(x1.T)).cuda()
        wide[:, 64:] = 7.0     # (whatever lies beyond the component columns is not the kernels' to read)
        w, _ = petal.ica_par(wide[:, :64].T, 0.0, 1, w0, mode, ctx)
        assert ctx.stats()["x_zero_copy"] == 1, ctx.stats()
        diff += int(np.count_nonzero(w.view(np.uint8) != first.view(np.uint8)))
    return float(diff), 0.0, 0.0


# ------------------------------------------------------------------------------------------- D. whole fits
FIT_SHAPES = [   # (n, d, nc, dtype, seed)
    (20000, 24, 8, np.float32, 31),
    (5000, 6, 6, np.float64, 32),
    (30000, 128, 8, np.float32, 33),
    (60000, 64, 32, np.float32, 34),
    (20000, 96, 64, np.float32, 35),
]


def ica_par_ref(fun, x1, tol, max_iter, w_init):
    """po.ica_par (src/ica.rs:319-361, textbook semantics) with the contrast in logcosh's place: float64 numpy"""
    w = po.symmetric_decorrelation(w_init)
    p_inv = 1.0 / x1.shape[1]
    for i in range(max_iter):
        g, gd = contrast(fun, w @ x1)
        w1 = po.symmetric_decorrelation(g @ x1.T * p_inv - (gd.sum(axis=1) * p_inv)[:, None] * w)
        lim = np.max(np.abs(np.abs(np.einsum("ij,ij->i", w1, w)) - 1.0))
        if lim < tol:
            return w1, i + 1
        w = w1
    return w, max_iter


def fit_check(ctx, fun, n, d, nc, dtype, seed):
    """parity_cases.ica_strict_parity for a contrast: X1_lib = diag(s) X1_oracle (s: the library's sign convention for the whitening rows,
    the component of largest magnitude positive), so the library's fit from w_init is the reference's from w_init . diag(s)."""
    x = po.synth_ica(n, d, nc, seed=seed, dtype=np.float64).astype(dtype)
    x64 = x.astype(np.float64)
    w0 = np.random.default_rng(seed + 7).standard_normal((nc, nc))
    means, xt, k, x1 = po.FastIcaOracle(n_components=nc, whiten="eigh").whitening(x64)
    s = np.sign(k[np.arange(nc), np.abs(k).argmax(axis=1)])
    w, n_iter = ica_par_ref(fun, x1, 1e-4, 200, w0 * s[None, :])
    yo = (x64 - means) @ (w @ k).T
    m = petal.FastIca(ctx=ctx, n_components=nc, fun=fun)
    y = np.asarray(m.fit_transform(x, w_init=w0.astype(dtype)), dtype=np.float64)
    assert np.all(np.isfinite(y))
    c = np.abs(y.T @ yo)            # (the sources W K Xc = W X1 / sqrt(n) have unit norm over the samples)
    perm = c.argmax(axis=1)
    assert perm.tolist() == list(range(nc)), perm          # not even a permutation: the same rows in the same order
    dev = float(max(np.abs(1.0 - np.diag(c)).max(), np.abs(c - np.eye(nc)).max()))
    assert dev <= (2e-3 if dtype == np.float32 else 1e-7), dev
    assert abs(m.n_iter - n_iter) <= (1 if dtype == np.float32 else 0), (m.n_iter, n_iter)
    assert 1 < n_iter < 200, n_iter
    return dev, m.n_iter, n_iter


# ------------------------------------------------------------------------------------------- the case tables
class Case(kc.Case):
    pass


def all_cases(device=True, reduced=False):
    """reduced: without the two largest float32 rows (the CPU suite's table, as kernel_entry_cases.all_cases)"""
    cases = []
    for fun in FUNS:
        for n, nc, dt, kmax, seed in ICA_ROWS + EXTRA_ROWS:
            if reduced and (n, nc) in ((20011, 64), (70033, 49)):
                continue
            for k in range(1, kmax + 1):
                cases.append(Case(f"{fun}-{n}x{nc}-{dt}-k{k}", step_check, fun, n, nc, dt, kmax, seed, k))
    n, nc, dt, kmax, seed = OUTLIER_ROW
    cases.append(Case(f"exp-outlier-{n}x{nc}-{dt}", step_check, "exp", n, nc, dt, kmax, seed, 1, outlier=True))
    for fun in FUNS:
        for n, nc, dt, seed in LAYOUT_ROWS:
            if reduced and nc == 64:
                continue
            cases.append(Case(f"{fun}-layouts-{n}x{nc}-{dt}", layout_check, fun, n, nc, dt, seed, device))
    return cases


def main():
    import time
    cases = all_cases()
    print("# case | GEMM mode | error | model error | error / model | error / max(model, floor) | bound | cond(D)   (layout cases: error = number of differing entries)")
    t0 = time.time()
    worst = {}
    for mode in ("bf16x3", "fp32"):
        ctx = petal.Context(0)
        ctx.set_gemm_mode(mode)
        for c in cases:
            err, model, bound = c.run(ctx)
            if c.fn is not step_check:
                print(f"{c.id:34s} {mode:7s} {err:10.3e}{'' if err == 0 else '   <-- DIFFERENT BYTES'}")
                continue
            dt = c.args[3]
            floored = bound / (MULT32 if dt == "f32" else MULT64)
            ratio = err / model if model > 0 else float("nan")
            flag = "" if err <= bound else "   <-- ABOVE THE BOUND"
            print(f"{c.id:34s} {mode:7s} {err:10.3e} {model:10.3e} {ratio:8.3f} {err / floored:8.3f} {bound:10.3e} {step_check.last['cond_d']:8.1f}{flag}", flush=True)
            key = (dt, mode)
            if err / floored > worst.get(key, (0, ""))[0]:
                worst[key] = (err / floored, c.id)
        ctx.close()
    for (dt, mode), (r, cid) in sorted(worst.items()):
        print(f"# {dt}, {mode}: largest error / max(model, floor) {r:.3f} ({cid})")
    print(f"# multipliers in force: float32 {MULT32}, float64 {MULT64}")
    print(f"# wall time {time.time() - t0:.0f} s (references computed once, both modes)")


if __name__ == "__main__":
    main()
