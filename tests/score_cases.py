"""Row scores against a fitted projection (include/petal_hip_score.h: petal_score_rows) -- inputs, references and bounds, in the manner
of tests/kernel_entry_cases.py and tests/contrast_cases.py.  Shared by tests/test_gpu_score.py (the HIP library, both GEMM modes) and
tests/test_score_host.py (references and models against their own bounds, no GPU).

The statement, with xc = x - means (when centring) and y = xc . components^T, per row i:
    q_i = |xc_i|^2,   residual_i = max(q_i - sum_j y_ij^2, 0),   weighted_i = sum_j w_j y_ij^2          (w = None: all ones)
The REFERENCE is this statement in numpy.longdouble on the inputs as rounded to the dtype under test; the MODEL is the same statement
with every array and operation in that dtype (numpy), never the library's output.  Errors, over the rows with q_i > 0:
    e_res = max_i |residual_i - ref_i| / q_i          e_w = max_i |weighted_i - ref_i| / (q_i max_j |w_j|)
and each is held to  MULT max(e_model, eps)  with its own e_model (eps = the dtype's machine epsilon).  The residual is a difference of
two sums of about q_i, so its error is an ABSOLUTE few eps q_i whatever its size: that is the cancellation floor the documents state,
and the reason both measures are taken relative to q_i.  Rows with q_i = 0 (one is planted in every case: a row equal to the means, or
a zero row without centring) must come out exactly 0 in both columns.

The multipliers START at the project's starting values, 4 for float32 and 16 for float64 (kernel_entry_cases.py); they are to be
lowered to about twice the largest error / bound-base ratio measured on the MI355X over the table in both GEMM modes
(profiles/score_errors.txt holds the ratios) and never raised.

Data: k directions of variance 4 .. 1 along the orthonormal rows of `components`, isotropic noise in their complement carrying `tail`
times the variance of the kept part (1 down to 1e-6: the residual is then that fraction of q), and means three standard deviations
off the origin.  With k = d there is no complement: the true residual is rounding-sized and the result must still never be negative.

`python tests/score_cases.py` runs the table on petal.Context(0) in both GEMM modes and prints one line per case."""
import os
import sys
from functools import lru_cache

import numpy as np

if __name__ == "__main__":      # (run as a script: the package is found from the repository root)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import petal_decomposition_amd as petal

LD = np.longdouble
# started at 4 and 16; after the first runs on the MI355X (profiles/score_errors.txt, both GEMM modes): float64 lowered to about twice the
# largest ratio measured, 2.205 (4099 x 1024, k = 138, weighted).  float32 stays at its starting value: twice its largest ratio (2.316:
# 4099 x 1024, k = 138, fp32-MFMA mode) is already above it.
MULT32 = 4.0
MULT64 = 4.5
_DT = {"f32": np.float32, "f64": np.float64}


class Case:
    """n x d data, k components; weights: None | "inv" (1 / lambda_j) | "zeros" (1 / lambda_j with every other one zero);
    layout: "host" (row-major numpy) | "hostF" (column-major numpy) | "dev" (torch tensor on the device, streamed in place, device
    outputs); want_y: the projections are asked for as well"""

    def __init__(self, n, d, k, dt, tail=1e-2, centering=True, weights=None, layout="host", want_y=False, seed=0):
        self.n, self.d, self.k, self.dt, self.tail = n, d, k, dt, tail
        self.centering, self.weights, self.layout, self.want_y, self.seed = centering, weights, layout, want_y, seed

    @property
    def id(self):
        return (f"{self.n}x{self.d}-k{self.k}-{self.dt}-tail{self.tail:g}-{'c' if self.centering else 'nc'}-w{self.weights}-"
                f"{self.layout}{'-y' if self.want_y else ''}")

    __repr__ = __str__ = lambda self: self.id

    @property
    def key(self):
        return (self.n, self.d, self.k, self.dt, self.tail, self.centering, self.weights, self.seed)


# Every path of op_gemm_xp_scores: the any-shape kernel (n = 63), the matrix-core kernels at one wave (64), several workgroups with a
# ragged last one (4099) and many (70033); feature counts of one 16-column step, 100 (padded on the way in), and 8 / 16 / 32 chunks of
# 32; k of one column, one ragged tile, one full panel (80), one column more (81: two panels), 138 (two panels: 5 + 4 tiles) and
# k = d.
CASES = [
    Case(63, 100, 7, "f32", weights="inv", want_y=True),
    Case(63, 16, 16, "f64", tail=0.0, weights="inv"),
    Case(64, 16, 16, "f32", tail=0.0, weights="zeros", want_y=True),
    Case(64, 256, 80, "f32", tail=1.0),
    Case(64, 256, 81, "f64", tail=1e-4, weights="inv", want_y=True),
    Case(4099, 512, 64, "f32", tail=1e-2, weights="inv", layout="dev", want_y=True),
    Case(4099, 512, 64, "f32", tail=1e-2, weights="inv", want_y=True),
    Case(4099, 512, 64, "f32", tail=1e-6),
    Case(4099, 512, 81, "f32", tail=1e-3, weights="zeros", want_y=True),
    Case(4099, 1024, 138, "f32", tail=1e-1, weights="inv", layout="dev"),
    Case(4099, 100, 7, "f32", tail=1.0, weights="inv", layout="hostF", want_y=True),
    Case(4099, 256, 1, "f32", tail=1e-2, centering=False),
    Case(4099, 256, 256, "f32", tail=0.0, weights="inv"),
    Case(70033, 256, 7, "f32", tail=1e-4, weights="zeros", layout="dev", want_y=True),
    Case(4099, 512, 64, "f64", tail=1e-6, weights="inv", layout="dev", want_y=True),
    Case(4099, 256, 81, "f64", tail=1e-2, weights="zeros", want_y=True),
    Case(4099, 1024, 138, "f64", tail=1.0),
    Case(4099, 100, 7, "f64", tail=1e-3, weights="inv", layout="hostF", centering=False, want_y=True),
    Case(4099, 16, 16, "f64", tail=0.0, weights="inv", layout="dev"),
    Case(70033, 16, 1, "f64", tail=1e-1, weights="inv"),
]


def all_cases(reduced=False):
    """reduced: the table without its 70033-row cases (the CPU suite's share)"""
    return [c for c in CASES if not (reduced and c.n > 5000)]


# ------------------------------------------------------------------------------------------- inputs
@lru_cache(maxsize=None)
def inputs(n, d, k, dt, tail, centering, weights, seed):
    """(x, components, means, w or None, planted row), all rounded to the dtype under test and read-only"""
    T = _DT[dt]
    rng = np.random.default_rng([n, d, k, seed, 7])
    comp = np.linalg.qr(rng.standard_normal((d, k)))[0].T                     # k x d, orthonormal rows
    lam = np.linspace(4.0, 1.0, k)
    x = (rng.standard_normal((n, k)) * np.sqrt(lam)) @ comp
    if d > k and tail > 0:
        noise = rng.standard_normal((n, d))
        noise -= (noise @ comp.T) @ comp
        x += noise * np.sqrt(tail * lam.sum() / (d - k))
    mu = 3.0 * np.sqrt(x.var(axis=0).mean()) * rng.choice([-1.0, 1.0], d)   # three standard deviations off the origin
    x += mu
    x, comp, mu = x.astype(T), np.ascontiguousarray(comp.astype(T)), mu.astype(T)      # (comp row-major: the raw entry takes it as it lies)
    planted = n // 3
    x[planted] = mu if centering else 0
    w = None
    if weights is not None:
        w = 1.0 / lam
        if weights == "zeros":
            w[::2] = 0.0
        w = w.astype(T)
    for a in (x, comp, mu) + ((w,) if w is not None else ()):
        a.setflags(write=False)
    return x, comp, mu, w, planted


def statement(x, comp, mu, w, centering, T):
    """(residual, weighted, q) with every array and operation in T (long double: the reference; the dtype under test: the model)"""
    x, comp = np.asarray(x, dtype=T), np.asarray(comp, dtype=T)
    xc = x - np.asarray(mu, dtype=T) if centering else x
    y = np.einsum("ij,kj->ik", xc, comp) if T is LD else xc @ comp.T
    q = (xc * xc).sum(axis=1, dtype=T)
    y2 = y * y
    res = np.maximum(q - y2.sum(axis=1, dtype=T), T(0))
    wt = y2.sum(axis=1, dtype=T) if w is None else (y2 * np.asarray(w, dtype=T)).sum(axis=1, dtype=T)
    assert res.dtype == T and wt.dtype == T and q.dtype == T
    return res, wt, q


@lru_cache(maxsize=None)
def reference(key):
    x, comp, mu, w, _ = inputs(*key)
    out = statement(x, comp, mu, w, key[5], LD)
    for a in out:
        a.setflags(write=False)
    return out


def errors(res, wt, key):
    """(e_res, e_w) of a result against the reference, over the rows with q > 0; asserts exact zeros where q = 0"""
    _, _, _, w, planted = inputs(*key)
    rres, rwt, q = reference(key)
    res, wt = np.asarray(res), np.asarray(wt)
    assert np.all(np.isfinite(res)) and np.all(np.isfinite(wt))
    assert np.all(res >= 0), float(res.min())
    zero = q == 0
    assert zero[planted]
    assert np.all(res[zero] == 0) and np.all(wt[zero] == 0), (res[zero], wt[zero])
    live = ~zero
    wmax = LD(1) if w is None else LD(np.abs(w).max())
    e_res = float((np.abs(res[live].astype(LD) - rres[live]) / q[live]).max())
    e_w = float((np.abs(wt[live].astype(LD) - rwt[live]) / (q[live] * wmax)).max()) if wmax > 0 else 0.0
    return e_res, e_w


@lru_cache(maxsize=None)
def model_errors(key):
    x, comp, mu, w, _ = inputs(*key)
    res, wt, _ = statement(x, comp, mu, w, key[5], _DT[key[3]])
    return errors(res, wt, key)


def bounds(key, mult32=None, mult64=None):
    """(bound on e_res, bound on e_w)"""
    T = _DT[key[3]]
    mult = (MULT32 if mult32 is None else mult32) if T is np.float32 else (MULT64 if mult64 is None else mult64)
    eps = float(np.finfo(T).eps)
    em_res, em_w = model_errors(key)
    return mult * max(em_res, eps), mult * max(em_w, eps)


# ------------------------------------------------------------------------------------------- the library
def laid_out(case, x):
    """x in the case's layout: numpy (row- or column-major) or a torch device tensor"""
    if case.layout == "hostF":
        xf = np.asfortranarray(x)
        assert not xf.flags["C_CONTIGUOUS"] or x.shape[1] == 1
        return xf
    if case.layout == "dev":
        import torch
        return torch.from_numpy(np.array(x)).cuda()
    return x


def to_numpy(a):
    return a.cpu().numpy() if petal._is_torch(a) else np.asarray(a)


def run(case, ctx):
    """(scores n x 2, y or None) as numpy arrays, from the library"""
    x, comp, mu, w, _ = inputs(*case.key)
    out, y = petal.score_rows(laid_out(case, x), comp, mu, weights=w, centering=case.centering, want_y=case.want_y, ctx=ctx)
    if case.layout == "dev":
        assert petal._is_torch(out) and out.is_cuda
    return to_numpy(out), (to_numpy(y) if y is not None else None)


def check(case, ctx, report=None):
    out, y = run(case, ctx)
    assert out.shape == (case.n, 2) and out.dtype == _DT[case.dt]
    e_res, e_w = errors(out[:, 0], out[:, 1], case.key)
    b_res, b_w = bounds(case.key)
    em_res, em_w = model_errors(case.key)
    eps = float(np.finfo(_DT[case.dt]).eps)
    line = (f"{case.id}: e_res {e_res:.3e} (model {em_res:.3e}, bound {b_res:.3e}, ratio to max(model, eps) {e_res / max(em_res, eps):.3f})  "
            f"e_w {e_w:.3e} (model {em_w:.3e}, bound {b_w:.3e}, ratio {e_w / max(em_w, eps):.3f})")
    print(line)
    if report is not None:
        report.append(line)
    assert e_res <= b_res, (case.id, "residual", e_res, b_res)
    assert e_w <= b_w, (case.id, "weighted", e_w, b_w)
    if case.want_y:
        assert y.shape == (case.n, case.k) and y.dtype == _DT[case.dt]
    return out, y


if __name__ == "__main__":
    c = petal.Context(0)
    for mode in ("bf16x3", "fp32"):
        c.set_gemm_mode(mode)
        print(f"# GEMM mode {mode}")
        for case in all_cases():
            try:
                check(case, c)
            except AssertionError as e:     # (a missed bound is a finding to print, the table goes on; anything else ends the run)
                print(f"FAIL {case.id}: {e}")
