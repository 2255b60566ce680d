"""The FastICA step and tail kernels, the textbook symmetric decorrelation and svd_flip through their own ABI entries
(petal_ica_par with tol = 0, petal_symmetric_decorrelation, petal_svd_flip), against references that do not forgive what a
converged fit forgives.  Shared by tests/test_gpu_kernel_entry.py (the HIP library, both GEMM modes) and
tests/test_kernel_entry_hostsim.py (the host simulation, a reduced table: it proves references and bounds without a GPU).

A. `ica_par(x1, tol = 0, max_iter = k)` runs exactly k iterations: W_k = polar(G X1^T / n - diag(g') W_{k-1}), W_0 = polar(w_init)
   -- one launch of the step kernel and one of the tail per iteration.  The reference is the same statement in numpy.longdouble
   (64-bit mantissa), the polar factor by the plain Newton-Schulz iteration, certified per case (see polar_ld).  The bound is a
   multiple of the error of a MODEL, the same statement in the precision under test and never the library's output:
     float32: every array and operation in numpy float32, polar factor from numpy's float32 SVD      |W - W_ld| <= 3.6 max(e_model, 2^-24)
     float64: the project's oracle po.ica_par (the crate's route: eigh of D D^T)                      |W - W_ld| <= 4.8 max(e_model, 2^-52 (nc + sqrt n))
   (float32: the crate's route would cost eps32 cond(D)^2 and make the bound vacuous; float64: an SVD model is better conditioned
   than what the crate and the device's Jacobi route above 64 components do.  The float64 floor is what a sum of n terms of
   order one carries when its rounding errors add at random.)  A bound above 1e-4, the loop's own stopping rule, proves nothing:
   every case asserts that its bound stays below it.
B. `symmetric_decorrelation(W, TEXTBOOK)` against polar_ld(W) over sizes x condition numbers:
     |Wout - polar_ld(W)| and |Wout Wout^T - I| <= 2^-52 (16 + cond_2(W)^2)  (+ 2^-23 for float32 input / output)
   derived, not fitted: the crate forms W W^T (condition cond^2), and a relative error eps in its smallest eigenvalue reaches
   (W W^T)^(-1/2) as eps cond^2 / 2.  The oracle's float64 restatement is the model; the CPU suite holds IT to the bound too.
C. `svd_flip(u, vt)` against the rule of src/pca.rs:815-850 restated below (flip_rule): EXACT, sign bits of zeros included.

Each check takes a ctx and returns (error, model_error, bound).  `python tests/kernel_entry_cases.py` runs every case on
petal.Context(0) in both GEMM modes and prints one line per case: the report kept in profiles/kernel_entry_errors.txt."""
import os
import sys

import numpy as np

if __name__ == "__main__":      # (run as a script: the package and the oracle are found from the repository root)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import petal_decomposition_amd as petal
from oracle import petal_oracle as po

LD = np.longdouble
# The multiples of the model's error in table A.  They started at 4 (float32: another summation order, W rounded to three bf16 planes,
# tanh_fast's absolute error) and 16 (float64: Newton-Schulz / Jacobi against the oracle's eigh, another algorithm) and were
# tightened to twice the largest error / model ratio measured on the MI355X over the table, both GEMM modes
# (profiles/kernel_entry_errors.txt): float32 1.78 (256 x 16, k = 2, split-product mode), float64 2.39 (3000 x 5, k = 3).
MULT32 = 3.6
MULT64 = 4.8
GUARD = 1e-4      # the loop's stopping rule: a bound above it proves nothing


# ------------------------------------------------------------------------------------------- the long-double reference
def polar_ld(d):
    """Orthogonal polar factor (D D^T)^(-1/2) D by the PLAIN Newton-Schulz iteration X <- 1.5 X - 0.5 (X X^T) X from
    X0 = D / ||D||_F, all in long double, until ||X X^T - I||_F < 1e-17 nc.  (Not seeded from a float64 factor:
    polar(M D) != polar(D).)  Certifies itself: polar(D) D^T is the symmetric factor, so it must come out symmetric, and D must
    have full rank.  Returns (factor, iterations)."""
    assert np.finfo(LD).eps < 2e-19, "needs the x86 80-bit long double"
    d = np.asarray(d, dtype=LD)
    nc = d.shape[0]
    sv = np.linalg.svd(d.astype(np.float64), compute_uv=False)
    assert sv.min() > 0.0, "reference certificate: singular input"
    x = d / np.sqrt((d * d).sum())
    eye = np.eye(nc, dtype=LD)
    for it in range(1, 400):
        t = x @ x.T
        r = t - eye
        if np.sqrt((r * r).sum()) < LD(1e-17) * nc:
            break
        x = LD(1.5) * x - LD(0.5) * (t @ x)
    else:
        raise AssertionError("reference certificate: the Newton-Schulz iteration did not converge")
    h = x @ d.T
    asym = np.abs(h - h.T).max() / np.abs(h).max()
    assert asym < 1e-17, f"reference certificate: polar(D) D^T asymmetric by {float(asym):.1e}"
    return x, it


def ica_steps_ld(x1, w_init, kmax):
    """W_0 = polar(w_init); W_k = polar(tanh(W X1) X1^T / n - diag(rowmean(1 - tanh^2)) W): [(W_k, cond_2(D_k), max |S_k|)] for
    k = 1 .. kmax, in long double.  x1 (nc x n) and w_init arrive already rounded to the dtype under test."""
    x = np.asarray(x1, dtype=LD)
    n = x.shape[1]
    w, _ = polar_ld(w_init)
    out = []
    for _ in range(kmax):
        s = w @ x
        g = np.tanh(s)
        gp = (LD(1) - g * g).sum(axis=1) / LD(n)
        d = (g @ x.T) / LD(n) - gp[:, None] * w
        w, _ = polar_ld(d)
        out.append((w, float(np.linalg.cond(d.astype(np.float64))), float(np.abs(s).max())))
    return out


def _polar_svd32(d):
    u, _, vt = np.linalg.svd(d)
    return u @ vt


def ica_steps_model32(x1, w_init, kmax):
    """the same statement with every array and operation in numpy float32, the polar factor from numpy's float32 SVD"""
    x = np.ascontiguousarray(x1, dtype=np.float32)
    n = np.float32(x.shape[1])
    w = _polar_svd32(np.asarray(w_init, dtype=np.float32))
    out = []
    for _ in range(kmax):
        g = np.tanh(w @ x)
        gp = (np.float32(1) - g * g).sum(axis=1, dtype=np.float32) / n
        w = _polar_svd32((g @ x.T) / n - gp[:, None] * w)
        assert w.dtype == np.float32
        out.append(w)
    return out


# ------------------------------------------------------------------------------------------- A. the FastICA loop, k iterations
# (n, nc, dtype, kmax, seed): the kernels the shape is meant to reach, read off op_ica_prepare / op_ica_step / op_ica_tail
# (csrc/kernels/host_small.inc), split-product mode | fp32-MFMA mode
ICA_ROWS = [
    (255, 3, "f32", 1, 11),      # k_ica_simple<float> (n < 256) in both modes; tail on scalar products
    (256, 16, "f32", 3, 12),     # k_ica3<1>, tail NTS = 1 | k_ica_mfma<1>
    (4099, 17, "f32", 3, 13),    # k_ica_planes<1> + k_ica3p<2>, ragged last 32-row block, tail on scalar products | k_ica_mfma<2>
    (20000, 32, "f32", 1, 14),   # k_ica_planes<1> + k_ica3p<2>, tail NTS = 2 | k_ica_mfma<2>
    (5000, 40, "f32", 3, 15),    # k_ica3<3> (NT = 3: no prepared planes) | k_ica_mfma<3>
    (9000, 48, "f32", 1, 16),    # k_ica3<3>, tail NTS = 3 | k_ica_mfma<3>
    (20011, 64, "f32", 3, 17),   # k_ica_planes<2> + k_ica3p<4>, tail NTS = 4 | k_ica_mfma<4>
    (70033, 49, "f32", 1, 18),   # k_ica3p<4>, 2189 row blocks > 2048: two blocks per wave, last wave one | three tiles per wave, last wave one
    (3000, 65, "f32", 2, 19),    # nc > 64: op_gemm_xp, k_tanh_inplace, op_colsum, op_gemm_atb, k_ica_big_out; Jacobi tail (MB = 0)
    (2000, 80, "f32", 2, 20),    # the same, five component tiles
    (300, 2, "f64", 1, 21),      # k_ica_simple<double>
    (3000, 5, "f64", 3, 22),     # k_ica_simple<double>
    (3000, 33, "f64", 1, 23),    # k_ica_simple<double>, tail on scalar products (MB = 3)
    (2000, 80, "f64", 1, 24),    # the GEMM path on the fp64 kernels, Jacobi tail
]
# saturated input (x1 * 20: max |W0 x| > 50, tanh_fast's exp2 overflows / underflows and must still give +-1) and the layouts of x1
ICA_EXTRA_ROWS = [(4099, 17, "f32", 13), (20011, 64, "f32", 17), (3000, 5, "f64", 22)]
_DT = {"f32": np.float32, "f64": np.float64}
_cache = {}


def ica_inputs(n, nc, dt, seed, scale=1.0):
    """x1 (nc x n, C-contiguous, whitened as the existing FastICA tests whiten) and w_init = Q + 0.1 N / sqrt(nc), both rounded to dt.
    (The perturbation is scaled by 1 / sqrt(nc) so that its spectral norm stays near 0.2 at every size: cond(w_init) < 2 -- asserted
    -- and the first decorrelation adds nothing to the error budget.)"""
    key = ("in", n, nc, dt, seed, scale)
    if key not in _cache:
        x = po.synth_ica(n, nc, nc, seed=seed, dtype=np.float64)
        _, _, _, x1 = po.FastIcaOracle(whiten="eigh").whitening(x)
        rng = np.random.default_rng(seed + 1000)
        q, _ = np.linalg.qr(rng.standard_normal((nc, nc)))
        w0 = q + 0.1 * rng.standard_normal((nc, nc)) / np.sqrt(nc)
        assert np.linalg.cond(w0) < 2.0
        _cache[key] = (np.ascontiguousarray((x1 * scale).astype(_DT[dt])), np.ascontiguousarray(w0.astype(_DT[dt])))
    return _cache[key]


def ica_reference(n, nc, dt, kmax, seed, scale=1.0):
    """(long-double trajectory, model trajectory) of a row: computed once, whatever the GEMM mode and the k asked for"""
    key = ("ref", n, nc, dt, kmax, seed, scale)
    if key not in _cache:
        x1, w0 = ica_inputs(n, nc, dt, seed, scale)
        ref = ica_steps_ld(x1, w0, kmax)
        if dt == "f32":
            model = ica_steps_model32(x1, w0, kmax)
        else:
            model = [po.ica_par(x1, 0.0, k, w0)[0] for k in range(1, kmax + 1)]
        _cache[key] = (ref, model)
    return _cache[key]


def ica_bound(n, nc, dt, e_model):
    if dt == "f32":
        return MULT32 * max(e_model, 2.0 ** -24)
    return MULT64 * max(e_model, 2.0 ** -52 * (nc + np.sqrt(n)))


def ica_step_check(ctx, n, nc, dt, kmax, seed, k, scale=1.0):
    """k iterations of the loop from the same x1 and w_init, W compared elementwise with the long double"""
    x1, w0 = ica_inputs(n, nc, dt, seed, scale)
    ref, model = ica_reference(n, nc, dt, kmax, seed, scale)
    w_ld, cond_d, smax = ref[k - 1]
    if scale != 1.0:
        assert ref[0][2] > 50.0, ref[0][2]      # the case saturates: |W0 x| beyond where exp2 overflows in float32
    w, ni = petal.ica_par(x1, 0.0, k, w0, petal.ICA_TEXTBOOK, ctx)
    assert ni == k, (ni, k)
    assert w.dtype == _DT[dt]
    e_model = float(np.abs(model[k - 1].astype(LD) - w_ld).max())
    err = float(np.abs(w.astype(LD) - w_ld).max())
    bound = ica_bound(n, nc, dt, e_model)
    assert bound <= GUARD, f"vacuous bound {bound:.2e} (cond(D) = {cond_d:.0f}): another seed or a smaller k, never another guard"
    ica_step_check.last = {"cond_d": cond_d, "smax": smax}
    return err, e_model, bound


def ica_layout_check(ctx, n, nc, dt, seed, device):
    """The ABI takes the crate's nc x n matrix in any layout: a C-contiguous nc x n host array (its transposed view is gathered on the
    device), the transpose of a C-contiguous n x nc host array (pitched copy), device tensors in both layouts, and for nc = 64 the
    first 64 columns of an n x 80 device tensor viewed transposed (zero-copy ingest, leading dimension 80 > nc).  The same kernels on
    the same numbers: the SAME BYTES.  Returns the number of W entries that differ from the first layout's, summed over the layouts."""
    x1, w0 = ica_inputs(n, nc, dt, seed)
    first, ni = petal.ica_par(x1, 0.0, 1, w0, petal.ICA_TEXTBOOK, ctx)
    assert ni == 1 and np.all(np.isfinite(first))
    others = [np.ascontiguousarray(x1.T).T]
    if device:
        import torch
        others.append(torch.from_numpy(x1).cuda())
        others.append(torch.from_numpy(np.ascontiguousarray(x1.T)).cuda().T)
    diff = 0
    for x in others:
        assert tuple(x.shape) == (nc, n)
        w, _ = petal.ica_par(x, 0.0, 1, w0, petal.ICA_TEXTBOOK, ctx)
        diff += int(np.count_nonzero(w.view(np.uint8) != first.view(np.uint8)))
    if device and nc == 64:
        wide = torch.zeros((n, 80), dtype=torch.float32 if dt == "f32" else torch.float64, device="cuda")
        wide[:, :64] = torch.from_numpy(np.ascontiguousarray(x1.T)).cuda()
        wide[:, 64:] = 7.0     # (whatever lies beyond the component columns is not the kernels' to read)
        w, _ = petal.ica_par(wide[:, :64].T, 0.0, 1, w0, petal.ICA_TEXTBOOK, ctx)
        assert ctx.stats()["x_zero_copy"] == 1, ctx.stats()
        diff += int(np.count_nonzero(w.view(np.uint8) != first.view(np.uint8)))
    return float(diff), 0.0, 0.0


# ------------------------------------------------------------------------------------------- B. textbook symmetric decorrelation
DECORR_SIZES = [1, 2, 3, 15, 16, 17, 33, 48, 64, 65, 96, 130]
DECORR_CONDS = [1.0, 1e2, 1e4, 1e6]


def decorr_input(nc, cond, dt):
    """W = 37 U diag(logspace(0, -log10 cond, nc)) V^T from seeded orthogonal U, V (37: the scaling by ||W||_F is checked too)"""
    rng = np.random.default_rng(5000 + 7 * nc + int(round(np.log10(cond))))
    u, _ = np.linalg.qr(rng.standard_normal((nc, nc)))
    v, _ = np.linalg.qr(rng.standard_normal((nc, nc)))
    return np.ascontiguousarray((37.0 * (u * np.logspace(0.0, -np.log10(cond), nc)) @ v.T).astype(_DT[dt]))


def decorr_check(ctx, nc, cond, dt):
    w = decorr_input(nc, cond, dt)
    key = ("polar", nc, cond, dt)
    if key not in _cache:
        q, _ = polar_ld(w)
        sv = np.linalg.svd(w.astype(np.float64), compute_uv=False)
        e_model = float(np.abs(po.symmetric_decorrelation(w.astype(np.float64)).astype(LD) - q).max())
        _cache[key] = (q, float(sv.max() / sv.min()), e_model)
    q, cond2, e_model = _cache[key]
    out = petal.symmetric_decorrelation(w, petal.ICA_TEXTBOOK, ctx)
    assert out.dtype == _DT[dt] and out.shape == (nc, nc)
    o = out.astype(LD)
    err = float(np.abs(o - q).max())
    orth = float(np.abs(o @ o.T - np.eye(nc, dtype=LD)).max())
    bound = 2.0 ** -52 * (16.0 + cond2 * cond2) + (2.0 ** -23 if dt == "f32" else 0.0)
    decorr_check.last = {"err": err, "orth": orth, "cond2": cond2}
    return max(err, orth), e_model, bound


# ------------------------------------------------------------------------------------------- C. svd_flip
def flip_rule(u, vt):
    """src/pca.rs:815-850 restated: the pairs are the columns of u zipped with the rows of vt; in each column the FIRST element of
    maximal |u| decides (the scan replaces its candidate only on a strict '>', pca.rs:830, and starts from the first element,
    pca.rs:821-827); when that element's sign bit is set (Rust's signum: -1 for -0.0 too) every element of the column and of the
    row is multiplied by -1 -- every sign bit changes, those of zeros included.  Returns the expected (u, vt)."""
    u, vt = u.copy(), vt.copy()
    for j in range(min(u.shape[1], vt.shape[0])):
        if u.shape[0] == 0:
            continue
        a = np.abs(u[:, j])
        first = int(np.flatnonzero(a == a.max())[0])
        if np.signbit(u[first, j]):
            u[:, j] = -u[:, j]
            vt[j, :] = -vt[j, :]
    return u, vt


FLIP_NS = [1, 2, 255, 256, 257, 4099, 100003]
FLIP_COLS = [1, 7, 64, 65, 200]
FLIP_DELTAS = [-1, 0, 2]
_PLANTS = ["adjacent", "lanes", "same_final_lane", "other_final_lane", "first_last", "zero_neg", "zero_pos", "last_row", "none"]


def flip_input(n, cols, vrows, dt, seed):
    """Integer-valued data in [-40, 40] with the value 77, beyond the data's range, planted in chosen columns: the maximum twice with
    opposite signs -- in adjacent rows; in rows r and r + 1 .. r + 3 of one 256-row part (other row lanes of k_absmax_part2); in
    parts p and p + 64 (the SAME lane of k_absmax_final: needs 256-row parts and more than 64 of them); in neighbouring parts
    (different lanes); in the first and the last row -- the earlier one negative in half of the columns, the later one in the other
    half; an all-zero column starting with -0.0 and one starting with +0.0; a column whose only maximum is in the last row."""
    rng = np.random.default_rng(seed)
    u = rng.integers(-40, 41, (n, cols)).astype(_DT[dt])
    vt = rng.integers(-40, 41, (vrows, 1 + seed % 37)).astype(_DT[dt])
    planted = []
    for j in range(cols):
        kind = _PLANTS[(j + seed) % len(_PLANTS)]
        s = -1.0 if ((j + seed) // len(_PLANTS)) % 2 == 0 else 1.0      # sign of the EARLIER of the two maxima
        pair = None
        if kind == "adjacent" and n >= 2:
            r = int(rng.integers(0, n - 1)); pair = (r, r + 1)
        elif kind == "lanes" and n >= 5:
            b = 256 * int(rng.integers(0, (n + 255) // 256 - (n % 256 in (1, 2, 3, 4))))    # a 256-row part with five rows or more
            r = b + int(rng.integers(0, min(256, n - b) - 4))
            pair = (r, r + 1 + j % 3)
        elif kind == "same_final_lane" and n > 256 * 66:
            p = int(rng.integers(0, n // 256 - 64)); pair = (256 * p + int(rng.integers(0, 256)), 256 * (p + 64) + int(rng.integers(0, 256)))
        elif kind == "other_final_lane" and n > 512:
            p = int(rng.integers(0, n // 256 - 1)); pair = (256 * p + int(rng.integers(0, 256)), 256 * (p + 1) + int(rng.integers(0, 256)))
        elif kind == "first_last" and n >= 2:
            pair = (0, n - 1)
        elif kind == "zero_neg":
            u[:, j] = 0.0; u[0, j] = -0.0
        elif kind == "zero_pos":
            u[:, j] = 0.0
            if n >= 2:
                u[1:, j] = -0.0      # (not greater than |+0.0|: the first element still decides)
        elif kind == "last_row":
            u[n - 1, j] = -77.0 if s < 0 else 77.0
        else:
            kind = "none"
        if pair:
            assert 0 <= pair[0] < pair[1] < n, (kind, pair, n)
            u[pair[0], j] = 77.0 * s
            u[pair[1], j] = -77.0 * s
        planted.append(kind)
    return u, vt, planted


def flip_check(ctx, n, cols, vrows, dt, seed, device=False, strided=False):
    """svd_flip in place on u (n x cols) and vt (vrows x d) against flip_rule: equal values and equal sign bits.  Returns the number
    of elements that differ.  strided: u is every second column of a wider host array, whose other columns must stay untouched."""
    u, vt, _ = flip_input(n, cols, vrows, dt, seed)
    ue, ve = flip_rule(u, vt)
    if device:
        import torch
        ut, vtt = torch.from_numpy(u).cuda(), torch.from_numpy(vt).cuda()
        petal.svd_flip(ut, vtt, ctx)
        uo, vo = ut.cpu().numpy(), vtt.cpu().numpy()
    elif strided:
        wide = np.full((n, 2 * cols), 5.0, dtype=u.dtype)
        wide[:, ::2] = u
        petal.svd_flip(wide[:, ::2], vt, ctx)
        assert np.all(wide[:, 1::2] == 5.0)
        uo, vo = wide[:, ::2], vt
    else:
        petal.svd_flip(u, vt, ctx)
        uo, vo = u, vt
    bad = int(np.count_nonzero(uo != ue)) + int(np.count_nonzero(np.signbit(uo) != np.signbit(ue)))
    bad += int(np.count_nonzero(vo != ve)) + int(np.count_nonzero(np.signbit(vo) != np.signbit(ve)))
    return float(bad), 0.0, 0.0


def flip_cases(device_too):
    """every (n, u.cols) pair once, vt.rows - u.cols, dtype and memory space rotating over them, the extremes with the other row
    counts too: 40 cases + the strided one"""
    cases = []
    for i, n in enumerate(FLIP_NS):
        for j, cols in enumerate(FLIP_COLS):
            cases.append((n, cols, cols + FLIP_DELTAS[(i + j) % 3], ["f32", "f64"][(i + j) % 2], 100 * i + j, device_too and (i + 2 * j) % 4 < 2))
    for t, (n, cols, delta) in enumerate([(1, 1, 0), (1, 200, -1), (100003, 1, 2), (100003, 200, 2), (100003, 200, 0)]):
        cases.append((n, cols, cols + delta, ["f64", "f32"][t % 2], 900 + t, device_too and t % 2 == 1))
    return cases


# ------------------------------------------------------------------------------------------- the case tables
class Case:
    def __init__(self, name, fn, *args, **kw):
        self.id, self.fn, self.args, self.kw = name, fn, args, kw

    def run(self, ctx):
        return self.fn(ctx, *self.args, **self.kw)

    def __repr__(self):
        return self.id


def all_cases(device=True, reduced=False):
    """device: torch.cuda inputs too (the HIP library); reduced: the CPU suite's table -- without the two largest float32 rows of A
    (and what hangs on them); every dtype, every k, every kernel family, all of B and C stay."""
    cases = []
    for n, nc, dt, kmax, seed in ICA_ROWS:
        if reduced and (n, nc) in ((20011, 64), (70033, 49)):
            continue
        for k in range(1, kmax + 1):
            cases.append(Case(f"ica-{n}x{nc}-{dt}-k{k}", ica_step_check, n, nc, dt, kmax, seed, k))
    for n, nc, dt, seed in ICA_EXTRA_ROWS:
        if reduced and nc == 64:
            continue
        cases.append(Case(f"ica-saturated-{n}x{nc}-{dt}", ica_step_check, n, nc, dt, 1, seed, 1, scale=20.0))
        cases.append(Case(f"ica-layouts-{n}x{nc}-{dt}", ica_layout_check, n, nc, dt, seed, device))
    for nc in DECORR_SIZES:
        for cond in DECORR_CONDS:
            cases.append(Case(f"decorr-{nc}-cond1e{int(round(np.log10(cond)))}-f64", decorr_check, nc, cond, "f64"))
            if cond <= 1e2:
                cases.append(Case(f"decorr-{nc}-cond1e{int(round(np.log10(cond)))}-f32", decorr_check, nc, cond, "f32"))
    for t, (n, cols, vrows, dt, seed, dev) in enumerate(flip_cases(device)):
        cases.append(Case(f"flip-{n}x{cols}-vt{vrows}-{dt}-{'cuda' if dev else 'host'}", flip_check, n, cols, vrows, dt, seed, device=dev))
    cases.append(Case("flip-4099x65-vt65-f32-strided", flip_check, 4099, 65, 65, "f32", 77, strided=True))
    return cases


def main():
    import time
    cases = all_cases()
    print("# case | GEMM mode | error | model error | error / model | bound   (exact cases: error = number of differing elements)")
    t0 = time.time()
    worst = {}
    for mode in ("bf16x3", "fp32"):
        ctx = petal.Context(0)
        ctx.set_gemm_mode(mode)
        for c in cases:
            err, model, bound = c.run(ctx)
            ratio = err / model if model > 0 else float("nan")
            flag = "" if err <= bound else "   <-- ABOVE THE BOUND"
            print(f"{c.id:40s} {mode:7s} {err:10.3e} {model:10.3e} {ratio:8.3f} {bound:10.3e}{flag}")
            if c.fn is ica_step_check:
                key = (c.args[2], mode)
                floor = 2.0 ** -24 if c.args[2] == "f32" else 2.0 ** -52 * (c.args[1] + np.sqrt(c.args[0]))
                if ratio > worst.get(key, (0, 0, ""))[0]:
                    worst[key] = (ratio, err / max(model, floor), c.id)
        ctx.close()
    for (dt, mode), (r, rf, cid) in sorted(worst.items()):
        print(f"# table A, {dt}, {mode}: largest error / model {r:.3f} ({cid}; {rf:.3f} of max(model, floor))")
    print(f"# wall time {time.time() - t0:.0f} s (references computed once, both modes)")


if __name__ == "__main__":
    main()
