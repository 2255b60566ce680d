"""Segmented Pca (include/petal_hip_segments.h: petal_pca_fit_segments and its transform entries) -- inputs, references, models and
bounds, in the manner of tests/score_cases.py.  Shared by tests/test_gpu_segments.py (the HIP library: the segment kernel, and the loop
for d > 64) and tests/test_segments_host.py (references and models against their own bounds, and the loop on the host simulation).

Inputs: per segment of n_b rows a planted spectrum sigma_i = 10 sqrt(n_b) 0.7^i (i < min(n_b, d)) on seeded random orthonormal factors,
plus N(0, 1) column means (one case: means 40 column standard deviations off the origin), rounded to the dtype under test.

The REFERENCE: the segment centred in numpy.longdouble, rounded to float64, numpy.linalg.svd; svd_flip restated from pca.rs:815-850 (per
column of U the first element of largest magnitude decides; a negative one flips the column and the row of V^T).  The MODEL is the
statement of the segment kernel at working precision -- float64 means, float64 centred Gram matrix, numpy.linalg.eigh -- with outputs
rounded to the data's type; never the library's output.

Errors per segment: singular values relative to sigma_1; components elementwise (rows are unit vectors); y relative to the largest
|y| of the segment; means relative to the largest |mean| or column scale; the total variance relatively.  Each is held to
    MULT max(model error, d eps)          eps of the data's type
per segment and quantity.  The multipliers start at the project's starting values (4 for float32, 16 for float64); after the first run
on the MI355X the largest ratio per family goes to profiles/segments_errors.txt and each multiplier comes down to twice that, rounded
up -- never up.

Signs: a component's sign is asserted wherever, in the reference's column of U, the deciding |u| exceeds the runner-up by more than
1e-3 relative; elsewhere the comparison is sign-invariant (the project's rule for near-ties).
Components are compared where the reference has sigma_j > 1e-3 sigma_1: the Gram route's accuracy statement (eps (sigma_1 / sigma_j)^2
over the gap) promises nothing for a direction below that.  In this table only exact rank deficiency falls below (the one-row centred
segment, sigma = 0: its singular value and means are asserted, as everywhere).  For the same reason centred segments have at least
k + 1 rows (k centred rows have rank k - 1: the k-th direction is arbitrary and its sigma is rounding noise of size sqrt(eps) sigma_1 on
the Gram route); segments of exactly k rows are fitted uncentred.

`python tests/segments_cases.py` runs the table on petal.Context(0) and prints one line per case."""
import os
import sys
from functools import lru_cache

import numpy as np

if __name__ == "__main__":      # (run as a script: the package is found from the repository root)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import petal_decomposition_amd as petal

LD = np.longdouble
# started at 4 and 16; after the first run on the MI355X (profiles/segments_errors.txt): the largest ratio of an error to max(model error,
# d eps) was 0.113 for float32 (sigma, 3 x 3 uncentred: the outputs' own rounding against a floor of d eps) and 3.425 for float64
# (components at k = d = 17), so twice that, rounded up
MULT32 = 1.0
MULT64 = 7.0
SIGN_MARGIN = 1e-3
RESOLVED = 1e-3
_DT = {"f32": np.float32, "f64": np.float64}


def mix(k, nseg, centering, seed=0):
    """nseg lengths mixed from {k, k + 1, 63, 64, 65, 257, 1000}: the wave, workgroup and two-trips-per-thread boundaries (k itself only
    without centring; 1000 once in every 40 segments of a long batch)"""
    pool = ([k] if not centering else []) + [k + 1, 63, 64, 65, 257, 1000]
    pool = [max(p, k + (1 if centering else 0)) for p in pool]
    rng = np.random.default_rng([k, nseg, seed])
    out = []
    for b in range(nseg):
        p = pool[b % len(pool)]
        if p == 1000 and nseg > 8 and b % 40 != len(pool) - 1:
            p = pool[int(rng.integers(0, len(pool) - 1))]
        out.append(int(p))
    return tuple(out)


class Case:
    """d columns, k components ("d": k = d), segment lengths; layout: "host" (row-major numpy) | "hostF" (column-major numpy) | "dev" (a
    strided torch device tensor: a column slice of a wider matrix; device y); off: the means are `off` column standard deviations away"""

    def __init__(self, d, k, lengths, dt, centering=True, layout="host", want_y=False, off=0.0, seed=0):
        self.d, self.k, self.lengths, self.dt = d, (d if k == "d" else k), tuple(lengths), dt
        self.centering, self.layout, self.want_y, self.off, self.seed = centering, layout, want_y, off, seed

    @property
    def nseg(self):
        return len(self.lengths)

    @property
    def id(self):
        ls = "+".join(map(str, self.lengths)) if self.nseg <= 3 else f"{self.nseg}segs"
        return (f"d{self.d}-k{self.k}-{ls}-{self.dt}-{'c' if self.centering else 'nc'}-{self.layout}{'-y' if self.want_y else ''}"
                f"{'-off%g' % self.off if self.off else ''}")

    __repr__ = __str__ = lambda self: self.id

    @property
    def key(self):
        return (self.d, self.k, self.lengths, self.dt, self.centering, self.off, self.seed)

    @property
    def on_kernel(self):
        return self.d <= 64


# d of one tile (1, 3, 16), one column more (17), three and four tiles ragged and full (33, 48, 64), and 65 on the loop; k of 1, 4 and d
# (k = d where the planted spectrum stays resolved: d <= 17); 1, 2 and 300 segments (more than one workgroup per CU).
CASES = [
    Case(1, 1, (2, 63), "f64"),
    Case(3, "d", (3, 65), "f32", centering=False, want_y=True),
    Case(3, 1, (1, 64), "f64"),                                            # the one-row centred segment: sigma = 0
    Case(16, 4, mix(4, 300, True), "f64", want_y=True),
    Case(16, 4, mix(4, 300, True, 1), "f32", layout="dev", want_y=True),
    Case(16, "d", (16, 257), "f64", centering=False, layout="hostF", want_y=True),
    Case(16, 1, (1000,), "f32"),
    Case(17, "d", (18, 1000), "f64", want_y=True),
    Case(17, 4, (4, 65), "f32", centering=False, layout="hostF"),
    Case(33, 4, (63, 257), "f64", layout="dev", want_y=True),
    Case(33, 1, mix(1, 300, True), "f32"),
    Case(48, 4, (64, 1000), "f32", want_y=True),
    Case(48, 4, (257,), "f64", centering=False, layout="hostF"),
    Case(64, 4, (65, 1000), "f64", want_y=True),
    Case(64, 4, mix(4, 300, True, 2), "f32", layout="dev", want_y=True),
    Case(64, 1, (257, 64), "f64", off=40.0),
    Case(65, 4, (66, 257), "f64", want_y=True),
    Case(65, 4, (4, 65), "f32", centering=False, layout="dev"),
]


def all_cases(reduced=False):
    """reduced: the table without its 300-segment cases (the CPU suite's share)"""
    return [c for c in CASES if not (reduced and c.nseg > 8)]


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.int64)


# ------------------------------------------------------------------------------------------- inputs
@lru_cache(maxsize=None)
def inputs(d, k, lengths, dt, centering, off, seed):
    """x (all rows, rounded to the dtype under test, read-only)"""
    T = _DT[dt]
    rng = np.random.default_rng([d, k, len(lengths), seed, 11])
    blocks = []
    for n in lengths:
        r = min(n, d)
        u = np.linalg.qr(rng.standard_normal((n, r)))[0]
        v = np.linalg.qr(rng.standard_normal((d, r)))[0]
        sig = 10.0 * np.sqrt(n) * 0.7 ** np.arange(r)
        xb = (u * sig) @ v.T
        mu = rng.standard_normal(d)
        if off:
            mu = off * np.sqrt((xb * xb).mean()) * rng.choice([-1.0, 1.0], d)
        blocks.append(xb + mu)
    x = np.concatenate(blocks, axis=0).astype(T) if blocks else np.zeros((0, d), T)
    x.setflags(write=False)
    return x


def svd_flip(u, vt):
    """pca.rs:815-850: (u, vt, margin per column) -- margin: by how much, relatively, the deciding |u| exceeds the runner-up"""
    u, vt = u.copy(), vt.copy()
    margin = np.ones(u.shape[1])
    for j in range(u.shape[1]):
        a = np.abs(u[:, j])
        i = int(np.argmax(a))                       # the first index of the largest magnitude (the crate skips on abs <= absmax)
        if a[i] == 0:
            margin[j] = 0.0
            continue
        rest = np.delete(a, i)
        margin[j] = 1.0 if rest.size == 0 else float((a[i] - rest.max()) / a[i])
        if u[i, j] < 0:
            u[:, j] = -u[:, j]
            vt[j] = -vt[j]
    return u, vt, margin


class Seg:
    """one segment's results: comp (k x d), mean (d), sing (k), tv, y (n x k), margin (k; reference only)"""


def _segment(xb, k, centering, how, T):
    s = Seg()
    n, d = xb.shape
    if how == "reference":
        mu = xb.astype(LD).mean(axis=0) if centering and n else np.zeros(d, LD)
        xc = (xb.astype(LD) - mu).astype(np.float64)
        u, sig, vt = np.linalg.svd(xc, full_matrices=False)
        u, vt, margin = svd_flip(u, vt)
        s.mean, s.sing, s.comp = np.asarray(mu, np.float64), sig[:k], vt[:k]
        s.tv, s.y, s.margin = float((sig * sig).sum()), u[:, :k] * sig[:k], margin[:k]
        s.sing_all = sig
        return s
    mu = xb.astype(np.float64).mean(axis=0) if centering and n else np.zeros(d)
    xc = xb.astype(np.float64) - mu
    lam, v = np.linalg.eigh(xc.T @ xc)
    lam, v = lam[::-1], v[:, ::-1]
    sig = np.sqrt(np.maximum(lam, 0.0))
    y = xc @ v[:, :k]
    _, vt, _ = svd_flip(y, v[:, :k].T)
    sg = np.sign((vt * v[:, :k].T).sum(axis=1))
    sg[sg == 0] = 1.0
    s.mean, s.sing, s.comp = mu.astype(T), sig[:k].astype(T), vt.astype(T)
    s.tv, s.y = T(np.trace(xc.T @ xc)), (y * sg).astype(T)
    return s


def _all(key, how):
    d, k, lengths, dt, centering, off, seed = key
    x = inputs(*key)
    off_ = offsets_of(lengths)
    return [_segment(x[off_[b]:off_[b + 1]], k, centering, how, _DT[dt]) for b in range(len(lengths))]


@lru_cache(maxsize=None)
def reference(key):
    return _all(key, "reference")


@lru_cache(maxsize=None)
def model(key):
    return _all(key, "model")


def seg_errors(got, ref, T):
    """{quantity: error} of one segment's results against its reference"""
    k = ref.sing.shape[0]
    s1 = float(ref.sing_all[0]) if ref.sing_all.size and ref.sing_all[0] > 0 else 1.0
    e = {"sing": float(np.abs(np.asarray(got.sing, np.float64) - ref.sing).max() / s1) if k else 0.0}
    scale = max(float(np.abs(ref.mean).max()) if ref.mean.size else 0.0, s1 / np.sqrt(max(ref.y.shape[0], 1)), 1e-300)
    e["mean"] = float(np.abs(np.asarray(got.mean, np.float64) - ref.mean).max() / scale) if ref.mean.size else 0.0
    e["tv"] = abs(float(got.tv) - ref.tv) / ref.tv if ref.tv > 0 else abs(float(got.tv))
    ec, ey = 0.0, 0.0
    ymax = float(np.abs(ref.y).max()) if ref.y.size else 0.0
    for j in range(k):
        if not ref.sing[j] > RESOLVED * s1:
            continue
        gc, rc = np.asarray(got.comp[j], np.float64), ref.comp[j]
        dc = np.abs(gc - rc).max()
        gy = None if got.y is None else np.asarray(got.y[:, j], np.float64)
        dy = 0.0 if gy is None else np.abs(gy - ref.y[:, j]).max()
        if not ref.margin[j] > SIGN_MARGIN:          # a near-tie: either sign, but the same one for the component and its y
            dc2 = np.abs(gc + rc).max()
            if dc2 < dc:
                dc, dy = dc2, (0.0 if gy is None else np.abs(gy + ref.y[:, j]).max())
        ec, ey = max(ec, float(dc)), max(ey, float(dy) / ymax if ymax > 0 else 0.0)
    e["comp"], e["y"] = ec, ey
    return e


QUANTITIES = ("sing", "mean", "tv", "comp", "y")


@lru_cache(maxsize=None)
def model_errors(key):
    T = _DT[key[3]]
    return [seg_errors(m, r, T) for m, r in zip(model(key), reference(key))]


def mult_of(dt, mult32=None, mult64=None):
    return (MULT32 if mult32 is None else mult32) if dt == "f32" else (MULT64 if mult64 is None else mult64)


def bounds(key, mult32=None, mult64=None):
    """per segment {quantity: bound}"""
    T = _DT[key[3]]
    floor = max(key[0], 1) * float(np.finfo(T).eps)
    mult = mult_of(key[3], mult32, mult64)
    return [{q: mult * max(em[q], floor) for q in QUANTITIES} for em in model_errors(key)]


def signed_share(cases):
    """(pairs asserted with sign, all (segment, component) pairs) over the cases"""
    signed = total = 0
    for c in cases:
        for r in reference(c.key):
            total += r.margin.size
            signed += int((r.margin > SIGN_MARGIN).sum())
    return signed, total


# ------------------------------------------------------------------------------------------- the library
def laid_out(case, x):
    if case.layout == "hostF":
        xf = np.asfortranarray(x)
        assert not xf.flags["C_CONTIGUOUS"] or x.shape[1] == 1
        return xf
    if case.layout == "dev":
        import torch
        wide = torch.zeros((x.shape[0], x.shape[1] + 3), dtype=torch.from_numpy(np.zeros(1, x.dtype)).dtype, device="cuda")
        wide[:, 1:1 + x.shape[1]] = torch.from_numpy(np.array(x)).cuda()
        return wide[:, 1:1 + x.shape[1]]
    return x


def to_numpy(a):
    return a.cpu().numpy() if petal._is_torch(a) else np.asarray(a)


def fit(case, ctx):
    """(model, y or None as numpy) from the library"""
    x = inputs(*case.key)
    hostsim = getattr(ctx.lib, "_petal_host_buffers", False)      # (the host simulation has no device tensors)
    xin = x if (case.layout == "dev" and hostsim) else laid_out(case, x)
    m = petal.SegmentedPca(case.k, centering=case.centering, ctx=ctx)
    off = offsets_of(case.lengths)
    y = None
    if case.want_y:
        y = m.fit_transform(xin, off)
        if petal._is_torch(xin) and xin.is_cuda:
            assert petal._is_torch(y) and y.is_cuda
        y = to_numpy(y)
    else:
        m.fit(xin, off)
    return m, y


def segments_of(m, y, lengths):
    off = offsets_of(lengths)
    out = []
    for b in range(len(lengths)):
        s = Seg()
        s.comp, s.mean, s.sing, s.tv = m.components[b], m.mean[b], m.singular_values[b], m.total_variance[b]
        s.y = None if y is None else y[off[b]:off[b + 1]]
        out.append(s)
    return out


def check(case, ctx, report=None):
    T = _DT[case.dt]
    m, y = fit(case, ctx)
    assert m.components.shape == (case.nseg, case.k, case.d) and m.components.dtype == T
    assert m.mean.shape == (case.nseg, case.d) and m.singular_values.shape == (case.nseg, case.k)
    assert np.all(m.status == 0)
    if y is not None:
        assert y.shape == (sum(case.lengths), case.k) and y.dtype == T
    ref, bnd, em = reference(case.key), bounds(case.key), model_errors(case.key)
    floor = max(case.d, 1) * float(np.finfo(T).eps)
    worst = {q: (0.0, 0.0, 0.0, 0) for q in QUANTITIES}       # (ratio to max(model, floor), error, bound, segment)
    failures = []
    for b, got in enumerate(segments_of(m, y, case.lengths)):
        e = seg_errors(got, ref[b], T)
        for q in QUANTITIES:
            ratio = e[q] / max(em[b][q], floor)
            if ratio > worst[q][0]:
                worst[q] = (ratio, e[q], bnd[b][q], b)
            if not e[q] <= bnd[b][q]:
                failures.append((case.id, q, b, e[q], bnd[b][q]))
    line = f"{case.id}: kernel_segments {m.kernel_segments}  " + "  ".join(
        f"{q} ratio {worst[q][0]:.3f} (e {worst[q][1]:.2e}, bound {worst[q][2]:.2e}, seg {worst[q][3]})" for q in QUANTITIES)
    print(line)
    if report is not None:
        report.append(line)
    assert not failures, failures[:5]
    return m, y


if __name__ == "__main__":
    c = petal.Context(0)
    for case in all_cases():
        try:
            check(case, c)
        except AssertionError as e:     # (a missed bound is a finding to print, the table goes on; anything else ends the run)
            print(f"FAIL {case.id}: {e}")
