"""IncrementalPca (include/petal_hip_ipca.h): the generators, the long-double reference of the statistic, the float64 numpy model of the
batch recurrence, the case tables with their bounds, and the checks the GPU suite and the host suite share.

The statistic is (n, mean, M2 = sum (x - mean)(x - mean)^T).  Its error is measured against a numpy.longdouble two-pass reference of the
concatenated data (widened exactly from the stored type) and expressed over the error of the MODEL -- the recurrence of the header
restated in float64 numpy, batch by batch -- with a floor so that exact zeros do not divide by zero:

    ratio = max |M2 - ref| / max(max |M2_model - ref|, FLOOR_EPS eps64 max diag(ref))

MULTIPLIER holds, per family, twice the largest ratio measured on the device and on the host simulation (profiles/ipca_errors.txt;
the convention of profiles/smallmat_errors.txt), and on every case but the drift case the bound itself -- multiplier x max(model, floor)
-- must stay below CAP = 1e-12 of the largest diagonal entry of M2, so that the bound cannot hide a lost precision.

Run as a script on a machine with the GPU it writes profiles/ipca_errors.txt: the device's rows and the host simulation's."""
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
from parity_cases import rowwise_rel  # noqa: E402

EPS64 = float(np.finfo(np.float64).eps)
FLOOR_EPS = 4.0          # the floor of the model error: 4 eps64 of the largest diagonal entry of the reference M2
CAP = 1e-12              # of the largest diagonal entry: no bound of a non-drift case may exceed it
KERNEL_MAX_D = petal.IPCA_KERNEL_MAX_D


# ------------------------------------------------------------------------------------------- batches
def cut(n, lengths):
    """row ranges [(a, b), ...] of consecutive batches of the given lengths; they must add up to n"""
    edges = np.concatenate([[0], np.cumsum(lengths)])
    assert edges[-1] == n, (n, lengths)
    return [(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]


def unequal(n, parts, seed=0):
    """n rows in `parts` unequal non-empty batches (1 part: the whole matrix)"""
    if parts == 1:
        return [n]
    rng = np.random.default_rng(seed + parts)
    w = rng.random(parts) + 0.2
    lens = np.maximum(1, np.floor(w / w.sum() * n).astype(int))
    lens[-1] += n - lens.sum()
    assert lens.min() >= 1 and lens.sum() == n
    return [int(v) for v in lens]


# ------------------------------------------------------------------------------------------- 1. exact integers
# Batch lengths of the integer test: 0 (no-op), 1, 15 / 16 / 17 (one short of, exactly, one past the kernel's 16-row step), 200 (three
# row chunks of the launcher's split: 80 + 80 + 40 rows at these widths).
INT_LENGTHS = (0, 1, 15, 16, 17, 200)
INT_WIDTHS = (1, 5, 16, 33, 65)          # below one 16-column tile, one tile, a 32-row slice plus one, a 64-column panel plus one
INT_WIDTHS_GPU = INT_WIDTHS + (64, 257)  # the seams of the 32 x 64 wave tiles: exactly one panel; four panels plus one column


def int_batches(d, dtype, seed=0, count=9):
    """batches of integers in [-8, 8] with lengths drawn from INT_LENGTHS (each length at least once)"""
    rng = np.random.default_rng(1000 * d + seed)
    lens = list(INT_LENGTHS) + [int(v) for v in rng.choice(INT_LENGTHS, size=count - len(INT_LENGTHS))]
    rng.shuffle(lens)
    return [rng.integers(-8, 9, size=(m, d)).astype(dtype) for m in lens]


def check_integers_exact(ctx, d, dtype, expect_kernel):
    """centering off: after every batch get_state equals the int64 Gram matrix of the rows seen, bit for bit"""
    m = petal.IncrementalPca(min(d, 2), centering=False, ctx=ctx)
    gram, seen, nonempty = np.zeros((d, d), dtype=np.int64), 0, 0
    for b in int_batches(d, dtype):
        m.partial_fit(b)
        bi = b.astype(np.int64)
        gram += bi.T @ bi
        seen += b.shape[0]
        nonempty += b.shape[0] > 0
        st = m.state()
        assert st["n"] == seen
        assert st["m2"].tobytes() == gram.astype(np.float64).tobytes(), (d, dtype, b.shape)
        assert not st["mean"].any()
    info = m.info()
    assert info["batches"] == nonempty and info["kernel_batches"] == (nonempty if expect_kernel else 0), info
    m.close()


# ------------------------------------------------------------------------------------------- 2. the centred statistic
StatCase = namedtuple("StatCase", "family name n d dt lengths offset drift seed")
# family f64 / f32: a mean several standard deviations from zero, graded column scales; drift: every batch 40 sigma beyond the last.
STAT_CASES = [
    StatCase("f64", "f64-1000x33", 1000, 33, "f64", (1, 15, 16, 17, 200, 301, 450), 3.0, 0.0, 21),
    StatCase("f64", "f64-777x65", 777, 65, "f64", (400, 77, 300), 5.0, 0.0, 22),
    StatCase("f32", "f32-1000x33", 1000, 33, "f32", (1, 15, 16, 17, 200, 301, 450), 3.0, 0.0, 23),
    StatCase("f32", "f32-3000x16", 3000, 16, "f32", (64, 2000, 936), 5.0, 0.0, 24),
]
# the shapes only the kernel path has a reason for: the tile seams, and a batch of more than three row chunks
STAT_CASES_GPU = STAT_CASES + [
    StatCase("f64", "f64-900x64", 900, 64, "f64", (300, 1, 599), 3.0, 0.0, 25),
    StatCase("f32", "f32-900x257", 900, 257, "f32", (17, 500, 383), 3.0, 0.0, 26),
    StatCase("f32", "f32-5000x64", 5000, 64, "f32", (4000, 1000), 3.0, 0.0, 27),      # 4000 rows: 62 row chunks
]
DRIFT_CASE = StatCase("drift", "drift-8x500x16", 4000, 16, "f64", (500,) * 8, 0.0, 40.0, 28)
# twice the largest measured ratio per family (profiles/ipca_errors.txt: f64 0.571, f32 1.885, drift 1.049 -- each on the host simulation's
# two-pass path; the streaming kernel's are 0.22, 0.88 and 0.24)
MULTIPLIER = {"f64": 1.15, "f32": 3.8, "drift": 2.1}


def np_dtype(c):
    return np.float32 if c.dt == "f32" else np.float64


@functools.lru_cache(maxsize=None)
def stat_inputs(c):
    """the case's batches (read-only, in its dtype): unit-variance noise times column scales 1 .. 4 about a mean `offset` sigma from zero;
    drift: batch b sits b * drift sigma further along every column"""
    rng = np.random.default_rng(c.seed)
    scale = np.linspace(1.0, 4.0, c.d)
    out = []
    for b, (a, e) in enumerate(cut(c.n, c.lengths)):
        x = (rng.standard_normal((e - a, c.d)) + c.offset + b * c.drift) * scale
        x = x.astype(np_dtype(c))
        x.setflags(write=False)
        out.append(x)
    return tuple(out)


def reference_stat(batches, centering=True):
    """(n, mean, M2) of the concatenation in numpy.longdouble: two passes, the data widened exactly from its stored type"""
    x = np.concatenate([np.asarray(b) for b in batches]).astype(np.longdouble)
    n = x.shape[0]
    mean = x.mean(axis=0) if centering else np.zeros(x.shape[1], dtype=np.longdouble)
    xc = x - mean
    return n, mean, xc.T @ xc


def model_stat(batches, centering=True, accumulate=np.float64):
    """The recurrence of include/petal_hip_ipca.h restated in numpy, batch by batch: the centre is the running mean (the first batch: the
    mean of its first min(m, 64) rows), x is widened to float64 before the centre is subtracted, s and G are accumulated in
    `accumulate` (float64: the model; float32: what a kernel with float32 accumulators would deliver), the update is float64."""
    n, mean, m2 = 0, None, None
    for b in batches:
        b = np.asarray(b)
        m, d = b.shape
        if mean is None:
            mean, m2 = np.zeros(d), np.zeros((d, d))
        if m == 0:
            continue
        x = b.astype(np.float64)
        if not centering:
            m2 = m2 + (x.astype(accumulate).T @ x.astype(accumulate)).astype(np.float64)
            n += m
            continue
        c = x[:min(m, 64)].mean(axis=0) if n == 0 else mean
        xc = (x - c).astype(accumulate)
        s = xc.sum(axis=0, dtype=accumulate).astype(np.float64)
        g = (xc.T @ xc).astype(np.float64)
        n += m
        mean = c + s / n
        m2 = m2 + g - np.outer(s, s) / n
    return n, mean, m2


def stat_errors(state, ref, model):
    """(error of M2, model error of M2, floor, ratio, error of the mean over eps64 (|mean| + sigma)) against the long-double reference"""
    _, rmean, rm2 = ref
    top = float(np.max(np.diag(rm2)))
    err = float(np.max(np.abs(state["m2"].astype(np.longdouble) - rm2)))
    merr = float(np.max(np.abs(model[2].astype(np.longdouble) - rm2)))
    floor = FLOOR_EPS * EPS64 * top
    sigma = np.sqrt(np.diag(rm2).astype(np.float64) / max(ref[0], 1))
    mean_err = float(np.max(np.abs(state["mean"].astype(np.longdouble) - rmean) / (EPS64 * (np.abs(rmean.astype(np.float64)) + sigma))))
    return err, merr, floor, err / max(merr, floor), mean_err, top


def feed(ctx, batches, k, centering=True, device=False):
    m = petal.IncrementalPca(k, centering=centering, ctx=ctx)
    for b in batches:
        if device:
            import torch
            b = torch.from_numpy(np.array(b)).cuda()
        m.partial_fit(b)
    return m


def check_statistic(ctx, c, expect_kernel, device=False):
    """the centred statistic of a case inside its model-tied bound, and the bound inside the cap; returns the ratio"""
    batches = stat_inputs(c)
    m = feed(ctx, batches, 1, True, device)
    st = m.state()
    info = m.info()
    m.close()
    ref, model = reference_stat(batches), model_stat(batches)
    err, merr, floor, ratio, mean_err, top = stat_errors(st, ref, model)
    bound = MULTIPLIER[c.family] * max(merr, floor)
    print(f"{c.name}: M2 error {err / top:.2e} of the largest diagonal entry, model {merr / top:.2e}, floor {floor / top:.2e}, ratio {ratio:.2f} "
          f"(multiplier {MULTIPLIER[c.family]}); mean error {mean_err:.2f} eps; kernel batches {info['kernel_batches']} of {info['batches']}")
    assert st["n"] == c.n == ref[0]
    assert info["kernel_batches"] == (info["batches"] if expect_kernel else 0), info
    assert np.array_equal(st["m2"], st["m2"].T)                     # symmetric to the bit: both triangles are written from one value
    assert err <= bound, (c.name, err / top, bound / top)
    # the mean, in units of eps64 (|mean| + sigma): every update rounds c + s / n' once (half a unit per batch), and the sums behind it --
    # of (x - c) on the kernel path, of x itself on the two-pass path -- are sequential float64 sums of up to m terms, whose rounding
    # walks to about sqrt(m) / 2 units (m / 2 at the very worst); two units of head-room
    assert mean_err <= 0.5 * len(batches) + 0.5 * np.sqrt(max(b.shape[0] for b in batches)) + 2.0, mean_err
    if c.family != "drift":
        assert bound <= CAP * top, (c.name, bound / top)
    return ratio, err / top, merr / top


# ------------------------------------------------------------------------------------------- 3. model parity
ParityCase = namedtuple("ParityCase", "n d k dt seed")
PARITY_CASES = [ParityCase(300, 16, 4, "f64", 31), ParityCase(2000, 100, 8, "f32", 32), ParityCase(50, 130, 5, "f64", 33)]   # the last: rows < d
PARITY_CASES_GPU = PARITY_CASES + [ParityCase(300, 1040, 4, "f64", 34)]     # wider than the kernel takes: must report the fallback
PARTS = (1, 3, 7)


def parity_id(c):
    return f"{c.n}x{c.d}-k{c.k}-{c.dt}"


def bar(c):
    """the project's parity bar: component rows and singular values, relative"""
    return 1e-5 if c.dt == "f32" else 1e-9


@functools.lru_cache(maxsize=None)
def parity_inputs(c):
    x = po.synth_pca(c.n, c.d, c.k, seed=c.seed, dtype=np_dtype(c))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def parity_reference(c, centering):
    """numpy's float64 SVD of the (centred) concatenation: (components k x d, singular values k, means, total variance)"""
    x = parity_inputs(c).astype(np.float64)
    mu = x.mean(axis=0) if centering else np.zeros(c.d)
    _, s, vt = np.linalg.svd(x - mu, full_matrices=False)
    return vt[:c.k], s[:c.k], mu, float(np.sum(s * s))


def model_errors(got, ref, k):
    """(components, singular values, means, total variance) of a fitted model against a reference 4-tuple: relative errors; components
    row by row after aligning signs"""
    comp, sing, mu, tv = ref
    return (float(rowwise_rel(np.asarray(got[0], dtype=np.float64), comp).max()) if k else 0.0,
            float(np.abs(np.asarray(got[1], dtype=np.float64) / sing - 1).max()) if k else 0.0,
            float(np.abs(np.asarray(got[2], dtype=np.float64) - mu).max() / max(1.0, np.abs(mu).max())),
            abs(float(got[3]) / tv - 1))


def fitted(m):
    return m.components(), m.singular_values(), m.mean(), m._total_variance


def check_sign_rule(comp, ref_comp, margin=1e-3):
    """every component whose top two magnitudes differ by a margin (in the reference, so that a library within the bar must pick the
    same entry) has that entry positive; returns how many components were decided"""
    a = np.abs(np.asarray(ref_comp, dtype=np.float64))
    decided = 0
    for j in range(a.shape[0]):
        top2 = np.sort(a[j])[-2:] if a.shape[1] > 1 else np.array([0.0, a[j, 0]])
        if top2[0] < (1.0 - margin) * top2[1]:
            decided += 1
            assert comp[j, int(np.argmax(a[j]))] > 0, (j, comp[j, int(np.argmax(a[j]))])
    return decided


def check_parity(ctx, c, centering, expect_kernel, device=False):
    """1, 3 and 7 unequal batches against numpy's SVD, against the library's own Pca.fit, and against each other, all within the bar;
    the sign rule wherever it is decided"""
    x = parity_inputs(c)
    ref = parity_reference(c, centering)
    whole = petal.Pca(c.k, centering, ctx=ctx).fit(np.array(x))
    tol, fits = bar(c), []
    for parts in PARTS:
        batches = [x[a:b] for a, b in cut(c.n, unequal(c.n, parts, c.seed))]
        m = feed(ctx, batches, c.k, centering, device)
        info = m.info()
        assert info["n_samples_seen"] == c.n and info["batches"] == parts
        assert info["kernel_batches"] == (parts if expect_kernel else 0), info
        got = fitted(m)
        assert got[0].dtype == np_dtype(c) and got[0].shape == (c.k, c.d)
        e_ref, e_lib = model_errors(got, ref, c.k), model_errors(got, fitted(whole), c.k)
        print(f"{parity_id(c)} {'centred' if centering else 'uncentred'} in {parts}: against numpy {max(e_ref):.2e}, against Pca.fit "
              f"{max(e_lib):.2e}  (bar {tol:.0e})")
        assert max(e_ref) <= tol and max(e_lib) <= tol, (parts, e_ref, e_lib)
        assert check_sign_rule(got[0], ref[0]) >= 1
        fits.append(got)
        m.close()
    for a in fits:
        for b in fits:
            assert max(model_errors(a, (b[0].astype(np.float64), b[1].astype(np.float64), b[2].astype(np.float64), float(b[3])), c.k)) <= tol


# ------------------------------------------------------------------------------------------- 5. merge and state
def check_merge_and_state(ctx, c, expect_kernel):
    x = parity_inputs(c)
    ref = parity_reference(c, True)
    split = c.n // 3
    one = feed(ctx, [x[:split], x[split:2 * split], x[2 * split:]], c.k)
    left, right = feed(ctx, [x[:split]], c.k), feed(ctx, [x[split:2 * split], x[2 * split:]], c.k)
    right_before = right.state()
    left.merge(right)
    assert left.n_samples_seen == c.n and left.info()["merges"] == 1
    for key in ("mean", "m2"):
        assert right.state()[key].tobytes() == right_before[key].tobytes()          # `other` is unchanged
    assert max(model_errors(fitted(left), ref, c.k)) <= bar(c)
    assert max(model_errors(fitted(left), tuple(np.asarray(v, dtype=np.float64) for v in fitted(one)), c.k)) <= bar(c)
    # an empty handle changes no byte; neither does an unopened model
    before = left.state()
    empty = petal.IncrementalPca(c.k, ctx=ctx).partial_fit(x[:0])
    left.merge(empty).merge(petal.IncrementalPca(c.k, ctx=ctx))
    after = left.state()
    assert after["n"] == before["n"] and all(after[key].tobytes() == before[key].tobytes() for key in ("mean", "m2"))
    # merging INTO an empty handle takes the other statistic as it is
    empty.merge(one)
    assert all(empty.state()[key].tobytes() == one.state()[key].tobytes() for key in ("mean", "m2")) and empty.n_samples_seen == c.n
    # get_state -> set_state into a fresh handle -> identical finalize bytes
    st = one.state()
    copy = petal.IncrementalPca.from_state(st, c.k, ctx=ctx)
    for a, b in zip(one.finalize(), copy.finalize()):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    # finalize twice and with another k leaves the state as it is, and gives the same bytes again
    first = one.finalize()
    other_k = one.finalize(max(c.k - 2, 1))
    again = one.finalize()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
    assert other_k[0].shape == (max(c.k - 2, 1), c.d)
    assert max(model_errors((other_k[0], other_k[2], other_k[1], other_k[3][0]), tuple(v[:max(c.k - 2, 1)] if i < 2 else v for i, v in enumerate(ref)),
                            max(c.k - 2, 1))) <= bar(c)
    assert all(one.state()[key].tobytes() == st[key].tobytes() for key in ("mean", "m2")) and one.state()["n"] == st["n"]
    assert one.info()["kernel_batches"] == (3 if expect_kernel else 0)
    for m in (one, left, right, empty, copy):
        m.close()


# ------------------------------------------------------------------------------------------- the drift case
def drift_loss(state, ref, c):
    """the error of M2 in units of eps64 n sigma_i sigma_j, sigma the WITHIN-batch spread of the columns (the scale of the part of the
    statistic that is not the drift itself), and in units of eps64 times the largest diagonal entry (the scale of the drift)"""
    scale = np.linspace(1.0, 4.0, c.d)
    err = np.abs(state["m2"].astype(np.longdouble) - ref[2]).astype(np.float64)
    return float(np.max(err / (EPS64 * c.n * np.outer(scale, scale)))), float(np.max(err) / (EPS64 * float(np.max(np.diag(ref[2])))))


def merged_in_chunks(ctx, batches, k, device=False):
    """every batch into a handle of its own, merged pairwise in order: the cancellation-free way to fit a drifting stream"""
    total = petal.IncrementalPca(k, ctx=ctx)
    for b in batches:
        part = feed(ctx, [b], k, True, device)
        total.merge(part)
        part.close()
    return total


# ------------------------------------------------------------------------------------------- profiles/ipca_errors.txt
def main(argv):
    """device rows (when a GPU is there) and host-simulation rows into profiles/ipca_errors.txt (--stdout: print only)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hostsim
    layers = []
    if "hostsim" not in argv:
        layers.append((petal.Context(0), STAT_CASES_GPU + [DRIFT_CASE], "MI355X, streaming kernel", True))
    layers.append((hostsim.context(), STAT_CASES + [DRIFT_CASE], "host simulation, two-pass path", False))
    lines = [f"# IncrementalPca: error of M2 against the long-double reference over max(model error, {FLOOR_EPS:g} eps64 max diag), per case",
             "# (errors in units of the largest diagonal entry of M2; the multipliers of tests/ipca_cases.py are twice the largest ratio per family)"]
    worst = {}
    for ctx, cases, label, kernel in layers:
        lines.append(f"# -- {label}")
        lines.append("# case                  error       model       ratio")
        for c in cases:
            ratio, err, merr = check_statistic(ctx, c, expect_kernel=kernel)
            worst[c.family] = max(worst.get(c.family, 0.0), ratio)
            lines.append(f"{c.name:22s}  {err:.3e}   {merr:.3e}   {ratio:.3f}")
    lines.append("# largest ratio per family: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    lines.append("# multipliers in force:      " + ", ".join(f"{k} {v:g}" for k, v in sorted(MULTIPLIER.items())))
    if "--stdout" not in argv:
        with open(os.path.join(ROOT, "profiles", "ipca_errors.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main(sys.argv)
