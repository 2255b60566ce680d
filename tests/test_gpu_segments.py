"""Segmented Pca (petal_pca_fit_segments and its transform entries, include/petal_hip_segments.h) on a real MI355X: every case of
tests/segments_cases.py against its bound on the segment kernel (d <= 64) and on the loop (d = 65), with and without poisoned workspace;
segment independence, run-to-run and host / device determinism to the byte; the kernel against the looped petal_pca_fit; y_out against
petal_transform_segments and the round trip at k = d; a planted NaN segment.  Run with -m gpu."""
import numpy as np
import pytest

import header_kit as kit
import segments_cases as sg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["plain", "poison"])
def ctx(request):
    import petal_decomposition_amd as petal
    c = petal.Context(0)          # raises (no CPU fallback) when the HIP library or the GPU is missing
    if request.param == "poison":
        c.set_option("poison", 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def plain():
    import petal_decomposition_amd as petal
    c = petal.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("case", sg.all_cases(), ids=repr)
def test_table_within_bound(ctx, case):
    m, _ = sg.check(case, ctx)
    assert m.kernel_segments == (case.nseg if case.on_kernel else 0)


def _case(d, k, dt, nseg):
    hits = [c for c in sg.all_cases() if (c.d, c.k, c.dt, c.nseg) == (d, k, dt, nseg)]
    assert hits
    return hits[0]


def _fit(ctx, x, off, k, centering=True, want_y=True):
    import petal_decomposition_amd as petal
    m = petal.SegmentedPca(k, centering=centering, ctx=ctx)
    if not want_y:
        return m.fit(x, off), None
    return m, sg.to_numpy(m.fit_transform(x, off))


def _same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


@pytest.mark.parametrize("row", [(16, 4, "f64", 300), (64, 4, "f32", 300)], ids=repr)
def test_segments_are_independent_bit_for_bit(plain, row):
    """segment b of a 300-segment call equals the same rows fitted as a one-segment call, and itself with the batch reversed"""
    case = _case(*row)
    x, off, B = sg.inputs(*case.key), sg.offsets_of(case.lengths), case.nseg
    m, y = _fit(plain, x, off, case.k)
    assert m.kernel_segments == B
    order = np.arange(B)[::-1]
    xr = np.concatenate([x[off[b]:off[b + 1]] for b in order])
    offr = sg.offsets_of([case.lengths[b] for b in order])
    mr, yr = _fit(plain, xr, offr, case.k)
    for i, b in enumerate(order):
        assert _same(mr.components[i], m.components[b]) and _same(mr.mean[i], m.mean[b]), b
        assert _same(mr.singular_values[i], m.singular_values[b]) and _same(mr.total_variance[i], m.total_variance[b]), b
        assert _same(yr[offr[i]:offr[i + 1]], y[off[b]:off[b + 1]]), b
    for b in (0, 1, 7, 150, B - 1):
        one, y1 = _fit(plain, np.ascontiguousarray(x[off[b]:off[b + 1]]), [0, case.lengths[b]], case.k)
        assert one.kernel_segments == 1
        assert _same(one.components[0], m.components[b]) and _same(one.mean[0], m.mean[b]), b
        assert _same(one.singular_values[0], m.singular_values[b]) and _same(y1, y[off[b]:off[b + 1]]), b


@pytest.mark.parametrize("row", [(16, 4, "f64", 300), (17, 17, "f64", 2), (48, 4, "f32", 2), (64, 4, "f32", 300)], ids=repr)
def test_two_identical_calls_give_identical_bytes(ctx, row):
    case = _case(*row)
    x, off = sg.inputs(*case.key), sg.offsets_of(case.lengths)
    a, ya = _fit(ctx, x, off, case.k, case.centering)
    b, yb = _fit(ctx, x, off, case.k, case.centering)
    assert _same(a.components, b.components) and _same(a.mean, b.mean) and _same(a.singular_values, b.singular_values)
    assert _same(a.total_variance, b.total_variance) and _same(ya, yb)


@pytest.mark.parametrize("row", [(16, 4, "f32", 300), (33, 4, "f64", 2), (65, 4, "f64", 2)], ids=repr)
def test_host_and_device_outputs_are_identical(plain, row):
    import torch
    case = _case(*row)
    x, off = sg.inputs(*case.key), sg.offsets_of(case.lengths)
    h, yh = _fit(plain, x, off, case.k, case.centering)
    for xd in (torch.from_numpy(np.array(x)).cuda(), sg.laid_out(case, x) if case.layout == "dev" else torch.from_numpy(np.array(x)).cuda()):
        import petal_decomposition_amd as petal
        m = petal.SegmentedPca(case.k, centering=case.centering, ctx=plain)
        yd = m.fit_transform(xd, off)
        assert yd.is_cuda
        assert _same(h.components, m.components) and _same(h.singular_values, m.singular_values) and _same(yh, yd.cpu().numpy())


@pytest.mark.parametrize("row", [(16, 16, "f64", 2), (64, 4, "f64", 2), (48, 4, "f32", 2)], ids=repr)
def test_kernel_and_looped_pca_both_meet_the_reference(plain, row):
    """different solvers, so no bitwise claim: each is within the bounds of the reference"""
    import petal_decomposition_amd as petal
    case = _case(*row)
    T = sg._DT[case.dt]
    x, off = sg.inputs(*case.key), sg.offsets_of(case.lengths)
    m, y = _fit(plain, x, off, case.k, case.centering)
    assert m.kernel_segments == case.nseg
    ref, bnd = sg.reference(case.key), sg.bounds(case.key)
    for b, got in enumerate(sg.segments_of(m, y, case.lengths)):
        one = petal.Pca(case.k, centering=case.centering, ctx=plain)
        s = sg.Seg()
        s.y = one.fit_transform(np.ascontiguousarray(x[off[b]:off[b + 1]]))
        s.comp, s.mean, s.sing, s.tv = one.components(), one.mean(), one.singular_values(), one._total_variance
        for name, seg in (("kernel", got), ("loop", s)):
            e = sg.seg_errors(seg, ref[b], T)
            print(f"{case.id} seg {b} {name}: " + "  ".join(f"{q} {e[q]:.2e} (bound {bnd[b][q]:.2e})" for q in sg.QUANTITIES))
            for q in sg.QUANTITIES:
                assert e[q] <= bnd[b][q], (name, b, q, e[q], bnd[b][q])


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("d", [16, 64])
def test_transform_entries_agree_with_the_fit(plain, d, dt):
    """y_out of the fit against petal_transform_segments of the fitted model, and inverse(transform(x)) = x at k = d.  Both sides form
    (x - mu) . v in fp64 and round once to the data's type; the transform entries read components and means ROUNDED to that type, a
    relative d eps each, and V is orthonormal to the Jacobi solver's d eps64: the differences are held to MULT d eps of the largest
    |y| and |x - mu|."""
    import petal_decomposition_amd as petal
    T = sg._DT[dt]
    lengths = (d, 65, 257, d + 1)
    rng = np.random.default_rng([d, 5])
    x = (rng.standard_normal((sum(lengths), d)) * np.linspace(2.0, 0.5, d) + rng.standard_normal(d)).astype(T)
    off = sg.offsets_of(lengths)
    tol = sg.mult_of(dt) * d * float(np.finfo(T).eps)
    for k in (4, d):
        m = petal.SegmentedPca(k, centering=False, ctx=plain)
        y = m.fit_transform(x, off)
        assert m.kernel_segments == len(lengths) and np.all(m.status == 0)
        y2 = m.transform(x, off)
        assert y2.shape == y.shape and y2.dtype == T
        assert float(np.abs(y2.astype(np.float64) - y).max()) <= tol * float(np.abs(y).max())
        if k == d:
            back = m.inverse_transform(y2, off)
            assert float(np.abs(back.astype(np.float64) - x).max()) <= tol * float(np.abs(x).max())
    # centred, on device tensors
    import torch
    m = petal.SegmentedPca(d, ctx=plain)
    xd = torch.from_numpy(x).cuda()
    off2 = sg.offsets_of([d + 1, 65, 257, d])
    yd = m.fit_transform(xd, off2)
    y2 = m.transform(xd, off2)
    back = m.inverse_transform(y2, off2)
    assert back.is_cuda and float((back - xd).abs().max()) <= tol * float(np.abs(x).max())
    assert float((y2 - yd).abs().max()) <= tol * float(yd.abs().max())


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_a_nan_segment_is_a_status_and_touches_nothing_else(ctx, dt):
    import petal_decomposition_amd as petal
    T = sg._DT[dt]
    d, k, B = 16, 4, 20
    lengths = sg.mix(k, B, True, 3)
    rng = np.random.default_rng(17)
    x = (rng.standard_normal((sum(lengths), d)) * np.linspace(3.0, 0.3, d) + 1.0).astype(T)
    off = sg.offsets_of(lengths)
    good, yg = _fit(ctx, x, off, k)
    xb = x.copy()
    xb[off[7] + lengths[7] // 2, 5] = np.nan
    bad, yb = _fit(ctx, xb, off, k)
    assert bad.kernel_segments == B and list(bad.status) == [1 if b == 7 else 0 for b in range(B)]
    assert np.all(np.isnan(bad.components[7])) and np.all(np.isnan(bad.singular_values[7])) and np.isnan(bad.total_variance[7])
    assert np.all(np.isnan(yb[off[7]:off[8]]))
    keep = np.ones(B, dtype=bool)
    keep[7] = False
    assert _same(bad.components[keep], good.components[keep]) and _same(bad.mean[keep], good.mean[keep])
    assert _same(bad.singular_values[keep], good.singular_values[keep]) and _same(bad.total_variance[keep], good.total_variance[keep])
    rows = np.ones(x.shape[0], dtype=bool)
    rows[off[7]:off[8]] = False
    assert _same(yb[rows], yg[rows])
    # without `status` the call is the crate's error, naming the segment
    import ctypes as C
    keepalive = []
    mx = petal.describe(xb, keepalive)
    o = np.ascontiguousarray(off, dtype=np.int64)
    comp, mu, s, tv = np.zeros((B, k, d), T), np.zeros((B, d), T), np.zeros((B, k), T), np.zeros(B, T)
    rc = ctx.lib.petal_pca_fit_segments(ctx._h, C.byref(mx), o.ctypes.data_as(petal._L), B, k, 1, comp.ctypes.data, mu.ctypes.data,
                                        s.ctypes.data, tv.ctypes.data, None, None, None)
    assert rc == petal.PETAL_LINALG_ERROR
    msg = (ctx.lib.petal_last_error(ctx._h) or b"").decode()
    assert "segment 7" in msg and "did not converge" in msg


def test_cpp_facade_on_gpu():
    """the C++ SegmentedPca over the HIP library: the batch against Pca per segment, the round trip, a NaN segment, the messages"""
    kit.run_cpp_facade("segments", "kernel", kit.HIP_LIBRARY, "hip")
