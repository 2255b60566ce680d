"""Segmented Pca (include/petal_hip_segments.h) without a GPU: tests/segments_cases.py's references and models against their own bounds;
the entry on the host simulation -- whose device-op layer has no segment op, so the call loops over Pca's own code on row-slice views --
against the reference, against per-segment petal_pca_fit calls bit for bit, and its argument, status and empty-shape contracts; the new
header against the built libraries, the Python table and the Rust binding; the C++ facade; the resource notes of the new kernels."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import header_kit as kit
import hostsim
import segments_cases as sg
from header_kit import resources  # noqa: F401  (the fixture)
import petal_decomposition_amd as petal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "petal_hip_segments.h")
FFI = os.path.join(ROOT, "rust", "petal-decomposition-hip", "src", "ffi_segments.rs")
ENTRIES = ["petal_inverse_transform_segments", "petal_pca_fit_segments", "petal_transform_segments"]


@pytest.fixture(scope="module")
def ctx():
    c = hostsim.context()
    yield c
    c.close()


# ------------------------------------------------------------------------------------------- references, models, bounds
@pytest.mark.parametrize("case", sg.all_cases(reduced=True), ids=repr)
def test_reference_and_model_stay_inside_the_bound(case):
    """The model is inside the bound the library is held to, with the multipliers in force, and the bound says something: at the
    starting multipliers it is far below the size of the quantities (1 for all of them, as they are scaled)."""
    em, bnd, start = sg.model_errors(case.key), sg.bounds(case.key), sg.bounds(case.key, mult32=4.0, mult64=16.0)
    worst = {q: max(e[q] for e in em) for q in sg.QUANTITIES}
    print(f"{case.id}: model errors " + "  ".join(f"{q} {worst[q]:.2e}" for q in sg.QUANTITIES))
    for e, b, s in zip(em, bnd, start):
        for q in sg.QUANTITIES:
            assert e[q] <= b[q] <= s[q] <= 1e-4, (case.id, q, e[q], b[q], s[q])
    lead = 1e-5 if case.dt == "f32" else 1e-9       # the model's own distance from the reference (k = d: eps (sigma_1 / sigma_d)^2 over the gap)
    assert all(worst[q] <= lead for q in sg.QUANTITIES), worst


def test_multipliers_never_exceed_the_starting_values():
    assert 1.0 <= sg.MULT32 <= 4.0 and 1.0 <= sg.MULT64 <= 16.0


def test_most_pairs_are_asserted_with_sign():
    signed, total = sg.signed_share(sg.all_cases())
    print(f"{signed} of {total} (segment, component) pairs asserted with sign")
    assert total > 2000 and signed >= 0.9 * total


def test_the_table_reaches_every_path():
    cases = sg.all_cases()
    assert {c.d for c in cases} == {1, 3, 16, 17, 33, 48, 64, 65}
    assert {1, 4} <= {c.k for c in cases} and any(c.k == c.d > 4 for c in cases)
    assert {c.nseg for c in cases} == {1, 2, 300}
    assert {c.dt for c in cases} == {"f32", "f64"} and {c.centering for c in cases} == {True, False}
    assert {c.layout for c in cases} == {"host", "hostF", "dev"} and {c.want_y for c in cases} == {True, False}
    lengths = {n for c in cases for n in c.lengths}
    assert {1, 63, 64, 65, 257, 1000} <= lengths
    assert any(n == c.k for c in cases for n in c.lengths) and any(n == c.k + 1 for c in cases for n in c.lengths)
    assert any(c.off for c in cases) and any(not c.on_kernel for c in cases)


# ------------------------------------------------------------------------------------------- the entry on the host simulation
@pytest.mark.parametrize("case", sg.all_cases(reduced=True), ids=repr)
def test_entry_on_the_host_simulation(ctx, case):
    m, _ = sg.check(case, ctx)
    assert m.kernel_segments == 0


def _data(lengths, d, dt=np.float64, seed=3):
    rng = np.random.default_rng(seed)
    n = int(sum(lengths))
    x = (rng.standard_normal((n, d)) * np.linspace(3.0, 0.5, d) + rng.standard_normal(d)).astype(dt)
    return x, sg.offsets_of(lengths)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_batch_equals_per_segment_fits_bit_for_bit(ctx, dt):
    lengths, d, k = (40, 5, 131, 64), 7, 3
    x, off = _data(lengths, d, dt)
    m = petal.SegmentedPca(k, ctx=ctx)
    y = m.fit_transform(x, off)
    assert m.kernel_segments == 0 and np.all(m.status == 0)
    for b in range(len(lengths)):
        one = petal.Pca(k, ctx=ctx)
        yb = one.fit_transform(np.ascontiguousarray(x[off[b]:off[b + 1]]))
        np.testing.assert_array_equal(m.components[b], one.components())
        np.testing.assert_array_equal(m.mean[b], one.mean())
        np.testing.assert_array_equal(m.singular_values[b], one.singular_values())
        np.testing.assert_array_equal(m.explained_variance_ratio[b], one.explained_variance_ratio())
        np.testing.assert_array_equal(y[off[b]:off[b + 1]], yb)
    # lengths= and a 3-D input say the same as offsets
    m2 = petal.SegmentedPca(k, ctx=ctx).fit(x, lengths=lengths)
    np.testing.assert_array_equal(m2.components, m.components)
    x3 = x[:120].reshape(3, 40, d)
    m3 = petal.SegmentedPca(k, ctx=ctx)
    y3 = m3.fit_transform(x3)
    m4 = petal.SegmentedPca(k, ctx=ctx).fit(x[:120], [0, 40, 80, 120])
    assert y3.shape == (3, 40, k)
    np.testing.assert_array_equal(m3.components, m4.components)


def _raw_fit(ctx, x, off, k, status=True, nseg=None):
    keep = []
    mx = petal.describe(x, keep)
    off = np.ascontiguousarray(np.asarray(off, dtype=np.int64))
    nseg = off.size - 1 if nseg is None else nseg
    d = x.shape[1]
    comp, mu, s, tv = np.zeros((max(nseg, 1), k, d)), np.zeros((max(nseg, 1), d)), np.zeros((max(nseg, 1), k)), np.zeros(max(nseg, 1))
    st = np.zeros(max(nseg, 1), dtype=np.int32)
    ks = C.c_int64(-1)
    rc = ctx.lib.petal_pca_fit_segments(ctx._h, C.byref(mx), off.ctypes.data_as(petal._L), nseg, k, 1, comp.ctypes.data, mu.ctypes.data,
                                        s.ctypes.data, tv.ctypes.data, st.ctypes.data_as(C.POINTER(C.c_int32)) if status else None, None,
                                        C.byref(ks))
    return rc, (ctx.lib.petal_last_error(ctx._h) or b"").decode(), (comp, mu, s, tv, st, ks.value)


def test_offsets_are_validated(ctx):
    x, _ = _data((10, 10), 4)
    rc, msg, _ = _raw_fit(ctx, x, [1, 10, 20], 2)
    assert rc == petal.PETAL_INVALID_INPUT and "offsets[0] should be 0" in msg
    rc, msg, _ = _raw_fit(ctx, x, [0, 12, 8, 20], 2)
    assert rc == petal.PETAL_INVALID_INPUT and "offsets[2] = 8 is below offsets[1] = 12" in msg
    rc, msg, _ = _raw_fit(ctx, x, [0, 10, 19], 2)
    assert rc == petal.PETAL_INVALID_INPUT and "offsets[2] should be the number of rows 20 (it is 19)" in msg
    with pytest.raises(petal.InvalidInput, match=r"offsets\[0\] should be 0"):
        petal.SegmentedPca(2, ctx=ctx).fit(x, [2, 20])
    with pytest.raises(petal.InvalidInput, match="needs offsets or lengths"):
        petal.SegmentedPca(2, ctx=ctx).fit(x)


def test_a_short_segment_is_named(ctx):
    x, _ = _data((10, 10), 4)
    rc, msg, _ = _raw_fit(ctx, x, [0, 9, 11, 20], 3)
    assert rc == petal.PETAL_INVALID_INPUT and msg == "segment 1: every dimension should be at least 3"
    rc, msg, _ = _raw_fit(ctx, x, [0, 10, 20], 5)                # d < k
    assert rc == petal.PETAL_INVALID_INPUT and msg == "segment 0: every dimension should be at least 5"


def test_a_non_finite_segment_is_a_status(ctx):
    lengths, d, k = (20, 9, 33, 12), 5, 2
    x, off = _data(lengths, d)
    good = petal.SegmentedPca(k, ctx=ctx)
    yg = good.fit_transform(x, off)
    for poison in (np.nan, np.inf):
        xb = x.copy()
        xb[off[2] + 4, 1] = poison
        m = petal.SegmentedPca(k, ctx=ctx)
        y = m.fit_transform(xb, off)
        assert list(m.status) == [0, 0, 1, 0] and m.kernel_segments == 0
        assert np.all(np.isnan(m.components[2])) and np.all(np.isnan(m.singular_values[2])) and np.isnan(m.total_variance[2])
        assert np.all(np.isnan(y[off[2]:off[3]]))
        for b in (0, 1, 3):
            np.testing.assert_array_equal(m.components[b], good.components[b])
            np.testing.assert_array_equal(m.singular_values[b], good.singular_values[b])
            np.testing.assert_array_equal(y[off[b]:off[b + 1]], yg[off[b]:off[b + 1]])
        rc, msg, _ = _raw_fit(ctx, xb, off, k, status=False)
        assert rc == petal.PETAL_LINALG_ERROR and "segment 2" in msg and "did not converge" in msg
    rc, _, out = _raw_fit(ctx, x, off, k, status=False)
    assert rc == petal.PETAL_OK and out[5] == 0


def test_empty_shapes_are_legal(ctx):
    x, _ = _data((10,), 4)
    rc, msg, out = _raw_fit(ctx, x[:0], [0], 2)                       # no segments
    assert rc == petal.PETAL_OK, msg
    assert out[5] == 0
    rc, msg, out = _raw_fit(ctx, x, [0, 0, 10, 10], 0)                # k == 0, empty segments among them
    assert rc == petal.PETAL_OK, msg
    comp, mu, s, tv, st, _ = out
    np.testing.assert_array_equal(mu[0], 0)
    np.testing.assert_array_equal(mu[2], 0)
    np.testing.assert_allclose(mu[1], x.mean(axis=0), rtol=1e-14)
    assert tv[0] == 0 and tv[2] == 0 and list(st) == [0, 0, 0]
    np.testing.assert_allclose(tv[1], ((x - x.mean(axis=0)) ** 2).sum(), rtol=1e-13)
    rc, msg, _ = _raw_fit(ctx, x, [0, 0, 10], 1)                      # an empty segment with k > 0 is too short
    assert rc == petal.PETAL_INVALID_INPUT and msg.startswith("segment 0:")
    m = petal.SegmentedPca(0, ctx=ctx)
    y = m.fit_transform(x, [0, 4, 10])
    assert y.shape == (10, 0) and m.components.shape == (2, 0, 4)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_round_trip_at_full_rank(ctx, dt):
    lengths, d = (9, 30, 6), 6
    x, off = _data(lengths, d, dt)
    m = petal.SegmentedPca(d, ctx=ctx).fit(x, off)
    y = m.transform(x, off)
    back = m.inverse_transform(y, off)
    tol = 40 * np.finfo(dt).eps * float(np.abs(x).max())
    assert y.shape == (45, d) and float(np.abs(back - x).max()) <= tol
    y2 = petal.SegmentedPca(d, ctx=ctx).fit_transform(x, off)
    assert float(np.abs(y2 - y).max()) <= tol * np.sqrt(d)
    with pytest.raises(petal.InvalidInput, match="# of columns should be 6"):
        m.transform(x[:, :5], off)
    with pytest.raises(petal.InvalidInput, match="segments"):
        m.transform(x, [0, 45])


# ------------------------------------------------------------------------------------------- the header, Python, Rust, C++
def test_header_is_exported_and_bound_by_python():
    fns = kit.header_functions(HEADER)
    kit.check_python_table("petal_hip_segments.h", fns, ENTRIES)
    kit.check_exported(fns, want_hip=True)
    assert fns["petal_pca_fit_segments"] == ("i32", ["ptr", "ptr", "ptr", "i64", "i64", "i32"] + ["ptr"] * 7)
    assert '#include "petal_hip.h"' in open(HEADER).read()


def test_rust_binding_matches_the_header():
    assert kit.rust_functions(FFI) == kit.header_functions(HEADER)
    src = os.path.join(ROOT, "rust", "petal-decomposition-hip", "src")
    lib = open(os.path.join(src, "lib.rs")).read()
    assert "mod ffi_segments;" in lib and "SegmentedPca" in lib
    pca = open(os.path.join(src, "pca.rs")).read()
    for name in ENTRIES:
        assert f"ffi_segments::{name}" in pca
    assert "pub struct SegmentedPca" in pca
    for name in ("fit", "fit_transform", "transform", "inverse_transform", "status", "kernel_segments"):
        assert re.search(rf"impl<A: HipScalar> SegmentedPca<A> \{{.*pub fn {name}\b", pca, flags=re.S), name


def test_cpp_facade_on_host_simulation():
    kit.run_cpp_facade("segments", "loop", hostsim.build(), "hostsim")


# ------------------------------------------------------------------------------------------- kernel budgets
LDS_PER_CU = 160 * 1024
FIT_KERNELS = [(t, mb) for t in ("float", "double") for mb in (1, 2, 3, 4)]


@pytest.mark.parametrize("t,mb", FIT_KERNELS, ids=[f"{t}-{mb}" for t, mb in FIT_KERNELS])
def test_segment_kernel_budget(resources, t, mb):
    """no spill, no scratch; the LDS of an instantiation (static: the notes hold it) lets 8 workgroups share a CU at d <= 16 and 2 at
    d = 64, and the registers allow as many 256-thread workgroups (four waves: one per SIMD each) as the LDS does"""
    r = resources[f"void petal::k_pca_segments<{t}, {mb}>"]
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
    per_cu = {1: 8, 2: 4, 3: 3, 4: 2}[mb]
    assert r["lds"] * per_cu <= LDS_PER_CU, (r["lds"], per_cu)
    assert r["waves_per_simd"] >= min(per_cu, 2), r
    assert r["max_wg"] == 256


@pytest.mark.parametrize("t", ["float", "double"])
@pytest.mark.parametrize("fwd", ["true", "false"])
def test_projection_kernel_budget(resources, t, fwd):
    r = resources[f"void petal::k_seg_project<{t}, {fwd}>"]
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
    assert r["lds"] * 2 <= LDS_PER_CU and r["waves_per_simd"] >= 2
