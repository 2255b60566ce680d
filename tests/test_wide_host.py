"""Exact Pca on wide data (include/petal_hip_wide.h) without a GPU, on the host simulation -- whose device-op layer has no row-Gram
kernel, so K and the components come from the fallback built on op_cvt_to_f64 and op_dgemm and `last_route` reports kernel = 0: the
statements of the row Gram matrix (exact integers, the long-double bound and its cap), the whole host sequencing of the dual route
against the oracle and against its numpy model, the auto rule, k = n, non-finite input, the options; the new header against the built
libraries, the Python table, the Rust binding and the C++ facade."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import header_kit as kit
import hostsim
import wide_cases as wc
from header_kit import resources  # noqa: F401  (the fixture)
import petal_decomposition_amd as petal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "petal_hip_wide.h")
FFI = os.path.join(ROOT, "rust", "petal-decomposition-hip", "src", "ffi_wide.rs")
ENTRIES = ["petal_pca_last_route", "petal_row_gram"]


@pytest.fixture(scope="module")
def ctx():
    c = hostsim.context()
    yield c
    c.close()


# ------------------------------------------------------------------------------------------- the row Gram matrix: the statement
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("form", ["host", "host-fortran"])
def test_integer_row_gram_is_exact(ctx, dt, form):
    """every n at the narrow widths, every width at three n (the fallback's products are slow on the host at 257 x 4099)"""
    for n in wc.INT_N:
        for d in wc.INT_D[:5]:
            wc.check_integers_exact(ctx, n, d, dt, form, expect_kernel=False)
    for n in (1, 17, 33):
        for d in wc.INT_D[5:] + (wc.INT_D_RAGGED[dt],):
            wc.check_integers_exact(ctx, n, d, dt, form, expect_kernel=False)


@pytest.mark.parametrize("case", wc.GRAM_CASES, ids=lambda c: c.name)
def test_row_gram_against_long_double(ctx, case):
    wc.check_gram_against_long_double(ctx, case, expect_kernel=False)


@pytest.mark.parametrize("case", wc.GRAM_CASES, ids=lambda c: c.name)
def test_fp32_accumulation_would_break_the_cap(case):
    """why every product and sum is float64: the numpy model alone stays within the cap on these inputs, the same statement with
    float32 products and sums misses it by decades -- the bound cannot hide a lost precision"""
    ref = wc.gram_reference(case)
    top = float(np.max(np.diag(ref)))
    e64 = float(np.max(np.abs(wc.gram_model(case).astype(np.longdouble) - ref))) / top
    e32 = float(np.max(np.abs(wc.gram_model(case, accumulate=np.float32).astype(np.longdouble) - ref))) / top
    print(f"{case.name}: float64 {e64:.2e}, float32 {e32:.2e} of the largest diagonal entry (cap {wc.CAP:.0e})")
    assert max(wc.MULTIPLIER.values()) * max(e64, wc.FLOOR_EPS * wc.EPS64) <= wc.CAP
    assert e32 > 100 * wc.CAP


def test_same_call_twice_gives_the_same_bytes(ctx):
    wc.check_same_bytes_twice(ctx, wc.GRAM_CASES[0])


def test_row_gram_arguments(ctx):
    x = np.arange(12.0).reshape(3, 4)
    with pytest.raises(petal.InvalidInput):
        petal.row_gram(x, np.zeros(3), ctx=ctx)                       # the centre has d values
    assert petal.row_gram(np.zeros((0, 4)), ctx=ctx).shape == (0, 0)
    assert not petal.row_gram(np.zeros((3, 0)), ctx=ctx).any()
    mx = petal.describe(x, [])
    assert ctx.lib.petal_row_gram(ctx._h, C.byref(mx), None, None, None) == petal.PETAL_INVALID_INPUT
    assert ctx.lib.petal_row_gram(ctx._h, None, None, None, None) == petal.PETAL_INVALID_INPUT
    assert ctx.lib.petal_pca_last_route(None, (C.c_int64 * 4)()) == petal.PETAL_INVALID_INPUT
    assert ctx.lib.petal_pca_last_route(ctx._h, None) == petal.PETAL_INVALID_INPUT
    other = hostsim.context()
    try:
        other.set_collective(lambda *a: 0, 0, 2)
        with pytest.raises(petal.InvalidInput, match="sharded"):
            petal.row_gram(x, ctx=other)
    finally:
        other.close()


# ------------------------------------------------------------------------------------------- fits
@pytest.mark.parametrize("case", wc.FIT_CASES, ids=lambda c: c.name)
def test_numpy_model_of_the_dual_route_matches_the_oracle(case):
    """tells a tolerance failure from a kernel failure: the route itself, in float64 numpy, is within the case's tolerance"""
    comp, sing, mu, tv, y = wc.model_dual_fit(wc.fit_inputs(case), case.k, case.centering, 1e-6 if case.dt == "f32" else 1e-10)
    wc.compare_with_oracle(case, comp, sing, mu, tv, y, wc.tol_of(case))


@pytest.mark.parametrize("case", wc.FIT_CASES, ids=lambda c: c.name)
def test_dual_fit_matches_the_oracle(ctx, case):
    wc.check_fit_parity(ctx, case, expect_kernel=False)


@pytest.mark.parametrize("case", [wc.FIT_CASES[0], wc.FIT_CASES[1]], ids=lambda c: c.name)
def test_dual_against_primal_on_one_ctx(ctx, case):
    wc.check_dual_against_primal(ctx, case)


@pytest.mark.parametrize("shape,route", wc.AUTO_RULE, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_auto_rule(ctx, shape, route):
    """the whole table: (64, 2064) dual; (64, 2048) -- d at the threshold --, (3000, 256) and (2100, 2064) -- n above d -- primal.  On the
    planted data of these cases the primal fits converge in the subspace iteration: seconds on the host simulation, (2100, 2064) the
    longest at about twelve."""
    wc.check_auto_rule(ctx, shape, route)


def test_sharded_ctx_keeps_the_primal_route():
    """a two-rank collective hook (this rank's rows alone reach the sums: the hook adds nothing) keeps the primal route at (64, 2064)
    under the auto rule, and at a small width where the dual route is asked for"""
    other = hostsim.context()
    try:
        other.set_collective(lambda *a: 0, 0, 2)
        assert other.get_option("pca_dual") == 0.0
        m = petal.Pca.new(2, other).fit(wc.sharded_rule_input())
        assert m.last_route() == {"route": 0, "kernel": 0, "order": 2064, "chunks": 0}
        x = np.random.default_rng(3).standard_normal((20, 48))
        other.set_option("pca_dual", 1)
        m = petal.Pca.new(2, other).fit(x)
        assert m.last_route() == {"route": 0, "kernel": 0, "order": 48, "chunks": 0}
    finally:
        other.close()


def test_k_equals_n_centred_ends_in_a_zero_row(ctx):
    wc.check_k_equals_n(ctx, expect_kernel=False)


def test_non_finite_input_does_not_converge(ctx):
    wc.check_non_finite_raises(ctx)


def test_transform_round_trip_of_a_dual_fitted_model(ctx):
    """(the host simulation has no row-score kernel: reconstruction_error is compared on the GPU)"""
    c = wc.ROUND_TRIP_CASE
    tol = wc.tol_of(c)
    m = wc.check_fit_parity(ctx, c, expect_kernel=False)
    o, _, _ = wc.fit_oracle(c)
    x = wc.fit_inputs(c)
    yo = o.transform(x.astype(np.float64))
    y = np.asarray(m.transform(x), dtype=np.float64)
    s = np.sign(np.sum(y * yo, axis=0))
    assert np.abs(y * s - yo).max() <= 100 * tol * np.abs(yo).max()
    xr, xo = m.inverse_transform(m.transform(x)), o.inverse_transform(yo)
    assert np.abs(xr - xo).max() <= 100 * tol * np.abs(xo).max()


# ------------------------------------------------------------------------------------------- options
def test_options_round_trip(ctx):
    assert petal.OPTIONS["pca_dual"] == 33 and petal.OPTIONS["pca_dual_fallback"] == 34
    assert ctx.get_option("pca_dual") == 0.0 and ctx.get_option("pca_dual_fallback") == 0.0
    for v, want in ((1, 1.0), (-1, -1.0), (7, 1.0), (-0.5, -1.0), (0, 0.0)):
        ctx.set_option("pca_dual", v)
        assert ctx.get_option("pca_dual") == want
    ctx.set_option("pca_dual_fallback", 1)
    assert ctx.get_option("pca_dual_fallback") == 1.0
    ctx.set_option("pca_dual_fallback", 0)
    assert ctx.get_option(34) == 0.0
    with pytest.raises(petal.InvalidInput):
        ctx.set_option("pca_dual", float("nan"))
    with pytest.raises(petal.InvalidInput):
        ctx.set_option(16, 1)                                                    # petal_hip.h's next free number stays unknown
    with pytest.raises(petal.InvalidInput):
        ctx.set_option(35, 1)
    out = C.c_double()
    assert ctx.lib.petal_ctx_get_option(ctx._h, 16, C.byref(out)) == petal.PETAL_INVALID_INPUT
    # a fit that returns before any route reports zeros
    petal.Pca.new(0, ctx).fit(np.zeros((0, 4)))
    assert petal.Pca.new(0, ctx).last_route() == {"route": 0, "kernel": 0, "order": 0, "chunks": 0}


# ------------------------------------------------------------------------------------------- the header, Python, Rust, C++
def test_header_is_exported_and_bound_by_python():
    fns = kit.header_functions(HEADER)
    kit.check_python_table("petal_hip_wide.h", fns, ENTRIES)
    kit.check_exported(fns)
    assert fns["petal_pca_last_route"] == ("i32", ["ptr", "ptr"])
    assert fns["petal_row_gram"] == ("i32", ["ptr", "ptr", "ptr", "ptr", "ptr"])
    text = open(HEADER).read()
    assert '#include "petal_hip.h"' in text
    assert int(re.search(r"#define\s+PETAL_OPT_PCA_DUAL\s+(\d+)", text).group(1)) == petal.OPTIONS["pca_dual"]
    assert int(re.search(r"#define\s+PETAL_OPT_PCA_DUAL_FALLBACK\s+(\d+)", text).group(1)) == petal.OPTIONS["pca_dual_fallback"]
    assert f"d > {wc.DUAL_MIN_D}" in text
    for word in ("ZERO ROW", "Not in this version", "sharded wide fits", "FastICA whitening on wide data", "SegmentedPca's kernel",
                 "small-sigma accurate route"):
        assert word in text, word                                                 # the disclosures the header owes


def test_rust_binding_and_cpp_facade_match_the_header():
    text = re.sub(r"//.*$", "", open(FFI).read(), flags=re.M)
    assert kit.rust_functions(FFI) == kit.header_functions(HEADER)
    assert int(re.search(r"PETAL_OPT_PCA_DUAL:\s*c_int\s*=\s*(\d+)", text).group(1)) == petal.OPTIONS["pca_dual"]
    assert int(re.search(r"PETAL_OPT_PCA_DUAL_FALLBACK:\s*c_int\s*=\s*(\d+)", text).group(1)) == petal.OPTIONS["pca_dual_fallback"]
    src = os.path.join(ROOT, "rust", "petal-decomposition-hip", "src")
    lib = open(os.path.join(src, "lib.rs")).read()
    assert "mod ffi_wide;" in lib and "PETAL_OPT_PCA_DUAL_FALLBACK" in lib and "PcaRoute" in lib
    pca = open(os.path.join(src, "pca.rs")).read()
    assert "ffi_wide::petal_pca_last_route" in pca and "pub struct PcaRoute" in pca
    assert re.search(r"impl<A: HipScalar> Pca<A> \{.*pub fn last_route\b", pca, flags=re.S)
    hpp = open(os.path.join(ROOT, "include", "petal_decomposition.hpp")).read()
    assert '#include "petal_hip_wide.h"' in hpp and "petal_pca_last_route" in hpp and "PcaRoute last_route() const" in hpp


def test_cpp_facade_on_host_simulation():
    kit.run_cpp_facade("wide", "fallback", hostsim.build(), "hostsim")


# ------------------------------------------------------------------------------------------- kernel budgets
def test_row_gram_kernel_budget(resources):
    """the figures DESIGN.md section 4 quotes, read from the built library's code-object notes: no scratch, no spills, no LDS, four waves
    per SIMD in all four instantiations (float / double, centred or not); the slab sum likewise at eight"""
    hits = {k: v for k, v in resources.items() if re.search(r"k_row_gram<(float|double), (true|false)>$", k)}
    assert len(hits) == 4, sorted(hits)
    for name, r in hits.items():
        print(name, r)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["lds"] == 0, (name, r)
        assert r["agpr"] == 32 and r["vgpr"] <= 128 and r["waves_per_simd"] >= 4 and r["max_wg"] == 256, (name, r)
    s = resources["petal::k_row_gram_sum"]
    assert s["scratch"] == 0 and s["vgpr_spill"] == 0 and s["sgpr_spill"] == 0 and s["lds"] == 0 and s["waves_per_simd"] == 8, s
