"""KernelPca (include/petal_hip_kpca.h) without a GPU, on the host simulation -- whose device-op layer has neither k_kmap nor k_kapply,
so the map, the fused pass and the epilogue come from the fallback built on op_cvt_to_f64, op_dgemm and a phi loop on the host, and
`info()` reports kernel = 0: the statement of petal_kernel_apply (exact integers, the exact rbf diagonal, the long-double bound and its
cap), the whole host sequencing of fit / fit_transform / transform against the numpy model, every error; the new header against the
built libraries, the Python table, the Rust binding and the C++ facade; the register / scratch budget of the kernels in the built
library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import header_kit as kit
import hostsim
import kpca_cases as kc
from header_kit import resources  # noqa: F401  (the fixture)
import petal_decomposition_amd as petal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "petal_hip_kpca.h")
FFI = os.path.join(ROOT, "rust", "petal-decomposition-hip", "src", "ffi_kpca.rs")
ENTRIES = ["petal_kernel_apply", "petal_kpca_destroy", "petal_kpca_fit", "petal_kpca_get", "petal_kpca_transform"]


@pytest.fixture(scope="module")
def ctx():
    c = hostsim.context()
    yield c
    c.close()


# ------------------------------------------------------------------------------------------- A, B: petal_kernel_apply
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("form", ["host", "host-fortran"])
def test_integer_kernel_apply_is_exact(ctx, dt, form):
    for shape in kc.INT_SHAPES:
        kc.check_integers_exact(ctx, shape, dt, form, expect_kernel=False)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_rbf_diagonal_is_exactly_one(ctx, dt):
    for (n, d) in ((1, 1), (17, 3), (33, 19), (129, 67), (257, 1000)):
        kc.check_rbf_diagonal_is_one(ctx, n, d, dt, "host", expect_kernel=False)


@pytest.mark.parametrize("case", kc.APPLY_CASES, ids=lambda c: c.name)
def test_kernel_apply_against_long_double(ctx, case):
    kc.check_apply_against_long_double(ctx, case, expect_kernel=False)


@pytest.mark.parametrize("case", [c for c in kc.APPLY_CASES if c.spec.kernel in ("linear", "poly", "rbf") and c.spec.gamma != 0.02],
                         ids=lambda c: c.name)
def test_fp32_accumulation_would_break_the_cap(case):
    """why every product and sum is float64: the numpy model alone stays within the cap on these inputs under the largest multiplier;
    the same cross product accumulated in float32 misses it by decades (linear, poly and rbf at 1 / d, whose kernel value moves with the
    cross term; tanh at 32 and a cosine of rows 40 sigma off zero are saturated on these inputs)"""
    ref, model, scale = kc.apply_reference(case)
    xq, xt, a, mean = kc.apply_inputs(case.m, case.n, case.d, case.dt)
    s = kc.resolved(case.spec, case.d)
    cen = mean if s.kernel == "rbf" else np.zeros(case.d)
    q, t = (xq.astype(np.float64) - cen), (xt.astype(np.float64) - cen)
    g32 = (q.astype(np.float32) @ t.astype(np.float32).T).astype(np.float64)
    k32 = kc.phi(s, g32, (q * q).sum(axis=1)[:, None], (t * t).sum(axis=1)[None, :])
    e32 = float(np.abs((k32 @ a).astype(np.longdouble) - ref).max()) / scale
    print(f"{case.name}: float64 {model / scale:.2e}, float32 cross product {e32:.2e} of the scale (cap {kc.CAP:.0e})")
    assert max(kc.MULTIPLIER.values()) * max(model / scale, kc.FLOOR_EPS * kc.EPS64) <= kc.CAP
    assert e32 > 100 * kc.CAP


def test_same_call_twice_gives_the_same_bytes(ctx):
    kc.check_same_bytes_twice(ctx, kc.APPLY_CASES[2])


def test_kernel_apply_arguments(ctx):
    x = np.arange(12.0).reshape(3, 4)
    with pytest.raises(petal.InvalidInput):
        petal.kernel_apply(x, x, np.ones((3, 2)), centre=np.zeros(3), ctx=ctx)       # the centre has d values
    with pytest.raises(petal.InvalidInput):
        petal.kernel_apply(x, x, np.ones((2, 2)), ctx=ctx)                           # a has n rows
    with pytest.raises(petal.InvalidInput, match="# of columns should be 4"):
        petal.kernel_apply(x[:, :3], x, np.ones((3, 2)), ctx=ctx)
    with pytest.raises(petal.InvalidInput, match="dtype"):
        petal.kernel_apply(x.astype(np.float32), x, np.ones((3, 2)), ctx=ctx)
    assert petal.kernel_apply(np.zeros((0, 4)), x, np.ones((3, 2)), ctx=ctx).shape == (0, 2)
    assert not petal.kernel_apply(x, np.zeros((0, 4)), np.ones((0, 2)), "rbf", ctx=ctx).any()
    mx = petal.describe(x, [])
    spec = petal.petal_kernel_spec(0, 3, 0.0, 1.0)
    assert ctx.lib.petal_kernel_apply(ctx._h, C.byref(mx), C.byref(mx), C.byref(spec), None, 2, None, None, None) == petal.PETAL_INVALID_INPUT
    assert ctx.lib.petal_kernel_apply(ctx._h, None, C.byref(mx), C.byref(spec), None, 2, None, None, None) == petal.PETAL_INVALID_INPUT
    assert ctx.lib.petal_kpca_get(None, None, None, None) == petal.PETAL_INVALID_INPUT
    assert ctx.lib.petal_kpca_transform(ctx._h, None, C.byref(mx), C.byref(mx)) == petal.PETAL_INVALID_INPUT
    ctx.lib.petal_kpca_destroy(None)


# ------------------------------------------------------------------------------------------- C: fits
@pytest.mark.parametrize("case", kc.FIT_CASES, ids=lambda c: c.name)
def test_fit_matches_the_model(ctx, case):
    kc.check_model_is_well_posed(case)
    kc.check_fit_against_model(ctx, case, expect_kernel=False)


@pytest.mark.parametrize("case", kc.FIT_CASES, ids=lambda c: c.name)
def test_transform_of_new_rows_matches_the_model(ctx, case):
    kc.check_transform_new_rows(ctx, case, expect_kernel=False)


@pytest.mark.parametrize("case", kc.FIT_CASES[12:14], ids=lambda c: c.name)
def test_fortran_order_input(ctx, case):
    kc.check_fit_against_model(ctx, case, expect_kernel=False, form="host-fortran")


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_linear_kernel_is_pca(ctx, dt):
    for (n, d) in kc.FIT_SHAPES:
        kc.check_linear_equals_pca(ctx, n, d, dt)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_k_equals_n_ends_in_a_zero_column(ctx, dt):
    kc.check_k_equals_n(ctx, dt)


def test_forced_fallback_is_the_path_of_this_layer(ctx):
    kc.check_fallback_against_kernel(ctx, kc.FIT_CASES[14], expect_kernel=False)


def test_fallback_walks_the_query_rows_in_blocks(ctx):
    """2100 query rows against 2049 training rows: the fallback's score block holds 2^22 / 2049 = 2047 rows, so two blocks; against
    float64 numpy"""
    rng = np.random.default_rng(5)
    xq, xt, a = rng.standard_normal((2100, 5)), rng.standard_normal((2049, 5)), rng.standard_normal((2049, 3))
    out = petal.kernel_apply(xq, xt, a, "rbf", gamma=0.3, ctx=ctx)
    k = kc.kernel_matrix(kc.Spec("rbf", 0.3), xq, xt, None, np.float64)
    assert np.abs(out - k @ a).max() <= 1e-12 * (np.abs(k) @ np.abs(a)).max()


def test_errors(ctx):
    def sharded():
        other = hostsim.context()
        other.set_collective(lambda *a: 0, 0, 2)
        return other
    kc.check_errors(ctx, sharded)


def test_zero_components_and_release(ctx):
    x = np.array(kc.fit_inputs(33, 19, "f64"))
    m = petal.KernelPca(0, "rbf", ctx=ctx)
    assert m.fit_transform(x).shape == (33, 0) and m.transform(x[:5]).shape == (5, 0) and m.eigenvalues().shape == (0,)
    other = hostsim.context()
    m = petal.KernelPca(2, "cosine", ctx=other).fit(x)
    with pytest.raises(petal.InvalidInput, match="another ctx"):
        ctx.check(ctx.lib.petal_kpca_transform(ctx._h, m._h, C.byref(petal.describe(x, [])), C.byref(petal.describe(np.zeros((33, 2)), []))))
    other.close()                                  # releases the model with its ctx
    with pytest.raises(petal.InvalidInput, match="not been fitted"):
        m.transform(x)


def test_option_round_trip(ctx):
    assert petal.OPTIONS["kpca_fallback"] == 36
    assert ctx.get_option("kpca_fallback") == 0.0
    ctx.set_option("kpca_fallback", 1)
    assert ctx.get_option(36) == 1.0
    ctx.set_option("kpca_fallback", 0)
    assert ctx.get_option("kpca_fallback") == 0.0
    with pytest.raises(petal.InvalidInput):
        ctx.set_option(37, 1)


# ------------------------------------------------------------------------------------------- the header, Python, Rust, C++
def _header_functions():
    return kit.header_functions(HEADER, drop=(r"typedef struct petal_kernel_spec \{.*?\} petal_kernel_spec;", r"typedef struct petal_kpca petal_kpca;"))


def test_header_is_exported_and_bound_by_python():
    fns = _header_functions()
    kit.check_python_table("petal_hip_kpca.h", fns, ENTRIES)
    kit.check_exported(fns)
    assert fns["petal_kpca_fit"] == ("i32", ["ptr", "ptr", "i64", "ptr", "ptr", "ptr"])
    assert fns["petal_kernel_apply"] == ("i32", ["ptr", "ptr", "ptr", "ptr", "ptr", "i64", "ptr", "ptr", "ptr"])
    text = open(HEADER).read()
    assert '#include "petal_hip.h"' in text
    assert int(re.search(r"#define\s+PETAL_OPT_KPCA_FALLBACK\s+(\d+)", text).group(1)) == petal.OPTIONS["kpca_fallback"]
    for name, code in petal.KERNELS.items():
        assert int(re.search(rf"#define\s+PETAL_KERNEL_{name.upper()}\s+(\d+)", text).group(1)) == code
    assert C.sizeof(petal.petal_kernel_spec) == 24
    for word in ("ZERO COLUMN", "laplacian is not included", "Not in this version", "sharded fits", "sparse input", "precomputed kernels",
                 "inverse_transform", "split-bf16", "incremental or Nystroem", "ITS OWN device copy", "float64 inside"):
        assert word in text, word                                                 # the disclosures the header owes


def test_rust_binding_and_cpp_facade_match_the_header():
    text = re.sub(r"//.*$", "", open(FFI).read(), flags=re.M)
    assert kit.rust_functions(FFI) == _header_functions()
    assert int(re.search(r"PETAL_OPT_KPCA_FALLBACK:\s*c_int\s*=\s*(\d+)", text).group(1)) == petal.OPTIONS["kpca_fallback"]
    for name, code in petal.KERNELS.items():
        assert int(re.search(rf"PETAL_KERNEL_{name.upper()}:\s*i32\s*=\s*(\d+)", text).group(1)) == code
    fields = re.search(r"pub struct PetalKernelSpec \{(.*?)\}", text, flags=re.S).group(1)
    assert re.findall(r"pub (\w+): (\w+)", fields) == [("kernel", "i32"), ("degree", "i32"), ("gamma", "f64"), ("coef0", "f64")]
    src = os.path.join(ROOT, "rust", "petal-decomposition-hip", "src")
    lib = open(os.path.join(src, "lib.rs")).read()
    assert "mod ffi_kpca;" in lib and "mod kpca;" in lib and "KernelPca" in lib and "PETAL_OPT_KPCA_FALLBACK" in lib
    kp = open(os.path.join(src, "kpca.rs")).read()
    for name in ENTRIES[1:]:
        assert f"ffi_kpca::{name}" in kp, name
    assert "pub struct KernelPca" in kp and "impl<A: HipScalar> Drop for KernelPca<A>" in kp
    hpp = open(os.path.join(ROOT, "include", "petal_decomposition.hpp")).read()
    assert '#include "petal_hip_kpca.h"' in hpp and "class KernelPca" in hpp
    for name in ENTRIES[1:]:
        assert name in hpp, name


def test_cpp_facade_on_host_simulation():
    kit.run_cpp_facade("kpca", "fallback", hostsim.build(), "hostsim")


# ------------------------------------------------------------------------------------------- D: kernel budgets
def test_kapply_kernel_budget(resources):
    """the figures DESIGN.md section 4 quotes, read from the built library's code-object notes: all twenty instantiations of the fused
    pass (float / double, five kernels, a 32- or a 64-column panel) without scratch, spills or LDS; the two output tiles of a panel live
    in 64 / 96 accumulation registers; at least two waves per SIMD, three for the 32-column panel of linear, poly and cosine"""
    hits = {k: v for k, v in resources.items() if re.search(r"k_kapply<(float|double), [0-4], [24]>$", k)}
    assert len(hits) == 20, sorted(hits)
    for name, r in hits.items():
        print(name, r)
        np_ = int(name[-2])
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["lds"] == 0 and r["max_wg"] == 256, (name, r)
        assert r["agpr"] == (64 if np_ == 2 else 96) and r["vgpr"] <= (176 if np_ == 2 else 208), (name, r)
        assert r["waves_per_simd"] >= 2, (name, r)
        if np_ == 2 and int(name[-5]) in (0, 1, 4):
            assert r["waves_per_simd"] >= 3, (name, r)


def test_fit_side_kernel_budget(resources):
    """k_kmap (and the row-sum tree it shares with k_kmeans: 256 doubles of LDS), k_kcentre, k_krownorm, k_kfinish: no scratch, no
    spills, eight waves per SIMD"""
    names = ["petal::k_kmap", "petal::k_kmeans", "petal::k_kcentre"] + \
        [f"void petal::{k}<{t}>" for k in ("k_krownorm", "k_kfinish") for t in ("float", "double")]
    for name in names:
        r = resources[name]
        print(name, r)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["waves_per_simd"] == 8, (name, r)
        assert r["lds"] == (2048 if name in ("petal::k_kmap", "petal::k_kmeans") else 0), (name, r)
    assert resources["petal::k_kmap"]["vgpr"] <= 64
