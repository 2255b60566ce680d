"""Nmf (include/petal_hip_nmf.h) without a GPU, on the host simulation -- whose device-op layer has none of the k_nmf_* kernels, so the
pass, the scan and the H update come from the composed path built on op_cvt_to_f64, op_dgemm and an element-wise step on the host, and
`info()` reports kernel = 0: the statement of petal_nmf_pass (exact operands, the long-double bound and its cap), the whole host
sequencing of fit / fit_transform / transform / inverse_transform against the numpy model, the stopping rule, the random
initialisation, every error; the model itself against scikit-learn; the new header against the built libraries, the Python table, the
Rust binding and the C++ facade; the register / scratch budget of the kernels in the built library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import header_kit as kit
import hostsim
import nmf_cases as nc
from header_kit import resources  # noqa: F401  (the fixture)
import petal_decomposition_amd as petal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "petal_hip_nmf.h")
FFI = os.path.join(ROOT, "rust", "petal-decomposition-hip", "src", "ffi_nmf.rs")
ENTRIES = ["petal_nmf_destroy", "petal_nmf_fit", "petal_nmf_get", "petal_nmf_inverse_transform", "petal_nmf_pass", "petal_nmf_transform"]


@pytest.fixture(scope="module")
def ctx():
    c = hostsim.context()
    yield c
    c.close()


# ------------------------------------------------------------------------------------------- 1, 2: petal_nmf_pass
@pytest.mark.parametrize("inner", [1, 3])
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_pass_on_exact_operands(ctx, dt, inner):
    for shape in nc.INT_SHAPES + nc.INT_SHAPES_PERSISTENT[:1]:
        nc.check_integers_exact(ctx, shape, dt, inner, expect_kernel=False)


def test_pass_on_exact_operands_fortran_order(ctx):
    for shape in ((17, 3, 24), (33, 17, 80)):
        nc.check_integers_exact(ctx, shape, "f32", 1, expect_kernel=False, form="host-fortran")


@pytest.mark.parametrize("case", nc.PASS_CASES, ids=lambda c: c.name)
def test_pass_against_long_double(ctx, case):
    nc.check_pass_against_long_double(ctx, case, expect_kernel=False)


@pytest.mark.parametrize("case", nc.PASS_CASES, ids=lambda c: c.name)
def test_fp32_accumulation_would_break_the_cap(case):
    """why every product and sum is float64: the numpy model alone stays within the cap on these inputs under the largest multiplier;
    the same statement with float32 products and sums misses it by decades in W_new, A and B"""
    x, w, h = nc.pass_inputs(case.n, case.d, case.k, case.dt)
    out32 = nc.model_pass(x, w, h, case.l1, case.l2, case.inner, np.float32)
    for name, o32, (ref, model, scale) in zip("WAB", out32, nc.pass_reference(case)):
        e32 = float(np.abs(o32.astype(np.longdouble) - ref).max()) / scale
        print(f"{case.name} {name}: float64 {model / scale:.2e}, float32 {e32:.2e} of the scale (cap {nc.CAP:.0e})")
        assert max(nc.MULTIPLIER.values()) * max(model / scale, nc.FLOOR_EPS * nc.EPS64) <= nc.CAP
        assert e32 > 100 * nc.CAP


def test_pass_arguments(ctx):
    x, w, h = (np.array(v) for v in nc.pass_inputs(83, 200, 17, "f64"))
    mx = petal.describe(x, [])
    spec = petal.petal_nmf_spec(1, 0.0, 0.0, 0.0, 0.0, 0.0)
    wo = np.zeros_like(w)
    D = petal._D
    assert ctx.lib.petal_nmf_pass(ctx._h, None, 17, w.ctypes.data_as(D), h.ctypes.data_as(D), C.byref(spec), 1, wo.ctypes.data_as(D), None, None,
                                  None) == petal.PETAL_INVALID_INPUT
    assert ctx.lib.petal_nmf_pass(ctx._h, C.byref(mx), 17, None, h.ctypes.data_as(D), C.byref(spec), 1, wo.ctypes.data_as(D), None, None,
                                  None) == petal.PETAL_INVALID_INPUT
    assert ctx.lib.petal_nmf_pass(ctx._h, C.byref(mx), 17, w.ctypes.data_as(D), h.ctypes.data_as(D), C.byref(spec), 1, wo.ctypes.data_as(D),
                                  wo.ctypes.data_as(D), None, None) == petal.PETAL_INVALID_INPUT      # a_out without b_out
    assert ctx.lib.petal_nmf_pass(ctx._h, C.byref(mx), 17, w.ctypes.data_as(D), h.ctypes.data_as(D), C.byref(spec), -1, wo.ctypes.data_as(D),
                                  None, None, None) == petal.PETAL_INVALID_INPUT
    assert ctx.lib.petal_nmf_get(None, None, None, None) == petal.PETAL_INVALID_INPUT
    assert ctx.lib.petal_nmf_transform(ctx._h, None, C.byref(mx), C.byref(mx)) == petal.PETAL_INVALID_INPUT
    assert ctx.lib.petal_nmf_inverse_transform(ctx._h, None, C.byref(mx), C.byref(mx)) == petal.PETAL_INVALID_INPUT
    out = C.c_void_p()
    assert ctx.lib.petal_nmf_fit(ctx._h, C.byref(mx), 3, None, None, None, 0, C.byref(out), None) == petal.PETAL_INVALID_INPUT
    assert ctx.lib.petal_nmf_fit(ctx._h, C.byref(mx), 3, C.byref(spec), None, None, 0, None, None) == petal.PETAL_INVALID_INPUT
    ctx.lib.petal_nmf_destroy(None)


# ------------------------------------------------------------------------------------------- 3, 5: fits and transforms
@pytest.mark.parametrize("case", nc.FIT_CASES, ids=lambda c: c.name)
def test_fit_matches_the_model(ctx, case):
    nc.check_fit_against_model(ctx, case, expect_kernel=False)


@pytest.mark.parametrize("case", nc.FIT_CASES[2:4] + nc.FIT_CASES[-2:], ids=lambda c: c.name)
def test_fortran_order_input(ctx, case):
    nc.check_fit_against_model(ctx, case, expect_kernel=False, form="host-fortran")


@pytest.mark.parametrize("case", nc.FIT_CASES[:1] + nc.FIT_CASES[3:4] + nc.FIT_CASES[-2:], ids=lambda c: c.name)
def test_transform_matches_the_model(ctx, case):
    nc.check_transform(ctx, case, expect_kernel=False)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_transform_with_thirteen_updates(ctx, dt):
    n, d, k = nc.FIT_SHAPES[0]
    nc.check_transform(ctx, nc.FitCase(f"{dt}-it13", n, d, k, dt, 13, 0.0, "same", 0.0), expect_kernel=False)


# ------------------------------------------------------------------------------------------- 4: the stopping rule
@pytest.mark.parametrize("case", nc.STOP_CASES, ids=lambda c: c.name)
def test_stopping_rule(ctx, case):
    nc.check_stopping_rule(ctx, case, expect_kernel=False)


# ------------------------------------------------------------------------------------------- 6, 7: random init, determinism
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_random_init_draws_from_the_pcg_stream(ctx, dt):
    nc.check_random_init(ctx, dt, expect_kernel=False)


def test_same_fit_twice_gives_the_same_bytes(ctx):
    nc.check_same_bytes_twice(ctx, nc.FIT_CASES[2])


# ------------------------------------------------------------------------------------------- 8: paths
def test_forced_fallback_is_the_path_of_this_layer(ctx):
    nc.check_fallback_against_kernel(ctx, nc.FIT_CASES[1], expect_kernel=False)


@pytest.mark.parametrize("shape", nc.OUTSIDE_SHAPES, ids=str)
def test_shapes_outside_the_kernel_envelope(ctx, shape):
    nc.check_outside_envelope(ctx, shape, "f64")


def test_composed_path_walks_the_rows_in_blocks(ctx):
    """8200 rows of 512 columns: the composed pass holds 2^22 / 512 = 8192 rows at a time, so two blocks; against the model"""
    rng = np.random.default_rng(5)
    n, d, k = 8200, 512, 2
    x = rng.random((n, d)).astype(np.float32)
    w, h = rng.random((n, k)) + 0.1, rng.random((k, d)) + 0.1
    wn, a, b = petal.nmf_pass(x, w, h, l1_w=0.5, inner_iters=2, ctx=ctx)
    mw, ma, mb = nc.model_pass(x, w, h, 0.5, 0.0, 2)
    assert max(nc.rel_max(wn, mw), nc.rel_max(a, ma), nc.rel_max(b, mb)) <= 1e-12


def test_option_round_trip(ctx):
    assert petal.OPTIONS["nmf_fallback"] == 38
    assert ctx.get_option("nmf_fallback") == 0.0
    ctx.set_option("nmf_fallback", 1)
    assert ctx.get_option(38) == 1.0
    ctx.set_option("nmf_fallback", 0)
    assert ctx.get_option("nmf_fallback") == 0.0
    for unknown in (35, 37, 39):
        with pytest.raises(petal.InvalidInput):
            ctx.set_option(unknown, 1)


# ------------------------------------------------------------------------------------------- 9: errors
def test_errors(ctx):
    def sharded():
        other = hostsim.context()
        other.set_collective(lambda *a: 0, 0, 2)
        return other
    nc.check_errors(ctx, sharded)


def test_release_with_the_ctx(ctx):
    x, w0, h0, _ = nc.fit_inputs(200, 48, 5, "f64")
    other = hostsim.context()
    m = petal.Nmf(5, max_iter=1, init="custom", ctx=other).fit(x, W=w0, H=h0)
    with pytest.raises(petal.InvalidInput, match="another ctx"):
        ctx.check(ctx.lib.petal_nmf_transform(ctx._h, m._h, C.byref(petal.describe(np.array(x), [])), C.byref(petal.describe(np.zeros((200, 5)), []))))
    other.close()                                  # releases the model with its ctx
    with pytest.raises(petal.InvalidInput, match="not been fitted"):
        m.transform(x)


# ------------------------------------------------------------------------------------------- 10: the model against scikit-learn
@pytest.mark.parametrize("reg", [False, True], ids=["plain", "regularised"])
def test_model_equals_sklearn(reg):
    sk = pytest.importorskip("sklearn.decomposition")
    n, d, k, iters = 200, 48, 5, 25
    x, w0, h0, xq = (np.array(v, dtype=np.float64) for v in nc.fit_inputs(n, d, k, "f64"))
    aw, ah, rho = (0.01, 0.02, 0.3) if reg else (0.0, 0.0, 0.0)
    est = sk.NMF(n_components=k, init="custom", solver="mu", beta_loss="frobenius", tol=0.0, max_iter=iters, alpha_W=aw, alpha_H=ah, l1_ratio=rho)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        w = est.fit_transform(x, W=w0.copy(), H=h0.copy())
        wq = est.transform(xq)
    pen = nc.penalties(n, d, aw, ah, rho)
    mo = nc.model_fit(x, w0, h0, iters, 0.0, pen)
    mq = nc.model_transform(xq, mo.h, k, iters, nc.penalties(xq.shape[0], d, aw, ah, rho))
    assert est.n_iter_ == mo.n_iter == iters
    assert max(nc.rel_max(mo.w, w), nc.rel_max(mo.h, est.components_), nc.rel_max(mq, wq)) <= 1e-12
    assert abs(mo.err - est.reconstruction_err_) <= 1e-12 * est.reconstruction_err_


def test_model_stops_where_sklearn_stops():
    sk = pytest.importorskip("sklearn.decomposition")
    for c in nc.STOP_CASES:
        x, w0, h0 = (np.array(v, dtype=np.float64) for v in nc.stop_inputs(c))
        est = sk.NMF(n_components=c.k, init="custom", solver="mu", tol=c.tol, max_iter=nc.STOP_MAX_ITER)
        est.fit_transform(x, W=w0.copy(), H=h0.copy())
        assert est.n_iter_ == nc.check_stop_case_is_decided(c).n_iter


# ------------------------------------------------------------------------------------------- 11: the header, Python, Rust, C++
def _header_functions():
    return kit.header_functions(HEADER, drop=(r"typedef struct petal_nmf_spec \{.*?\} petal_nmf_spec;", r"typedef struct petal_nmf petal_nmf;"))


def test_header_is_exported_and_bound_by_python():
    fns = _header_functions()
    kit.check_python_table("petal_hip_nmf.h", fns, ENTRIES)
    kit.check_exported(fns)
    assert fns["petal_nmf_fit"] == ("i32", ["ptr", "ptr", "i64", "ptr", "ptr", "ptr", "i64", "ptr", "ptr"])
    assert fns["petal_nmf_pass"] == ("i32", ["ptr", "ptr", "i64", "ptr", "ptr", "ptr", "i64", "ptr", "ptr", "ptr", "ptr"])
    text = open(HEADER).read()
    assert '#include "petal_hip.h"' in text
    assert int(re.search(r"#define\s+PETAL_OPT_NMF_FALLBACK\s+(\d+)", text).group(1)) == petal.OPTIONS["nmf_fallback"]
    assert C.sizeof(petal.petal_nmf_spec) == 48
    for word in ("Not in this version", "other beta-losses", "coordinate-descent", "NNDSVD", "CSR input", "sharded fits", "split-bf16",
                 "tolerance stop in transform", "natural follow-ups", "float64 inside", "the same bytes"):
        assert word in text, word                                                 # the disclosures the header owes


def test_rust_binding_and_cpp_facade_match_the_header():
    text = re.sub(r"//.*$", "", open(FFI).read(), flags=re.M)
    assert kit.rust_functions(FFI) == _header_functions()
    assert int(re.search(r"PETAL_OPT_NMF_FALLBACK:\s*c_int\s*=\s*(\d+)", text).group(1)) == petal.OPTIONS["nmf_fallback"]
    fields = re.search(r"pub struct PetalNmfSpec \{(.*?)\}", text, flags=re.S).group(1)
    assert re.findall(r"pub (\w+): (\w+)", fields) == [("max_iter", "i64"), ("tol", "f64"), ("l1_w", "f64"), ("l2_w", "f64"), ("l1_h", "f64"),
                                                        ("l2_h", "f64")]
    src = os.path.join(ROOT, "rust", "petal-decomposition-hip", "src")
    lib = open(os.path.join(src, "lib.rs")).read()
    assert "mod ffi_nmf;" in lib and "mod nmf;" in lib and "Nmf" in lib and "PETAL_OPT_NMF_FALLBACK" in lib
    nm = open(os.path.join(src, "nmf.rs")).read()
    for name in ENTRIES[:4] + ENTRIES[5:]:
        assert f"ffi_nmf::{name}" in nm, name
    assert "pub struct Nmf" in nm and "impl<A: HipScalar> Drop for Nmf<A>" in nm
    hpp = open(os.path.join(ROOT, "include", "petal_decomposition.hpp")).read()
    assert '#include "petal_hip_nmf.h"' in hpp and "class Nmf" in hpp
    for name in ENTRIES[:4] + ENTRIES[5:]:
        assert name in hpp, name


def test_cpp_facade_on_host_simulation():
    kit.run_cpp_facade("nmf", "fallback", hostsim.build(), "hostsim")


# ------------------------------------------------------------------------------------------- kernel budgets
def test_pass_kernel_budget(resources):
    """all 48 instantiations of the fused pass (float / double; 16, 32 or 64 padded components; 1, 2, 4 or 8 feature tiles per wave;
    with and without the accumulators of A and B) without scratch and without spilled registers; four waves per workgroup"""
    hits = {k: v for k, v in resources.items() if re.search(r"k_nmf_pass<(float|double), [124], [1248], (true|false)>$", k)}
    assert len(hits) == 48, sorted(hits)
    for name, r in hits.items():
        print(name, r)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["max_wg"] == 256, (name, r)
        assert r["waves_per_simd"] >= 1 and r["vgpr"] <= 512, (name, r)


def test_small_kernel_budget(resources):
    """k_nmf_scan, k_nmf_scan_sum, k_nmf_slabsum, k_nmf_hrule, k_nmf_dots: no scratch, no spills, eight waves per SIMD"""
    names = ["petal::k_nmf_scan_sum", "petal::k_nmf_slabsum", "petal::k_nmf_hrule", "petal::k_nmf_dots"] + \
        [f"void petal::k_nmf_scan<{t}>" for t in ("float", "double")]
    for name in names:
        r = resources[name]
        print(name, r)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["waves_per_simd"] == 8, (name, r)
