"""Nmf with the coordinate-descent solver (include/petal_hip_nmf_cd.h) without a GPU, on the host simulation -- whose device-op layer
has none of the k_nmf_cd_* kernels, so every pass and every H update takes the composed path (kernel 0): the model against
scikit-learn, the pass on exact operands and against long double, the fits against the model, transform, the stopping rule, the random
initialisation, the shapes outside the kernel's envelope, what did not move, every error; the new header against the built libraries,
the Python table, the Rust binding and the C++ facade; the register / scratch budget of the kernels in the built library."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest

import header_kit as kit
import hostsim
import nmf_cd_cases as cc
from header_kit import resources  # noqa: F401  (the fixture)
import petal_decomposition_amd as petal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "petal_hip_nmf_cd.h")
FFI = os.path.join(ROOT, "rust", "petal-decomposition-hip", "src", "ffi_nmf_cd.rs")
ENTRIES = ["petal_nmf_cd_hupdate", "petal_nmf_cd_pass", "petal_nmf_fit_solver", "petal_nmf_get_solver"]


@pytest.fixture(scope="module")
def ctx():
    c = hostsim.context()
    yield c
    c.close()


# ------------------------------------------------------------------------------------------- 1: the model against scikit-learn
SK_CASES = [(100, 80, 17, 0.0, 7, 0.0, 0.0), (37, 24, 3, 1e-4, 500, 0.0, 0.0), (60, 40, 5, 1e-3, 500, 0.01, 0.5)]


@pytest.mark.parametrize("shape", SK_CASES, ids=str)
def test_model_equals_sklearn(shape):
    sk = pytest.importorskip("sklearn.decomposition")
    n, d, k, tol, iters, alpha, rho = shape
    rng = np.random.default_rng(n + d + k)
    x = np.abs(rng.standard_normal((n, k))) @ np.abs(rng.standard_normal((k, d))) + 0.05 * np.abs(rng.standard_normal((n, d)))
    avg = np.sqrt(x.mean() / k)
    w0, h0 = avg * np.abs(rng.standard_normal((n, k))), avg * np.abs(rng.standard_normal((k, d)))
    xq = x[:11] * 0.5 + x[11:22] * 0.5
    est = sk.NMF(n_components=k, init="custom", solver="cd", tol=tol, max_iter=iters, alpha_W=alpha, alpha_H="same", l1_ratio=rho, shuffle=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        w = est.fit_transform(x, W=w0.copy(), H=h0.copy())
    mo = cc.model_fit(x, w0, h0, iters, tol, cc.penalties(n, d, alpha, "same", rho))
    if tol > 0:
        assert est.n_iter_ == mo.n_iter
    else:
        assert mo.n_iter == iters
    assert max(cc.rel_max(mo.w, w), cc.rel_max(mo.h, est.components_)) <= 1e-10
    assert abs(mo.err - est.reconstruction_err_) <= 1e-10 * est.reconstruction_err_
    if tol == 0:   # transform at tol = 0: from W = 0, exactly max_iter sweeps
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            wq = est.transform(xq)
        mq = cc.model_transform(xq, mo.h, iters, cc.penalties(xq.shape[0], d, alpha, "same", rho))
        assert cc.rel_max(mq, wq) <= 1e-10


# ------------------------------------------------------------------------------------------- 2, 3: petal_nmf_cd_pass, petal_nmf_cd_hupdate
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_pass_on_exact_operands(ctx, dt):
    for shape in cc.INT_SHAPES + cc.INT_SHAPES_PERSISTENT[:1]:
        cc.check_integers_exact(ctx, shape, dt, expect_kernel=False)


def test_pass_on_a_view_with_a_row_pitch_above_d(ctx):
    for shape in ((17, 3, 16), (33, 17, 80), (37, 64, 512)):
        for dt in ("f32", "f64"):
            cc.check_integers_exact(ctx, shape, dt, expect_kernel=False, pitch=True)


@pytest.mark.parametrize("case", cc.PASS_CASES, ids=lambda c: c.name)
def test_pass_against_long_double(ctx, case):
    cc.check_pass_against_long_double(ctx, case, expect_kernel=False)


@pytest.mark.parametrize("case", cc.H_CASES, ids=lambda c: c.name)
def test_hupdate_against_long_double(ctx, case):
    cc.check_hupdate_against_long_double(ctx, case, expect_kernel=False)


def test_padded_components_stay_zero_and_add_no_violation(ctx):
    """k = 3 pads to 16 and d = 24 to 32: with both penalties on, the result and the violation are the model's, which knows no padding"""
    x, w, h = cc.nc.pass_inputs(37, 80, 3, "f64")
    (wn, a, b, v), _ = petal.nmf_cd_pass(x, w, h, l1_w=0.5, l2_w=0.25, inner_iters=2, ctx=ctx, want_info=True)
    mw, ma, mb, mv = cc.model_pass(x, w, h, 0.5, 0.25, 2)
    assert max(cc.rel_max(wn, mw), cc.rel_max(a, ma), cc.rel_max(b, mb), cc.rel_max(v, mv)) <= 1e-12
    hn, hv = petal.nmf_cd_hupdate(ma[:, :24], mb, h[:, :24], l1_h=0.5, l2_h=0.25, ctx=ctx)
    mh, mhv = cc.model_hupdate(ma[:, :24], mb, h[:, :24], 0.5, 0.25)
    assert cc.rel_max(hn, mh) <= 1e-12 and abs(hv - mhv) <= 1e-12 * mhv


# ------------------------------------------------------------------------------------------- 4: fits and transforms
@pytest.mark.parametrize("case", cc.FIT_CASES, ids=lambda c: c.name)
def test_fit_matches_the_model(ctx, case):
    cc.check_fit_against_model(ctx, case, expect_kernel=False)


@pytest.mark.parametrize("updates", [None, 200])
@pytest.mark.parametrize("case", cc.FIT_CASES[3:4] + cc.FIT_CASES[15:16] + cc.FIT_CASES[-1:], ids=lambda c: c.name)
def test_transform_matches_the_model(ctx, case, updates):
    cc.check_transform(ctx, case, expect_kernel=False, updates=updates)


# ------------------------------------------------------------------------------------------- 5: the stopping rule
@pytest.mark.parametrize("case", cc.STOP_CASES, ids=lambda c: c.name)
def test_stopping_rule(ctx, case):
    cc.check_stopping_rule(ctx, case, expect_kernel=False)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_zero_violation_stops_at_iteration_one(ctx, dt):
    cc.check_zero_violation_stops_at_once(ctx, dt, expect_kernel=False)


def test_model_stops_where_sklearn_stops():
    sk = pytest.importorskip("sklearn.decomposition")
    for c in cc.STOP_CASES:
        x, w0, h0 = (np.array(v, dtype=np.float64) for v in cc.stop_inputs(c))
        est = sk.NMF(n_components=c.k, init="custom", solver="cd", tol=c.tol, max_iter=cc.STOP_MAX_ITER)
        est.fit_transform(x, W=w0.copy(), H=h0.copy())
        assert est.n_iter_ == cc.check_stop_case_is_decided(c).n_iter


# ------------------------------------------------------------------------------------------- 6, 7: random init, determinism, paths
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_random_init_draws_from_the_pcg_stream(ctx, dt):
    cc.check_random_init(ctx, dt, expect_kernel=False)


def test_same_fit_twice_gives_the_same_bytes(ctx):
    cc.check_same_bytes_twice(ctx, cc.FIT_CASES[7])


def test_forced_fallback_is_the_path_of_this_layer(ctx):
    cc.check_fallback_against_kernel(ctx, expect_kernel=False)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("shape", cc.OUTSIDE_SHAPES, ids=str)
def test_shapes_outside_the_kernel_envelope(ctx, shape, dt):
    cc.check_outside_envelope(ctx, shape, dt)


def test_composed_path_walks_the_rows_in_blocks(ctx):
    """8200 rows of 512 columns: the composed pass holds 2^22 / 512 = 8192 rows at a time, so two blocks; against the model"""
    rng = np.random.default_rng(5)
    n, d, k = 8200, 512, 2
    x = rng.random((n, d)).astype(np.float32)
    w, h = rng.random((n, k)) + 0.1, rng.random((k, d)) + 0.1
    wn, a, b, v = petal.nmf_cd_pass(x, w, h, l1_w=0.5, inner_iters=2, ctx=ctx)
    mw, ma, mb, mv = cc.model_pass(x, w, h, 0.5, 0.0, 2)
    assert max(cc.rel_max(wn, mw), cc.rel_max(a, ma), cc.rel_max(b, mb), cc.rel_max(v, mv)) <= 1e-12


@pytest.mark.parametrize("case", cc.nc.FIT_CASES[1:2] + cc.nc.FIT_CASES[10:11], ids=lambda c: c.name)
def test_nothing_existing_moved(ctx, case):
    cc.check_nothing_existing_moved(ctx, case)


# ------------------------------------------------------------------------------------------- 8: errors
def test_errors(ctx):
    def sharded():
        other = hostsim.context()
        other.set_collective(lambda *a: 0, 0, 2)
        return other
    cc.check_errors(ctx, hostsim.context, sharded)


def test_scipy_and_sklearn_are_imported_by_the_package_nowhere():
    text = open(os.path.join(ROOT, "petal-decomposition_amd", "__init__.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(scipy|sklearn)", text, flags=re.M)
    for rel in ("tests/nmf_cd_cases.py", "tests/test_gpu_nmf_cd.py"):
        text = open(os.path.join(ROOT, rel)).read()
        assert not re.search(r"^\s*(import|from)\s+(scipy|sklearn)", text, flags=re.M), rel


# ------------------------------------------------------------------------------------------- 9: the header, Python, Rust, C++
def test_header_is_exported_and_bound_by_python():
    fns = kit.header_functions(HEADER)
    kit.check_python_table("petal_hip_nmf_cd.h", fns, ENTRIES)
    kit.check_exported(fns)
    assert fns["petal_nmf_fit_solver"] == ("i32", ["ptr", "ptr", "i64", "ptr", "i64", "ptr", "ptr", "i64", "ptr", "ptr"])
    assert fns["petal_nmf_get_solver"] == ("i32", ["ptr", "ptr"])
    assert fns["petal_nmf_cd_pass"] == ("i32", ["ptr", "ptr", "i64", "ptr", "ptr", "ptr", "i64", "i32", "ptr", "ptr", "ptr", "ptr", "ptr"])
    assert fns["petal_nmf_cd_hupdate"] == ("i32", ["ptr", "i64", "i64", "ptr", "ptr", "ptr", "ptr", "ptr", "ptr", "ptr"])
    text = open(HEADER).read()
    assert '#include "petal_hip_nmf_kl_dense.h"' in text
    assert re.search(r"#define\s+PETAL_NMF_SOLVER_MU\s+0\b", text) and re.search(r"#define\s+PETAL_NMF_SOLVER_CD\s+1\b", text)
    assert (petal.NMF_SOLVER_MU, petal.NMF_SOLVER_CD) == (0, 1)
    for word in ("eps is not used", "grad = -z[t] + sum_r S[t][r] w[r]", "min(0, grad)", "max(w[t] - grad / S[t][t], 0)", "the CURRENT w",
                 "No shuffling", "W starts at ZERO", "No tolerance stop in transform", "tol = 0 runs exactly max_iter iterations",
                 "violation / violation_init <= tol", "Padded components stay zero", "no floating-point atomics", "the same bytes",
                 "rounded once", "a function of the shape alone", "formed afresh", "16, 32 or 64 padded components",
                 "at most 512 padded columns", "k = 33 .. 48", "PETAL_OPT_NMF_FALLBACK", "composed path", "unmeasured",
                 "nmf_cd_pass wrote outside the n x k block", "Not in this version", "Kullback-Leibler loss", "CSR input", "sharded fits",
                 "shuffle=True"):
        assert word in text, word                                                 # the disclosures the header owes
    # the existing signatures stay as they are, and the first header keeps its sentence and points here
    assert C.sizeof(petal.petal_nmf_spec) == 48
    other = open(os.path.join(ROOT, "include", "petal_hip_nmf.h")).read()
    assert "the coordinate-descent solver" in other and "petal_hip_nmf_cd.h" in other


def test_rust_binding_and_cpp_facade_match_the_header():
    assert kit.rust_functions(FFI) == kit.header_functions(HEADER)
    text = re.sub(r"//.*$", "", open(FFI).read(), flags=re.M)
    assert re.search(r"PETAL_NMF_SOLVER_MU:\s*i64\s*=\s*0\b", text) and re.search(r"PETAL_NMF_SOLVER_CD:\s*i64\s*=\s*1\b", text)
    src = os.path.join(ROOT, "rust", "petal-decomposition-hip", "src")
    lib = open(os.path.join(src, "lib.rs")).read()
    assert "mod ffi_nmf_cd;" in lib and "NmfSolver" in lib
    nm = open(os.path.join(src, "nmf.rs")).read()
    for name in ("petal_nmf_fit_solver", "petal_nmf_get_solver"):
        assert f"ffi_nmf_cd::{name}" in nm, name
    assert "pub enum NmfSolver" in nm and "pub solver: NmfSolver" in nm
    hpp = open(os.path.join(ROOT, "include", "petal_decomposition.hpp")).read()
    assert '#include "petal_hip_nmf_cd.h"' in hpp and "enum class NmfSolver" in hpp and "CoordinateDescent" in hpp
    for name in ("petal_nmf_fit_solver", "petal_nmf_get_solver"):
        assert name in hpp, name


def test_cpp_facade_on_host_simulation():
    kit.run_cpp_facade("nmf_cd", "host", hostsim.build(), "hostsim")


# ------------------------------------------------------------------------------------------- 10: kernel budgets
def test_kernel_budget(resources):
    """all 48 instantiations of the pass (float / double; 1, 2 or 4 component tiles; 1, 2, 4 or 8 feature tiles per wave; with A and B
    or without), the three forms of the H-side kernel and the violation sum: no scratch, no spilled register, 256 threads"""
    passes = {k: v for k, v in resources.items() if re.search(r"k_nmf_cd_pass<(float|double), [124], [1248], (true|false)>$", k)}
    side = {k: v for k, v in resources.items() if re.search(r"k_nmf_cd_hrule<[124]>$", k) or re.search(r"petal::k_nmf_cd_violsum\b", k)}
    assert (len(passes), len(side)) == (48, 4), (sorted(passes), sorted(side))
    for name, r in {**passes, **side}.items():
        print(name, r)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["max_wg"] == 256, (name, r)
    for name, r in passes.items():
        assert r["waves_per_simd"] >= 1 and r["vgpr"] <= 512, (name, r)
