"""Nmf with the Kullback-Leibler loss on dense data (include/petal_hip_nmf_kl_dense.h) without a GPU, on the host simulation -- whose
device-op layer has none of the k_nmf_kl_* kernels, so every pass takes the composed path (kernel_path 0): the pass on exact operands and
against long double, the fits against the model and the CSR route, transform, the stopping rule, the random initialisation, the shapes
outside the kernel's envelope, what did not move, every error; the new header against the built libraries, the Python table, the Rust
binding and the C++ facade; the register / scratch budget of the kernels in the built library."""
import ctypes as C
import os
import re

import pytest

import header_kit as kit
import hostsim
import nmf_kl_dense_cases as dc
from header_kit import resources  # noqa: F401  (the fixture)
import petal_decomposition_amd as petal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "petal_hip_nmf_kl_dense.h")
FFI = os.path.join(ROOT, "rust", "petal-decomposition-hip", "src", "ffi_nmf_kl_dense.rs")
ENTRIES = ["petal_nmf_fit_loss", "petal_nmf_kl_pass", "petal_nmf_transform_loss"]


@pytest.fixture(scope="module")
def ctx():
    c = hostsim.context()
    yield c
    c.close()


# ------------------------------------------------------------------------------------------- 1, 2: petal_nmf_kl_pass
def test_the_model_of_the_pass_is_the_model_of_the_sweep():
    """the dense model of this module equals nmf_kl_cases' CSR model on a matrix with zeros, to rounding"""
    import numpy as np
    x, w, h = (np.array(v) for v in dc.nc.pass_inputs(83, 200, 17, "f64"))
    x[::3, ::2] = 0.0
    img = dc.kc.image_of(dc.to_csr(x), x.shape, False)
    for inner in (0, 1, 3):
        mw, _, mc, mt = dc.model_pass(x, w, h, 0.25, 0.5, inner)
        sw, sc, st = dc.kc.model_kl_sweep(img, w, h.T.copy(), 0.25, 0.5, inner)
        assert dc.rel_max(mw, sw) <= 1e-13 and dc.rel_max(mc, sc) <= 1e-13
        if inner == 0:
            assert abs(mt - st) <= 1e-12 * abs(st)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_pass_on_exact_operands(ctx, dt):
    for shape in dc.INT_SHAPES + dc.INT_SHAPES_PERSISTENT:
        dc.check_integers_exact(ctx, shape, dt, expect_kernel=False)


def test_pass_on_a_view_with_a_row_pitch_above_d(ctx):
    for shape in ((17, 3, 16), (33, 17, 80), (37, 64, 512)):
        for dt in ("f32", "f64"):
            dc.check_integers_exact(ctx, shape, dt, expect_kernel=False, pitch=True)


@pytest.mark.parametrize("case", dc.PASS_CASES, ids=lambda c: c.name)
def test_pass_against_long_double(ctx, case):
    dc.check_pass_against_long_double(ctx, case, expect_kernel=False)


# ------------------------------------------------------------------------------------------- 3 .. 8: Nmf(dense_path="fused")
@pytest.mark.parametrize("case", dc.FIT_CASES, ids=lambda c: c.name)
def test_fit_matches_the_model_and_the_csr_route(ctx, case):
    m = dc.check_fit_against_model(ctx, case, expect_kernel=False)
    assert m.kernel_path == 0


@pytest.mark.parametrize("updates", [13, 200])
@pytest.mark.parametrize("case", dc.FIT_CASES[:1] + dc.FIT_CASES[11:12] + dc.FIT_CASES[-1:], ids=lambda c: c.name)
def test_transform_matches_the_model(ctx, case, updates):
    dc.check_transform(ctx, case, expect_kernel=False, updates=updates)


@pytest.mark.parametrize("case", dc.kc.STOP_CASES, ids=lambda c: c.name)
def test_stopping_rule(ctx, case):
    dc.check_stopping_rule(ctx, case, expect_kernel=False)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_random_init_draws_from_the_pcg_stream(ctx, dt):
    dc.check_random_init(ctx, dt, expect_kernel=False)


@pytest.mark.parametrize("case", dc.FIT_CASES[2:3] + dc.FIT_CASES[-1:], ids=lambda c: c.name)
def test_same_fit_twice_gives_the_same_bytes(ctx, case):
    dc.check_same_bytes_twice(ctx, case)


@pytest.mark.parametrize("case", dc.FIT_CASES[1:2], ids=lambda c: c.name)
def test_forced_fallback_is_the_composed_path(ctx, case):
    dc.check_fallback_against_kernel(ctx, case, expect_kernel=False)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("shape", dc.OUTSIDE_SHAPES, ids=str)
def test_shapes_outside_the_kernel_envelope(ctx, shape, dt):
    dc.check_outside_envelope(ctx, shape, dt)


@pytest.mark.parametrize("case", dc.FIT_CASES[1:2] + dc.FIT_CASES[10:11], ids=lambda c: c.name)
def test_nothing_existing_moved(ctx, case):
    dc.check_nothing_existing_moved(ctx, case)


def test_errors(ctx):
    def sharded():
        other = hostsim.context()
        other.set_collective(lambda *a: 0, 0, 2)
        return other
    dc.check_errors(ctx, hostsim.context, sharded)


def test_scipy_and_sklearn_are_imported_nowhere():
    for rel in ("tests/nmf_kl_dense_cases.py", "tests/test_nmf_kl_dense_host.py", "tests/test_gpu_nmf_kl_dense.py"):
        text = open(os.path.join(ROOT, rel)).read()
        assert not re.search(r"^\s*(import|from)\s+(scipy|sklearn)", text, flags=re.M), rel


# ------------------------------------------------------------------------------------------- 9: the header, Python, Rust, C++
def test_header_is_exported_and_bound_by_python():
    fns = kit.header_functions(HEADER)
    kit.check_python_table("petal_hip_nmf_kl_dense.h", fns, ENTRIES)
    kit.check_exported(fns)
    assert fns["petal_nmf_fit_loss"] == ("i32", ["ptr", "ptr", "i64", "ptr", "i64", "ptr", "ptr", "i64", "ptr", "ptr"])
    assert fns["petal_nmf_transform_loss"] == ("i32", ["ptr", "ptr", "ptr", "ptr"])
    assert fns["petal_nmf_kl_pass"] == ("i32", ["ptr", "ptr", "i64", "ptr", "ptr", "ptr", "i64", "ptr", "ptr", "ptr", "ptr", "ptr"])
    text = open(HEADER).read()
    assert '#include "petal_hip_nmf_kl.h"' in text
    for word in ("Not in this version", "sharded fits", "other beta", "tolerance stop in transform", "split-bf16", "no floating-point atomics",
                 "the same bytes", "rounded once", "a function of the shape alone", "without a reciprocal", "16, 32 or 64 padded components",
                 "at most 512 padded columns", "k = 33 .. 48", "PETAL_OPT_NMF_FALLBACK", "composed path", "has no cap", "unmeasured",
                 "three launches", "nmf_kl_pass wrote outside the n x k block", "stays the compressed CSR route"):
        assert word in text, word                                                 # the disclosures the header owes
    # the existing signatures stay as they are, and the CSR header still owes what it owed
    assert C.sizeof(petal.petal_nmf_spec) == 48
    other = open(os.path.join(ROOT, "include", "petal_hip_nmf_kl.h")).read()
    assert "petal_hip_nmf_kl_dense.h" in other and "fused dense Kullback-Leibler kernel" in other


def test_rust_binding_and_cpp_facade_match_the_header():
    assert kit.rust_functions(FFI) == kit.header_functions(HEADER)
    src = os.path.join(ROOT, "rust", "petal-decomposition-hip", "src")
    lib = open(os.path.join(src, "lib.rs")).read()
    assert "mod ffi_nmf_kl_dense;" in lib and "NmfDensePath" in lib
    nm = open(os.path.join(src, "nmf.rs")).read()
    for name in ("petal_nmf_fit_loss", "petal_nmf_transform_loss"):
        assert f"ffi_nmf_kl_dense::{name}" in nm, name
    assert "pub enum NmfDensePath" in nm and "dense_path" in nm
    hpp = open(os.path.join(ROOT, "include", "petal_decomposition.hpp")).read()
    assert '#include "petal_hip_nmf_kl_dense.h"' in hpp and "enum class NmfDensePath" in hpp
    for name in ("petal_nmf_fit_loss", "petal_nmf_transform_loss"):
        assert name in hpp, name


def test_cpp_facade_on_host_simulation():
    kit.run_cpp_facade("nmf_kl_dense", "host", hostsim.build(), "hostsim")


# ------------------------------------------------------------------------------------------- 10: kernel budgets
def test_kernel_budget(resources):
    """all 46 instantiations of the pass (float / double; 1, 2 or 4 component tiles; 1, 2, 4 or 8 feature tiles per wave; with the H side
    or without -- but not 4 x 8 with the H side, which op_nmf_kl_pass splits) and the two H-side kernels: no scratch, no spilled registers"""
    passes = {k: v for k, v in resources.items() if re.search(r"k_nmf_kl_pass<(float|double), [124], [1248], (true|false)>$", k)}
    side = {k: v for k, v in resources.items() if re.search(r"petal::k_nmf_kl_(hrule|rowsum)\b", k)}
    assert (len(passes), len(side)) == (46, 2), (sorted(passes), sorted(side))
    assert not [k for k in passes if re.search(r"<(float|double), 4, 8, true>$", k)]
    for name, r in {**passes, **side}.items():
        print(name, r)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
