"""Nmf on sparse CSR data (include/petal_hip_nmf_sparse.h) without a GPU, on the host simulation -- whose device-op layer has neither the
sparse product nor the sweep, so a handle is not resident, every fit and transform densifies and runs the dense entry (kernel_path 0,
bit for bit the dense result) and petal_nmf_sweep_csr is the plain host loop of the statement: the sweep on exact operands and against
long double with its cap, the host sequencing against the numpy model, the stopping rule, the random initialisation, every error; the
new header against the built libraries, the Python table, the Rust binding and the C++ facade; the register / scratch budget of the
kernels in the built library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import header_kit as kit
import hostsim
import nmf_sparse_cases as ns
from header_kit import resources  # noqa: F401  (the fixture)
import petal_decomposition_amd as petal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "petal_hip_nmf_sparse.h")
FFI = os.path.join(ROOT, "rust", "petal-decomposition-hip", "src", "ffi_nmf_sparse.rs")
ENTRIES = ["petal_nmf_fit_csr", "petal_nmf_sweep_csr", "petal_nmf_transform_csr"]


@pytest.fixture(scope="module")
def ctx():
    c = hostsim.context()
    yield c
    c.close()


# ------------------------------------------------------------------------------------------- 1, 2: petal_nmf_sweep_csr
def test_every_seam_occurs():
    seen = ns.row_counts_seen()
    assert set(ns.SEAM_COUNTS) <= seen, sorted(set(ns.SEAM_COUNTS) - seen)
    assert 2 * ns.ITEM_NNZ + 3 == 515


@pytest.mark.parametrize("inner", ns.INT_INNER)
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_sweep_on_exact_operands(ctx, dt, inner):
    for which in range(-1, len(ns.INT_SHAPES)):
        ns.check_sweep_exact(ctx, which, dt, inner, expect_kernel=False, ks=(1, 3, 17, 64))


@pytest.mark.parametrize("case", ns.SWEEP_CASES, ids=lambda c: c.name)
def test_sweep_against_long_double(ctx, case):
    ns.check_sweep_against_long_double(ctx, case, expect_kernel=False)


@pytest.mark.parametrize("case", ns.SWEEP_CASES[::4], ids=lambda c: c.name)
def test_fp32_accumulation_would_break_the_cap(case):
    """why every product and sum is float64: the numpy model alone stays within the cap on these inputs under the largest multiplier;
    the same statement with float32 products and sums misses it by decades"""
    _, x, g, f = ns.sweep_inputs(case.n, case.d, case.k, case.dt, case.transposed)
    out32 = ns.model_sweep(x.T if case.transposed else x, g, f, case.l1, case.l2, case.inner, np.float32)
    for name, o32, (ref, model, scale) in zip(("G", "Gram", "dot"), out32, ns.sweep_reference(case)):
        e32 = float(np.abs(np.asarray(o32, dtype=np.longdouble) - ref).max()) / scale
        print(f"{case.name} {name}: float64 {model / scale:.2e}, float32 {e32:.2e} of the scale (cap {ns.CAP:.0e})")
        assert max(ns.MULTIPLIER.values()) * max(model / scale, ns.FLOOR_EPS * ns.EPS64) <= ns.CAP
        assert e32 > 100 * ns.CAP


# ------------------------------------------------------------------------------------------- 3 .. 6: fits on the densifying path
@pytest.mark.parametrize("case", ns.FIT_CASES[::3] + ns.FIT_CASES[-2:], ids=lambda c: c.name)
def test_fit_matches_the_model(ctx, case):
    ns.check_fit_against_model(ctx, case, expect_kernel=False)


def test_duck_typed_csr_is_accepted(ctx):
    ns.check_fit_against_model(ctx, ns.FIT_CASES[1], expect_kernel=False, duck=True)


@pytest.mark.parametrize("updates", [13, 200])
@pytest.mark.parametrize("case", ns.FIT_CASES[:1] + ns.FIT_CASES[-1:], ids=lambda c: c.name)
def test_transform_matches_the_model(ctx, case, updates):
    ns.check_transform(ctx, case, expect_kernel=False, updates=updates)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_random_init_draws_from_the_pcg_stream(ctx, dt):
    ns.check_random_init(ctx, dt, expect_kernel=False)


@pytest.mark.parametrize("case", ns.STOP_CASES, ids=lambda c: c.name)
def test_stopping_rule(ctx, case):
    ns.check_stopping_rule(ctx, case, expect_kernel=False)


@pytest.mark.parametrize("case", ns.FIT_CASES[2:3] + ns.FIT_CASES[-1:], ids=lambda c: c.name)
def test_same_fit_twice_and_on_a_second_handle_gives_the_same_bytes(ctx, case):
    ns.check_same_bytes_twice(ctx, case)


@pytest.mark.parametrize("case", ns.FIT_CASES[1:2] + ns.FIT_CASES[4:5] + ns.FIT_CASES[-1:], ids=lambda c: c.name)
def test_every_fit_is_the_dense_fit_bit_for_bit(ctx, case):
    ns.check_fallback_equals_dense(ctx, case)


def test_errors(ctx):
    def sharded():
        other = hostsim.context()
        hook = petal.ALLREDUCE_FN(lambda *a: 0)

        def make(data, indices, indptr, shape):
            sx = petal.CsrMatrix(data, indices, indptr, shape, ctx=other)
            other.set_collective(hook, 0, 2)
            other._keep_hook = hook
            return sx
        return other, make
    ns.check_errors(ctx, hostsim.context, sharded)
    assert ctx.workspace_in_use() == (-1, -1)                   # the host simulation keeps no count


def test_scipy_is_imported_nowhere():
    for rel in ("petal-decomposition_amd/__init__.py", "tests/nmf_sparse_cases.py", "tests/test_nmf_sparse_host.py", "tests/test_gpu_nmf_sparse.py"):
        text = open(os.path.join(ROOT, rel)).read()
        assert not re.search(r"^\s*(import|from)\s+scipy", text, flags=re.M), rel


# ------------------------------------------------------------------------------------------- 8: the header, Python, Rust, C++
def test_header_is_exported_and_bound_by_python():
    fns = kit.header_functions(HEADER)
    kit.check_python_table("petal_hip_nmf_sparse.h", fns, ENTRIES)
    kit.check_exported(fns)
    assert fns["petal_nmf_fit_csr"] == ("i32", ["ptr", "ptr", "i64", "ptr", "ptr", "ptr", "i64", "ptr", "ptr", "ptr"])
    assert fns["petal_nmf_transform_csr"] == ("i32", ["ptr", "ptr", "ptr", "ptr", "ptr"])
    assert fns["petal_nmf_sweep_csr"] == ("i32", ["ptr", "ptr", "i32", "i64", "ptr", "ptr", "ptr", "i64", "ptr", "ptr", "ptr", "ptr"])
    text = open(HEADER).read()
    assert '#include "petal_hip_nmf.h"' in text and '#include "petal_hip_sparse.h"' in text
    for word in ("Not in this version", "sharded fits", "device-resident CSR arrays", "other beta-losses", "tolerance stop in transform",
                 "k > 64", "CSR output of inverse_transform", "is never formed", "No floating-point atomics".lower(), "the same bytes",
                 "rounded once", "function of the handle alone", "duplicate pair (+3, -1)", "too large to densify",
                 "at most 64 components", "PETAL_OPT_NMF_FALLBACK", "not resident", "unmeasured"):
        assert word in text, word                                                 # the disclosures the header owes
    # the headers whose entry sets are pinned elsewhere gained nothing
    for other in ("petal_hip.h", "petal_hip_nmf.h", "petal_hip_sparse.h"):
        assert "_csr(" not in open(os.path.join(ROOT, "include", other)).read().replace("petal_rpca_fit_csr(", "").replace(
            "petal_transform_csr(", ""), other


def test_rust_binding_and_cpp_facade_match_the_header():
    assert kit.rust_functions(FFI) == kit.header_functions(HEADER)
    src = os.path.join(ROOT, "rust", "petal-decomposition-hip", "src")
    lib = open(os.path.join(src, "lib.rs")).read()
    assert "mod ffi_nmf_sparse;" in lib
    nm = open(os.path.join(src, "nmf.rs")).read()
    for name in ("petal_nmf_fit_csr", "petal_nmf_transform_csr"):
        assert f"ffi_nmf_sparse::{name}" in nm, name
    for member in ("pub fn fit_csr", "pub fn fit_transform_csr", "pub fn transform_csr"):
        assert member in nm, member
    hpp = open(os.path.join(ROOT, "include", "petal_decomposition.hpp")).read()
    assert '#include "petal_hip_nmf_sparse.h"' in hpp
    for name in ("petal_nmf_fit_csr", "petal_nmf_transform_csr"):
        assert name in hpp, name


def test_cpp_facade_on_host_simulation():
    kit.run_cpp_facade("nmf_sparse", "fallback", hostsim.build(), "hostsim")


# ------------------------------------------------------------------------------------------- kernel budgets
def test_sweep_kernel_budget(resources):
    """all 12 instantiations of the sweep (float / double values; 8, 16 or 32 lanes per gathered row; from G or from a constant), the 6
    of the split-row kernel, the 3 of the Gram kernel and k_csr_densify: no scratch, no spilled registers"""
    sweeps = {k: v for k, v in resources.items() if re.search(r"k_nmf_sweep<(float|double), (8|16|32), (true|false)>$", k)}
    splits = {k: v for k, v in resources.items() if re.search(r"k_nmf_sweep_split<(16|32|64), (true|false)>$", k)}
    grams = {k: v for k, v in resources.items() if re.search(r"k_nmf_gram<(16|32|64)>$", k)}
    dens = {k: v for k, v in resources.items() if re.search(r"k_csr_densify<(float|double)>$", k)}
    scans = {k: v for k, v in resources.items() if re.search(r"k_nmf_valscan<(float|double)>$", k)}
    assert (len(sweeps), len(splits), len(grams), len(dens), len(scans)) == (12, 6, 3, 2, 2), (sorted(sweeps), sorted(splits), sorted(grams))
    for name, r in {**sweeps, **splits, **grams, **dens, **scans}.items():
        print(name, r)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
    for name, r in {**sweeps, **splits}.items():   # S (kp^2 doubles) and four waves' z and g in LDS; four waves per SIMD or more
        assert r["max_wg"] == 256 and r["vgpr"] <= 128 and r["lds"] <= 36864, (name, r)
