"""Nmf with the coordinate-descent solver on sparse CSR data (include/petal_hip_nmf_cd_sparse.h) without a GPU, on the host simulation
-- whose device-op layer has no sparse kernels: the handle is not resident, every fit and transform densifies (kernel_path 0, bit for
bit the dense solver="cd") and the sweep probe runs the plain host loop (kernel 0).  The probe on exact operands and against long
double, the fits against the model, transform, the stopping rule, the random initialisation, what did not move, every error; the new
header against the built libraries, the Python table, the Rust binding and the C++ facade; the register / scratch budget of the kernels
in the built library."""
import ctypes as C
import os
import re

import pytest

import header_kit as kit
import hostsim
import nmf_cd_sparse_cases as cs
from header_kit import resources  # noqa: F401  (the fixture)
import petal_decomposition_amd as petal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "petal_hip_nmf_cd_sparse.h")
FFI = os.path.join(ROOT, "rust", "petal-decomposition-hip", "src", "ffi_nmf_cd_sparse.rs")
ENTRIES = ["petal_nmf_cd_sweep_csr", "petal_nmf_fit_csr_solver", "petal_nmf_transform_csr_solver"]


@pytest.fixture(scope="module")
def ctx():
    c = hostsim.context()
    yield c
    c.close()


# ------------------------------------------------------------------------------------------- 1, 2: petal_nmf_cd_sweep_csr
@pytest.mark.parametrize("which", cs.INT_WHICH)
def test_sweep_on_exact_operands(ctx, which):
    for dt in ("f32", "f64"):
        cs.check_cd_sweep_exact(ctx, cs.int_case(which), which, dt, expect_kernel=False)


def test_sweep_on_tiny_matrices(ctx):
    for rows in cs.TINY_ROWS:
        for dt in ("f32", "f64"):
            cs.check_cd_sweep_exact(ctx, cs.tiny_case(rows), 100 + rows, dt, expect_kernel=False)


@pytest.mark.parametrize("case", cs.SWEEP_CASES, ids=lambda c: c.name)
def test_sweep_against_long_double(ctx, case):
    cs.check_sweep_against_long_double(ctx, case, expect_kernel=False)


def test_sweep_seeds_are_the_search_on_the_reference_alone():
    assert all(cs.reference_margin(c, cs.SWEEP_SEEDS.get(c.name, 0))[0] >= cs.MARGIN for c in cs.SWEEP_CASES)
    assert set(cs.SWEEP_SEEDS) <= {c.name for c in cs.SWEEP_CASES}


# ------------------------------------------------------------------------------------------- 3: fits and transforms
@pytest.mark.parametrize("case", cs.FIT_CASES[:6] + cs.FIT_CASES[12:15] + cs.FIT_CASES[-2:], ids=lambda c: c.name)
def test_fit_matches_the_model(ctx, case):
    cs.check_fit_against_model(ctx, case, expect_kernel=False)


def test_duck_input_takes_the_same_path(ctx):
    cs.check_fit_against_model(ctx, cs.FIT_CASES[4], expect_kernel=False, duck=True)


@pytest.mark.parametrize("updates", [3, 200])
@pytest.mark.parametrize("case", cs.FIT_CASES[2:3] + cs.FIT_CASES[-1:], ids=lambda c: c.name)
def test_transform_matches_the_model(ctx, case, updates):
    cs.check_transform(ctx, case, expect_kernel=False, updates=updates)


# ------------------------------------------------------------------------------------------- 4: the stopping rule
@pytest.mark.parametrize("case", cs.STOP_CASES, ids=lambda c: c.name)
def test_stopping_rule(ctx, case):
    cs.check_stopping_rule(ctx, case, expect_kernel=False)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_zero_violation_stops_at_iteration_one(ctx, dt):
    cs.check_zero_violation_stops_at_once(ctx, dt, expect_kernel=False)


# ------------------------------------------------------------------------------------------- 5, 6: random init, determinism, paths
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_random_init_draws_from_the_pcg_stream(ctx, dt):
    cs.check_random_init(ctx, dt, expect_kernel=False)


def test_same_fit_twice_gives_the_same_bytes(ctx):
    cs.check_same_bytes_twice(ctx, cs.FIT_CASES[7])


@pytest.mark.parametrize("case", cs.FIT_CASES[1:2] + cs.FIT_CASES[-1:], ids=lambda c: c.name)
def test_every_fit_of_this_layer_is_the_dense_fit(ctx, case):
    cs.check_fallback_equals_dense(ctx, case)


def test_more_than_64_components_densify(ctx):
    cs.check_fallback_equals_dense(ctx, cs.FitCase("f64-260x300-k65", 260, 300, 65, "f64", 2, 0.0, "same", 0.0))


@pytest.mark.parametrize("case", cs.FIT_CASES[1:2] + cs.FIT_CASES[-1:], ids=lambda c: c.name)
def test_nothing_existing_moved(ctx, case):
    cs.check_nothing_existing_moved(ctx, case)


# ------------------------------------------------------------------------------------------- 7: errors
def test_errors(ctx):
    def sharded():
        other = hostsim.context()

        def make(data, indices, indptr, shape):
            sx = petal.CsrMatrix(data, indices, indptr, shape, ctx=other)
            other.set_collective(lambda *a: 0, 0, 2)
            return sx
        return other, make
    cs.check_errors(ctx, hostsim.context, sharded).close()


def test_dense_image_beyond_the_limit_is_refused(ctx):
    cs.check_too_large_to_densify(ctx)


def test_scipy_and_sklearn_are_imported_nowhere():
    for rel in ("tests/nmf_cd_sparse_cases.py", "tests/test_gpu_nmf_cd_sparse.py", "dev/nmf_cd_sparse_bench.py"):
        text = open(os.path.join(ROOT, rel)).read()
        assert not re.search(r"^\s*(import|from)\s+(scipy|sklearn)", text, flags=re.M), rel


# ------------------------------------------------------------------------------------------- 8: the header, Python, Rust, C++
def test_header_is_exported_and_bound_by_python():
    fns = kit.header_functions(HEADER)
    kit.check_python_table("petal_hip_nmf_cd_sparse.h", fns, ENTRIES)
    kit.check_exported(fns)
    assert fns["petal_nmf_fit_csr_solver"] == ("i32", ["ptr", "ptr", "i64", "ptr", "i64", "ptr", "ptr", "i64", "ptr", "ptr", "ptr"])
    assert fns["petal_nmf_transform_csr_solver"] == ("i32", ["ptr", "ptr", "ptr", "ptr", "ptr"])
    assert fns["petal_nmf_cd_sweep_csr"] == ("i32", ["ptr", "ptr", "i32", "i64", "ptr", "ptr", "ptr", "i64", "i32", "ptr", "ptr", "ptr", "ptr", "ptr"])
    text = open(HEADER).read()
    assert '#include "petal_hip_nmf_cd.h"' in text and '#include "petal_hip_nmf_sparse.h"' in text
    for word in ("val[t] * F[idx[t], :]", "the CURRENT g_r", "min(0, grad)", "max(g_r[t] - grad / S[t][t], 0)", "l2 on the first k diagonal entries only",
                 "A row with no stored entries is still swept", "Padded components stay zero", "from_zero starts G at", "the NEW W",
                 "No shuffling", "violation / violation_init <= tol", "tol = 0 runs exactly max_iter iterations", "bit for bit",
                 "avg = sqrt(sum(X) / (n d) / k)", "inner = max_iter", "no tolerance stop", "widened to float64 on load",
                 "no floating-point atomics", "the sum of the violations", "the same bytes", "a second handle", "rounded once",
                 "to rounding, not to the byte", "k <= 64", "not resident", "PETAL_OPT_NMF_FALLBACK", "too large to densify", "kernel_path",
                 "two doubles back", "without a host round trip", "a duplicate pair", "negative values in data", "cross terms", "unmeasured",
                 "unknown solver", "nmf_cd_sweep wrote outside the R x k block", "a plain host loop", "a sharded ctx", "Not in this version",
                 "shuffle=True", "sharded fits"):
        assert word in text, word                                                 # the disclosures the header owes
    assert C.sizeof(petal.petal_nmf_spec) == 48
    assert "petal_hip_nmf_cd_sparse.h" in open(os.path.join(ROOT, "include", "petal_hip_nmf_cd.h")).read()   # the first header points here


def test_rust_binding_and_cpp_facade_match_the_header():
    assert kit.rust_functions(FFI) == kit.header_functions(HEADER)
    src = os.path.join(ROOT, "rust", "petal-decomposition-hip", "src")
    lib = open(os.path.join(src, "lib.rs")).read()
    assert "mod ffi_nmf_cd_sparse;" in lib and "NmfSparsePath" in lib
    nm = open(os.path.join(src, "nmf.rs")).read()
    for name in ("petal_nmf_fit_csr_solver", "petal_nmf_transform_csr_solver"):
        assert f"ffi_nmf_cd_sparse::{name}" in nm, name
    assert "pub enum NmfSparsePath" in nm and "pub sparse_path: NmfSparsePath" in nm
    hpp = open(os.path.join(ROOT, "include", "petal_decomposition.hpp")).read()
    assert '#include "petal_hip_nmf_cd_sparse.h"' in hpp and "enum class NmfSparsePath" in hpp and "Sweep" in hpp
    for name in ("petal_nmf_fit_csr_solver", "petal_nmf_transform_csr_solver"):
        assert name in hpp, name


def test_cpp_facade_on_host_simulation():
    kit.run_cpp_facade("nmf_cd_sparse", "host", hostsim.build(), "hostsim")


# ------------------------------------------------------------------------------------------- 9: kernel budgets
def test_kernel_budget(resources):
    """all 12 instantiations of the sweep (float / double; 8, 16 or 32 lanes per gathered row; from G or from zero), the 6 of the split
    kernel (16, 32 or 64 padded components; from G or from zero) and the 3 of the reduction: no scratch, no spilled register, 256
    threads"""
    sweeps = {k: v for k, v in resources.items() if re.search(r"k_nmf_cd_sweep<(float|double), (8|16|32), (true|false)>$", k)}
    splits = {k: v for k, v in resources.items() if re.search(r"k_nmf_cd_sweep_split<(16|32|64), (true|false)>$", k)}
    grams = {k: v for k, v in resources.items() if re.search(r"k_nmf_cd_gram<(16|32|64)>$", k)}
    assert (len(sweeps), len(splits), len(grams)) == (12, 6, 3), (sorted(sweeps), sorted(splits), sorted(grams))
    for name, r in {**sweeps, **splits, **grams}.items():
        print(name, r)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["max_wg"] == 256, (name, r)
    # the multiplicative path's kernels are the ones they were: the same instantiations, none with scratch
    old = {k: v for k, v in resources.items() if re.search(r"k_nmf_sweep<(float|double), (8|16|32), (true|false)>$", k) or
           re.search(r"k_nmf_gram<(16|32|64)>$", k)}
    assert len(old) == 15 and all(r["scratch"] == 0 and r["vgpr_spill"] == 0 for r in old.values()), sorted(old)
