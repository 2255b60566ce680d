"""Nmf with the Kullback-Leibler loss on sparse CSR data (include/petal_hip_nmf_kl.h) without a GPU, on the host simulation -- whose
device-op layer has neither the sparse product nor the sweep, so a handle is not resident and the driver runs over the plain host loop
of the statement (kernel_path 0; there is no densifying path for this loss): the sweep on exact operands and against long double with
its cap, the fits, transform, the stopping rule, the random initialisation, dense input, every error; the new header against the built
libraries, the Python table, the Rust binding and the C++ facade; the register / scratch budget of the kernels in the built library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import header_kit as kit
import hostsim
import nmf_kl_cases as kc
from header_kit import resources  # noqa: F401  (the fixture)
import petal_decomposition_amd as petal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "petal_hip_nmf_kl.h")
FFI = os.path.join(ROOT, "rust", "petal-decomposition-hip", "src", "ffi_nmf_kl.rs")
ENTRIES = ["petal_nmf_fit_csr_loss", "petal_nmf_get_loss", "petal_nmf_kl_sweep_csr"]


@pytest.fixture(scope="module")
def ctx():
    c = hostsim.context()
    yield c
    c.close()


# ------------------------------------------------------------------------------------------- 1, 2: petal_nmf_kl_sweep_csr
def test_the_model_is_the_dense_statement():
    """the CSR model equals the dense statement W <- W o ((X / (W H)) H^T) / (rowsum H + l1 + l2 W) on a matrix without duplicates"""
    c = kc.SWEEP_CASES[1]
    triple, x, g, f = kc.sweep_inputs(c.n, c.d, c.k, c.dt, False)
    xd = x.astype(np.float64)
    wh = g @ f.T
    wh[wh < kc.EPS] = kc.EPS
    want = g * (((xd / wh) @ f) / (f.sum(axis=0) + 0.25 + 0.5 * g))
    got = kc.model_kl_sweep(kc.image_of(triple, x.shape, False), g, f, 0.25, 0.5, 1)[0]
    assert kc.rel_max(got, want) <= 1e-13
    m = xd > kc.EPS
    term = kc.model_kl_sweep(kc.image_of(triple, x.shape, False), g, f, inner=0)[2]
    assert abs(term - (xd[m] * np.log(xd[m] / wh[m])).sum()) <= 1e-12 * np.abs(xd[m] * np.log(xd[m] / wh[m])).sum()


def test_split_rows_occur_where_the_tests_say():
    assert kc.split_rows(-1, False) and not kc.split_rows(-1, True)          # the seam matrix: split rows, and an image without any
    assert kc.split_rows(0, False) and kc.split_rows(0, True)
    assert set(kc.ns.SEAM_COUNTS) <= kc.ns.row_counts_seen()


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_sweep_on_exact_operands(ctx, dt):
    for which in range(-1, len(kc.INT_SHAPES)):
        kc.check_sweep_exact(ctx, which, dt, expect_kernel=False, ks=(1, 3, 17, 64))


@pytest.mark.parametrize("which", [-1, 0], ids=["seams", "257x130-dup"])
def test_inner_updates_are_chained_single_updates(ctx, which):
    kc.check_inner_is_chained_single_updates(ctx, which, "f64", expect_kernel=False)


@pytest.mark.parametrize("case", kc.SWEEP_CASES, ids=lambda c: c.name)
def test_sweep_against_long_double(ctx, case):
    kc.check_sweep_against_long_double(ctx, case, expect_kernel=False)


# ------------------------------------------------------------------------------------------- 3 .. 6: fits on the host loop
@pytest.mark.parametrize("case", kc.FIT_CASES[::3] + kc.FIT_CASES[-2:], ids=lambda c: c.name)
def test_fit_matches_the_model(ctx, case):
    kc.check_fit_against_model(ctx, case, expect_kernel=False)


def test_duck_typed_csr_is_accepted(ctx):
    kc.check_fit_against_model(ctx, kc.FIT_CASES[1], expect_kernel=False, duck=True)


@pytest.mark.parametrize("updates", [13, 200])
@pytest.mark.parametrize("case", kc.FIT_CASES[:1] + kc.FIT_CASES[-1:], ids=lambda c: c.name)
def test_transform_matches_the_model(ctx, case, updates):
    kc.check_transform(ctx, case, expect_kernel=False, updates=updates)


@pytest.mark.parametrize("case", kc.STOP_CASES, ids=lambda c: c.name)
def test_stopping_rule(ctx, case):
    kc.check_stopping_rule(ctx, case, expect_kernel=False)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_random_init_draws_from_the_pcg_stream(ctx, dt):
    kc.check_random_init(ctx, dt, expect_kernel=False)


@pytest.mark.parametrize("case", kc.FIT_CASES[2:3] + kc.FIT_CASES[-1:], ids=lambda c: c.name)
def test_same_fit_twice_and_on_a_second_handle_gives_the_same_bytes(ctx, case):
    kc.check_same_bytes_twice(ctx, case)


@pytest.mark.parametrize("case", kc.FIT_CASES[1:2] + kc.FIT_CASES[-1:], ids=lambda c: c.name)
def test_dense_input_is_the_csr_of_its_nonzeros(ctx, case):
    kc.check_dense_input_is_the_csr_of_its_nonzeros(ctx, case, expect_kernel=False)


@pytest.mark.parametrize("case", kc.FIT_CASES[1:2] + kc.FIT_CASES[-1:], ids=lambda c: c.name)
def test_explicit_frobenius_changes_nothing(ctx, case):
    kc.check_explicit_frobenius_changes_nothing(ctx, case)


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
    kc.check_errors(ctx, hostsim.context, sharded)


def test_scipy_and_sklearn_are_imported_nowhere():
    for rel in ("tests/nmf_kl_cases.py", "tests/test_nmf_kl_host.py", "tests/test_gpu_nmf_kl.py"):
        text = open(os.path.join(ROOT, rel)).read()
        assert not re.search(r"^\s*(import|from)\s+(scipy|sklearn)", text, flags=re.M), rel


# ------------------------------------------------------------------------------------------- 9: the header, Python, Rust, C++
def test_header_is_exported_and_bound_by_python():
    fns = kit.header_functions(HEADER)
    kit.check_python_table("petal_hip_nmf_kl.h", fns, ENTRIES)
    kit.check_exported(fns)
    assert fns["petal_nmf_fit_csr_loss"] == ("i32", ["ptr", "ptr", "i64", "ptr", "i64", "ptr", "ptr", "i64", "ptr", "ptr", "ptr"])
    assert fns["petal_nmf_get_loss"] == ("i32", ["ptr", "ptr"])
    assert fns["petal_nmf_kl_sweep_csr"] == ("i32", ["ptr", "ptr", "i32", "i64", "ptr", "ptr", "ptr", "i64", "ptr", "ptr", "ptr", "ptr"])
    text = open(HEADER).read()
    assert '#include "petal_hip_nmf_sparse.h"' in text
    for name, value in (("PETAL_NMF_LOSS_FROBENIUS", petal.NMF_LOSS_FROBENIUS), ("PETAL_NMF_LOSS_KL", petal.NMF_LOSS_KL)):
        assert int(re.search(rf"#define\s+{name}\s+(\d+)", text).group(1)) == value
    for word in ("Not in this version", "sharded fits", "k > 64", "fused dense Kullback-Leibler kernel", "other beta",
                 "loss term fused into the column sweep", "one-launch multi-update transform", "no floating-point atomics",
                 "the same bytes", "rounded once", "work items and the padding alone", "duplicate pair (+3, -1)", "act as their sum",
                 "v log v by itself", "at most 64 components", "PETAL_OPT_NMF_FALLBACK", "not resident", "no densifying path",
                 "unmeasured", "An explicit zero contributes nothing", "an empty row gives a zero row"):
        assert word in text, word                                                 # the disclosures the header owes
    # the existing signatures stay as they are: the spec has no loss field
    assert C.sizeof(petal.petal_nmf_spec) == 48


def test_rust_binding_and_cpp_facade_match_the_header():
    text = re.sub(r"//.*$", "", open(FFI).read(), flags=re.M)
    assert kit.rust_functions(FFI) == kit.header_functions(HEADER)
    for name, value in (("PETAL_NMF_LOSS_FROBENIUS", 0), ("PETAL_NMF_LOSS_KL", 1)):
        assert int(re.search(rf"{name}:\s*i64\s*=\s*(\d+)", text).group(1)) == value
    src = os.path.join(ROOT, "rust", "petal-decomposition-hip", "src")
    lib = open(os.path.join(src, "lib.rs")).read()
    assert "mod ffi_nmf_kl;" in lib and "NmfLoss" in lib
    nm = open(os.path.join(src, "nmf.rs")).read()
    for name in ("petal_nmf_fit_csr_loss", "petal_nmf_get_loss"):
        assert f"ffi_nmf_kl::{name}" in nm, name
    assert "pub enum NmfLoss" in nm
    hpp = open(os.path.join(ROOT, "include", "petal_decomposition.hpp")).read()
    assert '#include "petal_hip_nmf_kl.h"' in hpp and "enum class NmfLoss" in hpp
    for name in ("petal_nmf_fit_csr_loss", "petal_nmf_get_loss"):
        assert name in hpp, name


def test_cpp_facade_on_host_simulation():
    kit.run_cpp_facade("nmf_kl", "host", hostsim.build(), "hostsim")


# ------------------------------------------------------------------------------------------- kernel budgets
def test_sweep_kernel_budget(resources):
    """all 12 instantiations of the sweep (float / double values; 8, 16 or 32 lanes per gathered row; from G or from a constant), the 6
    of the split-row kernel, the 3 of the column-sum kernel and k_nmf_kl_vsum: no scratch, no spilled registers, no LDS in the sweep"""
    sweeps = {k: v for k, v in resources.items() if re.search(r"k_nmf_kl_sweep<(float|double), (8|16|32), (true|false)>$", k)}
    splits = {k: v for k, v in resources.items() if re.search(r"k_nmf_kl_split<(16|32|64), (true|false)>$", k)}
    sums = {k: v for k, v in resources.items() if re.search(r"k_nmf_kl_colsum<(16|32|64)>$", k)}
    vsums = {k: v for k, v in resources.items() if re.search(r"k_nmf_kl_vsum<(float|double)>$", k)}
    assert (len(sweeps), len(splits), len(sums), len(vsums)) == (12, 6, 3, 2), (sorted(sweeps), sorted(splits), sorted(sums), sorted(vsums))
    for name, r in {**sweeps, **splits, **sums, **vsums}.items():
        print(name, r)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
    for name, r in sweeps.items():                  # the rule runs in registers: four waves per SIMD or more, no LDS
        assert r["max_wg"] == 256 and r["vgpr"] <= 128 and r["lds"] == 0, (name, r)
