"""IncrementalPca (include/petal_hip_ipca.h) without a GPU, on the host simulation -- whose device-op layer has no streaming kernel, so
every batch takes the two-pass path built from the library's other ops and `info` reports 0 kernel batches: exact integer Gram matrices,
the centred statistic against the long-double reference inside its model-tied bound, model parity with numpy's SVD and the library's own
Pca.fit in 1, 3 and 7 batches, the sign rule, merge and state, the argument and error contract, the inherited model members; the new
header against the built libraries, the Python table and the Rust binding; the C++ facade; the resource notes of the new kernels."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import header_kit as kit
import hostsim
import ipca_cases as ic
from header_kit import resources  # noqa: F401  (the fixture)
import petal_decomposition_amd as petal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "petal_hip_ipca.h")
FFI = os.path.join(ROOT, "rust", "petal-decomposition-hip", "src", "ffi_ipca.rs")
ENTRIES = ["petal_ipca_create", "petal_ipca_destroy", "petal_ipca_finalize", "petal_ipca_get_state", "petal_ipca_info", "petal_ipca_merge",
           "petal_ipca_partial_fit", "petal_ipca_reset", "petal_ipca_set_state"]


@pytest.fixture(scope="module")
def ctx():
    c = hostsim.context()
    yield c
    c.close()


# ------------------------------------------------------------------------------------------- 1. exact integers
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("d", ic.INT_WIDTHS)
def test_integer_gram_matrix_is_exact_after_every_batch(ctx, d, dt):
    ic.check_integers_exact(ctx, d, dt, expect_kernel=False)


# ------------------------------------------------------------------------------------------- 2. the centred statistic
@pytest.mark.parametrize("case", ic.STAT_CASES + [ic.DRIFT_CASE], ids=lambda c: c.name)
def test_centred_statistic_against_long_double(ctx, case):
    ic.check_statistic(ctx, case, expect_kernel=False)


@pytest.mark.parametrize("case", ic.STAT_CASES, ids=lambda c: c.name)
def test_fp32_accumulation_would_break_the_cap(case):
    """why s and G are accumulated in float64: the same recurrence with float32 accumulators is further from the reference than the
    cap allows on the same inputs, while the float64 model is far inside it -- the bound cannot hide a lost precision"""
    batches = ic.stat_inputs(case)
    ref = ic.reference_stat(batches)
    top = float(np.max(np.diag(ref[2])))
    e64 = float(np.max(np.abs(ic.model_stat(batches)[2].astype(np.longdouble) - ref[2]))) / top
    e32 = float(np.max(np.abs(ic.model_stat(batches, accumulate=np.float32)[2].astype(np.longdouble) - ref[2]))) / top
    print(f"{case.name}: float64 accumulation {e64:.2e}, float32 accumulation {e32:.2e} of the largest diagonal entry (cap {ic.CAP:.0e})")
    assert e32 > ic.CAP and ic.MULTIPLIER[case.family] * max(e64, ic.FLOOR_EPS * ic.EPS64) <= ic.CAP


def test_the_model_is_the_recurrence_of_the_header():
    """one batch: the model is the two-pass statistic up to rounding; centring off: the plain Gram matrix"""
    x = np.random.default_rng(5).standard_normal((40, 6)) + 2.0
    n, mean, m2 = ic.model_stat([x[:7], x[7:7], x[7:]])
    rn, rmean, rm2 = ic.reference_stat([x])
    assert n == rn == 40 and np.allclose(mean, rmean.astype(np.float64), rtol=1e-14) and np.allclose(m2, rm2.astype(np.float64), rtol=1e-13)
    assert np.array_equal(ic.model_stat([x[:9], x[9:]], centering=False)[2], x[:9].T @ x[:9] + x[9:].T @ x[9:])


# ------------------------------------------------------------------------------------------- 3, 4. model parity and the sign rule
@pytest.mark.parametrize("centering", [True, False], ids=["centred", "uncentred"])
@pytest.mark.parametrize("case", ic.PARITY_CASES, ids=ic.parity_id)
def test_parity_in_one_three_and_seven_batches(ctx, case, centering):
    ic.check_parity(ctx, case, centering, expect_kernel=False)


def test_sign_rule_ties_go_to_the_lowest_index(ctx):
    """two columns that are exact copies: the components' two largest entries tie exactly, and the lower index decides"""
    rng = np.random.default_rng(9)
    f = rng.standard_normal((200, 1)) * 10.0
    x = np.concatenate([-f, -f, 0.1 * rng.standard_normal((200, 3))], axis=1)
    comp = petal.IncrementalPca(1, ctx=ctx).partial_fit(x[:90]).partial_fit(x[90:]).components()
    assert abs(comp[0, 0]) == abs(comp[0, 1]) > 0.7 and comp[0, 0] > 0


# ------------------------------------------------------------------------------------------- 5. merge and state
@pytest.mark.parametrize("case", ic.PARITY_CASES[:2], ids=ic.parity_id)
def test_merge_and_state(ctx, case):
    ic.check_merge_and_state(ctx, case, expect_kernel=False)


# ------------------------------------------------------------------------------------------- 6. the contract
def _raw(ctx, d, dt=petal.PETAL_F64, centering=1):
    h = C.c_void_p()
    rc = ctx.lib.petal_ipca_create(ctx._h, d, dt, centering, C.byref(h))
    return rc, h, (ctx.lib.petal_last_error(ctx._h) or b"").decode()


def test_contract_on_the_host_simulation(ctx):
    x = np.random.default_rng(3).standard_normal((64, 10)) + 1.0
    m = petal.IncrementalPca(3, ctx=ctx)
    assert m.n_samples_seen == 0 and m.components().shape == (3, 0)              # unfitted: the empty model of an unfitted Pca
    m.partial_fit(x[:0])                                                         # a 0-row batch opens the handle and is a no-op
    assert m.info() == {"d": 10, "dtype": petal.PETAL_F64, "centering": 1, "n_samples_seen": 0, "batches": 0, "kernel_batches": 0, "merges": 0}
    with pytest.raises(petal.InvalidInput, match="no rows have been seen"):
        m.finalize()
    assert m.components().shape == (3, 0)
    m.partial_fit(x[:40]).partial_fit(x[40:40]).partial_fit(x[40:])
    assert m.n_samples_seen == 64 and m.info()["batches"] == 2 and m.n_samples == 64
    with pytest.raises(petal.InvalidInput, match="# of columns should be 10"):
        m.partial_fit(x[:, :9])
    with pytest.raises(petal.InvalidInput, match="dtype differs"):
        m.partial_fit(x.astype(np.float32))
    with pytest.raises(petal.InvalidInput, match="every dimension should be at least 11"):
        m.finalize(11)
    with pytest.raises(petal.InvalidInput, match="negative parameter"):
        m.finalize(-1)
    few = petal.IncrementalPca(5, ctx=ctx).partial_fit(x[:4])
    with pytest.raises(petal.InvalidInput, match="every dimension should be at least 5"):   # rows seen below k
        few.components()
    comp, means, sing, tv = m.finalize(0)                                        # k = 0: the means and the total variance alone
    assert comp.shape == (0, 10) and sing.shape == (0,) and np.allclose(means, x.mean(axis=0)) and tv[0] > 0
    full = m.finalize(10)                                                        # k = d
    assert np.allclose(np.sum(full[2] ** 2), tv[0], rtol=1e-12)
    # a NaN or an infinity poisons the statistic; reset clears it
    good = m.finalize()
    for poison in (np.nan, np.inf):
        bad = x[:8].copy()
        bad[3, 2] = poison
        m.partial_fit(bad)
        with pytest.raises(petal.LinalgError, match="did not converge"):
            m.components()
        with pytest.raises(petal.LinalgError, match="did not converge"):
            m.finalize()
        m.reset()
        assert m.n_samples_seen == 0 and m.info()["batches"] == 0 and m.components().shape == (3, 0)
        m.partial_fit(x[:40]).partial_fit(x[40:])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(m.finalize(), good))
    # reset keeps the handle's d and dtype: a float32 model comes back float32
    x32 = x.astype(np.float32)
    m32 = petal.IncrementalPca(3, ctx=ctx).partial_fit(x32)
    first32 = m32.finalize()
    m32.reset().partial_fit(x32)
    assert m32.components().dtype == np.float32 and all(a.tobytes() == b.tobytes() for a, b in zip(m32.finalize(), first32))
    assert np.allclose(m32.singular_values(), petal.Pca(3, ctx=ctx).fit(x32).singular_values(), rtol=1e-5)
    # fit() starts afresh and loops partial_fit over row slices
    assert m.fit(x, batch_size=25).info()["batches"] == 3 and m.n_samples_seen == 64
    assert m.fit(x).info()["batches"] == 2                                        # default: 5 d rows a batch
    # merge: the handles must agree
    for other in (petal.IncrementalPca(3, centering=False, ctx=ctx).partial_fit(x), petal.IncrementalPca(3, ctx=ctx).partial_fit(x[:, :9]),
                  petal.IncrementalPca(3, ctx=ctx).partial_fit(x.astype(np.float32))):
        with pytest.raises(petal.InvalidInput, match="differ in d, dtype or centering"):
            m.merge(other)
    with pytest.raises(petal.InvalidInput, match="into itself"):
        m.merge(m)
    # set_state validates n; n == 0 ignores the rest
    st = m.state()
    for n in (-1.0, 2.5, np.nan):
        with pytest.raises(petal.InvalidInput, match="non-negative whole number"):
            petal.IncrementalPca.from_state({**st, "n": n}, 3, ctx=ctx)
    assert petal.IncrementalPca.from_state({**st, "n": 0.0}, 3, ctx=ctx).n_samples_seen == 0
    # the C entries: bad arguments
    rc, h, msg = _raw(ctx, -1)
    assert rc == petal.PETAL_INVALID_INPUT and not h and "negative shape" in msg
    rc, h, msg = _raw(ctx, 4, dt=7)
    assert rc == petal.PETAL_INVALID_INPUT and "unsupported dtype" in msg
    assert ctx.lib.petal_ipca_info(None, (C.c_int64 * 8)()) == petal.PETAL_INVALID_INPUT
    assert ctx.lib.petal_ipca_reset(None) == petal.PETAL_INVALID_INPUT
    ctx.lib.petal_ipca_destroy(None)
    # the forced-fallback option is a ctx option like the others
    ctx.set_option("ipca_fallback", 1)
    assert ctx.get_option("ipca_fallback") == 1.0
    ctx.set_option("ipca_fallback", 0)
    assert petal.OPTIONS["ipca_fallback"] == 32                                   # apart from petal_hip.h's 0 .. 15 ...
    with pytest.raises(petal.InvalidInput):
        ctx.set_option(16, 1)                                                    # ... whose next number stays unknown
    # another ctx, and a sharded one
    other = hostsim.context()
    try:
        theirs = petal.IncrementalPca(3, ctx=other).partial_fit(x)
        with pytest.raises(petal.InvalidInput, match="another ctx"):
            m.merge(theirs)
        hook = petal.ALLREDUCE_FN(lambda *a: 0)
        other.set_collective(hook, 0, 2)
        with pytest.raises(petal.InvalidInput, match="sharded"):
            theirs.partial_fit(x)
        with pytest.raises(petal.InvalidInput, match="sharded"):
            theirs.finalize()
        with pytest.raises(petal.InvalidInput, match="sharded"):
            petal.IncrementalPca(3, ctx=other).partial_fit(x)
    finally:
        other.close()
    with pytest.raises(petal.InvalidInput, match="ctx was closed"):
        theirs.info()                                                            # a ctx takes its statistics with it


# ------------------------------------------------------------------------------------------- 7. the inherited members
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_model_members_match_pca_fit_on_the_concatenation(ctx, dt):
    case = ic.PARITY_CASES[0] if dt == np.float64 else ic.PARITY_CASES[1]
    x = np.array(ic.parity_inputs(case))
    tol = ic.bar(case)
    whole = petal.Pca(case.k, ctx=ctx).fit(x)
    m = petal.IncrementalPca(case.k, ctx=ctx)
    for a, b in ic.cut(case.n, ic.unequal(case.n, 3, 1)):
        m.partial_fit(x[a:b])
    assert m.n_samples == whole.n_samples == case.n and m.n_components() == case.k
    assert np.allclose(m.explained_variance(), whole.explained_variance(), rtol=2 * tol, atol=0)
    assert np.allclose(m.explained_variance_ratio(), whole.explained_variance_ratio(), rtol=4 * tol, atol=0)
    assert np.isclose(m.noise_variance(), whole.noise_variance(), rtol=1e-4 if dt == np.float32 else 1e-8)
    sg = np.sign(np.sum(m.components().astype(np.float64) * whole.components(), axis=1))
    y, yw = m.transform(x), whole.transform(x)
    assert y.dtype == dt and np.abs(y * sg - yw).max() <= 20 * tol * np.abs(yw).max()
    back = m.inverse_transform(y)
    assert np.abs(back - whole.inverse_transform(yw)).max() <= 20 * tol * np.abs(x).max()
    # the host simulation has no row-score kernel: the members refuse here exactly as Pca's do (the GPU suite compares their values)
    for member in ("reconstruction_error", "hotelling_t2", "score_samples"):
        with pytest.raises(petal.InvalidInput, match="row scores not available"):
            getattr(m, member)(x[:8])
        with pytest.raises(petal.InvalidInput, match="row scores not available"):
            getattr(whole, member)(x[:8])
    # JSON: the reference's serde form, readable as a Pca
    loaded = petal.Pca.from_json(m.to_json(), dtype=dt, ctx=ctx)
    assert loaded.components().tobytes() == m.components().tobytes() and loaded.n_samples == case.n
    assert loaded.transform(x).tobytes() == y.tobytes()
    # a later batch refreshes the model
    before = m.singular_values().copy()
    m.partial_fit(x[:50])
    assert m.n_samples == case.n + 50 and not np.array_equal(m.singular_values(), before)


# ------------------------------------------------------------------------------------------- 8. the header, Python, Rust, C++
def _header_functions():
    return kit.header_functions(HEADER, prefix="petal_ipca_", drop=(r"typedef struct petal_ipca petal_ipca;",))


def test_header_is_exported_and_bound_by_python():
    fns = _header_functions()
    kit.check_python_table("petal_hip_ipca.h", fns, ENTRIES)
    kit.check_exported(fns)
    assert fns["petal_ipca_create"] == ("i32", ["ptr", "i64", "i32", "i32", "ptr"])
    assert fns["petal_ipca_finalize"] == ("i32", ["ptr", "ptr", "i64", "ptr", "ptr", "ptr", "ptr"])
    assert fns["petal_ipca_set_state"] == ("i32", ["ptr", "ptr", "f64", "ptr", "ptr"]) and fns["petal_ipca_destroy"] == ("void", ["ptr"])
    text = open(HEADER).read()
    assert '#include "petal_hip.h"' in text
    assert int(re.search(r"#define\s+PETAL_IPCA_KERNEL_MAX_D\s+(\d+)", text).group(1)) == petal.IPCA_KERNEL_MAX_D
    assert int(re.search(r"#define\s+PETAL_OPT_IPCA_FALLBACK\s+(\d+)", text).group(1)) == petal.OPTIONS["ipca_fallback"]
    for word in ("largest magnitude", "Cancellation", "sharded contexts", "forgetting factors", "sparse batches"):
        assert word in text, word                                                 # the disclosures the header owes


def test_rust_binding_matches_the_header():
    text = re.sub(r"//.*$", "", open(FFI).read(), flags=re.M)
    assert kit.rust_functions(FFI) == _header_functions()
    assert int(re.search(r"PETAL_IPCA_KERNEL_MAX_D:\s*i64\s*=\s*(\d+)", text).group(1)) == petal.IPCA_KERNEL_MAX_D
    assert int(re.search(r"PETAL_OPT_IPCA_FALLBACK:\s*c_int\s*=\s*(\d+)", text).group(1)) == petal.OPTIONS["ipca_fallback"]
    src = os.path.join(ROOT, "rust", "petal-decomposition-hip", "src")
    lib = open(os.path.join(src, "lib.rs")).read()
    assert "mod ffi_ipca;" in lib and "IncrementalPca" in lib
    pca = open(os.path.join(src, "pca.rs")).read()
    for name in ENTRIES:
        assert f"ffi_ipca::{name}" in pca, name
    assert "pub struct IncrementalPca" in pca
    for name in ("partial_fit", "merge", "reset", "state", "set_state", "model", "n_samples_seen"):
        assert re.search(rf"impl<A: HipScalar> IncrementalPca<A> \{{.*pub fn {name}\b", pca, flags=re.S), name


def test_cpp_facade_on_host_simulation():
    kit.run_cpp_facade("ipca", "fallback", hostsim.build(), "hostsim")


# ------------------------------------------------------------------------------------------- 9. kernel budgets
@pytest.mark.parametrize("t", ["float", "double"])
def test_gram_stream_budget(resources, t):
    """no scratch, no spills, and not fewer waves per SIMD than k_atb_f64 on the same data type gets in the same build"""
    atb = min(v["waves_per_simd"] for k, v in resources.items() if re.search(rf"k_atb_f64<{t}, (true|false), (true|false), 4>$", k))
    hits = {k: v for k, v in resources.items() if re.search(rf"k_gram_stream<{t}, (true|false)>$", k)}
    assert len(hits) == 2, sorted(hits)
    for name, r in hits.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["lds"] == 0, (name, r)
        assert r["waves_per_simd"] >= atb and r["max_wg"] == 256, (name, r, atb)


def test_merge_kernel_budget(resources):
    r = resources["petal::k_ipca_merge"]
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
    assert r["lds"] == (2 * 16 + 8 * 32 + 4 * 256) * 8 and r["max_wg"] == 1024 and r["vgpr"] <= 64      # a 1024-thread workgroup: 16 waves a CU and room for two
