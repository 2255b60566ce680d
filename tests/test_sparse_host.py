"""RandomizedPca on sparse CSR data (include/petal_hip_sparse.h) without a GPU: the numpy model of the pipeline inside the bars; every
validation message of petal_csr_create; the stable counting sort and the work items; the entries on the host simulation -- whose
device-op layer has no sparse product, so the handle keeps its host arrays, the fit and the transform densify and say so, and
petal_csr_gemm is a plain host loop -- against the oracle, against petal_rpca_fit on the densified matrix bit for bit, and their
argument contract; the new header against the built libraries, the Python table and the Rust binding; the C++ facade; the resource
notes of the new kernels."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import header_kit as kit
import hostsim
import sparse_cases as sc
from header_kit import resources  # noqa: F401  (the fixture)
import petal_decomposition_amd as petal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "petal_hip_sparse.h")
FFI = os.path.join(ROOT, "rust", "petal-decomposition-hip", "src", "ffi_sparse.rs")
ENTRIES = ["petal_csr_create", "petal_csr_destroy", "petal_csr_gemm", "petal_csr_image", "petal_csr_info", "petal_ctx_workspace_in_use",
           "petal_rpca_fit_csr", "petal_transform_csr"]


@pytest.fixture(scope="module")
def ctx():
    c = hostsim.context()
    yield c
    c.close()


# ------------------------------------------------------------------------------------------- the generator and the model
@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_generator_and_model_stay_inside_the_bar(case):
    """the inputs are sparse and wide in spectrum, and the pipeline the library runs -- restated in numpy with the data's storage type
    and fp64 accumulation -- sits a decade or more inside the bar on every case: the bar tests the kernels, not the algorithm"""
    x, (data, indices, indptr), _ = sc.inputs(case)
    o, _, _ = sc.reference(case)
    density = data.size / x.size
    comp, sing = sc.model_errors(case)
    print(f"{sc.case_id(case)}: density {density:.3f}  sigma_1 / sigma_k {o.singular[0] / o.singular[-1]:.0f}  model: components {comp:.2e}, "
          f"singular values {sing:.2e}  (bar {sc.bar(case):.0e})")
    ratio = o.singular[0] / o.singular[-1]
    if (case.du, case.dv) == (0.05, 0.05) and case.n * case.d >= 10 ** 6:     # the generator's defaults at a size where the draws average out
        assert 0.03 <= density <= 0.07 and 4e2 <= ratio <= 6e2
    else:                                                           # 33410 entries with k = 4, or thinner factors / k = 70: per case
        lo, hi, rlo, rhi = {(257, 130): (0.025, 0.035, 2e2, 3e2), (130, 257): (0.025, 0.035, 80, 1.2e2), (1500, 3000): (0.03, 0.05, 6e2, 9e2),
                            (1200, 300): (0.05, 0.07, 8e2, 1.2e3)}[(case.n, case.d)]
        assert lo <= density <= hi and rlo <= ratio <= rhi
    assert comp <= 0.2 * sc.bar(case) and sing <= 0.1 * sc.bar(case)


def test_fp32_accumulation_would_leave_no_room():
    """why the kernel accumulates in fp64: the same model with fp32 accumulation is far further from the oracle (1.8e-6 against 5e-8)"""
    c = sc.CASES[0]
    x, _, om = sc.inputs(c)
    o, _, _ = sc.reference(c)
    e64 = sc.rowwise_rel(sc.model_fit(x, om, c.k, c.n_iter, c.centering, np.float32)[0], o.components).max()
    e32 = sc.rowwise_rel(sc.model_fit(x, om, c.k, c.n_iter, c.centering, np.float32, accumulate=np.float32)[0], o.components).max()
    print(f"fp32 storage: fp64 accumulation {e64:.2e}, fp32 accumulation {e32:.2e}")
    assert e64 < e32 and e64 <= 1e-6


def test_the_table_reaches_every_path():
    assert {c.dt for c in sc.CASES} == {"f32", "f64"} and {c.centering for c in sc.CASES} == {True, False}
    assert any(c.n < c.d for c in sc.CASES) and any(c.n_iter == 0 for c in sc.CASES)
    assert any(c.k + sc.N_OVERSAMPLE > 64 for c in sc.CASES)          # column panels
    assert {(c.k + sc.N_OVERSAMPLE + 15) // 16 for c in sc.CASES} >= {1, 2, 5}


# ------------------------------------------------------------------------------------------- petal_csr_create's checks
def _create(ctx, rows, cols, indptr, indices, data):
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int32)
    data = np.asarray(data, dtype=np.float64)
    h = C.c_void_p()
    rc = ctx.lib.petal_csr_create(ctx._h, rows, cols, data.size, indptr.ctypes.data_as(petal._L), indices.ctypes.data_as(petal._I32),
                                  data.ctypes.data, petal.PETAL_F64, C.byref(h))
    msg = (ctx.lib.petal_last_error(ctx._h) or b"").decode()
    if h:
        ctx.lib.petal_csr_destroy(h)
    return rc, msg


def test_every_violation_names_its_position(ctx):
    ok = dict(rows=3, cols=4, indptr=[0, 2, 2, 5], indices=[3, 0, 1, 1, 2], data=[1, 2, 3, 4, 5])
    assert _create(ctx, **ok) == (petal.PETAL_OK, "")
    rc, msg = _create(ctx, **{**ok, "indptr": [1, 2, 2, 5]})
    assert rc == petal.PETAL_INVALID_INPUT and msg == "indptr[0] should be 0 (it is 1)"
    rc, msg = _create(ctx, **{**ok, "indptr": [0, 3, 2, 5]})
    assert rc == petal.PETAL_INVALID_INPUT and msg == "indptr should not decrease: indptr[2] = 2 is below indptr[1] = 3"
    rc, msg = _create(ctx, **{**ok, "indptr": [0, 2, 2, 4]})
    assert rc == petal.PETAL_INVALID_INPUT and msg == "indptr[3] should be the number of nonzeros 5 (it is 4)"
    rc, msg = _create(ctx, **{**ok, "indices": [3, 0, -1, 1, 2]})
    assert rc == petal.PETAL_INVALID_INPUT and msg == "indices[2] = -1 is outside [0, 4)"
    rc, msg = _create(ctx, **{**ok, "indices": [3, 0, 1, 4, 7]})
    assert rc == petal.PETAL_INVALID_INPUT and msg == "indices[3] = 4 is outside [0, 4)"          # the FIRST offender
    with pytest.raises(petal.InvalidInput, match=r"indices\[3\] = 4 is outside"):
        petal.CsrMatrix([1, 2, 3, 4, 5.0], [3, 0, 1, 4, 7], [0, 2, 2, 5], (3, 4), ctx=ctx)
    with pytest.raises(petal.InvalidInput, match="indptr should have 4 entries"):
        petal.CsrMatrix([1.0], [0], [0, 1], (3, 4), ctx=ctx)
    with pytest.raises(petal.InvalidInput, match="too many rows/columns"):
        petal.CsrMatrix([1.0], [0], [0, 1], (1, 2 ** 31), ctx=ctx)
    with pytest.raises(petal.InvalidInput, match="does not fit 32 bits"):
        petal.CsrMatrix([1.0], [2 ** 31], [0, 1], (1, 5), ctx=ctx)
    m = petal.CsrMatrix([1, 2], np.array([1, 0], dtype=np.int64), np.array([0, 2], dtype=np.int32), (1, 2), ctx=ctx)   # index types are converted
    assert m.dtype == np.float64 and m.info()["nnz"] == 2


# ------------------------------------------------------------------------------------------- the images and the work items
@pytest.mark.parametrize("shape", sc.INT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}-{s[2]}")
def test_counting_sort_is_stable_and_items_cover_every_nonzero_once(ctx, shape):
    data, indices, indptr, (n, d) = sc.int_matrix(*shape[:2], seed=3, long_by=shape[2])
    tagged = np.arange(data.size, dtype=np.float64)                 # every stored entry carries its own position
    sx = petal.CsrMatrix(tagged, indices, indptr, (n, d), ctx=ctx)
    info = sx.info()
    assert info["resident"] == 0 and info["item_nnz"] == sc.ITEM_NNZ == 256
    ptr0, idx0, val0, items0 = sx.image(False)
    np.testing.assert_array_equal(ptr0, indptr)
    np.testing.assert_array_equal(idx0, indices)
    np.testing.assert_array_equal(val0, tagged)
    ptr1, idx1, val1, items1 = sx.image(True)
    rows_of = np.repeat(np.arange(n), np.diff(indptr))
    np.testing.assert_array_equal(np.diff(ptr1), np.bincount(indices, minlength=d))
    pos = val1.astype(np.int64)                                     # where each entry of the transposed image came from
    assert sorted(pos.tolist()) == list(range(data.size))
    np.testing.assert_array_equal(idx1, rows_of[pos])
    for j in range(d):
        seg = slice(ptr1[j], ptr1[j + 1])
        assert np.all(indices[pos[seg]] == j)
        assert np.all(np.diff(idx1[seg]) >= 0)                      # rows ascending inside the column ...
        assert np.all(np.diff(pos[seg]) > 0)                        # ... and duplicates in their original order: the sort is stable
    for ptr, items, rows in ((ptr0, items0, n), (ptr1, items1, d)):
        assert np.all(items[:, 2] - items[:, 1] <= sc.ITEM_NNZ) and np.all(items[:, 2] >= items[:, 1])
        assert np.all(np.diff(items[:, 0]) >= 0) and set(items[:, 0].tolist()) == set(range(rows))     # every row, empty ones too, in order
        covered = np.concatenate([np.arange(a, b) for _, a, b in items])
        np.testing.assert_array_equal(covered, np.arange(data.size))                                   # once each, in position order
        for r, a, b in items:
            assert ptr[r] <= a and b <= ptr[r + 1]
        long = int(np.argmax(np.diff(ptr)))
        assert np.diff(ptr)[long] == 2 * sc.ITEM_NNZ + 3
        np.testing.assert_array_equal(items[items[:, 0] == long][:, 2] - items[items[:, 0] == long][:, 1], [256, 256, 3])
    sx.close()


# ------------------------------------------------------------------------------------------- the entries on the host simulation
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", sc.INT_SHAPES[:3], ids=lambda s: f"{s[0]}x{s[1]}-{s[2]}")
def test_product_on_the_host_loop_is_exact(ctx, shape, dt):
    info = sc.check_gemm_exact(ctx, *shape, dt, widths=(1, 17, 80))
    assert info["resident"] == 0


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_fall_back_meets_the_bars_and_says_it_ran(ctx, case):
    sc.check_parity(ctx, case, expect_kernel=False)


@pytest.mark.parametrize("case", [sc.CASES[3], sc.CASES[4]], ids=sc.case_id)
def test_fall_back_equals_the_dense_entry_bit_for_bit(ctx, case):
    x, (data, indices, indptr), om = sc.inputs(case)
    om = om.astype(sc.np_dtype(case))
    perm = np.concatenate([np.arange(a, b)[::-1] for a, b in zip(indptr[:-1], indptr[1:])])          # unsorted rows, same matrix
    duck = sc.Duck(data[perm], indices[perm], indptr, x.shape)
    kw = dict(centering=case.centering, ctx=ctx, n_iter=case.n_iter, n_oversample=sc.N_OVERSAMPLE)
    dense, sparse = petal.RandomizedPca(case.k, **kw), petal.RandomizedPca(case.k, **kw)
    yd = dense.fit_transform(sc.densify(data, indices, indptr, x.shape), omega=om)
    ys = sparse.fit_transform(duck, omega=om)                       # duck-typed: .data / .indices / .indptr / .shape, no scipy
    assert sparse.kernel_path == 0 and dense.kernel_path is None
    for a, b in ((yd, ys), (dense.components(), sparse.components()), (dense.singular_values(), sparse.singular_values()),
                 (dense.mean(), sparse.mean()), (dense.explained_variance_ratio(), sparse.explained_variance_ratio()),
                 (dense.transform(np.array(x)), sparse.transform(duck))):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert sparse.noise_variance() == dense.noise_variance() and sparse.n_samples == x.shape[0]


def _small(ctx, dt=np.float32, n=64, d=40):
    x = sc.synth_sparse(n, d, 4, 0, du=0.2, dv=0.2).astype(dt)
    data, indices, indptr = sc.to_csr(x)
    return x, data, indices, indptr, petal.CsrMatrix(data, indices, indptr, x.shape, ctx=ctx)


def test_contract_on_the_host_simulation(ctx):
    x, data, indices, indptr, sx = _small(ctx)
    for poison in (np.nan, np.inf):
        bad = data.copy()
        bad[5] = poison
        with pytest.raises(petal.LinalgError, match="did not converge"):
            petal.RandomizedPca(3, ctx=ctx, n_iter=2).fit(petal.CsrMatrix(bad, indices, indptr, x.shape, ctx=ctx))
    zero = petal.CsrMatrix(np.zeros(0, dtype=np.float32), [], np.zeros(65, dtype=np.int64), (64, 40), ctx=ctx)
    m = petal.RandomizedPca(3, ctx=ctx, n_iter=2)
    y = m.fit_transform(zero)
    np.testing.assert_array_equal(m.singular_values(), 0)
    np.testing.assert_array_equal(y, 0)
    m0 = petal.RandomizedPca(0, ctx=ctx)
    assert m0.fit_transform(sx).shape == (64, 0) and m0.kernel_path == 0
    mk = petal.RandomizedPca(40, ctx=ctx, n_iter=2).fit(sx)                                          # k = min(n, d)
    assert mk.components().shape == (40, 40)
    with pytest.raises(petal.InvalidInput, match="every dimension should be at least 41"):
        petal.RandomizedPca(41, ctx=ctx).fit(sx)
    m = petal.RandomizedPca(3, ctx=ctx, n_iter=2).fit(sx)
    narrow = petal.CsrMatrix(*sc.to_csr(x[:, :-1]), (64, 39), ctx=ctx)
    with pytest.raises(petal.InvalidInput, match="# of columns should be 40"):
        m.transform(narrow)
    for member in (m.reconstruction_error, m.hotelling_t2, m.score_samples):
        with pytest.raises(petal.InvalidInput, match="not available for sparse input"):
            member(sx)
    assert m.explained_variance().shape == (3,) and m.inverse_transform(m.transform(sx)).shape == x.shape
    assert ctx.workspace_in_use() == (-1, -1)                       # the host simulation keeps no count
    other = hostsim.context()
    try:
        with pytest.raises(petal.InvalidInput, match="another ctx"):
            petal.RandomizedPca(3, ctx=other).fit(sx)
        hook = petal.ALLREDUCE_FN(lambda *a: 0)
        sharded = petal.CsrMatrix(data, indices, indptr, x.shape, ctx=other)
        other.set_collective(hook, 0, 2)
        with pytest.raises(petal.InvalidInput, match="sharded"):
            petal.RandomizedPca(3, ctx=other).fit(sharded)
        with pytest.raises(petal.InvalidInput, match="sharded"):
            petal.csr_gemm(sharded, np.zeros((40, 2)))
    finally:
        other.close()
    with pytest.raises(petal.InvalidInput, match="was closed"):
        sharded.info()                                              # a ctx takes its sparse matrices with it


def test_scipy_is_imported_nowhere():
    for rel in ("petal-decomposition_amd/__init__.py", "tests/sparse_cases.py", "tests/test_sparse_host.py", "tests/test_gpu_sparse.py"):
        text = open(os.path.join(ROOT, rel)).read()
        assert not re.search(r"^\s*(import|from)\s+scipy", text, flags=re.M), rel


# ------------------------------------------------------------------------------------------- the header, Python, Rust, C++
def _header_functions():
    return kit.header_functions(HEADER, drop=(r"typedef struct petal_csr petal_csr;",))


def test_header_is_exported_and_bound_by_python():
    fns = _header_functions()
    kit.check_python_table("petal_hip_sparse.h", fns, ENTRIES)
    kit.check_exported(fns, want_hip=True)
    assert fns["petal_rpca_fit_csr"] == ("i32", ["ptr", "ptr", "i64", "i64", "i64", "i32"] + ["ptr"] * 7)
    assert fns["petal_csr_create"] == ("i32", ["ptr", "i64", "i64", "i64", "ptr", "ptr", "ptr", "i32", "ptr"])
    text = open(HEADER).read()
    assert '#include "petal_hip.h"' in text
    assert int(re.search(r"#define\s+PETAL_CSR_ITEM_NNZ\s+(\d+)", text).group(1)) == petal.CSR_ITEM_NNZ


def test_rust_binding_matches_the_header():
    text = re.sub(r"//.*$", "", open(FFI).read(), flags=re.M)
    assert kit.rust_functions(FFI) == _header_functions()
    assert int(re.search(r"PETAL_CSR_ITEM_NNZ:\s*i64\s*=\s*(\d+)", text).group(1)) == petal.CSR_ITEM_NNZ
    src = os.path.join(ROOT, "rust", "petal-decomposition-hip", "src")
    lib = open(os.path.join(src, "lib.rs")).read()
    assert "mod ffi_sparse;" in lib and "CsrMatrix" in lib
    pca = open(os.path.join(src, "pca.rs")).read()
    for name in ("petal_csr_create", "petal_csr_destroy", "petal_csr_info", "petal_rpca_fit_csr", "petal_transform_csr"):
        assert f"ffi_sparse::{name}" in pca
    assert "pub struct CsrMatrix" in pca
    for name in ("fit_csr", "fit_transform_csr", "transform_csr"):
        assert re.search(rf"impl<A: HipScalar, R: Rng> RandomizedPca<A, R> \{{.*pub fn {name}\b", pca, flags=re.S), name


def test_cpp_facade_on_host_simulation():
    kit.run_cpp_facade("sparse", "fallback", hostsim.build(), "hostsim")


# ------------------------------------------------------------------------------------------- kernel budgets
SPMM_KERNELS = [("float", g) for g in (4, 8, 16, 32)] + [("double", g) for g in (8, 16, 32)]


@pytest.mark.parametrize("t,g", SPMM_KERNELS, ids=[f"{t}-{g}" for t, g in SPMM_KERNELS])
def test_product_kernel_budget(resources, t, g):
    """no scratch, no spill, no LDS; registers for at least 16 waves a CU (four a SIMD) with four gathered rows in flight per sub-group"""
    r = resources[f"void petal::k_spmm<{t}, {g}>"]
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
    assert r["lds"] == 0 and r["waves_per_simd"] >= 4 and r["max_wg"] == 256


@pytest.mark.parametrize("name", ["k_spmm_combine<float>", "k_spmm_combine<double>", "k_csr_rowstats<float>", "k_csr_rowstats<double>"])
def test_side_kernel_budget(resources, name):
    r = resources[f"void petal::{name}"]
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["lds"] == 0, r


@pytest.mark.parametrize("t", ["float", "double"])
def test_tall_times_small_budget(resources, t):
    r = resources[f"void petal::k_tall_small<{t}>"]
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
    assert r["lds"] == 32 * 64 * 8 and r["waves_per_simd"] >= 4


def test_the_fit_uses_no_mode_dependent_product():
    """between its weak defaults and the end of the file algo.cpp's sparse part calls neither op_gemm_xp nor the non-precise op_gemm_atb"""
    text = open(os.path.join(ROOT, "petal-decomposition_amd", "csrc", "algo.cpp")).read()
    part = text[text.index("struct CsrRun"):text.index("void transform_csr(")]
    assert "op_gemm_xp" not in re.sub(r"//.*", "", part)
    assert all("/*precise=*/true" in line for line in part.splitlines() if "op_gemm_atb(" in line)
