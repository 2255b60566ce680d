"""RandomizedPca on sparse CSR data (include/petal_hip_sparse.h) on a real MI355X: the sparse product bit for bit on exact-integer matrices
(both images, both types, every column count that takes another kernel form, split rows, duplicates, empty rows), every case of
tests/sparse_cases.py against the oracle with the project's parity bars on the kernel path, the sparse fit against the library's own
dense fit, determinism to the byte, the argument and error contract, and a handle that outlives 50 fits.  Run with -m gpu."""
import numpy as np
import pytest

import header_kit as kit
import sparse_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import petal_decomposition_amd as petal
    c = petal.Context(0)          # raises (no CPU fallback) when the HIP library or the GPU is missing
    yield c
    c.close()


def _same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def _case(n, d):
    return [c for c in sc.CASES if (c.n, c.d) == (n, d)][0]


# ------------------------------------------------------------------------------------------- the product, bit for bit
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", sc.INT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}-{s[2]}")
def test_product_is_exact_on_integer_matrices(ctx, shape, dt):
    info = sc.check_gemm_exact(ctx, *shape, dt)
    assert info["resident"] == 1
    assert info["items"] >= info["rows"] + 2 and info["items_transposed"] >= info["cols"] + 2     # the long row and the long column were split in three


# ------------------------------------------------------------------------------------------- parity with the oracle
@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_parity_with_the_oracle_on_the_kernel_path(ctx, case):
    sc.check_parity(ctx, case, expect_kernel=True)


@pytest.mark.parametrize("case", [_case(2000, 1000), _case(130, 257), _case(1500, 3000)], ids=sc.case_id)
def test_sparse_fit_against_the_dense_fit_of_the_library(ctx, case):
    """The same matrix densified through RandomizedPca.fit gives components and singular values within twice the bar of the sparse fit:
    a float32 case, a float64 case with n < d, a float32 case with n < d.  (Each fit is held to the bar against the oracle.  The
    1200 x 300, k = 70 case of the table is not among them: the DENSE float32 fit is 2.4e-5 off there -- a finding about the dense
    path, EXPERIMENTS.md -- while the sparse fit holds 1.9e-6.)"""
    import petal_decomposition_amd as petal
    x, (data, indices, indptr), om = sc.inputs(case)
    om = om.astype(sc.np_dtype(case))
    kw = dict(centering=case.centering, ctx=ctx, n_iter=case.n_iter, n_oversample=sc.N_OVERSAMPLE)
    dense = petal.RandomizedPca(case.k, **kw).fit(np.array(x), omega=om)
    sparse = petal.RandomizedPca(case.k, **kw).fit(sc.Duck(data, indices, indptr, x.shape), omega=om)      # duck-typed input
    assert sparse.kernel_path == 1
    rel = sc.rowwise_rel(sparse.components().astype(np.float64), dense.components().astype(np.float64)).max()
    srel = np.abs(sparse.singular_values().astype(np.float64) / dense.singular_values() - 1).max()
    print(f"{sc.case_id(case)}: sparse against dense fit: components {rel:.3e}, singular values {srel:.3e}  (bound {2 * sc.bar(case):.0e})")
    assert rel <= 2 * sc.bar(case) and srel <= 2 * sc.bar(case)
    dec = sc.decided_signs(sc.reference(case)[1], case.k, margin=min(0.5, max(1e-3, 200 * sc.bar(case))))
    sgn = np.sum(sparse.components().astype(np.float64) * dense.components(), axis=1)
    assert np.all(sgn[dec] > 0)                             # svd_flip decided alike on both paths


def test_gemm_mode_and_plane_options_do_not_reach_a_sparse_fit():
    """the fp32-MFMA GEMM mode and the two-plane / steering / fused-pass options select dense kernels; a sparse fit is the same bytes
    under all of them (its dense products are op_tall_times_small and fp64 Gram matrices: no bf16 plane, no mode)"""
    import petal_decomposition_amd as petal
    case = _case(1200, 300)                                 # l = 80: every re-basing and U well inside the split-product kernels' range
    x, (data, indices, indptr), om = sc.inputs(case)
    om = om.astype(np.float32)
    got = []
    for setup in ("default", "fp32", "options"):
        c = petal.Context(0)
        try:
            if setup == "fp32":
                c.set_gemm_mode("fp32")
            if setup == "options":
                for name in ("two_plane_operands", "steering_passes", "fused_pass"):
                    c.set_option(name, 0)
            sx = petal.CsrMatrix(data, indices, indptr, x.shape, ctx=c)
            m = petal.RandomizedPca(case.k, ctx=c, n_iter=case.n_iter)
            y = m.fit_transform(sx, omega=om)
            assert m.kernel_path == 1
            got.append((m.components(), m.singular_values(), y, m.transform(sx)))
        finally:
            c.close()
    for other in got[1:]:
        for a, b in zip(got[0], other):
            assert _same(a, b)


def test_cpp_facade_on_gpu():
    """the C++ CsrMatrix and the sparse overloads of RandomizedPca over the HIP library: resident, kernel_path == 1, close to the dense fit"""
    kit.run_cpp_facade("sparse", "kernel", kit.HIP_LIBRARY, "hip")


# ------------------------------------------------------------------------------------------- determinism
def test_runs_and_handles_give_the_same_bytes(ctx):
    import petal_decomposition_amd as petal
    case = _case(2000, 1000)
    x, (data, indices, indptr), om = sc.inputs(case)
    om = om.astype(np.float32)
    p = np.random.default_rng(3).standard_normal((x.shape[1], 74))
    pt = np.random.default_rng(4).standard_normal((x.shape[0], 74))
    mu = np.random.default_rng(5).standard_normal(x.shape[1])
    got = []
    for handle in range(2):
        sx = petal.CsrMatrix(data, indices, indptr, x.shape, ctx=ctx)
        for _ in range(2):
            m = petal.RandomizedPca(case.k, ctx=ctx, n_iter=case.n_iter)
            y = m.fit_transform(sx, omega=om)
            got.append((m.components(), m.singular_values(), m.mean(), y, m.transform(sx), petal.csr_gemm(sx, p),
                        petal.csr_gemm(sx, pt, transposed=True, a=mu, s=pt.sum(axis=0))))
        sx.close()
    for other in got[1:]:
        for a, b in zip(got[0], other):
            assert _same(a, b)


# ------------------------------------------------------------------------------------------- the contract
def _small(ctx, dt=np.float32, n=64, d=40, seed=0):
    import petal_decomposition_amd as petal
    x = sc.synth_sparse(n, d, 4, seed, du=0.2, dv=0.2).astype(dt)
    data, indices, indptr = sc.to_csr(x)
    return x, data, indices, indptr, petal.CsrMatrix(data, indices, indptr, x.shape, ctx=ctx)


@pytest.mark.parametrize("poison", [np.nan, np.inf, -np.inf])
def test_a_non_finite_value_is_a_linalg_error(ctx, poison):
    import petal_decomposition_amd as petal
    x, data, indices, indptr, _ = _small(ctx)
    data = data.copy()
    data[data.size // 2] = poison
    sx = petal.CsrMatrix(data, indices, indptr, x.shape, ctx=ctx)
    for centering in (True, False):
        with pytest.raises(petal.LinalgError, match="did not converge"):
            petal.RandomizedPca(3, centering=centering, ctx=ctx, n_iter=2).fit(sx)
    # the ctx and the handle stay usable
    assert petal.csr_gemm(sx, np.zeros((x.shape[1], 2))).shape == (x.shape[0], 2)


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_an_all_zero_matrix_is_legal(ctx, dt):
    import petal_decomposition_amd as petal
    n, d = 70, 33
    empty = petal.CsrMatrix(np.zeros(0, dtype=dt), np.zeros(0, dtype=np.int32), np.zeros(n + 1, dtype=np.int64), (n, d), ctx=ctx)
    zeros = petal.CsrMatrix(np.zeros(5, dtype=dt), np.arange(5), np.r_[0, np.full(n, 5)], (n, d), ctx=ctx)     # explicit zeros only
    for sx in (empty, zeros):
        m = petal.RandomizedPca(3, ctx=ctx, n_iter=2)
        y = m.fit_transform(sx)
        assert m.kernel_path == 1
        np.testing.assert_array_equal(m.singular_values(), 0)
        np.testing.assert_array_equal(m.mean(), 0)
        np.testing.assert_array_equal(y, 0)
        assert np.all(np.isfinite(m.components()))


def test_k_zero_and_k_full(ctx):
    import petal_decomposition_amd as petal
    x, data, indices, indptr, sx = _small(ctx, np.float64, n=30, d=12)
    m = petal.RandomizedPca(0, ctx=ctx, n_iter=2)
    y = m.fit_transform(sx)
    assert y.shape == (30, 0) and m.components().shape == (0, 12)
    np.testing.assert_allclose(m.mean(), x.mean(axis=0), rtol=0, atol=1e-14 * np.abs(x).max())
    k = 12                                              # k = min(n, d): l is clipped to it
    m = petal.RandomizedPca(k, ctx=ctx, n_iter=3)
    y = m.fit_transform(sx)
    ref = np.linalg.svd(x - x.mean(axis=0), compute_uv=False)
    assert m.kernel_path == 1 and y.shape == (30, k)
    lead = ref > 1e-6 * ref[0]
    np.testing.assert_allclose(m.singular_values()[lead], ref[lead], rtol=1e-9)
    tv = ((x - x.mean(axis=0)) ** 2).sum()
    np.testing.assert_allclose(np.sum(m.singular_values() ** 2), tv, rtol=1e-9)
    with pytest.raises(petal.InvalidInput, match="every dimension should be at least 13"):
        petal.RandomizedPca(13, ctx=ctx).fit(sx)


def test_transform_checks_the_column_count(ctx):
    import petal_decomposition_amd as petal
    x, data, indices, indptr, sx = _small(ctx)
    m = petal.RandomizedPca(3, ctx=ctx, n_iter=2).fit(sx)
    narrow = petal.CsrMatrix(*sc.to_csr(x[:, :-1]), (x.shape[0], x.shape[1] - 1), ctx=ctx)
    with pytest.raises(petal.InvalidInput, match=f"# of columns should be {x.shape[1]}"):
        m.transform(narrow)
    for member in (m.reconstruction_error, m.hotelling_t2, m.score_samples):
        with pytest.raises(petal.InvalidInput, match="not available for sparse input"):
            member(sx)
    assert m.explained_variance().shape == (3,) and m.inverse_transform(m.transform(sx)).shape == x.shape


def test_a_sharded_ctx_is_refused():
    import petal_decomposition_amd as petal
    c = petal.Context(0)
    try:
        x, data, indices, indptr, sx = _small(c)
        hook = petal.ALLREDUCE_FN(lambda *a: 0)
        c.set_collective(hook, 0, 2)
        with pytest.raises(petal.InvalidInput, match="sharded"):
            petal.RandomizedPca(3, ctx=c).fit(sx)
        with pytest.raises(petal.InvalidInput, match="sharded"):
            petal.csr_gemm(sx, np.zeros((x.shape[1], 2)))
    finally:
        c.close()


def test_a_handle_that_outlives_fifty_fits_leaks_nothing():
    """the ctx allocator's own count of blocks handed out (a ctx of its own: no other handle comes or goes): eight at the most for the
    handle, and after every fit what it was after the first two"""
    import petal_decomposition_amd as petal
    c = petal.Context(0)
    try:
        before = c.workspace_in_use()
        assert before[0] >= 0                               # the HIP layer keeps the count
        x, data, indices, indptr, sx = _small(c, n=300, d=90)
        held = c.workspace_in_use()
        assert 0 < held[0] - before[0] <= 8 and held[1] - before[1] >= 2 * (4 + data.itemsize) * data.size
        seen = []
        for i in range(52):
            m = petal.RandomizedPca(5, ctx=c, n_iter=2)
            m.fit_transform(sx)
            m.transform(sx)
            seen.append(c.workspace_in_use())
        print("blocks, bytes in use: with the handle", held, "after fits 1, 2, 3, 52", seen[0], seen[1], seen[2], seen[-1])
        assert set(seen[2:]) == {seen[1]}, seen
        sx.close()
        after = c.workspace_in_use()
        assert (after[0] - before[0], after[1] - before[1]) == (seen[1][0] - held[0], seen[1][1] - held[1])
    finally:
        c.close()
