"""KernelPca (include/petal_hip_kpca.h) on the MI355X: the fused pass k_kapply through petal_kernel_apply -- exact integers bit for bit
over the tile, query-block and column-panel seams and every input form, the exact rbf diagonal, real data against numpy.longdouble
inside the model-tied bound, the same bytes twice -- and KernelPca itself: fit, fit_transform and transform against the numpy model for
all five kernels, the linear kernel against Pca, k = n, device and odd-pitch inputs, a model that outlives its input, the forced
fallback, every error."""
import numpy as np
import pytest

import header_kit as kit
import kpca_cases as kc
import petal_decomposition_amd as petal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = petal.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("form", kc.FORMS)
def test_integer_kernel_apply_is_exact(ctx, dt, form):
    for shape in kc.INT_SHAPES:
        kc.check_integers_exact(ctx, shape, dt, form, expect_kernel=True)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("form", kc.FORMS)
def test_rbf_diagonal_is_exactly_one(ctx, dt, form):
    for (n, d) in ((1, 1), (17, 3), (33, 19), (129, 67), (257, 1000)):
        kc.check_rbf_diagonal_is_one(ctx, n, d, dt, form, expect_kernel=True)


@pytest.mark.parametrize("case", kc.APPLY_CASES, ids=lambda c: c.name)
def test_kernel_apply_against_long_double(ctx, case):
    kc.check_apply_against_long_double(ctx, case, expect_kernel=True)


@pytest.mark.parametrize("case", kc.APPLY_CASES[-6:], ids=lambda c: c.name)
def test_same_call_twice_gives_the_same_bytes(ctx, case):
    kc.check_same_bytes_twice(ctx, case)


@pytest.mark.parametrize("case", kc.FIT_CASES, ids=lambda c: c.name)
def test_fit_matches_the_model(ctx, case):
    kc.check_model_is_well_posed(case)
    kc.check_fit_against_model(ctx, case, expect_kernel=True)


@pytest.mark.parametrize("case", kc.FIT_CASES, ids=lambda c: c.name)
def test_transform_of_new_rows_matches_the_model(ctx, case):
    kc.check_transform_new_rows(ctx, case, expect_kernel=True)


@pytest.mark.parametrize("form", ["device", "device-odd-pitch"])
@pytest.mark.parametrize("case", kc.FIT_CASES[12:18] + kc.FIT_CASES[26:28], ids=lambda c: c.name)
def test_device_inputs(ctx, case, form):
    kc.check_fit_against_model(ctx, case, expect_kernel=True, form=form)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_linear_kernel_is_pca(ctx, dt):
    for (n, d) in kc.FIT_SHAPES:
        kc.check_linear_equals_pca(ctx, n, d, dt)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_k_equals_n_ends_in_a_zero_column(ctx, dt):
    kc.check_k_equals_n(ctx, dt)


@pytest.mark.parametrize("kernel", ["rbf", "cosine"])
def test_model_outlives_its_input(ctx, kernel):
    """fit on a zero-copy torch tensor (128 float32 columns, contiguous), overwrite the tensor in place: transform still matches"""
    import torch
    n, d = 100, 128
    x = kc.fit_inputs(n, d, "f32")
    xq = kc.new_rows(50, d, "f32")
    t = torch.from_numpy(np.array(x)).cuda()
    m = petal.KernelPca(kc.FIT_K, kernel, ctx=ctx).fit(t)
    assert ctx.stats()["x_zero_copy"] == 1
    before = m.transform(xq)
    t.fill_(float("nan"))
    torch.cuda.synchronize()
    after = m.transform(xq)
    assert np.isfinite(after).all() and after.tobytes() == before.tobytes()
    mo = kc.model_fit_of(x, kc.Spec(kernel))
    yo = kc.model_transform(mo, x, xq, kc.FIT_K)
    s = np.sign(np.sum(after.astype(np.float64) * yo, axis=0))
    assert kc.scores_rel(after * s, yo, mo.lam, n).max() <= kc.tol_of("f32")


@pytest.mark.parametrize("case", kc.FIT_CASES[12:24], ids=lambda c: c.name)
def test_forced_fallback_agrees_with_the_kernel(ctx, case):
    kc.check_fallback_against_kernel(ctx, case, expect_kernel=True)


def test_errors(ctx):
    def sharded():
        other = petal.Context(0)
        other.set_collective(lambda *a: 0, 0, 2)
        return other
    kc.check_errors(ctx, sharded)


def test_wide_a_and_many_rows(ctx):
    """more than one column panel and more than one workgroup per panel at once, against float64 numpy (a loose, scale-tied check of
    the indexing; the exact and the long-double tests carry the accuracy)"""
    rng = np.random.default_rng(11)
    xq, xt = rng.standard_normal((1000, 40)).astype(np.float32), rng.standard_normal((300, 40)).astype(np.float32)
    a = rng.standard_normal((300, 150))
    out, info = petal.kernel_apply(xq, xt, a, "rbf", gamma=0.05, ctx=ctx, want_info=True)
    assert info["kernel"] == 1
    k = kc.kernel_matrix(kc.Spec("rbf", 0.05), xq, xt, None, np.float64)
    assert np.abs(out - k @ a).max() <= 1e-12 * (np.abs(k) @ np.abs(a)).max()


def test_cpp_facade_on_gpu():
    """tests/cpp/kpca_facade_tests.cpp against libpetal_hip.so: the C++ facade's KernelPca with k_kmap and k_kapply (the CPU suite runs
    the same program against the host simulation's fallback)"""
    kit.run_cpp_facade("kpca", "kernel", kit.HIP_LIBRARY, "hip")
