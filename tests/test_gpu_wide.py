"""Exact Pca on wide data (include/petal_hip_wide.h) on the MI355X: k_row_gram through petal_row_gram -- exact integers bit for bit over
the tile and chunk seams and every input form, real data against numpy.longdouble inside the model-tied bound, the same bytes twice --
and the dual route of Pca.fit reached at small d through pca_dual = 1: oracle parity, dual against primal, the auto rule, k = n,
non-finite input, the forced fallback, the transform round trip, and a 256 x 60000 fit the primal route could not hold."""
import numpy as np
import pytest

import header_kit as kit
import wide_cases as wc
import petal_decomposition_amd as petal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = petal.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("form", wc.FORMS)
def test_integer_row_gram_is_exact(ctx, dt, form):
    for n in wc.INT_N:
        for d in wc.INT_D:
            chunks = wc.check_integers_exact(ctx, n, d, dt, form, expect_kernel=True)
            assert chunks >= (3 if d == 4099 else 1)
        d = wc.INT_D_RAGGED[dt]
        chunks = wc.check_integers_exact(ctx, n, d, dt, form, expect_kernel=True)
        dp = (d + 15) // 16 * 16
        assert chunks >= 3 and dp % chunks != 0, (d, chunks)          # not all chunks alike: a ragged last one


@pytest.mark.parametrize("case", wc.GRAM_CASES, ids=lambda c: c.name)
def test_row_gram_against_long_double(ctx, case):
    wc.check_gram_against_long_double(ctx, case, expect_kernel=True)


@pytest.mark.parametrize("case", wc.GRAM_CASES[2:4], ids=lambda c: c.name)
def test_same_call_twice_gives_the_same_bytes(ctx, case):
    wc.check_same_bytes_twice(ctx, case)


@pytest.mark.parametrize("case", wc.FIT_CASES, ids=lambda c: c.name)
def test_dual_fit_matches_the_oracle(ctx, case):
    wc.check_fit_parity(ctx, case, expect_kernel=True)


def test_dual_fit_of_a_device_tensor(ctx):
    import torch
    c = wc.FIT_CASES[2]
    ctx.set_option("pca_dual", 1)
    try:
        m = petal.Pca(c.k, ctx=ctx)
        y = m.fit_transform(torch.from_numpy(np.array(wc.fit_inputs(c))).cuda())
        assert m.last_route()["kernel"] == 1
    finally:
        ctx.set_option("pca_dual", 0)
    wc.compare_with_oracle(c, m.components(), m.singular_values(), m.mean(), wc.total_variance_of(m), y.cpu().numpy(), wc.tol_of(c))


@pytest.mark.parametrize("case", wc.FIT_CASES[:4], ids=lambda c: c.name)
def test_dual_against_primal_on_one_ctx(ctx, case):
    wc.check_dual_against_primal(ctx, case)


@pytest.mark.parametrize("shape,route", wc.AUTO_RULE, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_auto_rule(ctx, shape, route):
    wc.check_auto_rule(ctx, shape, route)


def test_sharded_ctx_keeps_the_primal_route():
    other = petal.Context(0)
    try:
        other.set_collective(lambda *a: 0, 0, 2)
        m = petal.Pca.new(2, other).fit(wc.sharded_rule_input())
        assert m.last_route() == {"route": 0, "kernel": 0, "order": 2064, "chunks": 0}
    finally:
        other.close()


def test_k_equals_n_centred_ends_in_a_zero_row(ctx):
    wc.check_k_equals_n(ctx, expect_kernel=True)


def test_non_finite_input_does_not_converge(ctx):
    wc.check_non_finite_raises(ctx)


@pytest.mark.parametrize("case", wc.FIT_CASES[:4], ids=lambda c: c.name)
def test_forced_fallback_agrees_with_the_kernel(ctx, case):
    wc.check_fallback_equivalence(ctx, case)


def test_transform_round_trip_of_a_dual_fitted_model(ctx):
    wc.check_round_trip(ctx, expect_kernel=True)


def test_wide_fit_the_primal_route_could_not_hold(ctx):
    """256 x 60000 float32 at the default options: the auto rule takes the dual route (the primal one would need 2 x 28.8 GB and an
    eigenproblem of order 60000) and the model meets 2e-5 against numpy's thin float64 SVD"""
    n, d, k = 256, 60000, 8
    rng = np.random.default_rng(2024)
    s = 10.0 * 0.7 ** np.arange(k)
    x = ((rng.standard_normal((n, k)) * s) @ rng.standard_normal((k, d)) + 0.01 * rng.standard_normal((n, d)) + rng.standard_normal(d)).astype(np.float32)
    assert ctx.get_option("pca_dual") == 0.0
    m = petal.Pca.new(k, ctx).fit(x)
    r = m.last_route()
    assert r["route"] == 1 and r["kernel"] == 1 and r["order"] == n and r["chunks"] >= 3, r
    x64 = x.astype(np.float64)
    mu = x64.mean(axis=0)
    _, sv, vt = np.linalg.svd(x64 - mu, full_matrices=False)
    rel = wc.rowwise_rel(m.components().astype(np.float64), vt[:k])
    assert rel.max() <= 2e-5, rel.max()
    assert np.allclose(m.singular_values(), sv[:k], rtol=2e-5)
    assert np.allclose(m.mean(), mu, rtol=2e-5, atol=2e-5 * np.abs(mu).max())
    assert np.isclose(wc.total_variance_of(m), float(sv @ sv), rtol=2e-4)


def test_cpp_facade_on_gpu():
    """tests/cpp/wide_facade_tests.cpp against libpetal_hip.so: the dual route of the C++ facade's Pca with k_row_gram (the CPU suite runs
    the same program against the host simulation's fallback)"""
    kit.run_cpp_facade("wide", "kernel", kit.HIP_LIBRARY, "hip")
