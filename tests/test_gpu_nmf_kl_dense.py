"""Nmf with the Kullback-Leibler loss on dense data (include/petal_hip_nmf_kl_dense.h) on the MI355X: the fused pass k_nmf_kl_pass
through petal_nmf_kl_pass -- exact operands bit for bit over the row-tile, workgroup, component-tile and feature-tile seams (the split of
the H side at 64 padded components and more than 256 padded columns among them), real data against numpy.longdouble inside the
model-tied bound -- and Nmf(dense_path="fused") itself: fit, fit_transform and transform against the numpy model and against the CSR
route, the stopping rule, the random initialisation, the same bytes twice, the forced composed path, shapes outside the kernel's
envelope, device tensors, what did not move, every error."""

import pytest

import header_kit as kit
import nmf_kl_dense_cases as dc
import petal_decomposition_amd as petal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = petal.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_pass_on_exact_operands(ctx, dt):
    for shape in dc.INT_SHAPES + dc.INT_SHAPES_PERSISTENT:
        dc.check_integers_exact(ctx, shape, dt, expect_kernel=True)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_pass_on_a_device_view_with_a_row_pitch_above_d(ctx, dt):
    """taken zero-copy with its pitch; NaN behind every row"""
    for shape in ((17, 3, 16), (33, 17, 80), (37, 64, 512), (37, 64, 272)):
        dc.check_integers_exact(ctx, shape, dt, expect_kernel=True, pitch=True)
    assert ctx.stats()["x_zero_copy"] == 1


@pytest.mark.parametrize("case", dc.PASS_CASES, ids=lambda c: c.name)
def test_pass_against_long_double(ctx, case):
    dc.check_pass_against_long_double(ctx, case, expect_kernel=True)


@pytest.mark.parametrize("case", dc.FIT_CASES, ids=lambda c: c.name)
def test_fit_matches_the_model_and_the_csr_route(ctx, case):
    m = dc.check_fit_against_model(ctx, case, expect_kernel=True)
    assert m.kernel_path == (0 if case.fit.k == 33 else 1)     # k = 33 pads to 48 components: the composed path


@pytest.mark.parametrize("updates", [13, 200])
@pytest.mark.parametrize("case", dc.FIT_CASES[:1] + dc.FIT_CASES[11:12] + dc.FIT_CASES[-1:], ids=lambda c: c.name)
def test_transform_matches_the_model(ctx, case, updates):
    dc.check_transform(ctx, case, expect_kernel=True, updates=updates)


@pytest.mark.parametrize("case", dc.kc.STOP_CASES, ids=lambda c: c.name)
def test_stopping_rule(ctx, case):
    dc.check_stopping_rule(ctx, case, expect_kernel=True)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_random_init_draws_from_the_pcg_stream(ctx, dt):
    dc.check_random_init(ctx, dt, expect_kernel=True)


@pytest.mark.parametrize("case", dc.FIT_CASES[2:3] + dc.FIT_CASES[-1:], ids=lambda c: c.name)
def test_same_fit_twice_gives_the_same_bytes(ctx, case):
    dc.check_same_bytes_twice(ctx, case)


def test_same_pass_twice_gives_the_same_bytes(ctx):
    """more tiles than workgroups at the widest shape (the split H side): the slabs are added in a fixed order"""
    import numpy as np
    rng = np.random.default_rng(3)
    n = dc.nc.INT_N_PERSISTENT
    xr, wr, hr = rng.random((n, 512)).astype(np.float32), rng.random((n, 64)) + 0.05, rng.random((64, 512)) + 0.05
    a = petal.nmf_kl_pass(xr, wr, hr, l1_w=0.1, ctx=ctx)
    b = petal.nmf_kl_pass(xr, wr, hr, l1_w=0.1, ctx=ctx)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(a, b))
    mw, ma, mc, _ = dc.model_pass(xr, wr, hr, 0.1, 0.0, 1)
    assert max(dc.rel_max(a[0], mw), dc.rel_max(a[1], ma), dc.rel_max(a[2], mc)) <= 1e-12


@pytest.mark.parametrize("case", dc.FIT_CASES[1:2] + dc.FIT_CASES[17:18], ids=lambda c: c.name)
def test_forced_fallback_agrees_with_the_kernel(ctx, case):
    dc.check_fallback_against_kernel(ctx, case, expect_kernel=True)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("shape", dc.OUTSIDE_SHAPES, ids=str)
def test_shapes_outside_the_kernel_envelope(ctx, shape, dt):
    dc.check_outside_envelope(ctx, shape, dt)


@pytest.mark.parametrize("case", dc.FIT_CASES[3:4] + dc.FIT_CASES[16:17], ids=lambda c: c.name)
def test_device_input_stays_on_the_device(ctx, case):
    dc.check_device_input_stays_on_the_device(ctx, case)


@pytest.mark.parametrize("case", dc.FIT_CASES[1:2] + dc.FIT_CASES[10:11], ids=lambda c: c.name)
def test_nothing_existing_moved(ctx, case):
    dc.check_nothing_existing_moved(ctx, case)


def test_errors(ctx):
    def sharded():
        other = petal.Context(0)
        other.set_collective(lambda *a: 0, 0, 2)
        return other
    dc.check_errors(ctx, lambda: petal.Context(0), sharded)


def test_cpp_facade_on_gpu():
    """tests/cpp/nmf_kl_dense_facade_tests.cpp against libpetal_hip.so: the C++ facade's Nmf<A>::dense_path with k_nmf_kl_pass (the CPU
    suite runs the same program against the host simulation's composed path)"""
    kit.run_cpp_facade("nmf_kl_dense", "kernel", kit.HIP_LIBRARY, "hip")
