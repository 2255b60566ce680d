"""Nmf (include/petal_hip_nmf.h) on the MI355X: the fused pass k_nmf_pass through petal_nmf_pass -- exact operands bit for bit over the
row-tile, workgroup, component-tile and feature-tile seams, real data against numpy.longdouble inside the model-tied bound -- and Nmf
itself: fit, fit_transform, transform and inverse_transform against the numpy model for host and device inputs in both orders, the
stopping rule, the random initialisation, the same bytes twice, the forced composed path, shapes outside the kernel's envelope, every
error."""
import numpy as np
import pytest

import header_kit as kit
import nmf_cases as nc
import petal_decomposition_amd as petal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = petal.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("inner", [1, 3])
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_pass_on_exact_operands(ctx, dt, inner):
    for shape in nc.INT_SHAPES + nc.INT_SHAPES_PERSISTENT:
        nc.check_integers_exact(ctx, shape, dt, inner, expect_kernel=True)


@pytest.mark.parametrize("form", ["device", "host-fortran"])
def test_pass_on_exact_operands_other_forms(ctx, form):
    for shape in ((17, 3, 16), (33, 17, 80), (37, 64, 512)):
        for dt in ("f32", "f64"):
            nc.check_integers_exact(ctx, shape, dt, 1, expect_kernel=True, form=form)


@pytest.mark.parametrize("case", nc.PASS_CASES, ids=lambda c: c.name)
def test_pass_against_long_double(ctx, case):
    nc.check_pass_against_long_double(ctx, case, expect_kernel=True)


@pytest.mark.parametrize("case", nc.FIT_CASES, ids=lambda c: c.name)
def test_fit_matches_the_model(ctx, case):
    nc.check_fit_against_model(ctx, case, expect_kernel=True)


@pytest.mark.parametrize("form", ["device", "host-fortran"])
@pytest.mark.parametrize("case", nc.FIT_CASES[2:3] + nc.FIT_CASES[9:10] + nc.FIT_CASES[-2:], ids=lambda c: c.name)
def test_other_input_forms(ctx, case, form):
    nc.check_fit_against_model(ctx, case, expect_kernel=True, form=form)


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("case", nc.FIT_CASES[:1] + nc.FIT_CASES[3:4] + nc.FIT_CASES[-2:], ids=lambda c: c.name)
def test_transform_matches_the_model(ctx, case, form):
    nc.check_transform(ctx, case, expect_kernel=True, form=form)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_transform_with_thirteen_updates(ctx, dt):
    n, d, k = nc.FIT_SHAPES[0]
    nc.check_transform(ctx, nc.FitCase(f"{dt}-it13", n, d, k, dt, 13, 0.0, "same", 0.0), expect_kernel=True)


@pytest.mark.parametrize("case", nc.STOP_CASES, ids=lambda c: c.name)
def test_stopping_rule(ctx, case):
    nc.check_stopping_rule(ctx, case, expect_kernel=True)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_random_init_draws_from_the_pcg_stream(ctx, dt):
    nc.check_random_init(ctx, dt, expect_kernel=True)


@pytest.mark.parametrize("case", nc.FIT_CASES[2:3] + nc.FIT_CASES[-1:], ids=lambda c: c.name)
def test_same_fit_twice_gives_the_same_bytes(ctx, case):
    nc.check_same_bytes_twice(ctx, case)


def test_same_pass_twice_gives_the_same_bytes(ctx):
    """more tiles than workgroups at the widest shape: the slabs of A are added in a fixed order"""
    x, w, h, _ = nc.int_inputs(nc.INT_N_PERSISTENT, 64, 512, "f32")
    rng = np.random.default_rng(3)
    xr, wr, hr = rng.random(x.shape).astype(np.float32), rng.random(w.shape), rng.random(h.shape)
    a = petal.nmf_pass(xr, wr, hr, l1_w=0.1, ctx=ctx)
    b = petal.nmf_pass(xr, wr, hr, l1_w=0.1, ctx=ctx)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(a, b))
    mw, ma, mb = nc.model_pass(xr, wr, hr, 0.1, 0.0, 1)
    assert max(nc.rel_max(a[0], mw), nc.rel_max(a[1], ma), nc.rel_max(a[2], mb)) <= 1e-12


@pytest.mark.parametrize("case", nc.FIT_CASES[1:2] + nc.FIT_CASES[-1:], ids=lambda c: c.name)
def test_forced_fallback_agrees_with_the_kernel(ctx, case):
    nc.check_fallback_against_kernel(ctx, case, expect_kernel=True)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("shape", nc.OUTSIDE_SHAPES, ids=str)
def test_shapes_outside_the_kernel_envelope(ctx, shape, dt):
    nc.check_outside_envelope(ctx, shape, dt)


def test_device_view_with_an_odd_pitch(ctx):
    """a torch view whose rows do not allow 16-byte loads is copied into the kernels' layout: the kernel still runs"""
    c = nc.FIT_CASES[2]
    nc.check_fit_against_model(ctx, c, expect_kernel=True, form="device-odd-pitch")


def test_option_round_trip(ctx):
    assert ctx.get_option("nmf_fallback") == 0.0
    ctx.set_option("nmf_fallback", 1)
    assert ctx.get_option(petal.OPTIONS["nmf_fallback"]) == 1.0
    ctx.set_option("nmf_fallback", 0)
    assert ctx.get_option("nmf_fallback") == 0.0


def test_errors(ctx):
    def sharded():
        other = petal.Context(0)
        other.set_collective(lambda *a: 0, 0, 2)
        return other
    nc.check_errors(ctx, sharded)


def test_cpp_facade_on_gpu():
    """tests/cpp/nmf_facade_tests.cpp against libpetal_hip.so: the C++ facade's Nmf with k_nmf_pass (the CPU suite runs the same program
    against the host simulation's composed path)"""
    kit.run_cpp_facade("nmf", "kernel", kit.HIP_LIBRARY, "hip")
