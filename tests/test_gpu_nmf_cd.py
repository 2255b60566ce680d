"""Nmf with the coordinate-descent solver (include/petal_hip_nmf_cd.h) on the MI355X: the fused pass k_nmf_cd_pass through
petal_nmf_cd_pass and the H side k_nmf_cd_hrule through petal_nmf_cd_hupdate -- exact operands bit for bit over the row-tile, workgroup,
component-tile and feature-tile seams, real data against numpy.longdouble inside the model-tied bound -- and Nmf(solver="cd") itself:
fit, fit_transform, transform and inverse_transform against the numpy model, the stopping rule, the random initialisation, the same
bytes twice, the forced composed path, shapes outside the kernel's envelope, what did not move, every error."""

import numpy as np
import pytest

import header_kit as kit
import nmf_cd_cases as cc
import petal_decomposition_amd as petal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = petal.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_pass_on_exact_operands(ctx, dt):
    for shape in cc.INT_SHAPES + cc.INT_SHAPES_PERSISTENT:
        cc.check_integers_exact(ctx, shape, dt, expect_kernel=True)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_pass_on_a_view_with_a_row_pitch_above_d(ctx, dt):
    for shape in ((17, 3, 16), (33, 17, 80), (37, 64, 512), (37, 64, 272)):
        cc.check_integers_exact(ctx, shape, dt, expect_kernel=True, pitch=True)


@pytest.mark.parametrize("case", cc.PASS_CASES, ids=lambda c: c.name)
def test_pass_against_long_double(ctx, case):
    cc.check_pass_against_long_double(ctx, case, expect_kernel=True)


@pytest.mark.parametrize("case", cc.H_CASES, ids=lambda c: c.name)
def test_hupdate_against_long_double(ctx, case):
    cc.check_hupdate_against_long_double(ctx, case, expect_kernel=True)


@pytest.mark.parametrize("case", cc.FIT_CASES, ids=lambda c: c.name)
def test_fit_matches_the_model(ctx, case):
    cc.check_fit_against_model(ctx, case, expect_kernel=True)


@pytest.mark.parametrize("updates", [None, 200])
@pytest.mark.parametrize("case", cc.FIT_CASES[3:4] + cc.FIT_CASES[15:16] + cc.FIT_CASES[-1:], ids=lambda c: c.name)
def test_transform_matches_the_model(ctx, case, updates):
    cc.check_transform(ctx, case, expect_kernel=True, updates=updates)


@pytest.mark.parametrize("case", cc.STOP_CASES, ids=lambda c: c.name)
def test_stopping_rule(ctx, case):
    cc.check_stopping_rule(ctx, case, expect_kernel=True)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_zero_violation_stops_at_iteration_one(ctx, dt):
    cc.check_zero_violation_stops_at_once(ctx, dt, expect_kernel=True)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_random_init_draws_from_the_pcg_stream(ctx, dt):
    cc.check_random_init(ctx, dt, expect_kernel=True)


@pytest.mark.parametrize("case", cc.FIT_CASES[7:8] + cc.FIT_CASES[-1:], ids=lambda c: c.name)
def test_same_fit_twice_gives_the_same_bytes(ctx, case):
    cc.check_same_bytes_twice(ctx, case)


def test_same_pass_twice_gives_the_same_bytes(ctx):
    """more tiles than workgroups at the widest shape: the slabs and the violations are added in a fixed order"""
    rng = np.random.default_rng(3)
    n = cc.INT_N_PERSISTENT
    xr, wr, hr = rng.random((n, 512)).astype(np.float32), rng.random((n, 64)) + 0.05, rng.random((64, 512)) + 0.05
    a = petal.nmf_cd_pass(xr, wr, hr, l1_w=0.1, ctx=ctx)
    b = petal.nmf_cd_pass(xr, wr, hr, l1_w=0.1, ctx=ctx)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(a, b))
    mw, ma, mb, mv = cc.model_pass(xr, wr, hr, 0.1, 0.0, 1)
    assert max(cc.rel_max(a[0], mw), cc.rel_max(a[1], ma), cc.rel_max(a[2], mb), cc.rel_max(a[3], mv)) <= 1e-11


def test_forced_fallback_agrees_with_the_kernel(ctx):
    cc.check_fallback_against_kernel(ctx, expect_kernel=True)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("shape", cc.OUTSIDE_SHAPES, ids=str)
def test_shapes_outside_the_kernel_envelope(ctx, shape, dt):
    cc.check_outside_envelope(ctx, shape, dt)


def test_device_input_stays_on_the_device(ctx):
    import torch
    c = cc.FIT_CASES[7]
    x, w0, h0, xq = cc.fit_inputs(c.n, c.d, c.k, c.dt)
    mo = cc.fit_model(c)
    m = cc.make(ctx, c)
    w = m.fit_transform(torch.from_numpy(np.array(x)).cuda(), W=w0, H=h0)
    wq = m.transform(torch.from_numpy(np.array(xq)).cuda())
    assert w.is_cuda and wq.is_cuda and m.info()["fit_kernel"] == 1 and m.info()["transform_kernel"] == 1
    assert max(cc.rel_max(w, mo.w), cc.rel_max(wq, cc.model_transform(np.asarray(xq, dtype=np.float64), mo.h, c.max_iter, cc.case_penalties(c)))) \
        <= cc.tol_of(c.dt)


@pytest.mark.parametrize("case", cc.nc.FIT_CASES[1:2] + cc.nc.FIT_CASES[10:11], ids=lambda c: c.name)
def test_nothing_existing_moved(ctx, case):
    cc.check_nothing_existing_moved(ctx, case)


def test_errors(ctx):
    def sharded():
        other = petal.Context(0)
        other.set_collective(lambda *a: 0, 0, 2)
        return other
    cc.check_errors(ctx, lambda: petal.Context(0), sharded)


def test_cpp_facade_on_gpu():
    """tests/cpp/nmf_cd_facade_tests.cpp against libpetal_hip.so: the C++ facade's Nmf<A>::solver with k_nmf_cd_pass (the CPU suite runs
    the same program against the host simulation's composed path)"""
    kit.run_cpp_facade("nmf_cd", "kernel", kit.HIP_LIBRARY, "hip")
