"""Nmf with the coordinate-descent solver on sparse CSR data (include/petal_hip_nmf_cd_sparse.h) on the MI355X: the cd sweep kernel
k_nmf_cd_sweep (four rows per wave) through petal_nmf_cd_sweep_csr -- exact operands bit for bit over the seams of the 64-entry load,
of the 256-entry item and of the four-item wave, real data against numpy.longdouble inside the project's bound -- and
Nmf(solver="cd", sparse_path="sweep") itself: fit, fit_transform and transform against the numpy model on the densified matrix, the
stopping rule, the random initialisation, the same bytes twice and on a second handle, the densifying fall-back, what did not move,
every error."""

import numpy as np
import pytest

import header_kit as kit
import nmf_cd_sparse_cases as cs
import petal_decomposition_amd as petal
from sparse_cases import to_csr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = petal.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------- 1. exact operands
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("which", cs.INT_WHICH)
def test_sweep_on_exact_operands(ctx, which, dt):
    cs.check_cd_sweep_exact(ctx, cs.int_case(which), which, dt, expect_kernel=True)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_sweep_on_tiny_matrices(ctx, dt):
    for rows in cs.TINY_ROWS:
        cs.check_cd_sweep_exact(ctx, cs.tiny_case(rows), 100 + rows, dt, expect_kernel=True)


# ------------------------------------------------------------------------------------------- 2. real data against long double
@pytest.mark.parametrize("case", cs.SWEEP_CASES, ids=lambda c: c.name)
def test_sweep_against_long_double(ctx, case):
    cs.check_sweep_against_long_double(ctx, case, expect_kernel=True)


# ------------------------------------------------------------------------------------------- 3. fits and transforms
@pytest.mark.parametrize("case", cs.FIT_CASES, ids=lambda c: c.name)
def test_fit_matches_the_model(ctx, case):
    cs.check_fit_against_model(ctx, case, expect_kernel=True)


@pytest.mark.parametrize("case", cs.FIT_CASES[4:5] + cs.FIT_CASES[-1:], ids=lambda c: c.name)
def test_duck_input_takes_the_same_path(ctx, case):
    cs.check_fit_against_model(ctx, case, expect_kernel=True, duck=True)


@pytest.mark.parametrize("updates", [3, 200])
@pytest.mark.parametrize("case", cs.FIT_CASES[2:3] + cs.FIT_CASES[17:18] + cs.FIT_CASES[-1:], ids=lambda c: c.name)
def test_transform_matches_the_model(ctx, case, updates):
    cs.check_transform(ctx, case, expect_kernel=True, updates=updates)


# ------------------------------------------------------------------------------------------- 4. the stopping rule
@pytest.mark.parametrize("case", cs.STOP_CASES, ids=lambda c: c.name)
def test_stopping_rule(ctx, case):
    cs.check_stopping_rule(ctx, case, expect_kernel=True)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_zero_violation_stops_at_iteration_one(ctx, dt):
    cs.check_zero_violation_stops_at_once(ctx, dt, expect_kernel=True)


# ------------------------------------------------------------------------------------------- 5. random init, determinism, paths
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_random_init_draws_from_the_pcg_stream(ctx, dt):
    cs.check_random_init(ctx, dt, expect_kernel=True)


@pytest.mark.parametrize("case", cs.FIT_CASES[7:8] + cs.FIT_CASES[-1:], ids=lambda c: c.name)
def test_same_fit_twice_and_on_a_second_handle_gives_the_same_bytes(ctx, case):
    cs.check_same_bytes_twice(ctx, case)


def test_same_sweep_twice_gives_the_same_bytes(ctx):
    """more 16-row tiles than the reduction has workgroups (5000 rows), split rows among them: G, Gram, dot and the violations are added
    in a fixed order"""
    rng = np.random.default_rng(11)
    n, d, k = 5000, 300, 33
    x = (rng.random((n, d)) * (rng.random((n, d)) < 0.03)).astype(np.float32)
    x[7, :] = 1.0
    g, f = rng.random((n, k)) + 0.05, rng.random((d, k)) + 0.05
    runs = []
    for _ in range(2):
        sx = cs.csr(ctx, *to_csr(x), x.shape)
        try:
            runs.append(petal.nmf_cd_sweep(sx, g, f, l1=0.1, l2=0.2, inner_iters=2))
        finally:
            sx.close()
    assert all(np.asarray(p).tobytes() == np.asarray(q).tobytes() for p, q in zip(runs[0], runs[1]))
    mg, mgram, mdot, mv = cs.model_cd_sweep(x, g, f, 0.1, 0.2, 2)
    assert max(cs.rel_max(runs[0][0], mg), cs.rel_max(runs[0][1], mgram), abs(runs[0][2] - mdot) / mdot, cs.rel_max(runs[0][3], mv)) <= 1e-11


@pytest.mark.parametrize("case", cs.FIT_CASES[1:2] + cs.FIT_CASES[-1:], ids=lambda c: c.name)
def test_forced_fallback_is_the_dense_fit_and_agrees_with_the_sweep(ctx, case):
    x, w0, h0, _ = cs.fit_inputs(case.n, case.d, case.k, case.dt)
    sx = cs.csr(ctx, *to_csr(x), x.shape)
    try:
        m = cs.make(ctx, case)
        w = m.fit_transform(sx, W=w0, H=h0)
        assert m.kernel_path == 1
    finally:
        sx.close()
    ctx.set_option("nmf_fallback", 1)
    try:
        f = cs.check_fallback_equals_dense(ctx, case)
        assert f.info()["fit_kernel"] == 0
        wf = f.fit_transform(cs.Duck(*to_csr(x), x.shape), W=w0, H=h0)
    finally:
        ctx.set_option("nmf_fallback", 0)
    tol = cs.tol_of(case.dt)
    assert max(cs.rel_max(wf, w), cs.rel_max(f.components, m.components)) <= tol
    assert abs(f.reconstruction_err - m.reconstruction_err) <= tol * m.reconstruction_err


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_more_than_64_components_densify(ctx, dt):
    c = cs.FitCase(f"{dt}-260x300-k65", 260, 300, 65, dt, 3, 0.0, "same", 0.0)
    m = cs.check_fallback_equals_dense(ctx, c)
    mo = cs.fit_model(c)
    assert max(cs.rel_max(m.components, mo.h), abs(m.reconstruction_err - mo.err) / mo.err) <= cs.tol_of(dt)


def test_dense_image_beyond_the_limit_is_refused(ctx):
    cs.check_too_large_to_densify(ctx)


# ------------------------------------------------------------------------------------------- 6. nothing moved
@pytest.mark.parametrize("case", cs.FIT_CASES[1:2] + cs.FIT_CASES[-1:], ids=lambda c: c.name)
def test_nothing_existing_moved(ctx, case):
    cs.check_nothing_existing_moved(ctx, case)


# ------------------------------------------------------------------------------------------- 7. errors and lifetime
def test_errors_and_workspace(ctx):
    def sharded():
        other = petal.Context(0)
        holder = []

        def make(data, indices, indptr, shape):
            sx = petal.CsrMatrix(data, indices, indptr, shape, ctx=other)
            other.set_collective(lambda *a: 0, 0, 2)
            holder.append(sx)
            return sx
        return other, make
    base = ctx.workspace_in_use()
    m = cs.check_errors(ctx, lambda: petal.Context(0), sharded)
    blocks, nbytes = ctx.workspace_in_use()
    assert blocks == base[0] + 2 and nbytes > base[1]            # the live model holds H and H H^T, nothing else is out
    m.close()
    assert ctx.workspace_in_use() == base


# ------------------------------------------------------------------------------------------- 8. the C++ facade
def test_cpp_facade_on_gpu():
    """tests/cpp/nmf_cd_sparse_facade_tests.cpp against libpetal_hip.so: the C++ facade's Nmf<A>::sparse_path with k_nmf_cd_sweep (the
    CPU suite runs the same program against the host simulation's densifying path)"""
    kit.run_cpp_facade("nmf_cd_sparse", "kernel", kit.HIP_LIBRARY, "hip")
