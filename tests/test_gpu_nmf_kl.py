"""Nmf with the Kullback-Leibler loss on sparse CSR data (include/petal_hip_nmf_kl.h) on the MI355X: the sweep k_nmf_kl_sweep /
k_nmf_kl_split / k_nmf_kl_colsum through petal_nmf_kl_sweep_csr -- exact operands bit for bit over the load, item and split seams on
both images, several updates in one call against chained single updates, real data against numpy.longdouble inside the model-tied
bound -- and Nmf(beta_loss="kullback-leibler") itself on a resident CsrMatrix: fit, fit_transform and transform against the numpy model,
the stopping rule, the random initialisation, the same bytes twice and on a second handle, dense input, the forced fall-back, every
error, the workspace count."""

import numpy as np
import pytest

import header_kit as kit
import nmf_kl_cases as kc
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
@pytest.mark.parametrize("which", range(-1, len(kc.INT_SHAPES)), ids=lambda w: "seams" if w < 0 else "x".join(map(str, kc.INT_SHAPES[w])))
def test_sweep_on_exact_operands(ctx, which, dt):
    kc.check_sweep_exact(ctx, which, dt, expect_kernel=True)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("which", [-1, 0], ids=["seams", "257x130-dup"])
def test_inner_updates_are_chained_single_updates(ctx, which, dt):
    """the seam matrix has split rows (one launch pair per update) and its transposed image has none (the updates loop in the kernel);
    both images of 257 x 130 have split rows"""
    assert kc.split_rows(-1, False) and not kc.split_rows(-1, True) and kc.split_rows(0, False) and kc.split_rows(0, True)
    kc.check_inner_is_chained_single_updates(ctx, which, dt, expect_kernel=True)


# ------------------------------------------------------------------------------------------- 2. long double
@pytest.mark.parametrize("case", kc.SWEEP_CASES, ids=lambda c: c.name)
def test_sweep_against_long_double(ctx, case):
    kc.check_sweep_against_long_double(ctx, case, expect_kernel=True)


# ------------------------------------------------------------------------------------------- 3. fits
@pytest.mark.parametrize("case", kc.FIT_CASES, ids=lambda c: c.name)
def test_fit_matches_the_model(ctx, case):
    kc.check_fit_against_model(ctx, case, expect_kernel=True)


def test_duck_typed_csr_is_accepted(ctx):
    kc.check_fit_against_model(ctx, kc.FIT_CASES[2], expect_kernel=True, duck=True)


# ------------------------------------------------------------------------------------------- 4. transform
@pytest.mark.parametrize("updates", [13, 200])
@pytest.mark.parametrize("case", kc.FIT_CASES[:1] + kc.FIT_CASES[15:16] + kc.FIT_CASES[-2:], ids=lambda c: c.name)
def test_transform_matches_the_model(ctx, case, updates):
    kc.check_transform(ctx, case, expect_kernel=True, updates=updates)


# ------------------------------------------------------------------------------------------- 5. the stopping rule
@pytest.mark.parametrize("case", kc.STOP_CASES, ids=lambda c: c.name)
def test_stopping_rule(ctx, case):
    kc.check_stopping_rule(ctx, case, expect_kernel=True)


# ------------------------------------------------------------------------------------------- 6. random initialisation, determinism, dense input
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_random_init_draws_from_the_pcg_stream(ctx, dt):
    kc.check_random_init(ctx, dt, expect_kernel=True)


@pytest.mark.parametrize("case", kc.FIT_CASES[2:3] + kc.FIT_CASES[-1:], ids=lambda c: c.name)
def test_same_fit_twice_and_on_a_second_handle_gives_the_same_bytes(ctx, case):
    kc.check_same_bytes_twice(ctx, case)


@pytest.mark.parametrize("case", kc.FIT_CASES[1:2] + kc.FIT_CASES[-1:], ids=lambda c: c.name)
def test_dense_input_is_the_csr_of_its_nonzeros(ctx, case):
    kc.check_dense_input_is_the_csr_of_its_nonzeros(ctx, case, expect_kernel=True)


def test_a_device_tensor_is_copied_to_the_host_and_takes_the_same_path(ctx):
    import torch
    case = kc.FIT_CASES[1]
    x, w0, h0, xq = kc.fit_inputs(case.n, case.d, case.k, case.dt)
    _, want = kc.fit_bytes(ctx, case, np.array(x), np.array(xq))
    m = kc.make(ctx, case)
    w = m.fit_transform(torch.from_numpy(np.array(x)).cuda(), W=w0, H=h0)
    wq = m.transform(torch.from_numpy(np.array(xq)).cuda())
    assert w.is_cuda and wq.is_cuda and m.kernel_path == 1
    assert (kc.to_numpy(w).tobytes(), m.components.tobytes(), kc.to_numpy(wq).tobytes()) == (want[0], want[1], want[4])


@pytest.mark.parametrize("case", kc.FIT_CASES[1:2] + kc.FIT_CASES[-1:], ids=lambda c: c.name)
def test_explicit_frobenius_changes_nothing(ctx, case):
    kc.check_explicit_frobenius_changes_nothing(ctx, case)


# ------------------------------------------------------------------------------------------- 7. the fall-back
@pytest.mark.parametrize("case", kc.FIT_CASES[1:2] + kc.FIT_CASES[-1:], ids=lambda c: c.name)
def test_forced_fallback_takes_the_host_loop_and_agrees_with_the_kernel(ctx, case):
    x, w0, h0, xq = kc.fit_inputs(case.n, case.d, case.k, case.dt)
    sx, sq = kc.csr(ctx, *to_csr(x), x.shape), kc.csr(ctx, *to_csr(xq), xq.shape)
    try:
        m = kc.make(ctx, case)
        w = m.fit_transform(sx, W=w0, H=h0)
        wq = m.transform(sq)
        assert m.kernel_path == 1 and m.info()["fit_kernel"] == 1
        ctx.set_option("nmf_fallback", 1)
        try:
            f = kc.make(ctx, case)
            wf = f.fit_transform(sx, W=w0, H=h0)
            assert f.kernel_path == 0 and f.info()["fit_kernel"] == 0
            wqf = f.transform(sq)
            assert f.kernel_path == 0 and f.info()["transform_kernel"] == 0
        finally:
            ctx.set_option("nmf_fallback", 0)
        tol = kc.tol_of(case.dt)
        assert max(kc.rel_max(wf, w), kc.rel_max(f.components, m.components), kc.rel_max(wqf, wq)) <= tol
        assert abs(f.reconstruction_err - m.reconstruction_err) <= tol * m.reconstruction_err
        assert abs(f.err_init - m.err_init) <= tol * m.err_init
    finally:
        sx.close()
        sq.close()


# ------------------------------------------------------------------------------------------- 8. errors and lifetime
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
    m = kc.check_errors(ctx, lambda: petal.Context(0), sharded)
    blocks, nbytes = ctx.workspace_in_use()
    assert blocks == base[0] + 2 and nbytes > base[1]            # the live model holds H and its (unused) H H^T block, nothing else is out
    m.close()
    assert ctx.workspace_in_use() == base
    # k > 64 on a resident handle, at the probe
    x = kc.fit_inputs(260, 300, 5, "f64")[0]
    sx = kc.csr(ctx, *to_csr(x), x.shape)
    try:
        with kc.raises_with(petal.InvalidInput, "at most 64 components"):
            petal.nmf_kl_sweep(sx, np.ones((260, 65)), np.ones((300, 65)))
    finally:
        sx.close()
    assert ctx.workspace_in_use() == base


# ------------------------------------------------------------------------------------------- 9. the C++ facade
def test_cpp_facade_on_gpu():
    """tests/cpp/nmf_kl_facade_tests.cpp against libpetal_hip.so: the C++ facade's Nmf with NmfLoss::KullbackLeibler on a CsrMatrix with
    k_nmf_kl_sweep (the CPU suite runs the same program against the host simulation's host loop)"""
    kit.run_cpp_facade("nmf_kl", "kernel", kit.HIP_LIBRARY, "hip")
