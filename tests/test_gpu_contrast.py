"""The FastICA contrast functions exp and cube on a real MI355X, in both GEMM modes: every step-kernel path through petal.ica_par with
the contrast in the mode word (tests/contrast_cases.py holds the references, the table and the bounds), bitwise layout independence
and run-to-run determinism, whole fits against a float64 loop with the same contrast, the sharded code path, and the step statistics.
Run with -m gpu."""
import numpy as np
import pytest

import header_kit as kit
import contrast_cases as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["bf16x3", "fp32"])
def ctx(request):
    import petal_decomposition_amd as petal
    c = petal.Context(0)          # raises (no CPU fallback) when the HIP library or the GPU is missing
    c.set_gemm_mode(request.param)
    c.gemm_mode_name = request.param
    yield c
    c.close()


# (the references and models do not depend on the GEMM mode: contrast_cases caches them per case, the second mode costs the device calls only)
@pytest.mark.parametrize("case", cc.all_cases(device=True), ids=repr)
def test_contrast_kernel_entry(ctx, case):
    err, model, bound = case.run(ctx)
    print(f"{case.id} {ctx.gemm_mode_name}: error {err:.3e}, model {model:.3e}, bound {bound:.3e}")
    assert err <= bound, (case.id, ctx.gemm_mode_name, err, model, bound)


@pytest.mark.parametrize("fun", cc.FUNS)
@pytest.mark.parametrize("row", [(4099, 17, "f32", 13), (70033, 49, "f32", 18), (3000, 65, "f32", 19), (3000, 33, "f64", 23)], ids=repr)
def test_two_identical_calls_give_identical_bytes(ctx, fun, row):
    """the per-wave partial sums are combined in a fixed order on every path: fused (ragged block), two blocks per wave, more than 64
    components (the column sums of g'), the generic kernel"""
    import petal_decomposition_amd as petal
    n, nc, dt, seed = row
    x1, w0 = cc.ica_inputs(n, nc, dt, seed)
    a, _ = petal.ica_par(x1, 0.0, 2, w0, cc.mode_of(fun), ctx)
    b, _ = petal.ica_par(x1, 0.0, 2, w0, cc.mode_of(fun), ctx)
    assert np.all(np.isfinite(a)) and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("fun", cc.FUNS)
def test_the_contrast_is_not_logcosh(ctx, fun):
    """(the three contrasts give three different iterates: a mode word that were dropped on the way would not)"""
    import petal_decomposition_amd as petal
    x1, w0 = cc.ica_inputs(4099, 17, "f32", 13)
    base, _ = petal.ica_par(x1, 0.0, 1, w0, petal.ICA_TEXTBOOK, ctx)
    explicit, _ = petal.ica_par(x1, 0.0, 1, w0, petal.ICA_TEXTBOOK | petal.ICA_CONTRAST_LOGCOSH, ctx)
    other, _ = petal.ica_par(x1, 0.0, 1, w0, cc.mode_of(fun), ctx)
    assert base.tobytes() == explicit.tobytes()
    assert float(np.abs(other - base).max()) > 1e-3


@pytest.mark.parametrize("mode", [48, 240, 256])
def test_undefined_contrast_field(ctx, mode):
    import petal_decomposition_amd as petal
    x1, w0 = cc.ica_inputs(256, 16, "f32", 12)
    with pytest.raises(petal.InvalidInput, match="FastICA"):
        petal.ica_par(x1, 0.0, 1, w0, mode, ctx)


@pytest.mark.parametrize("fun", cc.FUNS)
@pytest.mark.parametrize("shape", cc.FIT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}-nc{s[2]}-{np.dtype(s[3]).name}")
def test_whole_fit(ctx, fun, shape):
    n, d, nc, dtype, seed = shape
    dev, n_iter, n_iter_ref = cc.fit_check(ctx, fun, n, d, nc, dtype, seed)
    print(f"{fun} {n}x{d} nc={nc} {np.dtype(dtype).name} {ctx.gemm_mode_name}: deviation from identity {dev:.3e}, n_iter {n_iter} (reference {n_iter_ref})")


def test_step_statistics_are_unchanged(ctx):
    """one launch of the step per iteration whatever the contrast, and the per-launch work figures are those of the logcosh step"""
    import petal_decomposition_amd as petal
    x = cc.po.synth_ica(20000, 24, 8, seed=31, dtype=np.float64).astype(np.float32)
    w0 = np.random.default_rng(38).standard_normal((8, 8)).astype(np.float32)
    ctx.set_profiling(2)
    try:
        seen = {}
        for fun in ("logcosh",) + cc.FUNS:
            m = petal.FastIca(ctx=ctx, n_components=8, fun=fun, tol=0.0, max_iter=5)     # tol = 0: exactly max_iter iterations
            m.fit(x, w_init=w0)
            st = ctx.stats()
            assert m.n_iter == 5 and st["n_iter"] == 5, (fun, m.n_iter, st)
            assert st["ica_step_launches"] == m.n_iter, (fun, st)
            assert st["ica_step_ms"] > 0.0, (fun, st)
            seen[fun] = (st["ica_step_flops"], st["ica_step_bytes"])
        assert seen["exp"] == seen["cube"] == seen["logcosh"] == (4.0 * 8 * 8 * 20000, 4.0 * 8 * 20000), seen
    finally:
        ctx.set_profiling(0)


def test_cpp_facade_fits_on_gpu():
    """tests/cpp/contrast_facade_tests.cpp against libpetal_hip.so: exp and cube fits through the C++ facade's `contrast` member"""
    kit.run_cpp_facade("contrast", "fits", kit.HIP_LIBRARY, "hip")


def test_sharded_path_single_rank(ctx):
    """An exp fit through the complete sharded code path (PETAL_OPT_FORCE_COLLECTIVE on a one-rank communicator: rank info, the
    all-reduce of [GX | g'] in every iteration, the convergence flag read every fourth iteration).  A one-rank all-reduce is the
    identity, so the sharded path must reproduce the plain fit: the same bytes (measured so on the MI355X in both GEMM modes), for
    the whole fit and for ica_par alone."""
    import os
    import socket
    import torch
    import torch.distributed as dist
    import petal_decomposition_amd as petal
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    try:
        x = cc.po.synth_ica(20000, 24, 8, seed=31, dtype=np.float64).astype(np.float32)
        w0 = np.random.default_rng(38).standard_normal((8, 8)).astype(np.float32)
        ref = petal.FastIca(ctx=ctx, n_components=8, fun="exp")
        yr = np.asarray(ref.fit_transform(x, w_init=w0))
        c2 = petal.Context(0, stream=torch.cuda.current_stream().cuda_stream)
        try:
            c2.set_gemm_mode(ctx.gemm_mode_name)
            c2.use_rccl()
            c2.set_option("force_collective", 1)
            m = petal.FastIca(ctx=c2, n_components=8, fun="exp")
            y = np.asarray(m.fit_transform(x, w_init=w0))
            st = c2.stats()
            assert st["allreduce_calls"] >= m.n_iter + 2, st      # the sharded path RAN: prologue, covariance, one per iteration
            assert m.n_iter == ref.n_iter, (m.n_iter, ref.n_iter)
            assert m.components.tobytes() == ref.components.tobytes()
            assert y.tobytes() == yr.tobytes()
            # the loop alone: the same whitened data and start on both sides
            x1, w0p = cc.ica_inputs(20000, 32, "f32", 14)
            plain, ni = petal.ica_par(x1, 0.0, 3, w0p, cc.mode_of("exp"), ctx)
            shard, ni2 = petal.ica_par(x1, 0.0, 3, w0p, cc.mode_of("exp"), c2)
            assert ni == ni2 == 3 and c2.stats()["allreduce_calls"] >= 3, c2.stats()
            assert shard.tobytes() == plain.tobytes()
        finally:
            c2.close()
    finally:
        dist.destroy_process_group()
