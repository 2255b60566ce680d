"""The lower bf16 planes of every split-product kernel -- K1, K2, the fused pass, the Gram kernel, the score kernel -- and their steering
forms (PETAL_OPT_STEERING_HOOK) on a real MI355X, in both GEMM modes: operands with a bit budget, the float64 product as the reference
to the last bit.  tests/plane_cases.py holds the designs, the certificate, the tables and the assertion.  Run with -m gpu."""
import pytest

import plane_cases as pl

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["bf16x3", "fp32"])
def ctx(request):
    import petal_decomposition_amd as petal
    c = petal.Context(0)          # raises (no CPU fallback) when the HIP library or the GPU is missing
    c.set_gemm_mode(request.param)
    c.gemm_mode_name = request.param
    yield c
    c.close()


def _run(ctx, case):
    runner = pl.DeviceRunner(ctx, split=ctx.gemm_mode_name == "bf16x3")
    calls, exact, bad, bounded, ratio = case.run(runner)
    print(f"{case.id} {ctx.gemm_mode_name}: {calls} calls, {exact} exact elements, {bad} mismatches, {bounded} bounded elements, worst error / bound {ratio:.4f}")
    assert exact > 0 and bad == 0 and ratio <= 1.0
    assert ctx.get_option("steering_hook") == 0 and ctx.get_option("gram_split_hook") == 0 and ctx.get_option("fused_pass_min_rows") == 8192


@pytest.mark.parametrize("case", pl.k1_cases(), ids=repr)
def test_k1_planes(ctx, case):
    """k_xp3 on three planes, and under the hook on a two-plane P (five piece products) and, beyond 80 columns, a two-plane X (four)"""
    _run(ctx, case)


@pytest.mark.parametrize("case", pl.k2_cases(), ids=repr)
def test_k2_planes(ctx, case):
    """k_atb3: the narrow-workgroup and the eight-wave forms, the ragged rows of the last chunk; under the hook P4 where the form has it"""
    _run(ctx, case)


@pytest.mark.parametrize("case", pl.fused_cases(), ids=repr)
def test_fused_pass_planes(ctx, case):
    """k_pow3 with and without z, k_pow3f under the hook: fused = 1 in split-product mode is asserted by the runner"""
    _run(ctx, case)


@pytest.mark.parametrize("case", pl.gram_cases(), ids=repr)
def test_gram_planes(ctx, case):
    _run(ctx, case)


@pytest.mark.parametrize("case", pl.score_cases(), ids=repr)
def test_score_kernel_planes(ctx, case):
    """the y that petal_score_rows writes beside the scores"""
    _run(ctx, case)


def test_steering_hook_is_an_option_of_the_ctx(ctx):
    import petal_decomposition_amd as petal
    assert petal.OPTIONS["steering_hook"] == 15 and ctx.get_option(15) == 0
    ctx.set_option("steering_hook", 1)
    assert ctx.get_option("steering_hook") == 1
    ctx.set_option("steering_hook", 0)
    with pytest.raises(petal.InvalidInput):
        ctx.set_option(16, 1)
