"""The FastICA step / tail kernels, the textbook symmetric decorrelation and svd_flip through their own ABI entries on a real MI355X,
in both GEMM modes: tests/kernel_entry_cases.py holds the references, the tables and the bounds.  Run with -m gpu."""
import pytest

import kernel_entry_cases as kc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["bf16x3", "fp32"])
def ctx(request):
    import petal_decomposition_amd as petal
    c = petal.Context(0)          # raises (no CPU fallback) when the HIP library or the GPU is missing
    c.set_gemm_mode(request.param)
    c.gemm_mode_name = request.param
    yield c
    c.close()


# (the references and models do not depend on the GEMM mode: kernel_entry_cases caches them per case, the second mode costs the device calls only)
@pytest.mark.parametrize("case", kc.all_cases(device=True), ids=repr)
def test_kernel_entry(ctx, case):
    err, model, bound = case.run(ctx)
    print(f"{case.id} {ctx.gemm_mode_name}: error {err:.3e}, model {model:.3e}, bound {bound:.3e}")
    assert err <= bound, (case.id, ctx.gemm_mode_name, err, model, bound)
