"""The fp64 small-matrix kernels (Cholesky / triangular solves, the fp64 GEMM forms, the symmetric eigen-solvers, the one-sided Jacobi
SVD) through the probe entries of include/petal_hip_probe.h on a real MI355X, against long-double references:
tests/smallmat_cases.py holds the references, the tables and the bounds.  One ctx; both GEMM modes only for the one route that depends
on the mode (the left triangular solve inside the product launcher).  Run with -m gpu."""
import pytest

import smallmat_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import petal_decomposition_amd as petal
    c = petal.Context(0)          # raises (no CPU fallback) when the HIP library or the GPU is missing
    yield c
    c.close()


def _params():
    out = []
    for c in sc.all_cases(device=True):
        for mode in (("bf16x3", "fp32") if c.both_modes() else ("bf16x3",)):
            out.append(pytest.param(c, mode, id=c.id + ("-" + mode if c.both_modes() else "")))
    return out


@pytest.mark.parametrize("case,mode", _params())
def test_smallmat(ctx, case, mode):
    ctx.set_gemm_mode(mode)
    try:
        rows = case.run(ctx)
    finally:
        ctx.set_gemm_mode("bf16x3")
    for q, err, model, bound in rows:
        print(f"{case.id} [{case.form}] {q}: error {err:.3e}, model {model:.3e}, bound {bound:.3e}")
    for q, err, model, bound in rows:
        assert err <= bound, (case.id, q, err, model, bound)
