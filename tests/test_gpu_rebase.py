"""The composite operations that steer the optimistic RandomizedPca fit -- op_rebase_xp, op_rebase_power_pass, op_power_pass_means --
through the probe entries of include/petal_hip_probe.h on a real MI355X: exact-integer re-basing bit for bit, re-basing on real
iterates against long double, and the means fold held to bounds derived from its inputs.  tests/rebase_cases.py holds the references,
the tables and the bounds.  One ctx, both GEMM modes.  Run with -m gpu."""
import pytest

import rebase_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import petal_decomposition_amd as petal
    c = petal.Context(0)          # raises (no CPU fallback) when the HIP library or the GPU is missing
    yield c
    c.close()


@pytest.mark.parametrize("case,mode", [pytest.param(c, m, id=f"{c.id}-{m}") for c, m in rc.params(device=True)])
def test_rebase(ctx, case, mode):
    rows = case.run(ctx, mode, device=True)
    rc.check_rows(case, mode, rows)
