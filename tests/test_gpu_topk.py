"""The top-k subspace eigen-solver (topk_eigh through gram_topk_eigh / gram_eigen) and its residual verdict kernel (k_ritz_residual)
through the probe entries of include/petal_hip_probe.h on a real MI355X, against long-double references and a float64 model of the
iteration: tests/topk_cases.py holds the references, the model with its certificate, the tables and the bounds.  Run with -m gpu."""
import pytest

import topk_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import petal_decomposition_amd as petal
    c = petal.Context(0)          # raises (no CPU fallback) when the HIP library or the GPU is missing
    yield c
    c.close()


@pytest.mark.parametrize("case", tc.all_cases(device=True), ids=repr)
def test_topk(ctx, case):
    rows = case.run(ctx)
    for q, err, model, bound in rows:
        print(f"{case.id} [{case.form}] {q}: error {err:.3e}, model {model:.3e}, bound {bound:.3e}")
    for q, err, model, bound in rows:
        assert err <= bound, (case.id, q, err, model, bound)


def test_seed_cache():
    import petal_decomposition_amd as petal
    tc.topk_cache_check(lambda: petal.Context(0), device=True)
