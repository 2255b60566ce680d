"""The whitening stage of fastica_fit on a real MI355X, in both GEMM modes, held directly against long double through the max_iter = 0
handle: tests/whitening_cases.py holds the inputs, the references, the models, the bounds and the case table.  Run with -m gpu."""
import pytest

import whitening_cases as wc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["bf16x3", "fp32"])
def ctx(request):
    import petal_decomposition_amd as petal
    c = petal.Context(0)          # raises (no CPU fallback) when the HIP library or the GPU is missing
    c.set_gemm_mode(request.param)
    c.gemm_mode_name = request.param
    yield c
    c.close()


_runs = {}


def _run(ctx, case):
    """one run of the case per GEMM mode, shared by the two tests below (asserts n_iter == 0, the stats words of the table, every cap and
    certificate); printed once"""
    key = (ctx.gemm_mode_name, case.id)
    if key not in _runs:
        family, st, rows = _runs[key] = case.run(ctx)
        print(f"{case.id} {ctx.gemm_mode_name} {family}: ica_gram_split {st['ica_gram_split']}, ica_redo {st['ica_redo']}, "
              f"means_folded {st['means_folded']}")
        for q, err, model, bound in rows:
            print(f"{case.id} {ctx.gemm_mode_name} {q}: error {err:.3e}, model {model:.3e}, bound {bound:.3e}")
    return _runs[key]


# (the references and models do not depend on the GEMM mode: whitening_cases caches them per case, the second mode costs the device calls
# and the long-double products of what came back)
@pytest.mark.parametrize("case", wc.all_cases(device=True), ids=repr)
def test_whitening(ctx, case):
    """whiteness, leak, rows, signs, kmatch, y and transform"""
    family, _, rows = _run(ctx, case)
    for q, err, model, bound in rows:
        if q != "means":
            assert err <= bound, (case.id, ctx.gemm_mode_name, family, q, err, model, bound)


# (the means on their own: the one quantity that is not a property of the whitening matrix)
@pytest.mark.parametrize("case", wc.all_cases(device=True), ids=repr)
def test_whitening_means(ctx, case):
    family, _, rows = _run(ctx, case)
    for q, err, model, bound in rows:
        if q == "means":
            assert err <= bound, (case.id, ctx.gemm_mode_name, family, q, err, model, bound)
