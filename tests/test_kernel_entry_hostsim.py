"""tests/kernel_entry_cases.py on the host simulation (tests/hostsim.py): the same check functions, references and bounds as the
device module, a reduced table.  What it proves on a machine without a GPU is the TEST: that the long-double references certify
themselves, that the restated svd_flip rule is the crate's, and that every bound is one the reference arithmetic itself -- the
float32 model, the float64 oracle -- stays inside."""
import pytest

import hostsim
import kernel_entry_cases as kc


@pytest.fixture(scope="module")
def ctx():
    c = hostsim.context()
    yield c
    c.close()


@pytest.mark.parametrize("case", kc.all_cases(device=False, reduced=True), ids=repr)
def test_kernel_entry_on_the_host_simulation(ctx, case):
    err, model, bound = case.run(ctx)
    print(f"{case.id}: error {err:.3e}, model {model:.3e}, bound {bound:.3e}")
    assert err <= bound, (case.id, err, model, bound)
    if case.fn is kc.decorr_check:
        assert model <= bound, (case.id, model, bound)      # the bound cannot drift below what the reference algorithm delivers
