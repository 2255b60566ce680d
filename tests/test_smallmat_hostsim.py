"""tests/smallmat_cases.py on the host simulation (tests/hostsim.py): the same check functions, references and bounds as the device
module, a reduced table.  What it proves on a machine without a GPU is the TEST -- that the long-double references certify
themselves, that every bound is one the float64 model stays inside, that no bound is vacuous -- and it holds oracle/cpu_ops.cpp to
the contract the device kernels are held to."""
import pytest

import hostsim
import smallmat_cases as sc


@pytest.fixture(scope="module")
def ctx():
    c = hostsim.context()
    yield c
    c.close()


@pytest.mark.parametrize("case", sc.all_cases(device=False), ids=repr)
def test_smallmat_on_the_host_simulation(ctx, case):
    rows = case.run(ctx)
    for q, err, model, bound in rows:
        print(f"{case.id} [{case.form}] {q}: error {err:.3e}, model {model:.3e}, bound {bound:.3e}")
    for q, err, model, bound in rows:
        assert err <= bound, (case.id, q, err, model, bound)
        assert model <= bound, (case.id, q, model, bound)      # the bound cannot drift below what the reference algorithm delivers
