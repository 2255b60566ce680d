"""tests/rebase_cases.py on the host simulation (tests/hostsim.py): the same check functions, references and bounds as the device
module, a reduced table -- table A for routes 0 and 1 at two block counts, a few rows of tables B and C, the refusals.  What it proves
on a machine without a GPU is the TEST: that the exact-integer certificates hold on the references alone, that the long-double
references and the derived bounds fit a second implementation of the same statements -- and it holds oracle/cpu_ops.cpp to the
contract the device kernels are held to (the folded column sums of the steering form are those of the two-plane values)."""
import pytest

import hostsim
import rebase_cases as rc


@pytest.fixture(scope="module")
def ctx():
    c = hostsim.context()
    yield c
    c.close()


@pytest.mark.parametrize("case,mode", [pytest.param(c, m, id=f"{c.id}-{m}") for c, m in rc.params(device=False)])
def test_rebase_on_the_host_simulation(ctx, case, mode):
    rows = case.run(ctx, mode, device=False)
    rc.check_rows(case, mode, rows)
