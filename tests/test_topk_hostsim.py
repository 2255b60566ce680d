"""tests/topk_cases.py on the host simulation (tests/hostsim.py): the same check functions, references, model and bounds as the device
module, a reduced table.  What it proves on a machine without a GPU is the TEST -- that the references certify themselves, that the
float64 model of topk_eigh puts at least two rows of the table into every outcome class under its certificate, that every bound is one
the float64 model stays inside -- and it holds the host algorithm (the same csrc/algo.cpp) and oracle/cpu_ops.cpp::op_ritz_residual to
the contract the device is held to."""
import os
import re

import pytest

import hostsim
import topk_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    c = hostsim.context()
    yield c
    c.close()


@pytest.mark.parametrize("case", tc.all_cases(device=False), ids=repr)
def test_topk_on_the_host_simulation(ctx, case):
    rows = case.run(ctx)
    for q, err, model, bound in rows:
        print(f"{case.id} [{case.form}] {q}: error {err:.3e}, model {model:.3e}, bound {bound:.3e}")
    for q, err, model, bound in rows:
        assert err <= bound, (case.id, q, err, model, bound)
        assert model <= bound, (case.id, q, model, bound)      # the bound cannot drift below what the reference algorithm delivers


def test_seed_cache_on_the_host_simulation():
    tc.topk_cache_check(hostsim.context, device=False)


def test_the_model_fills_every_outcome_class():
    """on the model alone, the FULL (device) table: every certificate holds and at least two rows land in each class"""
    count = {}
    for row in tc.topk_rows(device=True):
        m = tc.model_of_row(*row)
        count[m["cls"]] = count.get(m["cls"], 0) + 1
        if m["close"]:
            count["close"] = count.get("close", 0) + 1
    for cls in ("first", "later", "rate", "drop", "close", "nonfinite"):
        assert count.get(cls, 0) >= 2, (cls, count)


def test_table_covers_the_orders_pair_counts_and_families():
    rows = tc.topk_rows(device=True)
    assert {r[2] for r in rows} == {89, 100, 160, 200, 256}
    assert {r[3] for r in rows} == {1, 8, 16, 17, 64, 65, 72, 130}
    for fam in "abcdefgh":
        assert {r[4] for r in rows if r[0] == fam} == {tc.F32, tc.F64}, fam
    assert all(tc.applies(r[2], r[3]) for r in rows)
    assert [(d, nc, tc.applies(d, nc)) for d, nc, _ in tc.SHAPE_ROWS] == tc.SHAPE_ROWS
    assert {c.args[:2] for c in tc.rr_cases(True) if c.fn is tc.rr_shape_check} == {(r, n) for r in tc.RR_ROWS for n in tc.RR_NC}


def test_probe_bad_shapes_modes_and_types_are_invalid_input(ctx):
    import numpy as np
    import petal_decomposition_amd as petal
    a = np.eye(20)
    for bad in (lambda: petal.probe_topk_eigh(a, 21, ctx=ctx), lambda: petal.probe_topk_eigh(a, 2, mode=3, ctx=ctx),
                lambda: petal.probe_topk_eigh(a, 2, dtype=7, ctx=ctx),
                lambda: petal.probe_ritz_residual(np.zeros((2, 3)), np.zeros((2, 3)), 4, np.zeros(4), ctx=ctx),
                lambda: petal.probe_ritz_residual(np.zeros((2, 3)), np.zeros((2, 3)), 2, np.zeros(2), w_len=1, ctx=ctx)):
        with pytest.raises(petal.InvalidInput):
            bad()


def test_probe_on_a_sharded_ctx_is_invalid_input():
    import numpy as np
    import petal_decomposition_amd as petal
    c = hostsim.context()
    try:
        c.set_collective(lambda *a: 0, 0, 2)       # rank 0 of 2: the probes refuse before anything is reduced
        with pytest.raises(petal.InvalidInput):
            petal.probe_topk_eigh(np.eye(100), 8, ctx=c)
        with pytest.raises(petal.InvalidInput):
            petal.probe_ritz_residual(np.zeros((4, 3)), np.zeros((4, 3)), 2, np.ones(2), ctx=c)
    finally:
        c.close()


def test_probe_header_and_binding_name_the_same_entries():
    import petal_decomposition_amd as petal
    text = open(os.path.join(ROOT, "include", "petal_hip_probe.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = {m.group(1): m.group(2).count(",") + 1 for m in re.finditer(r"\bint\s+(petal_probe_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}
    assert decl == {n: len(args) for n, _, args in petal.ABI_PROBE}
    assert {"petal_probe_ritz_residual", "petal_probe_topk_eigh"} <= set(decl)
