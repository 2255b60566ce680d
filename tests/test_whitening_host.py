"""tests/whitening_cases.py on the host simulation (tests/hostsim.py): the same checks, references and bounds as the device module, the
whole table minus B5.  What it proves on a machine without a GPU is the TEST -- that every reference certifies itself, that the model
sits inside every bound, that every bound sits inside its cap -- and that a subtly wrong whitening fails: three mutants of the numpy
model, each of which must exceed a bound.  The stats words are recorded and none asserted (on the host simulation ica_gram_split is
always 0 and ica_redo is 1 from 256 features on)."""
import numpy as np
import pytest

import hostsim
import whitening_cases as wc


@pytest.fixture(scope="module")
def ctx():
    c = hostsim.context()
    c.gemm_mode_name = "host"
    yield c
    c.close()


_runs = {}


def _run(ctx, case):
    """one run of the case, shared by the two tests below; printed once"""
    if case.id not in _runs:
        family, st, rows = _runs[case.id] = case.run(ctx)
        print(f"{case.id} {family}: ica_gram_split {st['ica_gram_split']}, ica_redo {st['ica_redo']}, means_folded {st['means_folded']}")
        for q, err, model, bound in rows:
            print(f"{case.id} {q}: error {err:.3e}, model {model:.3e}, bound {bound:.3e}")
    return _runs[case.id]


@pytest.mark.parametrize("case", wc.all_cases(device=False), ids=repr)
def test_whitening_on_the_host_simulation(ctx, case):
    """whiteness, leak, rows, signs, kmatch, y and transform"""
    for q, err, model, bound in _run(ctx, case)[2]:
        if q != "means":
            assert err <= bound, (case.id, q, err, model, bound)
            assert model <= bound, (case.id, q, model, bound)      # the bound cannot drift below what the reference algorithm delivers


# (the means on their own: the one quantity that is not a property of the whitening matrix)
@pytest.mark.parametrize("case", wc.all_cases(device=False), ids=repr)
def test_whitening_means_on_the_host_simulation(ctx, case):
    for q, err, model, bound in _run(ctx, case)[2]:
        if q == "means":
            assert err <= bound, (case.id, q, err, model, bound)
            assert model <= bound, (case.id, q, model, bound)


def _exceeded(rows):
    return [q for q, err, _, bound in rows if err > bound]


# the float32 mutants are held to the WIDER of the two float32 families' bounds: what survives there survives everywhere
@pytest.mark.parametrize("name, family", [("A1-300x20-nc5-f64", "f64-gram"), ("B1-300x20-nc5-f32", "f32-split"),
                                          ("B2-4099x256-nc16-f32", "f32-split")])
def test_mutant_one_row_of_k_scaled_by_1e_4(name, family):
    assert not _exceeded(wc.mutant_rows(name, family, None)), "the unmutated model must pass"
    killed = _exceeded(wc.mutant_rows(name, family, "row"))
    print(name, "killed by", killed)
    assert "white" in killed, killed


# (B3q, not B3: at 4099 rows the provisional centre is the mean of 4096 of them, 4e-4 column standard deviations from the true one, and
# a covariance left there is white to 1.1e-6 -- inside the split-product family's starting bound.  From 8192 rows on it is a sample.)
@pytest.mark.parametrize("name", ["B3q-8195x256-nc16-f32-offset40"])
def test_mutant_covariance_left_at_the_provisional_centre(name):
    assert not _exceeded(wc.mutant_rows(name, "f32-split", None)), "the unmutated model must pass"
    rows = wc.mutant_rows(name, "f32-split", "centre")
    for q, err, model, bound in rows:
        print(f"{name} [centre] {q}: error {err:.3e}, model {model:.3e}, bound {bound:.3e}")
    assert "white" in _exceeded(rows), rows


def test_mutant_sign_rule_taking_the_last_maximum():
    x = wc.tie_input()
    c = x.T @ x
    assert np.array_equal(x.sum(axis=0), np.zeros(3)) and np.array_equal(c, [[28, 12, 0], [12, 28, 0], [0, 0, 4]])
    lam, u = np.linalg.eigh(c)
    p = u[:, ::-1][:, :2]
    assert np.all(np.abs(p[0]) == np.abs(p[1])), "certificate: the input must tie exactly"
    eye = np.eye(2)
    good = wc.model(x, 2, eye)[0]
    bad = wc.model(x, 2, eye, mutant="last")[0]
    assert wc.sign_rule_violations(good, p, exact_ties=True) == (0, 2)
    assert wc.sign_rule_violations(bad, p, exact_ties=True)[0] >= 1
    # ... and the near-tie rule alone decides nothing here: the mutant is only visible where the tie is exact
    assert wc.sign_rule_violations(bad, p) == (0, 0)
