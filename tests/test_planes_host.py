"""tests/plane_cases.py without a GPU: what is proved here is the TEST.  1. every case's certificate holds (the pieces re-add, x - mu is
exact, at least half of every call's elements are in the exact class, the rotation covers what it claims).  2. the faithful numpy model
of the piece products -- float32 accumulation in a shuffled order -- passes the very assertion the device result is given to.  3. every
mutant of that model (a lower piece product dropped, m and l swapped, l aliased to m, a lower plane read one lane group further) FAILS it
in at least one case of every kernel's table: a subtly wrong kernel would be noticed.  4. a reduced table runs through the host
simulation with the steering hook on and off, which pins oracle/cpu_ops.cpp's two-plane rounding against the numpy split."""
import numpy as np
import pytest

import hostsim
import plane_cases as pl


@pytest.mark.parametrize("table", list(pl.TABLES))
def test_certificates_and_the_faithful_model(table):
    runner = pl.ModelRunner()
    for case in pl.TABLES[table]():
        calls, exact, bad, bounded, ratio = case.run(runner)
        assert 1 <= calls <= pl.MAX_CALLS and exact > 0 and bad == 0 and ratio <= 1.0, (case.id, calls, exact, bad, bounded, ratio)


def test_split_pieces_and_granularity():
    rng = np.random.default_rng(1)
    x = pl.bbit(rng, (4096,), 24, rng.integers(-20, 21, 4096))
    (h, m, l), val = pl.planes(x)
    assert np.array_equal(val, x)
    for piece in (h, m, l):      # every piece is a bf16 number: at most 8 significant bits
        assert np.all(np.abs(piece.astype(np.float64)) / pl.gran(np.where(piece == 0, 1, piece)) < 256.5)
    assert np.all(np.abs(x - pl.split2(x)) <= np.abs(x) * 2.0 ** -16)
    x16 = pl.bbit(rng, (4096,), 16, rng.integers(-20, 21, 4096))
    assert np.array_equal(pl.split2(x16), x16)      # 16 bits live on two planes
    assert np.array_equal(pl.gran(np.array([0.0, 1.0, 6.0, 0.375, -80.0])), [np.inf, 1.0, 2.0, 0.125, 16.0])


def test_a_design_over_budget_is_not_certified():
    """22 bits x 8 terms over two binades: sum |terms| >= 2^24 q, the certificate refuses the elements (their fp32 sum depends on the order)"""
    rng = np.random.default_rng(2)
    u = pl.bbit(rng, (8, 4), 22, rng.integers(0, 2, (8, 1)) * np.ones((1, 4), dtype=np.int64))
    v = np.ones((8, 3), dtype=np.float32)
    p = pl.Product("over", u, v)
    with pytest.raises(AssertionError, match="fewer than half"):
        p.analyse()


def _small_cases(table):
    return [c for c in pl.TABLES[table]() if c.small and not c.hook][:16]


@pytest.mark.parametrize("table", list(pl.TABLES))
def test_every_mutant_is_killed_in_every_kernel_table(table):
    cases = _small_cases(table)
    assert cases
    for mutant in pl.MUTANTS:
        killed = []
        for case in cases:
            try:
                _run_some(case, mutant)
            except AssertionError as e:
                if "certified-exact elements differ" in str(e):
                    killed.append(case.id)
                    break
                raise
        assert killed, f"{table}: the mutant {mutant.name} survives every small case"


def _run_some(case, mutant):
    """the first calls of a case on the mutated model (the coverage of the whole rotation is not the point here)"""
    case.setup()
    runner = pl.ModelRunner(mutant)
    for c in range(3):
        call = case.call(c)
        products = case.products(call, runner.forms(call, False))
        case.check(call, products, runner.execute(call, products), f"{case.id} [{mutant.name}] call {c}:")


def test_a_mismatch_names_the_position_and_the_plane():
    case = pl.K1Case("k1", 64, 32, 16, "x24")
    with pytest.raises(AssertionError) as e:
        _run_some(case, pl.MUTANTS[4])      # the l h' piece product dropped
    msg = str(e.value)
    assert "out[" in msg and "mod 32" in msg and "chunk" in msg and "drop-lh'" in msg, msg


@pytest.fixture(scope="module")
def sim():
    c = hostsim.context()
    c.set_gemm_mode("bf16x3")      # (the simulation rounds to two planes where the split-product kernels do)
    yield c
    c.close()


def _sim_cases():
    out = []
    for d in pl.SINGLE + ["multi"]:
        out += [pl.K1Case("k1", 64, 32, 16, d), pl.K1Case("k1", 333, 48, 74, d, centred=True, bias=True, hook=True),
                pl.K1Case("k1", 777, 80, 138, d, centred=True, bias=True, hook=True),
                pl.K2Case(256, 64, 80, d, "a"), pl.K2Case(777, 32, 138, d, "a", hook=True, p4_shape=True), pl.K2Case(256, 64, 80, d, "both")]
    for d in ["mixed", "p16", "multi"]:
        out += [pl.FusedCase(96, 256, 16, d), pl.FusedCase(96, 256, 48, d, centred=True, want_z=True), pl.FusedCase(96, 256, 74, d, centred=True, hook=True)]
    out += [pl.GramCase(64, 64, "mixed"), pl.GramCase(64, 64, "multi", centred=True)]
    return out      # (the simulation has no score operation: tests/test_score_host.py covers that entry's host side)


@pytest.mark.parametrize("case", _sim_cases(), ids=repr)
def test_planes_on_the_host_simulation(sim, case):
    """the simulation multiplies in float64: every certified-exact element must come out exactly, with the operands rounded to two planes
    where the hook asks for a steering form -- cpu_ops.cpp's two_plane against the numpy split2"""
    calls, exact, bad, bounded, ratio = case.run(pl.DeviceRunner(sim, split=True, sim=True))
    assert exact > 0 and bad == 0 and ratio <= 1.0
    assert sim.get_option("steering_hook") == 0


def test_the_default_build_steers_with_four_piece_products():
    """the steering cases assume PETAL_STEER_PIECES = 4 (h h', h m', m h', m m'): the source's default, and the build defines no macros"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "petal-decomposition_amd", "csrc", "kernels", "k_gemm_split_k1.inc")).read()
    assert re.search(r"#ifndef PETAL_STEER_PIECES\s*\n#define PETAL_STEER_PIECES 4\b", src)
    assert "-D" not in open(os.path.join(root, "petal-decomposition_amd", "build.py")).read()
