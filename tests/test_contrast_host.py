"""The FastICA contrast functions (exp, cube) without a GPU: tests/contrast_cases.py's references and models against their own bounds on
the reduced table; what the host simulation -- which has the logcosh step only -- answers to the contrast field of `mode`; the
constants of the header, the Python facade and the Rust bindings; the register budgets of the new step kernels."""
import os
import re

import numpy as np
import pytest

import contrast_cases as cc
import header_kit as kit
import hostsim
import kernel_entry_cases as kc
from header_kit import resources  # noqa: F401  (the fixture)
import petal_decomposition_amd as petal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    c = hostsim.context()
    yield c
    c.close()


# ------------------------------------------------------------------------------------------- references, models, bounds
_STEP_CASES = [c for c in cc.all_cases(device=False, reduced=True) if c.fn is cc.step_check]


@pytest.mark.parametrize("case", _STEP_CASES, ids=repr)
def test_reference_and_model_stay_inside_the_bound(case):
    """The long-double certificates pass, the model -- the same statement in the precision under test -- is inside the bound that the
    library is held to, and that bound is not vacuous: neither with the multipliers in force nor with the starting values 4 / 16."""
    fun, n, nc, dt, kmax, seed, k = case.args
    outlier = case.kw.get("outlier", False)
    e_model, bound, cond_d, smax = cc.model_check(fun, n, nc, dt, kmax, seed, k, outlier)
    start = cc.bound_of(n, nc, dt, e_model, mult32=4.0, mult64=16.0)
    print(f"{case.id}: model {e_model:.3e}, bound {bound:.3e} (at 4 / 16: {start:.3e}), cond(D) {cond_d:.1f}, max |S| {smax:.2f}")
    assert e_model <= bound, (case.id, e_model, bound)
    assert bound <= start <= kc.GUARD, (case.id, bound, start)
    assert cond_d <= 5.8e3, (case.id, cond_d)
    if outlier:
        assert smax > 100.0, smax


def test_multipliers_never_exceed_the_starting_values():
    assert 1.0 < cc.MULT32 <= 4.0 and 1.0 < cc.MULT64 <= 16.0


def test_contrast_formulas():
    """g' is the derivative of g (central differences in long double), g(0) = 0, and g'(0) = 1, 1, 0: what the ragged-block bookkeeping
    of the step kernels rests on"""
    u = np.linspace(-4.0, 4.0, 161).astype(np.longdouble)
    h = np.longdouble(1e-6)
    for fun, gp0 in (("logcosh", 1.0), ("exp", 1.0), ("cube", 0.0)):
        g, gd = cc.contrast(fun, u)
        num = (cc.contrast(fun, u + h)[0] - cc.contrast(fun, u - h)[0]) / (2 * h)
        assert float(np.abs(num - gd).max()) < 1e-9, fun
        g0, gd0 = cc.contrast(fun, np.zeros(1, dtype=np.longdouble))
        assert float(g0[0]) == 0.0 and float(gd0[0]) == gp0, fun


# ------------------------------------------------------------------------------------------- the host simulation: logcosh only
def _small():
    return kc.ica_inputs(3000, 5, "f64", 22)


def test_explicit_logcosh_is_todays_result(ctx):
    x1, w0 = _small()
    a, na = petal.ica_par(x1, 1e-4, 200, w0, petal.ICA_TEXTBOOK, ctx)
    b, nb = petal.ica_par(x1, 1e-4, 200, w0, petal.ICA_TEXTBOOK | petal.ICA_CONTRAST_LOGCOSH, ctx)
    assert 1 < na < 200 and na == nb and a.tobytes() == b.tobytes()
    x = kc.po.synth_ica(2000, 6, 6, seed=3, dtype=np.float64)
    w = np.random.default_rng(4).standard_normal((6, 6))
    ya = petal.FastIca(ctx=ctx).fit_transform(x, w_init=w)
    yb = petal.FastIca(ctx=ctx, fun="logcosh").fit_transform(x, w_init=w)
    yc = petal.FastIcaBuilder().context(ctx).fun("logcosh").build().fit_transform(x, w_init=w)
    assert ya.tobytes() == yb.tobytes() == yc.tobytes()


@pytest.mark.parametrize("fun", cc.FUNS)
def test_host_simulation_refuses_other_contrasts(ctx, fun):
    """never silently a tanh fit: the device-op layer of the simulation has no such step, and says so"""
    x1, w0 = _small()
    with pytest.raises(petal.InvalidInput, match="contrast not available in this device-op layer"):
        petal.ica_par(x1, 0.0, 1, w0, cc.mode_of(fun), ctx)
    x = kc.po.synth_ica(500, 4, 4, seed=3, dtype=np.float64)
    with pytest.raises(petal.InvalidInput, match="contrast not available in this device-op layer"):
        petal.FastIca(ctx=ctx, fun=fun).fit(x, w_init=np.eye(4))


@pytest.mark.parametrize("mode", [48, 64, 240, 256, 16 | 512, -1])
def test_undefined_contrast_field_is_invalid_input(ctx, mode):
    x1, w0 = _small()
    with pytest.raises(petal.InvalidInput, match="FastICA"):
        petal.ica_par(x1, 0.0, 1, w0, mode, ctx)
    x = kc.po.synth_ica(500, 4, 4, seed=3, dtype=np.float64)
    m = petal.FastIca(ctx=ctx, mode=mode)
    with pytest.raises(petal.InvalidInput, match="FastICA"):
        m.fit(x, w_init=np.eye(4))


def test_semantics_reach_the_tail_without_the_contrast_bits(ctx):
    """REFERENCE_LITERAL | CONTRAST_LOGCOSH must stay the literal fit (the simulation tests `mode == 1`)"""
    x1, w0 = kc.ica_inputs(3000, 5, "f64", 22)
    lit, _ = petal.ica_par(x1, 0.0, 2, w0, petal.ICA_REFERENCE_LITERAL, ctx)
    txt, _ = petal.ica_par(x1, 0.0, 2, w0, petal.ICA_TEXTBOOK, ctx)
    both, _ = petal.ica_par(x1, 0.0, 2, w0, petal.ICA_REFERENCE_LITERAL | petal.ICA_CONTRAST_LOGCOSH, ctx)
    assert both.tobytes() == lit.tobytes()
    assert lit.tobytes() != txt.tobytes()       # (the two semantics do differ on this input: the line above is not vacuous)


# ------------------------------------------------------------------------------------------- constants and facades
def test_constants_agree_across_header_python_and_rust():
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "petal_hip.h")).read(), flags=re.S)
    ffi = re.sub(r"//.*$", "", open(os.path.join(ROOT, "rust", "petal-decomposition-hip", "src", "ffi.rs")).read(), flags=re.M)
    hconsts = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(PETAL_[A-Z_0-9]+)\s*=\s*(\d+)", header)}
    rconsts = {m.group(1): int(m.group(2)) for m in re.finditer(r"pub\s+const\s+(PETAL_\w+)\s*:\s*c_int\s*=\s*(\d+)", ffi)}
    want = {"PETAL_ICA_CONTRAST_LOGCOSH": 0, "PETAL_ICA_CONTRAST_EXP": 16, "PETAL_ICA_CONTRAST_CUBE": 32}
    for name, value in want.items():
        assert hconsts[name] == value and rconsts[name] == value, name
        assert getattr(petal, name[len("PETAL_"):]) == value, name
    assert hconsts["PETAL_ICA_SEMANTICS_MASK"] == rconsts["PETAL_ICA_SEMANTICS_MASK"] == petal.ICA_SEMANTICS_MASK == 15
    assert hconsts["PETAL_ICA_CONTRAST_MASK"] == rconsts["PETAL_ICA_CONTRAST_MASK"] == petal.ICA_CONTRAST_MASK == 240
    for value in want.values():
        assert value & petal.ICA_CONTRAST_MASK == value and value & petal.ICA_SEMANTICS_MASK == 0
    rust_ica = open(os.path.join(ROOT, "rust", "petal-decomposition-hip", "src", "ica.rs")).read()
    for name in want:
        assert f"ffi::{name}" in rust_ica, name
    assert re.search(r"pub fn contrast\(mut self, contrast: Contrast\) -> Self", rust_ica)


def test_builder_rejects_unknown_names():
    with pytest.raises(petal.InvalidInput, match="nope"):
        petal.FastIcaBuilder().fun("nope")
    with pytest.raises(petal.InvalidInput):
        petal.FastIca(fun="tanh")
    assert petal.FastIcaBuilder().fun("cube").build().fun == "cube"
    assert petal.FastIca().fun == "logcosh"


def test_mode_and_fun_cannot_both_name_a_contrast(ctx):
    x = kc.po.synth_ica(500, 4, 4, seed=3, dtype=np.float64)
    with pytest.raises(petal.InvalidInput, match="already carries a contrast"):
        petal.FastIca(ctx=ctx, mode=petal.ICA_CONTRAST_CUBE, fun="exp").fit(x, w_init=np.eye(4))
    # with the default fun the mode word goes through as it is: here to the simulation's refusal, not to a tanh fit
    with pytest.raises(petal.InvalidInput, match="contrast not available in this device-op layer"):
        petal.FastIca(ctx=ctx, mode=petal.ICA_TEXTBOOK | petal.ICA_CONTRAST_CUBE).fit(x, w_init=np.eye(4))


def test_json_form_is_untouched():
    """the crate's struct has no contrast field: the serde form of a model does not grow one"""
    import json
    m = petal.FastIca.with_seed(5)
    m.fun = "exp"
    assert sorted(json.loads(m.to_json())) == ["components", "means", "n_iter", "rng"]


def test_cpp_facade_on_host_simulation():
    kit.run_cpp_facade("contrast", "refuses", hostsim.build(), "hostsim")


# ------------------------------------------------------------------------------------------- kernel budgets
# the budgets of the logcosh kernels (tests/test_kernel_budgets.py): 32 components 4 waves / SIMD, 64 components the whole file
BUDGETS = [
    (r"k_ica3g<2, [12]>$", 128, 2), (r"k_ica3pg<2, [12]>$", 128, 2),
    (r"k_ica3g<4, [12]>$", 256, 2), (r"k_ica3pg<4, [12]>$", 256, 2),
    (r"k_ica3g<[13], [12]>$", 256, 4), (r"k_ica_mfma_g<[1-4], [12]>$", 256, 8),
    (r"k_ica_simple_g<(float|double), [12]>$", 256, 4), (r"k_contrast_inplace<(float|double), [12]>$", 256, 4),
]


@pytest.mark.parametrize("pattern,max_vgpr,count", BUDGETS, ids=[b[0] for b in BUDGETS])
def test_contrast_kernel_budget(resources, pattern, max_vgpr, count):
    hits = {k: v for k, v in resources.items() if re.search(pattern, k)}
    assert len(hits) == count, (pattern, sorted(hits))
    for name, r in hits.items():
        assert r["vgpr"] <= max_vgpr, f"{name}: {r['vgpr']} VGPRs > {max_vgpr}"
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
