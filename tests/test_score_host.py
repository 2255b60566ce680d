"""Row scores (include/petal_hip_score.h) without a GPU: tests/score_cases.py's references and models against their own bounds on the
reduced table; what the host simulation -- whose device-op layer has no score op -- answers, and in which order; the new header
against the built library, the Python table and the Rust binding; the facade's formulas against a float64 restatement of the
probabilistic-PCA log-density; the JSON form; the register budgets of the new kernels; the C++ facade."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import header_kit as kit
import hostsim
import score_cases as sc
from header_kit import resources  # noqa: F401  (the fixture)
import petal_decomposition_amd as petal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "petal_hip_score.h")
FFI = os.path.join(ROOT, "rust", "petal-decomposition-hip", "src", "ffi_score.rs")


@pytest.fixture(scope="module")
def ctx():
    c = hostsim.context()
    yield c
    c.close()


# ------------------------------------------------------------------------------------------- references, models, bounds
@pytest.mark.parametrize("case", sc.all_cases(reduced=True), ids=repr)
def test_reference_and_model_stay_inside_the_bound(case):
    """The model -- the statement in the precision under test -- is inside the bound the library is held to, with the multipliers in
    force; the planted q = 0 row is exactly zero in the reference; the bound says something (far below the size of q itself)."""
    em_res, em_w = sc.model_errors(case.key)
    b_res, b_w = sc.bounds(case.key)
    s_res, s_w = sc.bounds(case.key, mult32=4.0, mult64=16.0)
    print(f"{case.id}: model e_res {em_res:.3e} e_w {em_w:.3e}; bounds {b_res:.3e} {b_w:.3e} (at 4 / 16: {s_res:.3e} {s_w:.3e})")
    assert em_res <= b_res and em_w <= b_w
    assert b_res <= s_res <= 1e-4 and b_w <= s_w <= 1e-4
    res, wt, q = sc.reference(case.key)
    planted = sc.inputs(*case.key)[4]
    assert q[planted] == 0 and res[planted] == 0 and wt[planted] == 0
    assert np.all(res >= 0)
    if case.weights is None:   # residual + weighted = q
        assert float(np.abs(res + wt - q).max()) <= 1e-15 * float(q.max())


def test_multipliers_never_exceed_the_starting_values():
    assert 1.0 < sc.MULT32 <= 4.0 and 1.0 < sc.MULT64 <= 16.0


def test_the_table_reaches_every_path():
    cases = sc.all_cases()
    assert {c.n for c in cases} == {63, 64, 4099, 70033}
    assert {c.d for c in cases} == {16, 100, 256, 512, 1024}
    assert {1, 7, 64, 80, 81, 138} <= {c.k for c in cases} and any(c.k == c.d for c in cases)
    assert {c.dt for c in cases} == {"f32", "f64"} and not all(c.centering for c in cases)
    assert {c.weights for c in cases} == {None, "inv", "zeros"} and {c.layout for c in cases} == {"host", "hostF", "dev"}
    assert any(c.want_y for c in cases) and not all(c.want_y for c in cases)
    for dt in ("f32", "f64"):   # two column panels in both precisions, several workgroups each
        assert any(c.dt == dt and c.k > 80 and c.n > 256 for c in cases)


# ------------------------------------------------------------------------------------------- the host simulation
def _small(dt=np.float64):
    rng = np.random.default_rng(5)
    x = rng.standard_normal((40, 6)).astype(dt)
    comp = np.ascontiguousarray(np.linalg.qr(rng.standard_normal((6, 3)))[0].T.astype(dt))
    return x, comp, x.mean(axis=0).astype(dt)


def test_host_simulation_refuses_the_op(ctx):
    """never silently something else: the simulation's device-op layer has no score op, and says so"""
    x, comp, mu = _small()
    with pytest.raises(petal.InvalidInput, match="row scores not available in this device-op layer"):
        petal.score_rows(x, comp, mu, ctx=ctx)
    with pytest.raises(petal.InvalidInput, match="row scores not available in this device-op layer"):
        petal.score_rows(x, comp[:0], mu, ctx=ctx)            # (k = 0 is legal, and still the op's work)
    m = petal.Pca(3, ctx=ctx).fit(x)
    with pytest.raises(petal.InvalidInput, match="row scores not available in this device-op layer"):
        m.reconstruction_error(x)


def test_argument_errors_come_first(ctx):
    x, comp, mu = _small()
    with pytest.raises(petal.InvalidInput, match="# of columns should be 6"):
        petal.score_rows(x[:, :5], comp, mu, ctx=ctx)
    with pytest.raises(petal.InvalidInput, match="weights should be finite"):
        petal.score_rows(x, comp, mu, weights=[1.0, np.inf, 1.0], ctx=ctx)
    with pytest.raises(petal.InvalidInput, match="weights should be finite"):
        petal.score_rows(x, comp, mu, weights=[np.nan, 1.0, 1.0], ctx=ctx)
    m = petal.Pca(3, ctx=ctx).fit(x)
    with pytest.raises(petal.InvalidInput, match="# of columns should be 6"):
        m.hotelling_t2(x[:, :4])
    # the raw entry: shape and dtype of `out` / `y_out`
    keep = []
    mx = petal.describe(x, keep)

    def call(out, y=None, weights=None):
        mo = petal.describe(out, keep)
        my = petal.describe(y, keep) if y is not None else None
        rc = ctx.lib.petal_score_rows(ctx._h, C.byref(mx), comp.ctypes.data, mu.ctypes.data, 3, 6, 1, weights, C.byref(mo),
                                      C.byref(my) if my is not None else None)
        return rc, (ctx.lib.petal_last_error(ctx._h) or b"").decode()

    assert call(np.zeros((40, 3))) == (petal.PETAL_INVALID_INPUT, "output has the wrong shape")
    assert call(np.zeros((39, 2))) == (petal.PETAL_INVALID_INPUT, "output has the wrong shape")
    assert call(np.zeros((40, 2), dtype=np.float32)) == (petal.PETAL_INVALID_INPUT, "output dtype differs from input dtype")
    assert call(np.zeros((40, 2)), np.zeros((40, 4))) == (petal.PETAL_INVALID_INPUT, "output has the wrong shape")
    rc, msg = call(np.zeros((40, 2)), np.zeros((40, 3)))
    assert rc == petal.PETAL_INVALID_INPUT and "row scores not available" in msg


def test_no_rows_is_legal(ctx):
    x, comp, mu = _small()
    out, y = petal.score_rows(x[:0], comp, mu, want_y=True, ctx=ctx)
    assert out.shape == (0, 2) and y.shape == (0, 3)


# ------------------------------------------------------------------------------------------- the header, Python, Rust
def test_header_is_exported_and_bound_by_python():
    fns = kit.header_functions(HEADER)
    kit.check_python_table("petal_hip_score.h", fns, ["petal_score_rows"])
    kit.check_exported(fns, want_hip=True)
    assert '#include "petal_hip.h"' in open(HEADER).read()


def test_rust_binding_matches_the_header():
    assert kit.rust_functions(FFI) == kit.header_functions(HEADER)
    src = os.path.join(ROOT, "rust", "petal-decomposition-hip", "src")
    assert "mod ffi_score;" in open(os.path.join(src, "lib.rs")).read()
    pca = open(os.path.join(src, "pca.rs")).read()
    assert "ffi_score::petal_score_rows" in pca
    for name in ("explained_variance", "noise_variance", "reconstruction_error", "hotelling_t2", "score_samples"):
        assert len(re.findall(rf"pub fn {name}\b", pca)) == 2, name      # Pca and RandomizedPca


# ------------------------------------------------------------------------------------------- the facade's formulas
def _numpy_score_rows(x, components, means, weights=None, centering=True, want_y=False, ctx=None):
    """the statement in float64 numpy, standing in for the device op"""
    res, wt, _ = sc.statement(x, components, means, weights, centering, np.float64)
    return np.stack([res, wt], axis=1), None


@pytest.mark.parametrize("model", ["Pca", "RandomizedPca"])
def test_facade_formulas_against_the_ppca_density(ctx, monkeypatch, model):
    n, d, k = 300, 12, 4
    rng = np.random.default_rng(11)
    x = (rng.standard_normal((n, k)) * [5.0, 3.0, 2.0, 1.5]) @ np.linalg.qr(rng.standard_normal((d, k)))[0].T
    x += 0.3 * rng.standard_normal((n, d)) + 2.0
    m = petal.Pca(k, ctx=ctx) if model == "Pca" else petal.RandomizedPca.with_seed(k, 9, ctx=ctx)
    m.fit(x)
    xc = x - x.mean(axis=0)
    s = np.linalg.svd(xc, compute_uv=False)
    lam = m.explained_variance()
    np.testing.assert_allclose(lam, s[:k] ** 2 / (n - 1), rtol=1e-9)
    s2 = m.noise_variance()
    np.testing.assert_allclose(s2, (s[k:] ** 2).sum() / (n - 1) / (d - k), rtol=1e-8)
    monkeypatch.setattr(petal, "score_rows", _numpy_score_rows)
    v = m.components().astype(np.float64)
    y = xc @ v.T
    np.testing.assert_allclose(m.reconstruction_error(x), ((xc - y @ v) ** 2).sum(axis=1), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(m.hotelling_t2(x), (y * y / lam).sum(axis=1), rtol=1e-10)
    # probabilistic PCA: x ~ N(mu, C), C = V^T diag(lambda - s2) V + s2 I, as an explicit d x d covariance
    cov = v.T @ np.diag(lam - s2) @ v + s2 * np.eye(d)
    sign, logdet = np.linalg.slogdet(cov)
    assert sign > 0
    want = -0.5 * (d * np.log(2 * np.pi) + logdet + np.einsum("ij,ij->i", xc, np.linalg.solve(cov, xc.T).T))
    np.testing.assert_allclose(m.score_samples(x), want, rtol=1e-9)


def test_score_samples_needs_a_positive_noise_variance(ctx, monkeypatch):
    monkeypatch.setattr(petal, "score_rows", _numpy_score_rows)
    rng = np.random.default_rng(3)
    x = rng.standard_normal((50, 5))
    full = petal.Pca(5, ctx=ctx).fit(x)                       # k = min(n, d): nothing discarded
    assert full.noise_variance() == 0
    with pytest.raises(petal.InvalidInput, match="noise variance is not positive"):
        full.score_samples(x)
    low = rng.standard_normal((50, 2)) @ rng.standard_normal((2, 5))
    flat = petal.Pca(3, ctx=ctx).fit(low)                     # rank 2, three kept: a kept lambda is (numerically) zero
    flat._singular = np.array([flat._singular[0], flat._singular[1], 0.0])
    with pytest.raises(petal.InvalidInput):
        flat.score_samples(low)
    with pytest.raises(petal.InvalidInput, match="zero variance"):
        flat.hotelling_t2(low)


def test_json_form_is_unchanged(ctx):
    x, _, _ = _small()
    m = petal.Pca(3, ctx=ctx).fit(x)
    assert sorted(json.loads(m.to_json())) == ["centering", "components", "means", "n_samples", "singular", "total_variance"]
    r = petal.RandomizedPca.with_seed(3, 1, ctx=ctx).fit(x)
    assert sorted(json.loads(r.to_json())) == ["centering", "components", "means", "n_samples", "rng", "singular", "total_variance"]
    back = petal.Pca.from_json(m.to_json(), dtype=np.float64, ctx=ctx)
    np.testing.assert_array_equal(back.explained_variance(), m.explained_variance())
    assert back.noise_variance() == m.noise_variance()


def test_cpp_facade_on_host_simulation():
    kit.run_cpp_facade("score", "refuses", hostsim.build(), "hostsim")


# ------------------------------------------------------------------------------------------- kernel budgets
# the new kernel -> the kernel it derives from, in the instantiation petal_transform launches (no sum of squares): no occupancy step lost
# against it, no scratch, no spills.  The fp32-MFMA form has no uncentred 3-tile instantiation: it would take 194 registers, two waves per
# SIMD against three of k_xp_mfma<4, 3, false, false>, so the launcher never forms such a panel (test_no_uncentred_three_tile_form).
COUNTERPARTS = (
    [(f"k_xp3s<{nt}, {c}>", f"k_xp3<4, {nt}, 1, {c}, 4, 2, 3, false>") for nt in range(1, 6) for c in ("true", "false")] +
    [(f"k_xp_mfma_s<{nt}, {c}, {2 if nt == 1 else 4}>", f"k_xp_mfma<4, {nt}, {c}, false>") for nt in range(1, 5) for c in ("true", "false")
     if (nt, c) != (3, "false")] +
    [(f"k_xp_f64s<{nt}, {c}>", f"k_xp_f64<{nt}, {c}, false>") for nt in range(1, 6) for c in ("true", "false")] +
    [(f"k_xp_simple_s<{t}>", f"k_xp_simple<{t}>") for t in ("float", "double")])


def test_no_uncentred_three_tile_form(resources):
    names = [k for k in resources if "k_xp_mfma_s<" in k]
    assert len(names) == 7 and not any("k_xp_mfma_s<3, false" in k for k in names), names


@pytest.mark.parametrize("new,old", COUNTERPARTS, ids=[c[0] for c in COUNTERPARTS])
def test_score_kernel_budget(resources, new, old):
    a, b = resources["void petal::" + new], resources["void petal::" + old]
    assert a["scratch"] == 0 and a["vgpr_spill"] == 0 and a["sgpr_spill"] == 0, (new, a)
    assert a["waves_per_simd"] >= b["waves_per_simd"], (new, a["vgpr"], old, b["vgpr"])
