"""Row scores (petal_score_rows, include/petal_hip_score.h) on a real MI355X, in both GEMM modes: every case of tests/score_cases.py
against its bound, run-to-run and host / device output determinism to the byte, the projections against petal_transform's, the
q = residual + weighted identity against an independent k = 0 call, and the Pca / RandomizedPca members on 20000 x 512 fits.
Run with -m gpu."""
import numpy as np
import pytest

import header_kit as kit
import score_cases as sc

pytestmark = pytest.mark.gpu
LD = np.longdouble


@pytest.fixture(scope="module", params=["bf16x3", "fp32"])
def ctx(request):
    import petal_decomposition_amd as petal
    c = petal.Context(0)          # raises (no CPU fallback) when the HIP library or the GPU is missing
    c.set_gemm_mode(request.param)
    c.gemm_mode_name = request.param
    yield c
    c.close()


# (references and models do not depend on the GEMM mode: score_cases caches them per case)
@pytest.mark.parametrize("case", sc.all_cases(), ids=repr)
def test_scores_within_bound(ctx, case):
    sc.check(case, ctx)


def _case(n, d, k, dt, **kw):
    hits = [c for c in sc.all_cases() if (c.n, c.d, c.k, c.dt) == (n, d, k, dt) and all(getattr(c, a) == v for a, v in kw.items())]
    assert hits
    return hits[0]


# one case per kernel: any-shape, split-product / fp32-MFMA with one and with two panels, fp64 with one and two panels
_PATHS = [(63, 100, 7, "f32"), (4099, 512, 64, "f32"), (4099, 512, 81, "f32"), (4099, 1024, 138, "f32"), (4099, 512, 64, "f64"),
          (4099, 256, 81, "f64")]


@pytest.mark.parametrize("row", _PATHS, ids=repr)
def test_two_identical_calls_give_identical_bytes(ctx, row):
    case = _case(*row)
    a, ya = sc.run(case, ctx)
    b, yb = sc.run(case, ctx)
    assert a.tobytes() == b.tobytes()
    if ya is not None:
        assert ya.tobytes() == yb.tobytes()


@pytest.mark.parametrize("row", [(4099, 512, 64, "f32"), (4099, 512, 81, "f32"), (4099, 256, 81, "f64")], ids=repr)
def test_host_and_device_outputs_are_identical(ctx, row):
    """the same rows through a host matrix (staged in, results copied out) and a device tensor (streamed in place, results written by
    the kernel into the caller's tensor)"""
    import torch
    import petal_decomposition_amd as petal
    case = _case(*row, layout="host")
    x, comp, mu, w, _ = sc.inputs(*case.key)
    h, yh = petal.score_rows(x, comp, mu, weights=w, centering=case.centering, want_y=True, ctx=ctx)
    d, yd = petal.score_rows(torch.from_numpy(np.array(x)).cuda(), comp, mu, weights=w, centering=case.centering, want_y=True, ctx=ctx)
    assert d.is_cuda and yd.is_cuda
    assert h.tobytes() == d.cpu().numpy().tobytes()
    assert yh.tobytes() == yd.cpu().numpy().tobytes()
    # a strided device `out` (a column pair of a wider tensor) takes the same values
    wide = torch.zeros((case.n, 5), dtype=d.dtype, device="cuda")
    keep = []
    import ctypes as C
    mx, mo = petal.describe(torch.from_numpy(np.array(x)).cuda(), keep), petal.describe(wide[:, 1:3], keep)
    wh = petal._host(w, mx.dtype) if w is not None else None
    ctx.check(ctx.lib.petal_score_rows(ctx._h, C.byref(mx), comp.ctypes.data, mu.ctypes.data, case.k, case.d, int(case.centering),
                                       wh.ctypes.data if wh is not None else None, C.byref(mo), None))
    got = wide.cpu().numpy()
    assert got[:, 1:3].tobytes() == h.tobytes() and not got[:, [0, 3, 4]].any()


@pytest.mark.parametrize("case", [c for c in sc.all_cases() if c.want_y], ids=repr)
def test_projections_are_transforms_bytes(ctx, case):
    import petal_decomposition_amd as petal
    x, comp, mu, w, _ = sc.inputs(*case.key)
    _, y = sc.run(case, ctx)
    m = petal.Pca(case.k, centering=case.centering, ctx=ctx)
    m._store(comp, mu, np.ones(case.k, dtype=comp.dtype), np.ones(1, dtype=comp.dtype), case.n)
    t = sc.to_numpy(m.transform(sc.laid_out(case, x)))
    assert y.tobytes() == t.tobytes()


@pytest.mark.parametrize("row", [(4099, 512, 64, "f32"), (4099, 1024, 138, "f64"), (64, 256, 80, "f32"), (4099, 256, 1, "f32")], ids=repr)
def test_residual_plus_weighted_is_q(ctx, row):
    """weights = None: residual + weighted = q, with q from an independent call without components (k = 0: residual = q, weighted = 0).
    Both the k = 0 call's q and the sum are held to the residual bound itself: without weights the kernels deliver weighted = sum y^2, the
    very number they subtracted, so the sum is q less a rounding or two."""
    import petal_decomposition_amd as petal
    case = _case(*row, weights=None)
    x, comp, mu, _, _ = sc.inputs(*case.key)
    out, _ = petal.score_rows(x, comp, mu, centering=case.centering, ctx=ctx)
    q0, _ = petal.score_rows(x, comp[:0], mu, centering=case.centering, ctx=ctx)
    assert not q0[:, 1].any()
    _, _, q = sc.reference(case.key)
    b_res, _ = sc.bounds(case.key)
    live = q > 0
    e_q = float((np.abs(q0[live, 0].astype(LD) - q[live]) / q[live]).max())
    e_sum = float((np.abs(out[live, 0].astype(LD) + out[live, 1].astype(LD) - q0[live, 0].astype(LD)) / q[live]).max())
    print(f"{case.id} {ctx.gemm_mode_name}: q error {e_q:.3e}, |res + wt - q| / q {e_sum:.3e} (bound {b_res:.3e})")
    assert e_q <= b_res and e_sum <= b_res
    assert not q0[~live].any()


# ------------------------------------------------------------------------------------------- the models' members
FIT_N, FIT_D, FIT_K = 20000, 512, 16


def _fit(ctx, model):
    import petal_decomposition_amd as petal
    x = sc.inputs(FIT_N, FIT_D, FIT_K, "f32", 1e-2, True, None, 3)[0]
    m = petal.Pca(FIT_K, ctx=ctx) if model == "Pca" else petal.RandomizedPca.with_seed(FIT_K, 7, ctx=ctx)
    m.fit(x)
    return m, x


@pytest.mark.parametrize("model", ["Pca", "RandomizedPca"])
def test_model_scores(ctx, model):
    """reconstruction_error against the long-double statement (the score bound), and against the composition it replaces,
    |x - inverse_transform(transform(x))|^2 through the library: within the score bound plus the composition's own bound -- MULT32
    max(its float32 numpy model's error, eps), the model being y = xc V^T, xr = y V + mu, sum (x - xr)^2 with every array in float32
    against the same in long double -- plus the distance between the two statements in long double (V, a float32 fit, is orthonormal
    to rounding only).  All relative to q.  score_samples against the float64 density with an explicit d x d covariance
    C = V^T diag(lambda - s2) V + s2 I: the two score bounds carried through the formula, plus 8 |V V^T - I|_2 q / s2 for that same defect."""
    m, x = _fit(ctx, model)
    v, mu = m.components(), m.mean()
    eps = float(np.finfo(np.float32).eps)
    lam = np.asarray(m.explained_variance(), dtype=np.float64)
    s2 = float(m.noise_variance())
    assert s2 > 0 and np.all(lam > s2)
    w = (1.0 / lam).astype(np.float32)
    # the statement: reference, model, bound
    res_ld, wt_ld, q = sc.statement(x, v, mu, w, True, LD)
    res_32, wt_32, _ = sc.statement(x, v, mu, w, True, np.float32)
    wmax = float(w.max())
    b_res = sc.MULT32 * max(float((np.abs(res_32 - res_ld) / q).max()), eps)
    b_w = sc.MULT32 * max(float((np.abs(wt_32 - wt_ld) / (q * wmax)).max()), eps)
    r = m.reconstruction_error(x)
    t2 = m.hotelling_t2(x)
    e_res = float((np.abs(r - res_ld) / q).max())
    e_w = float((np.abs(t2 - wt_ld) / (q * wmax)).max())
    # the composition
    xl, vl, mul = x.astype(LD), v.astype(LD), mu.astype(LD)
    comp_ld = ((xl - ((np.einsum("ij,kj->ik", xl - mul, vl)) @ vl + mul)) ** 2).sum(axis=1)
    xc32 = x - mu
    comp_32 = ((x - ((xc32 @ v.T) @ v + mu)) ** 2).sum(axis=1, dtype=np.float32)
    b_comp = sc.MULT32 * max(float((np.abs(comp_32 - comp_ld) / q).max()), eps)
    d_stmt = float((np.abs(comp_ld - res_ld) / q).max())
    xr = m.inverse_transform(m.transform(x))
    comp_lib = ((x.astype(np.float64) - xr.astype(np.float64)) ** 2).sum(axis=1)
    e_comp = float((np.abs(r - comp_lib) / q).max())
    print(f"{model} {ctx.gemm_mode_name}: e_res {e_res:.3e} (bound {b_res:.3e}), e_w {e_w:.3e} (bound {b_w:.3e}), against the composition "
          f"{e_comp:.3e} (bound {b_res + b_comp + d_stmt:.3e}: composition {b_comp:.3e}, statements apart {d_stmt:.3e})")
    assert e_res <= b_res and e_w <= b_w
    assert e_comp <= b_res + b_comp + d_stmt
    # score_samples
    v64, xc = v.astype(np.float64), x.astype(np.float64) - mu.astype(np.float64)
    cov = v64.T @ np.diag(lam - s2) @ v64 + s2 * np.eye(FIT_D)
    sign, logdet = np.linalg.slogdet(cov)
    assert sign > 0
    want = -0.5 * (FIT_D * np.log(2 * np.pi) + logdet + np.einsum("ij,ij->i", xc, np.linalg.solve(cov, xc.T).T))
    defect = float(np.linalg.norm(v64 @ v64.T - np.eye(FIT_K), 2))
    q64 = q.astype(np.float64)
    tol = 0.5 * (b_res * q64 / s2 + b_w * q64 * wmax) + 8 * defect * q64 / s2 + 1e-9 * np.abs(want)
    ll = m.score_samples(x)
    worst = float((np.abs(ll - want) / tol).max())
    print(f"{model} {ctx.gemm_mode_name}: score_samples worst |error| / tolerance {worst:.3f} (|V V^T - I| {defect:.2e}, median tolerance {np.median(tol):.2e}, median |ll| {np.median(np.abs(want)):.1f})")
    assert worst <= 1.0
    # a device tensor in, device tensors out, the same values
    import torch
    rd = m.reconstruction_error(torch.from_numpy(np.array(x)).cuda())
    assert rd.is_cuda and rd.cpu().numpy().tobytes() == np.ascontiguousarray(r).tobytes()


def test_cpp_facade_on_gpu():
    """tests/cpp/score_facade_tests.cpp against libpetal_hip.so: the five members of the C++ facade's Pca / RandomizedPca against their
    definitions (the CPU suite runs the same program against the host simulation, where the op refuses)"""
    kit.run_cpp_facade("score", "scores", kit.HIP_LIBRARY, "hip")
