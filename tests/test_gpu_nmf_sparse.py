"""Nmf on sparse CSR data (include/petal_hip_nmf_sparse.h) on the MI355X: the sweep k_nmf_sweep / k_nmf_sweep_split / k_nmf_gram
through petal_nmf_sweep_csr -- exact operands bit for bit over the load, item and split seams on both images, real data against
numpy.longdouble inside the model-tied bound -- and Nmf itself on a resident CsrMatrix: fit, fit_transform and transform against the
numpy model on the densified matrix, the stopping rule, the random initialisation, the same bytes twice and on a second handle, the
forced fall-back, k > 64, the densify limit, every error, the workspace count."""

import numpy as np
import pytest

import header_kit as kit
import nmf_sparse_cases as ns
import petal_decomposition_amd as petal
from sparse_cases import densify, to_csr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = petal.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------- 1. exact operands
@pytest.mark.parametrize("inner", ns.INT_INNER)
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("which", range(-1, len(ns.INT_SHAPES)), ids=lambda w: "seams" if w < 0 else "x".join(map(str, ns.INT_SHAPES[w])))
def test_sweep_on_exact_operands(ctx, which, dt, inner):
    ns.check_sweep_exact(ctx, which, dt, inner, expect_kernel=True)


# ------------------------------------------------------------------------------------------- 2. long double
@pytest.mark.parametrize("case", ns.SWEEP_CASES, ids=lambda c: c.name)
def test_sweep_against_long_double(ctx, case):
    ns.check_sweep_against_long_double(ctx, case, expect_kernel=True)


# ------------------------------------------------------------------------------------------- 3. fits
@pytest.mark.parametrize("case", ns.FIT_CASES, ids=lambda c: c.name)
def test_fit_matches_the_model(ctx, case):
    ns.check_fit_against_model(ctx, case, expect_kernel=True)


@pytest.mark.parametrize("case", ns.FIT_CASES[2:3] + ns.FIT_CASES[-1:], ids=lambda c: c.name)
def test_duck_typed_csr_is_accepted(ctx, case):
    ns.check_fit_against_model(ctx, case, expect_kernel=True, duck=True)


@pytest.mark.parametrize("updates", [13, 200])
@pytest.mark.parametrize("case", ns.FIT_CASES[:1] + ns.FIT_CASES[15:16] + ns.FIT_CASES[-2:], ids=lambda c: c.name)
def test_transform_matches_the_model(ctx, case, updates):
    ns.check_transform(ctx, case, expect_kernel=True, updates=updates)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_dense_entries_at_48_padded_components(ctx, dt):
    """k = 33 .. 48 pads to 48 components in the dense entries, which k_nmf_pass has no form for: the dense fit and the dense transform of
    a CSR-fitted model take the composed path there, correctly (the sweep pads to 64 and runs)"""
    c = ns.FitCase(f"{dt}-260x300-k33-it3", 260, 300, 33, dt, 3, 0.0, "same", 0.0)
    x, w0, h0, xq = ns.fit_inputs(c.n, c.d, c.k, c.dt)
    mo = ns.fit_model(c)
    m = ns.make(ctx, c)
    w = m.fit_transform(np.array(x), W=w0, H=h0)
    wq = m.transform(np.array(xq))
    assert m.info()["fit_kernel"] == 0 and m.info()["transform_kernel"] == 0
    got = (ns.rel_max(w, mo.w), ns.rel_max(m.components, mo.h), abs(m.reconstruction_err - mo.err) / mo.err,
           ns.rel_max(wq, ns.model_transform(xq, mo.h, c.k, c.max_iter)))
    assert max(got) <= ns.tol_of(dt), got


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_random_init_draws_from_the_pcg_stream(ctx, dt):
    ns.check_random_init(ctx, dt, expect_kernel=True)


# ------------------------------------------------------------------------------------------- 4. the stopping rule
@pytest.mark.parametrize("case", ns.STOP_CASES, ids=lambda c: c.name)
def test_stopping_rule(ctx, case):
    ns.check_stopping_rule(ctx, case, expect_kernel=True)


# ------------------------------------------------------------------------------------------- 5. determinism
@pytest.mark.parametrize("case", ns.FIT_CASES[2:3] + ns.FIT_CASES[-1:], ids=lambda c: c.name)
def test_same_fit_twice_and_on_a_second_handle_gives_the_same_bytes(ctx, case):
    ns.check_same_bytes_twice(ctx, case)


def test_same_sweep_twice_gives_the_same_bytes(ctx):
    """kp = 64 on a matrix with several split rows: the partial rows are added in item order, the slabs of the Gram matrix in workgroup
    order"""
    rng = np.random.default_rng(3)
    x = rng.random((40, 900)) * (rng.random((40, 900)) < 0.5)
    g, f = rng.random((40, 64)), rng.random((900, 64))
    runs = []
    for _ in range(2):
        sx = ns.csr(ctx, *to_csr(x), x.shape, "f32")
        assert sx.info()["items"] >= 2 * 40                     # every row is split
        runs.append(petal.nmf_sweep(sx, g, f, l1=0.1, inner_iters=2))
        sx.close()
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes() and runs[0][2] == runs[1][2]
    mg, mgram, mdot = ns.model_sweep(x.astype(np.float32), g, f, 0.1, 0.0, 2)
    assert max(ns.rel_max(runs[0][0], mg), ns.rel_max(runs[0][1], mgram), abs(runs[0][2] - mdot) / mdot) <= 1e-12


# ------------------------------------------------------------------------------------------- 6. the fall-back
@pytest.mark.parametrize("case", ns.FIT_CASES[1:2] + ns.FIT_CASES[-1:], ids=lambda c: c.name)
def test_forced_fallback_is_the_dense_fit_and_agrees_with_the_sweep(ctx, case):
    x, w0, h0, _ = ns.fit_inputs(case.n, case.d, case.k, case.dt)
    sx = ns.csr(ctx, *to_csr(x), x.shape)
    try:
        m = ns.make(ctx, case)
        w = m.fit_transform(sx, W=w0, H=h0)
        assert m.kernel_path == 1
    finally:
        sx.close()
    ctx.set_option("nmf_fallback", 1)
    try:
        f = ns.check_fallback_equals_dense(ctx, case)
        assert f.info()["fit_kernel"] == 0
        wf = f.fit_transform(ns.Duck(*to_csr(x), x.shape), W=w0, H=h0)
    finally:
        ctx.set_option("nmf_fallback", 0)
    tol = ns.tol_of(case.dt)
    assert max(ns.rel_max(wf, w), ns.rel_max(f.components, m.components)) <= tol
    assert abs(f.reconstruction_err - m.reconstruction_err) <= tol * m.reconstruction_err


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_more_than_64_components_densify(ctx, dt):
    c = ns.FitCase(f"{dt}-260x300-k65", 260, 300, 65, dt, 3, 0.0, "same", 0.0)
    m = ns.check_fallback_equals_dense(ctx, c)
    mo = ns.fit_model(c)
    assert max(ns.rel_max(m.components, mo.h), abs(m.reconstruction_err - mo.err) / mo.err) <= ns.tol_of(dt)


def test_dense_image_beyond_the_limit_is_refused(ctx):
    """65536 x 65537 float32 is more than 2^32 bytes: refused before anything is allocated"""
    rows, cols = 65536, 65537
    indptr = np.zeros(rows + 1, dtype=np.int64)
    indptr[1:] = 3
    sx = petal.CsrMatrix(np.ones(3, dtype=np.float32), np.array([0, 5, 9], dtype=np.int32), indptr, (rows, cols), ctx=ctx)
    try:
        before = ctx.workspace_in_use()
        for kw, k in (({}, 65), ({"nmf_fallback": 1}, 2)):
            for opt, v in kw.items():
                ctx.set_option(opt, v)
            try:
                with ns.raises_with(petal.InvalidInput, "too large to densify"):
                    petal.Nmf(k, max_iter=1, init="random", ctx=ctx).fit(sx)
                with ns.raises_with(petal.InvalidInput, "at most 64 components"):
                    petal.Nmf(k, max_iter=1, init="random", ctx=ctx).fit(sx)
            finally:
                for opt in kw:
                    ctx.set_option(opt, 0)
        assert ctx.workspace_in_use() == before
        m = petal.Nmf(2, max_iter=1, init="random", ctx=ctx).fit(sx)          # the sweep takes it
        assert m.kernel_path == 1
        m.close()
    finally:
        sx.close()


# ------------------------------------------------------------------------------------------- 7. errors and lifetime
def test_errors_and_workspace(ctx):
    def sharded():
        other = petal.Context(0)
        holder = []

        def make(data, indices, indptr, shape):
            sx = petal.CsrMatrix(data, indices, indptr, shape, ctx=other)
            other.set_collective(lambda *a: 0, 0, 2)
            holder.append(sx)
            return sx
        return other, make
    base = ctx.workspace_in_use()
    m = ns.check_errors(ctx, lambda: petal.Context(0), sharded)
    blocks, nbytes = ctx.workspace_in_use()
    assert blocks == base[0] + 2 and nbytes > base[1]            # the live model holds H and H H^T, nothing else is out
    m.close()
    assert ctx.workspace_in_use() == base
    x = ns.fit_inputs(260, 300, 5, "f32")[0]
    sx = ns.csr(ctx, *to_csr(x), x.shape)
    held = ctx.workspace_in_use()
    assert held[0] > base[0]
    m = petal.Nmf(5, max_iter=3, tol=0.0, init="random", ctx=ctx)
    m.fit_transform(sx)
    m.transform(sx)
    assert ctx.workspace_in_use()[0] == held[0] + 2
    m.close()
    assert ctx.workspace_in_use() == held
    sx.close()
    assert ctx.workspace_in_use() == base


# ------------------------------------------------------------------------------------------- 8. the C++ facade
def test_cpp_facade_on_gpu():
    """tests/cpp/nmf_sparse_facade_tests.cpp against libpetal_hip.so: the C++ facade's Nmf on a CsrMatrix with k_nmf_sweep (the CPU suite
    runs the same program against the host simulation's densifying path)"""
    kit.run_cpp_facade("nmf_sparse", "kernel", kit.HIP_LIBRARY, "hip")
