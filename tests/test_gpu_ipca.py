"""IncrementalPca (include/petal_hip_ipca.h) on a real MI355X, on the streaming kernel (k_gram_stream + k_ipca_merge; `info` must report
every batch as a kernel batch wherever d <= 1024): exact integer Gram matrices at every tile seam, the centred statistic against the
long-double reference inside its model-tied bound, model parity in 1, 3 and 7 batches, the sign rule, merge and state, determinism to
the byte and host against device input, the drifting stream, and the kernel path against the forced two-pass path.  Run with -m gpu."""
import numpy as np
import pytest

import ipca_cases as ic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import petal_decomposition_amd as petal
    c = petal.Context(0)          # raises (no CPU fallback) when the HIP library or the GPU is missing
    yield c
    c.close()


def _same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


# ------------------------------------------------------------------------------------------- 1. exact integers
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("d", ic.INT_WIDTHS_GPU)
def test_integer_gram_matrix_is_exact_after_every_batch(ctx, d, dt):
    ic.check_integers_exact(ctx, d, dt, expect_kernel=True)


# ------------------------------------------------------------------------------------------- 2. the centred statistic
@pytest.mark.parametrize("case", ic.STAT_CASES_GPU, ids=lambda c: c.name)
def test_centred_statistic_against_long_double(ctx, case):
    ic.check_statistic(ctx, case, expect_kernel=True)


def test_centred_statistic_from_device_batches(ctx):
    """torch tensors: d = 16 streams in place (zero copy), d = 33 is packed on the device; same bound"""
    ic.check_statistic(ctx, ic.STAT_CASES[3], expect_kernel=True, device=True)
    ic.check_statistic(ctx, ic.STAT_CASES[2], expect_kernel=True, device=True)


# ------------------------------------------------------------------------------------------- 3, 4. model parity and the sign rule
@pytest.mark.parametrize("centering", [True, False], ids=["centred", "uncentred"])
@pytest.mark.parametrize("case", ic.PARITY_CASES, ids=ic.parity_id)
def test_parity_in_one_three_and_seven_batches(ctx, case, centering):
    ic.check_parity(ctx, case, centering, expect_kernel=True)


def test_wider_than_the_kernel_reports_the_fallback_and_meets_the_bar(ctx):
    case = ic.PARITY_CASES_GPU[-1]
    assert case.d > ic.KERNEL_MAX_D and case.d % 16 == 0
    ic.check_parity(ctx, case, True, expect_kernel=False)


# ------------------------------------------------------------------------------------------- 5. merge and state
@pytest.mark.parametrize("case", ic.PARITY_CASES[:2], ids=ic.parity_id)
def test_merge_and_state(ctx, case):
    ic.check_merge_and_state(ctx, case, expect_kernel=True)


# ------------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("case", [ic.STAT_CASES_GPU[-1], ic.STAT_CASES_GPU[1]], ids=lambda c: c.name)
def test_same_batches_same_bytes_and_host_equals_device_input(ctx, case):
    """no atomics anywhere: the same batches in the same order give the same bytes on every run, from host arrays and from torch tensors
    (62 row chunks in one batch of the first case; d = 65, which a device batch reaches through the packing kernel, in the second)"""
    batches = ic.stat_inputs(case)
    runs = []
    for device in (False, False, True):
        m = ic.feed(ctx, batches, 3, True, device)
        assert m.info()["kernel_batches"] == len(batches)
        runs.append((m.state(), m.finalize()))
        m.close()
    for st, res in runs[1:]:
        assert _same(st["m2"], runs[0][0]["m2"]) and _same(st["mean"], runs[0][0]["mean"]) and st["n"] == runs[0][0]["n"]
        assert all(_same(a, b) for a, b in zip(res, runs[0][1]))


# ------------------------------------------------------------------------------------------- drift
def test_drifting_stream_stays_inside_its_bound(ctx):
    """8 batches of 500 x 16 float64, each batch's mean 40 sigma beyond the last: the statistic inside its model-tied bound (the
    model carries the same cancellation), the fitted model inside the 1e-9 bar; the loss is printed for DESIGN.md section 7, with the
    merge of per-batch handles -- the cancellation-free form -- beside it"""
    import petal_decomposition_amd as petal
    c = ic.DRIFT_CASE
    batches = ic.stat_inputs(c)
    ic.check_statistic(ctx, c, expect_kernel=True)
    ref = ic.reference_stat(batches)
    m = ic.feed(ctx, batches, 3)
    chunks = ic.merged_in_chunks(ctx, batches, 3)
    model = ic.model_stat(batches)
    for name, fit in (("batch by batch", m), ("per-batch handles merged", chunks)):
        err, merr, floor, ratio, _, top = ic.stat_errors(fit.state(), ref, model)
        within, of_top = ic.drift_loss(fit.state(), ref, c)
        print(f"drift, {name}: M2 error {of_top:.2f} eps64 of the largest diagonal entry = {within:.0f} eps64 n sigma_i sigma_j of the within-batch "
              f"spread (ratio to the model {ratio:.2f})")
        assert err <= ic.MULTIPLIER["drift"] * max(merr, floor)      # the merge is held to the bound of the recurrence it replaces
    x = np.concatenate(batches)
    _, s, vt = np.linalg.svd(x - x.mean(axis=0), full_matrices=False)
    want = (vt[:3], s[:3], x.mean(axis=0), float(np.sum(s * s)))
    for fit in (m, chunks):
        errs = ic.model_errors(ic.fitted(fit), want, 3)
        print(f"drift: model against numpy {errs}")
        assert max(errs) <= 1e-9
    assert isinstance(m, petal.IncrementalPca)
    m.close()
    chunks.close()


# ------------------------------------------------------------------------------------------- kernel path against fallback path
@pytest.mark.parametrize("case", [ic.STAT_CASES_GPU[0], ic.STAT_CASES_GPU[5], ic.DRIFT_CASE], ids=lambda c: c.name)
def test_kernel_path_against_the_forced_two_pass_path(ctx, case):
    batches = ic.stat_inputs(case)
    kernel = ic.feed(ctx, batches, 1)
    assert kernel.info()["kernel_batches"] == len(batches)
    ctx.set_option("ipca_fallback", 1)
    try:
        two_pass = ic.feed(ctx, batches, 1)
        assert two_pass.info()["kernel_batches"] == 0 and two_pass.info()["batches"] == len(batches)
    finally:
        ctx.set_option("ipca_fallback", 0)
    ref, model = ic.reference_stat(batches), ic.model_stat(batches)
    _, merr, floor, _, _, top = ic.stat_errors(kernel.state(), ref, model)
    bound = ic.MULTIPLIER[case.family] * max(merr, floor)
    diff = float(np.max(np.abs(kernel.state()["m2"] - two_pass.state()["m2"])))
    print(f"{case.name}: kernel path against two-pass path {diff / top:.2e} of the largest diagonal entry (twice the bound: {2 * bound / top:.2e})")
    assert diff <= 2 * bound
    kernel.close()
    two_pass.close()


# ------------------------------------------------------------------------------------------- 7. the inherited members
def test_model_members_match_pca_fit_on_the_concatenation(ctx):
    import petal_decomposition_amd as petal
    case = ic.PARITY_CASES[1]
    x = np.array(ic.parity_inputs(case))
    tol = ic.bar(case)
    whole = petal.Pca(case.k, ctx=ctx).fit(x)
    m = petal.IncrementalPca(case.k, ctx=ctx).fit(x, batch_size=700)
    assert m.info()["kernel_batches"] == 3 and m.n_samples == case.n
    assert np.allclose(m.explained_variance(), whole.explained_variance(), rtol=2 * tol, atol=0)
    assert np.isclose(m.noise_variance(), whole.noise_variance(), rtol=1e-4)
    sg = np.sign(np.sum(m.components().astype(np.float64) * whole.components(), axis=1))
    y, yw = m.transform(x), whole.transform(x)
    assert np.abs(y * sg - yw).max() <= 20 * tol * np.abs(yw).max()
    q, qw = m.reconstruction_error(x), whole.reconstruction_error(x)
    scale = float(np.max(np.sum((x - x.mean(axis=0)).astype(np.float64) ** 2, axis=1)))
    assert np.abs(q - qw).max() <= 20 * tol * scale
    # the scores with the variances in their denominators (noise variance 1e-4 here) magnify float32 rounding: they are held to the
    # model's own serde image instead -- the same components through the same kernel, to the byte: the members are inherited unchanged
    loaded = petal.Pca.from_json(m.to_json(), dtype=np.float32, ctx=ctx)
    assert _same(loaded.components(), m.components()) and _same(loaded.transform(x), y) and _same(loaded.reconstruction_error(x), q)
    assert _same(loaded.hotelling_t2(x), m.hotelling_t2(x)) and _same(loaded.score_samples(x), m.score_samples(x))
    m.close()
