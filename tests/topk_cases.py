"""The top-k subspace eigen-solver (csrc/algo.cpp::topk_eigh, reached through gram_topk_eigh and gram_eigen: exact Pca, FastICA's
whitening, IncrementalPca, the wide Pca and KernelPca take their eigenpairs from it) and its one-launch residual verdict
(k_ritz_residual), each through a probe entry of its own (include/petal_hip_probe.h: petal_probe_topk_eigh, petal_probe_ritz_residual),
against long-double references.  Shared by tests/test_gpu_topk.py (the HIP library, the full table) and tests/test_topk_hostsim.py
(the host simulation, a reduced table: it proves references, certificates and bounds without a GPU and holds oracle/cpu_ops.cpp to the
same contract).  The layout, the references (orth_ld, planted), the floors and _bound's rules are those of tests/smallmat_cases.py.

Section A -- op_ritz_residual.  Small-integer operands: every sum of squares is exact in any order, so out3[0], out3[1] and w_out are
  held bit for bit, and w_out behind nc to the probe's NaN fill.  Real operands: against long double with the DERIVED bound of the
  statement sum_i (cv_i - theta vr_i)^2 -- the term t_i = cv_i - theta vr_i carries e_i = 1.01 u (|cv_i| + 2 |theta vr_i|) (a product
  and a difference; a fused multiply-add carries less), its square 2 |t_i| e_i + e_i^2, and the rows-term sum 1.01 (rows + 1) u sum
  (|t_i| + e_i)^2 in any order (16 partial sums added through LDS, or one loop) -- reported as a fraction of it, bound 1.  The operands
  are those of a converged step, cv = theta vr + a residual 1e-3 of it, where the cancellation makes the bound bite.
Section B -- the shapes topk_applies takes and refuses.
Section C -- outcome classes.  C = planted(lam); the MODEL (model()) restates topk_eigh in numpy float64: the same 64-bit LCG start
  block, the same schedule (product; one or two orthonormalisations; product; a Rayleigh-Ritz check on every second product), the same
  rate rule.  Householder QR stands for Cholesky-QR; the pivot ratio s_j / G_jj of the block's Gram matrix under the 1e-14 rule is
  evaluated as r_jj^2 / ||y_j||^2 of that QR, which is the same quantity in exact arithmetic and which float64 resolves far below
  1e-16 (the Gram matrix itself squares the condition number and resolves nothing below 1e-15).  The model predicts the outcome class
  and `checks`; a prediction counts only under its CERTIFICATE (certify()): every check's relative residual a factor 10 away from the
  verdict tolerance, the rate rule's deciding quantity a third away from 8, the rate 10 % away from 1, no pivot ratio within a factor 100
  of 1e-14, no wanted gap (planted, and of the first check's Ritz values) within a factor 10 of gap_tol.
  Where the Jacobi form answers the Ritz problem (orders above 138 with a wanted Ritz gap below gap_tol) the model takes the residual
  as at least 2 x 2^-53 p, what a product of rotations leaves; on fp64 data at p >= 144 that is above the tolerance for good, the
  certificate refuses such rows, and two of them are kept as a recorded finding (FINDING_ROWS) with everything but the outcome asserted.
  NO FALSE DELIVERY is asserted for every case whatever the model says: a delivered result has long-double residuals within the verdict
  tolerance plus the rounding of the library's own product (below), the planted eigenvalues in order, orthonormal columns.

Bounds: topk-w, topk-res, topk-orth are MULT x max(model error, floor) as in smallmat_cases.py (model: numpy.linalg.eigh); the vectors
are held to Davis-Kahan, a derived bound: the part of v_j outside the planted eigenspace of lam_j's cluster is at most (measured
long-double residual + the Weyl floor) / (gap to the planted eigenvalues outside the cluster).
`python tests/topk_cases.py [--hostsim]` prints one line per case and quantity: the report kept in profiles/topk_errors.txt."""
import os
import sys

import numpy as np

if __name__ == "__main__":      # (run as a script: the package is found from the repository root)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import petal_decomposition_amd as petal
import smallmat_cases as sc
from smallmat_cases import LD, U, Case, planted, _cached, _rng

# Multiples of max(model error, floor), per quantity: twice the largest error / max(model, floor) measured over the whole table on the
# MI355X and on the host simulation (profiles/topk_errors.txt: its last lines name the largest ratio of each quantity and its case),
# rounded up.  None comes near 16, the level at which a ratio is a finding and not a constant.
MULT = {
    "topk-w": 5.1,          # 2.510  topk-g-rank-d200-nc65-f64, mode 2: the full eigen-solver answers (host simulation: 1.880 topk-c-d100-nc8-f64)
    "topk-res": 5.1,        # 2.514  topk-g-rank-d200-nc65-f64, mode 2 (host simulation: 1.889 topk-c-d100-nc8-f64)
    "topk-orth": 12.7,      # 6.302  topk-d-1e+09-d200-nc8-f32, mode 2: k_eigh<0> behind the flagged two-stage solve at order 200
                            #        (host simulation: 2.272 topk-d-1e+09-d100-nc8-f32)
}
sc.MULT.update(MULT)        # (_bound looks its family up there)
F32, F64 = petal.PETAL_F32, petal.PETAL_F64


def block_width(d, nc):
    dp = (d + 15) // 16 * 16
    return min((nc + 16 + 15) // 16 * 16, dp)


def tolerances(dtype):
    """(gap_tol, verdict tolerance) as gram_topk_eigh sets them"""
    return (1e-8, 1e-12) if dtype == F32 else (1e-5, 3e-14)


# The orders at which op_eigh's launcher (csrc/kernels/host_pow3_eigh.inc) hands a flagged two-stage solve to the caller's verdict word
# instead of running the Jacobi form behind it (`ext_verdict`: 3 <= L <= 138).  This is the launcher's rule, not topk_eigh's: if it
# moves there, it has to move here, or the model mispredicts r3[2] of the optimistic form and the Jacobi floor below.
EXT_VERDICT_ORDERS = (3, 138)
# Above those orders the Jacobi form answers a flagged Ritz problem, and the Ritz pairs of a product of rotations carry a residual of
# about 2 x 2^-53 p: measured 3.2e-14 at p = 144, 3.5 ... 4.0e-14 at p = 160 on the MI355X (2^-53 p = 1.6 / 1.8e-14).  LAPACK's solver,
# which the model uses, leaves 2e-15 there, so the model takes its residual as at least this much where the Jacobi form answers.
JACOBI_RESIDUAL = 2.0


def applies(d, nc):
    """topk_applies"""
    p = block_width(d, nc)
    return not (nc <= 0 or p >= d or d <= 88 or p > 512)


# ------------------------------------------------------------------------------------------- Section A: op_ritz_residual
RR_ROWS = [1, 15, 16, 17, 100, 1040]
RR_NC = [1, 63, 64, 65, 128, 129, 496]


def _rr_operands(rows, nc, pad, integer, worst):
    rng = _rng(211, rows, nc, int(integer), worst)
    ldc, ldv = nc + pad, nc + pad + 3
    if integer:
        cv = rng.integers(-8, 9, (rows, ldc)).astype(np.float64)
        vr = rng.integers(-8, 9, (rows, ldv)).astype(np.float64)
        theta = rng.integers(-8, 9, nc).astype(np.float64)
        cv[:, worst] = 8.0 * np.where(np.arange(rows) % 2, 1.0, -1.0)        # |t| = 72 in every row: the largest column for certain
        vr[:, worst] = -cv[:, worst]
        theta[worst] = 8.0
    else:
        vr = rng.standard_normal((rows, ldv)) / np.sqrt(rows)
        theta = np.sort(rng.uniform(0.05, 3.0, nc))[::-1].copy()
        cv = np.zeros((rows, ldc))
        noise = rng.standard_normal((rows, nc))
        noise *= 1e-3 / np.sqrt((noise * noise).sum(axis=0))      # every column's residual has norm 1e-3 ...
        noise[:, worst] *= 3.0                                     # ... but one: the largest for certain
        cv[:, :nc] = theta * vr[:, :nc] + noise
        cv[:, nc:] = rng.standard_normal((rows, pad))
    return cv, vr, theta


def _rr_exact(cv, vr, theta, nc):
    """per column j < nc, in long double: the statement's sum and its rounding bound"""
    t = cv[:, :nc].astype(LD) - theta.astype(LD) * vr[:, :nc].astype(LD)
    e = LD(1.01 * U) * (np.abs(cv[:, :nc]).astype(LD) + 2 * np.abs(theta * vr[:, :nc]).astype(LD))
    rows = cv.shape[0]
    s = (t * t).sum(axis=0)
    bnd = (2 * np.abs(t) * e + e * e).sum(axis=0) + LD(1.01 * (rows + 1) * U) * ((np.abs(t) + e) ** 2).sum(axis=0)
    return s, bnd


def rr_shape_check(ctx, rows, nc, device=True):
    pad = 5
    res = []
    worsts = sorted({0, nc // 2, nc - 1})
    # ---- small integers: bit for bit
    bad = 0
    for worst in worsts:
        cv, vr, theta = _rr_operands(rows, nc, pad, True, worst)
        out3, w_out = petal.probe_ritz_residual(cv, vr, nc, theta, w_len=nc + 9, ctx=ctx)
        t = cv[:, :nc] - theta * vr[:, :nc]
        want = float((t * t).sum(axis=0).max())
        assert want == 72.0 * 72.0 * rows
        bad += int(out3[0] != want) + int(out3[1].tobytes() != theta[0].tobytes()) + int(out3[2] != 0.0)
        bad += int(w_out[:nc].tobytes() != theta.tobytes()) + int(not np.all(np.isnan(w_out[nc:])))
        assert bad == 0, f"worst column {worst}: out3 = {out3}, wanted [{want}, {theta[0]}, 0]; w_out intact: {w_out[:nc].tobytes() == theta.tobytes()}, " \
                         f"behind nc: {w_out[nc:]}"
    res.append(("rr-exact", float(bad), 0.0, 0.0))
    # ---- real operands against long double, as a fraction of the derived bound
    err = model = 0.0
    for worst in worsts:
        cv, vr, theta = _rr_operands(rows, nc, pad, False, worst)
        out3, w_out = petal.probe_ritz_residual(cv, vr, nc, theta, ctx=ctx)
        s, bnd = _rr_exact(cv, vr, theta, nc)
        assert int(np.argmax(s)) == worst and float(s[worst]) > 4 * float(np.delete(s, worst).max() if nc > 1 else 0.0)
        assert float(bnd[worst] / s[worst]) <= sc.GUARD
        assert out3[2] == 0.0 and out3[1] == theta[0] and w_out[:nc].tobytes() == theta.tobytes() and np.all(np.isnan(w_out[nc:]))
        tm = cv[:, :nc] - theta * vr[:, :nc]
        err = max(err, float(abs(LD(out3[0]) - s[worst]) / bnd[worst]))
        model = max(model, float(abs(LD((tm * tm).sum(axis=0).max()) - s[worst]) / bnd[worst]))
    res.append(("rr-frac", err, model, 1.0))
    return res


def rr_flags_check(ctx, device=True):
    """each of the two flag words NULL / 0 / 1 / -3: out3[2] = 1 exactly when a given word is non-zero; nc = 0; a NaN or an inf in a column
    below nc raises out3[2], one between nc and the leading dimension does not; the 1e300 rule on either side of its threshold"""
    rows, nc = 17, 65
    cv, vr, theta = _rr_operands(rows, nc, 5, True, 3)
    bad = []
    for f1 in (None, 0, 1, -3):
        for f2 in (None, 0, 1, -3):
            out3, _ = petal.probe_ritz_residual(cv, vr, nc, theta, f1, f2, ctx=ctx)
            want = 1.0 if (f1 not in (None, 0) or f2 not in (None, 0)) else 0.0
            if out3[2] != want or out3[0] != 72.0 * 72.0 * rows or out3[1] != theta[0]:
                bad.append((f1, f2, list(out3)))
    assert not bad, f"(flag, flag2, out3) not as ops.h says: {bad}"
    out3, w_out = petal.probe_ritz_residual(cv, vr, 0, theta, w_len=4, ctx=ctx)
    assert list(out3) == [0.0, 0.0, 0.0] and np.all(np.isnan(w_out)), f"nc = 0: out3 = {out3}, w_out = {w_out}"
    for val in (np.nan, np.inf, -np.inf):
        for arr in ("cv", "vr"):
            for col, want in ((0, 1.0), (63, 1.0), (64, 1.0), (nc - 1, 1.0), (nc, 0.0), (nc + 4, 0.0)):
                a, b = cv.copy(), vr.copy()
                (a if arr == "cv" else b)[rows - 1 if col % 2 else 0, col] = val
                if arr == "vr" and theta[min(col, nc - 1)] == 0:
                    continue        # (theta x inf would be NaN all the same, but the case is about a finite theta)
                out3, _ = petal.probe_ritz_residual(a, b, nc, theta, ctx=ctx)
                assert out3[2] == want, f"{val} in {arr}[:, {col}] (nc = {nc}): out3[2] = {out3[2]}, wanted {want}"
                if want == 0.0 or col != 3:
                    assert out3[0] == 72.0 * 72.0 * rows, f"{val} in {arr}[:, {col}]: out3[0] = {out3[0]}"
    # ops.h: "not below 1e300".  One row, vr = 0, theta = 1: the sum is cv^2 exactly rounded, on either side of the threshold
    below, above = np.sqrt(1e300) * (1 - 2.0 ** -50), np.sqrt(1e300) * (1 + 2.0 ** -50)
    assert below * below < 1e300 <= above * above
    for col in (0, 64):
        for x, want in ((below, 0.0), (above, 1.0)):
            a = np.zeros((1, nc + 2))
            a[0, col] = x
            out3, _ = petal.probe_ritz_residual(a, np.zeros((1, nc + 2)), nc, np.ones(nc), ctx=ctx)
            assert out3[2] == want and out3[0] == (x * x if want == 0.0 else 0.0), f"cv = {x!r} in column {col}: out3 = {out3}"
    return [("rr-flags", 0.0, 0.0, 0.0)]


def rr_cases(device):
    cases = []
    for rows in RR_ROWS:
        for nc in RR_NC:
            if not device and rows * nc > 100 * 129 and (rows, nc) != (17, 496):
                continue
            trips = (nc + 63) // 64
            cases.append(Case(f"rr-{rows}x{nc}", f"k_ritz_residual, {trips} trip{'s' if trips > 1 else ''} of its column loop", rr_shape_check, rows, nc,
                              device=device))
    cases.append(Case("rr-flags-nonfinite-1e300", "k_ritz_residual: flag words, nc = 0, NaN / inf, the 1e300 rule", rr_flags_check, device=device))
    return cases


# ------------------------------------------------------------------------------------------- the model of topk_eigh
def start_block(d, dp, p):
    """topk_eigh's fixed start block: a 64-bit LCG, the top 53 bits of each state as a value in [-1, 1), rows d .. dp - 1 zero"""
    def make():
        st, m = 0x9E3779B97F4A7C15, (1 << 64) - 1
        v = np.zeros(d * p)
        for i in range(d * p):
            st = (st * 6364136223846793005 + 1442695040888963407) & m
            v[i] = float(st >> 11) / float(1 << 52) - 1.0
        h = np.zeros((dp, p))
        h[:d] = v.reshape(d, p)
        return h
    return _cached(("seed", d, dp, p), make)


def model(cp, d, nc, dtype):
    """topk_eigh restated (module docstring) on the padded matrix cp: a dict with
      cls       'first' | 'later' (delivered at the first / a later check), 'rate' | 'budget' (gave up), 'drop' (refused for a dropped
                pivot), 'nonfinite'
      delivered, checks              what the synchronous form returns
      verdict, bad, close            the optimistic form: topk_verdict_ok, r3[2] on the DEVICE, and whether r3[2] is raised by the closeness
                                     verdict alone (the host simulation's eigen-solver has no such verdict: there r3[2] = bad and not close)
      jacobi                         the Jacobi form answered a Ritz problem (JACOBI_RESIDUAL)
      rels, rates, qs, ratios, gaps  what the certificate looks at"""
    dp = cp.shape[0]
    p = block_width(d, nc)
    gap_tol, vtol = tolerances(dtype)
    m = dict(cls=None, delivered=0, checks=0, verdict=0, bad=0, close=False, rels=[], rates=[], qs=[], ratios=[], gaps=[], p=p, jacobi=False)
    if not np.all(np.isfinite(cp[:d, :d])):
        # a NaN reaches every Gram matrix: each pivot fails the rule (dropped), the residual is NaN: refused at the first check
        m.update(cls="nonfinite", checks=1, bad=1)
        return m
    y = cp @ start_block(d, dp, p)
    dropped = False
    prev_rel, bad_rates = -1.0, 0
    for it in range(40):
        nrm2 = (y * y).sum(axis=0)
        q, r = np.linalg.qr(y)
        ratio = np.where(nrm2 > 0, np.diag(r) ** 2 / np.where(nrm2 > 0, nrm2, 1.0), 0.0)
        if not dropped:     # (behind a drop the library's block has a zero column where the model's has a direction: the flag alone decides)
            m["ratios"] += [float(x) for x in ratio]
        dropped = dropped or bool((ratio <= 1e-14).any())
        y = cp @ q
        if it % 2 == 0:
            continue
        m["checks"] += 1
        first = m["checks"] == 1
        if dropped:         # (the dropped column's Ritz pair is not modelled: the flag alone decides)
            if first:
                m["bad"] = 1
            m["cls"] = "drop"
            return m
        h = q.T @ y
        th, s = np.linalg.eigh((h + h.T) / 2)
        th, s = th[::-1], s[:, ::-1]
        v, cv = q @ s[:, :nc], y @ s[:, :nc]
        res2 = float((((cv - th[:nc] * v) ** 2).sum(axis=0)).max())
        rel = np.sqrt(res2) / th[0] if th[0] > 0 else -1.0
        nrm = max(abs(th[0]), abs(th[-1]))
        g = np.abs(np.diff(th[:nc + 1])) / nrm if nrm > 0 else np.zeros(nc)
        ext = EXT_VERDICT_ORDERS[0] <= p <= EXT_VERDICT_ORDERS[1]
        if rel >= 0 and not ext and (g < gap_tol).any():       # the Jacobi form answers this Ritz problem
            m["jacobi"] = True
            rel = max(rel, JACOBI_RESIDUAL * U * p)
        m["rels"].append(float(rel))
        if first:
            m["gaps"] += [float(x) for x in g]
            m["close"] = bool(ext and (g < gap_tol).any())
            m["bad"] = 1 if m["close"] else 0
            m["verdict"] = int(m["bad"] == 0 and th[0] > 0 and rel <= vtol)
        if th[0] > 0 and rel <= vtol:
            m.update(cls="first" if first else "later", delivered=1)
            return m
        if rel < 0:
            m["cls"] = "rate"
            return m
        if prev_rel > 0:
            rate = rel / prev_rel
            m["rates"].append(float(rate))
            qq = np.log(vtol / rel) / np.log(rate) if rate < 1.0 else np.inf
            m["qs"].append(float(qq))
            hopeless = not (rate < 1.0) or qq > 8.0
            bad_rates = bad_rates + 1 if hopeless else 0
            if bad_rates >= 2 or (hopeless and it >= 9):
                m["cls"] = "rate"
                return m
        prev_rel = rel
    m["cls"] = "budget"
    return m


def certify(m, lam, nc, dtype):
    """the margins under which the model's prediction counts (module docstring); raises AssertionError naming the one that fails"""
    gap_tol, vtol = tolerances(dtype)
    if m["cls"] == "nonfinite":
        return
    amb = [x for x in m["ratios"] if 1e-16 <= x <= 1e-12]
    assert not amb, f"certificate: pivot ratios within a factor 100 of 1e-14: {amb[:4]}"
    amb = [x for x in m["rels"] if vtol / 10 < x < vtol * 10]
    assert not amb, f"certificate: relative residuals within a factor 10 of {vtol:g}: {amb}"
    amb = [x for x in m["rates"] if 0.9 < x < 1.1]
    assert not amb, f"certificate: rates within 10 % of 1: {amb}"
    amb = [x for x in m["qs"] if 8.0 * 2 / 3 < x < 8.0 * 4 / 3]
    assert not amb, f"certificate: the rate rule's deciding quantity within a third of 8: {amb}"
    l64 = np.asarray(lam, dtype=np.float64)
    planted_gaps = list(np.abs(np.diff(l64[:nc + 1])) / l64[0]) if l64[0] > 0 else []
    amb = [x for x in planted_gaps + m["gaps"] if gap_tol / 10 < x < gap_tol * 10]
    assert not amb, f"certificate: wanted gaps within a factor 10 of {gap_tol:g}: {amb[:4]}"


# ------------------------------------------------------------------------------------------- Section C: spectra and checks
def spectrum(family, variant, d, nc, dtype):
    """lam (long double, descending, d values) of a family (module docstring of the issue's families a .. g)"""
    p = block_width(d, nc)
    gap_tol, _ = tolerances(dtype)
    i = np.arange(d, dtype=LD)
    block = LD(10) ** (-i / LD(max(p - 1, 1)))                  # 1 ... 0.1 over the block
    lam = block.copy()
    if family == "a":       # a gap behind the block: the tail at `variant` x lam_1 (0: rank p)
        lam[p:] = LD(variant) * LD(0.97) ** (i[p:] - p)
    elif family == "b":     # a slow gap: lam_{p+1} / lam_nc = variant
        lam[p:] = lam[nc - 1] * LD(variant) * LD(0.97) ** (i[p:] - p)
    elif family == "c":     # smooth decay, no gap
        lam = LD(3) - LD(2.7) * i / LD(d - 1)
    elif family == "d":     # the wanted pairs graded over `variant` = lam_1 / lam_nc, rank p.  Every wanted gap and every pivot ratio
        # (about (lam_j / lam_1)^2) has to stay clear of the certificate's windows, so the grading is in two runs: geometric down to
        # 3e-4 (1e5) or 0.5 (1e9), then the small end -- 1e5: lam_nc = 1e-5 alone, the block's tail 4 % below it (4e-7 away: closer than the fp64
        # flag's gap_tol for certain, far above the fp32 flag's); 1e9: all but two of the wanted pairs at 1.2e-9 ... 1e-9
        # (the first small column's pivot ratio is about (its lam / the smallest large lam)^2: the large run of the 1e9 spectrum stops
        # at 0.5 so that every small ratio lies below 1e-16)
        hi = nc - 1 if variant <= 1e6 else 2       # (two large columns: a larger random block is worse conditioned and lifts the small ratios)
        lam[:hi] = LD(3e-4 if variant <= 1e6 else 0.5) ** (i[:hi] / LD(max(hi - 1, 1)))
        lam[hi:nc] = (LD(1) if variant <= 1e6 else LD(1.2) - LD(0.2) * (i[hi:nc] - hi + 1) / LD(nc - hi)) / LD(variant)
        lam[nc:p] = lam[nc - 1] * (LD(0.96) - LD(0.3) * (i[nc:p] - nc) / LD(p - nc)) * (LD(1) if variant <= 1e6 else LD(1e-2))
        # (1e9: the first small column keeps all its small directions, its ratio is their number x (lam / lam_1)^2: the tail lies 1e-2 lower)
        lam[p:] = 0
    elif family == "e":     # inside the wanted set: an exact double ("double") | a pair 0.01 gap_tol apart ("pair"); rank p
        at = min(2, nc - 2)
        lam[at + 1] = lam[at] if variant == "double" else lam[at] - LD(0.01 * gap_tol)
        lam[p:] = 0
    elif family == "f":     # lam_nc = lam_nc+1; rank p
        lam[nc] = lam[nc - 1]
        lam[p:] = 0
    elif family == "g":     # rank below nc | the zero matrix
        lam[max(nc - 3, 0):] = 0
        if variant == "zero":
            lam[:] = 0
    else:
        raise KeyError(family)
    assert np.all(lam[:-1] >= lam[1:])
    return lam


def _clusters(lam64, nc, thr):
    """for each j < nc: the index range [lo, hi) of lam's cluster around j: neighbours closer than thr = gap_tol lam_1 chain up -- what
    the eigen-solvers themselves treat as one cluster (families e and f, and the small end of a graded spectrum where its gaps fall
    below gap_tol); every other pair is a cluster of one and is held by itself"""
    out = []
    for j in range(nc):
        lo = hi = j
        while lo > 0 and lam64[lo - 1] - lam64[lo] < thr:
            lo -= 1
        while hi + 1 < len(lam64) and lam64[hi] - lam64[hi + 1] < thr:
            hi += 1
        out.append((lo, hi + 1))
    return out


def _delivered_quantities(a, qmat, lam, w, v, nc):
    """long double: eigenvalue error / lam_1, residual norms (absolute, per column), |V^T V - I| (elementwise)"""
    al, vl, wl = a.astype(LD), v.astype(LD), w.astype(LD)
    r = al @ vl - vl * wl[None, :]
    res = np.sqrt((r * r).sum(axis=0))
    g = np.abs(vl.T @ vl - np.eye(nc, dtype=LD))
    return np.abs(wl - lam[:nc]), res, g


def topk_check(ctx, family, variant, d, nc, dtype, device=True, certified=True):
    """certified = False (FINDING_ROWS): the certificate must REFUSE the row; the model's outcome is then not asserted, everything else is"""
    dp = (d + 15) // 16 * 16
    p = block_width(d, nc)
    gap_tol, vtol = tolerances(dtype)
    assert applies(d, nc)
    nan_case = family == "h"

    def make():
        lam = spectrum("a" if nan_case else family, 1e-9 if nan_case else variant, d, nc, dtype)
        a, q = planted(lam, 17)
        cp = np.zeros((dp, dp))
        cp[:d, :d] = a
        wm, vm = sc._eig_model(a)
        return lam, a, q, cp, wm, vm
    lam, a, qmat, cp, wm, vm = _cached(("topkA", family, variant, d, nc, dtype if family == "e" else 0), make)
    if nan_case:
        a = a.copy()
        a[d // 3, d // 2] = np.nan
        cp = cp.copy()
        cp[:d, :d] = a
    m = _cached(("topkM", family, variant, d, nc, dtype), lambda: model(cp, d, nc, dtype))
    if certified:
        certify(m, lam, nc, dtype)
    else:
        try:
            certify(m, lam, nc, dtype)
        except AssertionError:
            pass
        else:
            raise AssertionError("a row kept as a finding is certified now: move it into TOPK_ROWS")
    norm = float(lam[0])
    lam64 = lam.astype(np.float64)
    weyl = U * np.sqrt(d) * norm
    abs_c_norm = float(np.linalg.norm(np.abs(a), 2)) if not nan_case else 0.0
    # the library's residual is that of R = (C Q) S against V = Q S, two products of inner dimensions dp and p: its distance from C V
    # is at most 1.01 (dp + 2 p + 6) u || |C| |Q| |S_j| ||_2 <= 1.01 (dp + 2 p + 6) u || |C| ||_2 sqrt(p)
    round_cv = 1.01 * (dp + 2 * p + 6) * U * abs_c_norm * np.sqrt(p)
    res = []
    flagged_planted = (not norm > 0) or bool((np.abs(np.diff(lam64[:nc + 1])) / norm < gap_tol).any())

    def held(tag, w, v, by_topk, full_tol=None):
        """eigenvalues, residuals, orthonormality and vectors of nc delivered pairs; the three measured quantities as rows of `res`"""
        assert np.all(np.isfinite(w)) and np.all(np.isfinite(v)), f"{tag}: NaN / inf in a delivered result"
        assert np.all(v[d:, :] == 0.0), f"{tag}: rows d .. dp - 1 of V not exactly zero"
        e_w, r_abs, g = _delivered_quantities(a, qmat, lam, w, v[:d], nc)
        _, rm_abs, gm = _delivered_quantities(a, qmat, lam, wm[:nc], vm[:, :nc], nc)
        s = norm if norm > 0 else 1.0
        if by_topk:
            # no false delivery: the residual the verdict accepted, in long double
            lim = (vtol * float(w[0]) + round_cv)
            worst = float(r_abs.max())
            assert worst <= lim, f"{tag}: FALSE DELIVERY: long-double residual {worst:.3e} above {vtol:g} w_1 + rounding = {lim:.3e}"
            # (the residual floor includes the tolerance the verdict accepts; a Ritz value's error is of second order in it)
            fl_w, fl_r, fl_o = U * d + d * vtol ** 2, U * d + vtol, U * max(d, p)
        else:
            fl_w, fl_r, fl_o, _ = sc._eig_floors(d, full_tol)
        two_stage = device and by_topk and not m["close"] and not flagged_planted
        # (V = Q S with S from the two-stage solver, which computes every eigenvector on its own: smallmat_cases._orth_weights, with
        # the floor's 2^-53 max(d, p) in the place of its 2^-53 L)
        wt = None
        if two_stage and norm > 0:
            rel = np.maximum(np.abs(lam64[:nc, None] - lam64[None, :nc]) / norm, gap_tol)
            wt = max(d, p) / (max(d, p) + 2.0 / rel)
            np.fill_diagonal(wt, 1.0)

        def o(gg):
            return float((gg * wt).max() if wt is not None else gg.max())
        cap = 32 * U * d
        res.append(("topk-w", float(e_w.max()) / s, float(np.abs(wm[:nc].astype(LD) - lam[:nc]).max()) / s,
                    sc._bound("topk-w", float(np.abs(wm[:nc].astype(LD) - lam[:nc]).max()) / s, fl_w, cap)))
        res.append(("topk-res", float(r_abs.max()) / s, float(rm_abs.max()) / s, sc._bound("topk-res", float(rm_abs.max()) / s, fl_r, cap)))
        res.append(("topk-orth", o(g), o(gm), sc._bound("topk-orth", o(gm), fl_o, cap)))
        # Davis-Kahan on the cluster of every wanted eigenvalue
        if norm > 0:
            worst_frac = 0.0
            # sin(v_j, planted eigenspace of the cluster) <= (||C v_j - w_j v_j|| + Weyl floor) / gap_j, gap_j = the distance of w_j from
            # the PLANTED eigenvalues outside the cluster: the theorem applied to the planted matrix Q diag(lam) Q^T, against which
            # v_j's residual is the measured one plus at most ||C - Q diag(lam) Q^T|| <= the Weyl floor
            for j, (lo, hi) in enumerate(_clusters(lam64, nc, gap_tol * norm)):
                rest = np.concatenate([lam64[:lo], lam64[hi:]])
                if not len(rest):
                    continue
                gap = float(np.abs(rest - w[j]).min())
                assert gap > 0
                x = v[:d, j].astype(LD)
                qc = qmat[:, lo:hi]
                out = x - qc @ (qc.T @ x)
                sin = float(np.sqrt((out * out).sum()))
                dk = (float(r_abs[j]) + weyl) / gap
                worst_frac = max(worst_frac, sin / dk)
                assert sin <= dk, f"{tag}: pair {j}: {sin:.3e} of v_j lies outside the planted eigenspace, Davis-Kahan allows {dk:.3e}"
            res.append(("topk-dk-frac", worst_frac, 0.0, 1.0))

    # ---- mode 0: the synchronous form
    r0 = petal.probe_topk_eigh(a, nc, dtype, 0, ctx=ctx)
    assert not certified or (r0["delivered"], r0["checks"]) == (m["delivered"], m["checks"]), \
        f"mode 0: delivered, checks = {r0['delivered']}, {r0['checks']}; the model ({m['cls']}) says {m['delivered']}, {m['checks']}"
    assert np.all(r0["v"][d:, :][np.isfinite(r0["v"][d:, :])] == 0.0), "mode 0: rows d .. dp - 1 of V hold something other than 0.0 / the fill"
    if r0["delivered"]:
        held("mode 0", r0["w"], r0["v"], True)
    # ---- mode 1: the optimistic form
    r1 = petal.probe_topk_eigh(a, nc, dtype, 1, ctx=ctx)
    want_bad = m["bad"] if device else int(m["bad"] and not m["close"])
    want_verdict = m["verdict"] if device else int(want_bad == 0 and m["cls"] == "first")
    assert r1["delivered"] == 1, "mode 1: the shape qualifies"
    assert not certified or (r1["verdict"], r1["r3"][2]) == (want_verdict, float(want_bad)), \
        f"mode 1: verdict, r3 = {r1['verdict']}, {r1['r3']}; the model ({m['cls']}, close = {m['close']}) says {want_verdict}, r3[2] = {want_bad}"
    if r1["verdict"]:
        held("mode 1", r1["w"], r1["v"], True)
    if certified and m["cls"] == "first" and not m["close"] and not flagged_planted:
        assert r1["w"].tobytes() == r0["w"].tobytes() and r1["v"].tobytes() == r0["v"].tobytes(), "mode 1's w / V are not mode 0's bytes"
    # ---- mode 2: gram_eigen as Pca calls it
    if not nan_case:
        r2 = petal.probe_topk_eigh(a, nc, dtype, 2, ctx=ctx)
        assert not certified or r2["delivered"] == m["delivered"], f"mode 2: .topk = {r2['delivered']}, the model ({m['cls']}) says {m['delivered']}"
        assert r2["diag"].tobytes() == np.diag(cp).copy().tobytes(), "mode 2: diag is not C's diagonal to the byte"
        assert np.all(r2["v"][d:, :] == 0.0) and np.all(r2["v"][:, d:] == 0.0) and np.all(r2["w"][d:] == 0.0), "mode 2: padding of V / lam not exactly zero"
        if r2["delivered"]:
            assert r2["w"][:nc].tobytes() == r0["w"].tobytes() and r2["v"][:, :nc].tobytes() == r0["v"].tobytes(), "mode 2's pairs are not mode 0's bytes"
            assert np.all(r2["v"][:, nc:] == 0.0) and np.all(r2["w"][nc:] == 0.0), "mode 2: V / lam behind the nc delivered pairs not zero"
        else:
            assert np.all(r2["w"][:d - 1] >= r2["w"][1:d]), "mode 2: eigenvalues not in descending order"
            held("mode 2", r2["w"][:nc], r2["v"][:, :nc], False, 1e-8 if dtype == F32 else 1e-15)
    return res


def topk_shape_check(ctx, d, nc, qualifies, device=True):
    """Section B: a shape topk_applies refuses comes back at once -- delivered = 0, checks = 0, w and V still the probe's NaN fill --
    in modes 0 and 1; one it takes runs (checks >= 1; mode 1: delivered = 1)"""
    assert applies(d, nc) == qualifies
    lam = np.where(np.arange(d) < block_width(d, nc), 10.0 ** (-np.arange(d) / 600.0), 0.0)
    a = _cached(("shapeA", d, nc), lambda: _shape_matrix(d, lam))
    for mode in (0, 1):
        r = petal.probe_topk_eigh(a, nc, F64, mode, ctx=ctx)
        if not qualifies:
            assert r["delivered"] == 0 and np.all(np.isnan(r["w"])) and np.all(np.isnan(r["v"])), f"mode {mode}: a refused shape wrote something"
            assert mode == 1 or r["checks"] == 0
            assert mode == 0 or (r["verdict"] == 0 and np.all(np.isnan(r["r3"])))
        elif mode == 0:
            assert r["checks"] >= 1, "mode 0: no Rayleigh-Ritz step on a shape that qualifies"
            if r["delivered"]:
                rr = a @ r["v"][:d] - r["v"][:d] * r["w"]
                assert np.sqrt((rr * rr).sum(axis=0)).max() <= 1e-11 * lam[0] and np.abs(r["w"] - lam[:nc]).max() <= 1e-11 * lam[0]
        else:
            assert r["delivered"] == 1 and np.all(np.isfinite(r["r3"]))
    return [("topk-shape", 0.0, 0.0, 0.0)]


def _shape_matrix(d, lam):
    """float64 only (no reference is taken from it): Q diag(lam) Q^T with Q from a QR of random numbers"""
    q, _ = np.linalg.qr(_rng(5, d).standard_normal((d, d)))
    a = (q * lam) @ q.T
    return (a + a.T) / 2


def topk_cache_check(ctx_factory, device=True):
    """the start block is cached per shape and ctx: shape A, then B, then A again on one ctx -- both A calls give the bytes of A on a
    fresh ctx, and the same call twice gives the same bytes"""
    la, lb = spectrum("a", 1e-9, 100, 8, F64), spectrum("a", 1e-9, 160, 17, F64)
    a, b = planted(la, 17)[0], planted(lb, 17)[0]

    def run(ctx, mat, nc):
        r = petal.probe_topk_eigh(mat, nc, F64, 0, ctx=ctx)
        assert r["delivered"] == 1
        return r["w"].tobytes() + r["v"].tobytes()
    c1 = ctx_factory()
    try:
        a1, a1b, _, a2 = run(c1, a, 8), run(c1, a, 8), run(c1, b, 17), run(c1, a, 8)
    finally:
        c1.close()
    c2 = ctx_factory()
    try:
        fresh = run(c2, a, 8)
    finally:
        c2.close()
    assert a1 == a1b, "the same call twice gives other bytes"
    assert a1 == fresh and a2 == fresh, "shape A after shape B differs from A on a fresh ctx"


SHAPE_ROWS = [(88, 8, False), (89, 8, True), (100, 84, False), (112, 80, True), (600, 497, False), (513, 496, True), (200, 0, False)]
# (family, variant, d, nc): every order and every pair count of the issue's lists where p < d, each family under both data-type flags
TOPK_ROWS = [
    ("a", 1e-9, 89, 1), ("a", 1e-9, 100, 8), ("a", 0.0, 160, 64), ("a", 1e-9, 200, 65), ("a", 1e-9, 256, 130), ("a", 0.0, 256, 72),
    # (a residual that falls by 1e-2 or 1e-4 per check passes within a factor 10 of the tolerance on most spectra: lam_p+1 / lam_nc is
    # "about" 1e-1 / 1e-2, chosen per data-type flag so that the certificate holds)
    ("b", 0.015, 100, 16), ("b", 0.015, 160, 17, F32), ("b", 0.012, 160, 17, F64), ("b", 0.02, 200, 72, F32), ("b", 0.012, 200, 72, F64),
    ("b", 0.08, 160, 17, F32), ("b", 0.08, 256, 8, F32), ("b", 0.07, 200, 16, F64), ("b", 0.075, 256, 64, F64),
    ("c", None, 256, 8), ("c", None, 200, 16), ("c", None, 100, 8),
    ("d", 1e5, 160, 16), ("d", 1e9, 200, 8), ("d", 1e5, 256, 17), ("d", 1e9, 100, 8),
    ("e", "double", 100, 8), ("e", "pair", 100, 8), ("e", "pair", 200, 65), ("e", "double", 256, 130, F32),
    ("f", None, 100, 8), ("f", None, 160, 17), ("f", None, 256, 72), ("f", None, 256, 130, F32),
    ("g", "rank", 100, 16), ("g", "zero", 160, 8), ("g", "rank", 200, 65),
    ("h", None, 100, 8), ("h", None, 256, 64),
]
# A FINDING, kept as rows the certificate refuses: fp64 data, a double or close wanted pair, p = 160.  The Jacobi form answers the Ritz
# problem (EXT_VERDICT_ORDERS), its residual of about 2 x 2^-53 p = 3.6e-14 lies above the fp64 tolerance 3e-14 for good, and the
# library spends three checks (rate 1), gives up and lets the full eigen-solver answer: a right result and a slow fit.  With the Jacobi
# floor the model says the same (0, 3), but a residual a factor 1.2 from the tolerance certifies nothing, so the outcome is not
# asserted; no false delivery, the padding, the diag and the accuracy of whatever reaches the outputs are.  The tolerance is kept
# (csrc/algo.cpp, above topk_verdict_ok, says why).
FINDING_ROWS = [("e", "double", 256, 130, F64), ("f", None, 256, 130, F64)]
_HOST_MAX_D = 160


def topk_rows(device):
    return [(r[0], r[1], r[2], r[3], dt) for r in TOPK_ROWS for dt in (F32, F64) if (device or r[2] <= _HOST_MAX_D) and (len(r) == 4 or r[4] == dt)]


def topk_cases(device):
    cases = [Case(f"topk-shape-d{d}-nc{nc}", "topk_applies: " + ("taken" if q else "refused"), topk_shape_check, d, nc, q, device=device)
             for d, nc, q in SHAPE_ROWS if device or d < 500]
    for f, v, d, nc, dt in topk_rows(device):
        tag = f"topk-{f}" + (f"-{v:g}" if isinstance(v, float) else f"-{v}" if v else "") + f"-d{d}-nc{nc}-{'f32' if dt == F32 else 'f64'}"
        cases.append(Case(tag, f"topk_eigh, p = {block_width(d, nc)}", topk_check, f, v, d, nc, dt, device=device))
    for f, v, d, nc, dt in FINDING_ROWS:
        if device:
            cases.append(Case(f"topk-{f}" + (f"-{v}" if v else "") + f"-d{d}-nc{nc}-f64-uncertified", f"topk_eigh, p = {block_width(d, nc)}: the Jacobi floor above 3e-14",
                              topk_check, f, v, d, nc, dt, device=device, certified=False))
    return cases


def all_cases(device=True):
    cases = rr_cases(device) + topk_cases(device)
    ids = [c.id for c in cases]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return cases


def model_of_row(f, v, d, nc, dt):
    """the model's outcome for a row of the table, on the CPU alone (the class-coverage test)"""
    dp = (d + 15) // 16 * 16
    lam = spectrum("a" if f == "h" else f, 1e-9 if f == "h" else v, d, nc, dt)
    a = planted(lam, 17)[0]
    cp = np.zeros((dp, dp))
    cp[:d, :d] = a
    if f == "h":
        cp[d // 3, d // 2] = np.nan
    m = _cached(("topkM", f, v, d, nc, dt), lambda: model(cp, d, nc, dt))
    certify(m, lam, nc, dt)
    return m


def main():
    import time
    host = "--hostsim" in sys.argv
    if host:
        import hostsim
        ctx = hostsim.context()
    else:
        ctx = petal.Context(0)
    cases = all_cases(device=not host)
    print(f"# {'host simulation' if host else 'device'}: case | quantity | error | model error | error / max(model, floor) | bound | form")
    t0 = time.time()
    worst = {}
    for c in cases:
        try:
            rows = c.run(ctx)
        except (AssertionError, petal.InvalidInput) as e:
            print(f"{c.id:36s} FAILED: {e}   [{c.form}]", flush=True)
            continue
        except petal.DeviceError as e:      # the device is in an unknown state: nothing more is started on it
            print(f"{c.id:36s} DEVICE ERROR, report ends here: {e}   [{c.form}]", flush=True)
            return
        for q, err, mod, bound in rows:
            denom = bound / MULT[q] if q in MULT else (bound if bound > 0 else float("nan"))
            ratio = err / denom if denom == denom and denom > 0 else float("nan")
            flag = "" if err <= bound else "   <-- ABOVE THE BOUND"
            print(f"{c.id:36s} {q:12s} {err:10.3e} {mod:10.3e} {ratio:8.3f} {bound:10.3e}   [{c.form}]{flag}", flush=True)
            fam = "-".join(c.id.split("-")[:2]) if c.id.startswith("topk-") else "rr"     # topk-a ... topk-h, topk-shape
            if ratio == ratio and ratio > worst.get(q, (0.0, ""))[0]:
                worst[q] = (ratio, c.id)
            if ratio == ratio and q in MULT and ratio > worst.get((q, fam), (0.0, ""))[0]:
                worst[(q, fam)] = (ratio, c.id)
    ctx.close()
    for k, (r, cid) in sorted(worst.items(), key=lambda kv: str(kv[0])):
        if isinstance(k, tuple):
            print(f"# {k[0]} in family {k[1]}: largest error / max(model, floor) {r:.3f} ({cid})")
        else:
            print(f"# {k}: largest error / max(model, floor) {r:.3f} ({cid})" + (f"; MULT {MULT[k]}" if k in MULT else ""))
    print(f"# {len(cases)} cases, wall time {time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
