"""The fp64 small-matrix kernels every fit rests on, each through a probe entry of its own (include/petal_hip_probe.h), against
references in numpy.longdouble.  Shared by tests/test_gpu_smallmat.py (the HIP library) and tests/test_smallmat_hostsim.py (the host
simulation, a reduced table: it proves references, certificates and bounds without a GPU and holds oracle/cpu_ops.cpp to the same
contract).

References (long double, each certifies itself)
  orth_ld        a product of L random Householder reflectors; |Q^T Q - I| < 1e-17 L
  chol_drop      the loop of oracle/cpu_ops.cpp::op_chol_inv (row-by-row upper Cholesky with the drop rule, back substitution on the
                 live indices), generic in the dtype: long double is the reference, float64 the model.  Certificate: no pivot ratio
                 s_j / G_jj of the reference lies in [rel_tol / 100, 100 rel_tol] -- the dead set does not hinge on a rounding
  planted        A = fl64(Q diag(lam) Q^T), symmetrised: by Weyl the eigenvalues of the fp64 input are lam +- 2^-53 sqrt(L) ||A||
  hestenes       one-sided Jacobi on the rows of M (round-robin, the disjoint pairs of a round at once), generic in the dtype; certificate:
                 rows mutually orthogonal to 8 eps_ld sqrt(L) (< 1e-17 here; the iteration stops at 4 eps_ld sqrt(L), the rounding noise
                 of an L-term long-double dot product: a fixed 1e-18 lies below it from L = 6 on and the iteration would never stop).  Its error in a singular value is of
                 second order in that angle
  GEMM           the long-double product with the DERIVED componentwise bound |C - C_ld| <= 1.01 (K + 2) 2^-53 (|alpha| |op A| |op B| +
                 |beta C|) |colscale|, which holds for any summation order (MFMA, split-K): error is reported as a fraction of it, bound 1

Models: the same statement in numpy float64 and never the library -- chol_drop in float64, numpy.linalg.eigh, numpy.linalg.svd
for absolute quantities, hestenes in float64 where LAPACK is not relatively accurate (graded eigenproblems, small singular values).
    bound = MULT x max(model error, floor)            floor = 2^-53 x the growth factor named at each quantity
and every case asserts bound <= 1e-3 of the quantity it bounds (GUARD): a looser bound proves nothing.

Each check takes a ctx and returns a list of (quantity, error, model error, bound); what is exact (padding that must be 0.0 and not
NaN, dead rows and columns, ndead, the verdict word, the order, the tie rule) is asserted inside the check.
`python tests/smallmat_cases.py` runs every case on petal.Context(0) and prints one line per case and quantity: the report kept in
profiles/smallmat_errors.txt."""
import os
import sys

import numpy as np

if __name__ == "__main__":      # (run as a script: the package is found from the repository root)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import petal_decomposition_amd as petal

LD = np.longdouble
U = 2.0 ** -53
GUARD = 1e-3
# Multiples of max(model error, floor), per family: twice the largest error / max(model, floor) measured on the MI355X over the whole
# table (profiles/smallmat_errors.txt: its last lines name the largest ratio of each family and its case, and the largest ratio of the
# float64 MODEL).  The margin covers box-to-box and summation-order differences.  No family comes near 16, the level at which a ratio
# is a finding and not a constant.  Where the floor, a worst-case growth factor, lies so far above both the kernel and the model that
# the kernel's ratio is below the model's, the model's ratio is doubled instead: a bound below the float64 model's own error would no
# longer be tied to the model (the host-simulation table asserts model <= bound for every row), so such a family is held to twice
# what the same statement in numpy float64 delivers -- still 9 to 30 times tighter than a multiple of the floor that is 16.
MULT = {
    "chol-fwd": 6.9,        # 3.443  chol-r1-B528-L33-cond1e+10-tol1e-14
    "chol-orth": 7.3,       # 3.642  chol-r1-id-L33-cond1e+10-tol1e-15
    "eig-w": 6.5,           # 3.205  eig-geo-L513-tol1e-15
    "eig-res": 6.5,         # 3.206  eig-geo-L513-tol1e-15
    "eig-orth": 8.7,        # 4.349  eig-geo-L513-tol1e-15 (k_eigh<0> behind the flagged two-stage solve: the plain 2^-53 L)
    "eig-angle": 0.46,      # 0.228  eig-pad-L3-Lz16-two-stage (model: 0.134 eig-geo-L3-tol1e-15)
    "eig-rel": 0.57,        # 0.053  eig-graded-L48-jacobi; the float64 Hestenes model has 0.281 (eig-graded-L16-jacobi), doubled here
    "svd-rel": 1.02,        # 0.297  svd-Rinv-L1; the float64 Hestenes model has 0.507 (svd-DQ-L3), doubled here
    "svd-orth": 7.8,        # 3.877  svd-Rinv-L98
    "svd-rows": 1.86,       # 0.250  svd-DB-L2; numpy.linalg.svd has 0.926 (svd-Rinv-L3), doubled here
}
_cache = {}


def _cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def _bound(family, model, floor, cap):
    """MULT x max(model, floor).  cap: the a-priori worst case of the model's own error (a textbook bound with its constant) -- a model
    further from the reference than that means the REFERENCE (or the model) is wrong, and a bound that grew with it would hide it."""
    assert model <= cap, f"{family}: the float64 model is {model:.2e} from the reference, its a-priori bound is {cap:.2e}: wrong reference?"
    b = MULT[family] * max(model, floor)
    assert b <= GUARD, f"vacuous bound {b:.2e} for {family} (model {model:.2e}, floor {floor:.2e})"
    return b


# ------------------------------------------------------------------------------------------- references
def orth_ld(L, *seed):
    def make():
        assert np.finfo(LD).eps < 2e-19, "needs the x86 80-bit long double"
        rng = _rng(101, L, *seed)
        q = np.eye(L, dtype=LD)
        for _ in range(L):
            v = rng.standard_normal(L).astype(LD)
            v /= np.sqrt((v * v).sum())
            q -= LD(2) * np.outer(q @ v, v)
        err = np.abs(q.T @ q - np.eye(L, dtype=LD)).max()
        assert err < LD(1e-17) * L, f"reference certificate: Q^T Q - I = {float(err):.1e}"
        return q
    return _cached(("q", L) + seed, make)


def planted(lam, *seed):
    """(A float64 symmetric, Q long double) with A = fl64(Q diag(lam) Q^T)"""
    lam = np.asarray(lam, dtype=LD)
    q = orth_ld(len(lam), *seed)
    a = ((q * lam) @ q.T).astype(np.float64)
    return (a + a.T) / 2.0, q


def chol_drop(g, rel_tol, dt):
    """oracle/cpu_ops.cpp::op_chol_inv restated in dtype dt: (T, R, dead, pivot ratios).  Dead column j: zero row and column j of T; T is
    the inverse of R on the live indices."""
    g = np.asarray(g).astype(dt)
    L = g.shape[0]
    r = np.zeros((L, L), dtype=dt)
    dead = np.zeros(L, dtype=bool)
    ratio = np.zeros(L, dtype=dt)
    tol = dt(rel_tol)
    for j in range(L):
        gjj = g[j, j]
        s = gjj - (r[:j, j] * r[:j, j]).sum()
        ratio[j] = s / gjj if gjj > 0 else dt(0)
        if not (gjj > 0) or not (s > tol * gjj):
            dead[j] = True
            continue
        rjj = np.sqrt(s)
        r[j, j] = rjj
        if j + 1 < L:
            r[j, j + 1:] = (g[j, j + 1:] - r[:j, j] @ r[:j, j + 1:]) / rjj
    live = np.flatnonzero(~dead)
    rl = r[np.ix_(live, live)]
    m = len(live)
    tl = np.zeros((m, m), dtype=dt)
    for i in range(m - 1, -1, -1):
        tl[i, i] = dt(1) / rl[i, i]
        if i + 1 < m:
            tl[i, i + 1:] = -(rl[i, i + 1:] @ tl[i + 1:, i + 1:]) / rl[i, i]
    t = np.zeros((L, L), dtype=dt)
    t[np.ix_(live, live)] = tl
    return t, r, dead, ratio


def chol_reference(g, rel_tol):
    t, r, dead, ratio = chol_drop(g, rel_tol, LD)
    amb = [(j, float(ratio[j])) for j in range(len(dead)) if g[j, j] > 0 and rel_tol / 100 <= ratio[j] <= 100 * rel_tol]
    assert not amb, f"reference certificate: pivot ratios next to rel_tol = {rel_tol:g}: {amb[:4]}"
    live = np.flatnonzero(~dead)
    if len(live):       # the reference's own backward error, and its inverse against the n u |T| |R| of a triangular inversion
        gl, rl, tl = np.asarray(g, dtype=LD)[np.ix_(live, live)], r[np.ix_(live, live)], t[np.ix_(live, live)]
        back = float(np.abs(rl.T @ rl - gl).max() / np.abs(gl).max())
        assert back < 1e-18, f"reference certificate: |R^T R - G| / |G| = {back:.1e}"
        inv = np.abs(tl @ rl - np.eye(len(live), dtype=LD)).max()
        assert inv <= len(dead) * 1.1e-19 * (np.abs(tl) @ np.abs(rl)).max(), f"reference certificate: |T R - I| = {float(inv):.1e}"
    return t, dead


def hestenes(m, dt, max_sweeps=60):
    """One-sided Jacobi on the ROWS of m in dtype dt: (singular values ascending, largest remaining cosine between two rows)."""
    w = np.array(m, dtype=dt)
    L = w.shape[0]
    if L == 1:
        return np.sqrt((w * w).sum(axis=1)), 0.0
    n = (L + 1) & ~1
    half = n // 2
    tol = dt(4 * np.finfo(dt).eps * np.sqrt(L))
    slots = np.arange(half)
    for _ in range(max_sweeps):
        rotated = False
        for r in range(n - 1):
            p = np.where(slots == 0, n - 1, (r + slots) % (n - 1))
            q = (n - 1 - slots + r) % (n - 1)
            p, q = np.minimum(p, q), np.maximum(p, q)
            keep = q < L
            p, q = p[keep], q[keep]
            a, b = w[p], w[q]
            al, be, ga = (a * a).sum(axis=1), (b * b).sum(axis=1), (a * b).sum(axis=1)
            act = np.abs(ga) > tol * np.sqrt(al * be)
            if not act.any():
                continue
            rotated = True
            p, q, a, b = p[act], q[act], a[act], b[act]
            zeta = (be[act] - al[act]) / (dt(2) * ga[act])
            t = np.where(zeta >= 0, dt(1), dt(-1)) / (np.abs(zeta) + np.sqrt(dt(1) + zeta * zeta))
            cs = dt(1) / np.sqrt(dt(1) + t * t)
            sn = cs * t
            w[p] = cs[:, None] * a - sn[:, None] * b
            w[q] = sn[:, None] * a + cs[:, None] * b
        if not rotated:
            break
    else:
        raise AssertionError("reference certificate: the Hestenes iteration did not converge")
    nrm = np.sqrt((w * w).sum(axis=1))
    gram = w @ w.T
    d = np.where(nrm > 0, nrm, dt(1))
    cosines = np.abs(gram / np.outer(d, d))
    np.fill_diagonal(cosines, 0)
    return np.sort(nrm), float(cosines.max())


def hestenes_ld(m):
    s, c = hestenes(m, LD)
    lim = 8 * float(np.finfo(LD).eps) * np.sqrt(m.shape[0])     # (the iteration stops at 4 eps sqrt(L); the check's own dot products add as much)
    assert c <= max(lim, 1e-18), f"reference certificate: rows orthogonal to {c:.1e} only"
    return s


# ------------------------------------------------------------------------------------------- Cholesky / triangular solves
REL_TOLS = [1e-6, 1e-12, 1e-14, 1e-15]       # the values algo.cpp passes
# the rel_tol a condition number may be paired with: the smallest pivot ratio of G is about 1 / cond and must stay clear of 100 rel_tol
_TOLS_FOR = {1.0: REL_TOLS, 1e3: REL_TOLS, 1e6: REL_TOLS[1:], 1e10: REL_TOLS[2:]}
CONDS = [1.0, 1e3, 1e6, 1e10]


def chol_input(L, cond, dups=(), zero_col=None):
    """G = fl64(3.7 Q diag(logspace(0, -log10 cond)) Q^T); dups: (i, j) pairs, row / column j an EXACT copy of i (made in long double,
    then rounded: the copies stay exact); zero_col: row / column set to zero (G_jj = 0)"""
    def make():
        q = orth_ld(L, 7)
        lam = (LD(10) ** (-LD(np.log10(cond)) * np.arange(L, dtype=LD) / max(L - 1, 1))) * LD(3.7)
        g = (q * lam) @ q.T
        g = (g + g.T) / LD(2)
        for i, j in dups:
            g[:, j] = g[:, i]
            g[j, :] = g[i, :]
        if zero_col is not None:
            g[:, zero_col] = 0
            g[zero_col, :] = 0
        g64 = g.astype(np.float64)
        assert np.array_equal(g64, g64.T)
        return g64
    return _cached(("G", L, cond, tuple(dups), zero_col), make)


def _colrel(x, ref):
    """largest column-relative error ||x_j - ref_j|| / ||ref_j|| over the columns of ref that are not zero"""
    e = np.sqrt(((x.astype(LD) - ref) ** 2).sum(axis=0))
    n = np.sqrt((ref * ref).sum(axis=0))
    ok = n > 0
    return float((e[ok] / n[ok]).max()) if ok.any() else 0.0


def chol_may_rt(L, Lz):
    """where op_chol_rt hands back the RT form on the device (ops.h): k_chol_rt4<Lz / 16>"""
    return L <= 140 and Lz % 16 == 0 and Lz <= 144


def chol_check(ctx, L, cond, rel_tol, route, Lz=None, brows=0, dups=(), zero_col=None, ndead_cols=0, ndead_in=0, device=True):
    g = chol_input(L, cond, dups, zero_col)
    t_ld, dead = _cached(("Tld", L, cond, tuple(dups), zero_col, rel_tol), lambda: chol_reference(g, rel_tol))
    t64, _, dead64, _ = _cached(("T64", L, cond, tuple(dups), zero_col, rel_tol), lambda: chol_drop(g, rel_tol, np.float64))
    assert np.array_equal(dead, dead64), "the float64 model drops other columns than the reference"
    Lz = Lz if Lz is not None else (L + 15) // 16 * 16
    rng = _rng(55, L, route, brows)
    b = None
    if route == 1 and brows:
        b = rng.standard_normal((brows, Lz))
    if route == 2:
        b = rng.standard_normal((Lz, Lz))
    out, nd, rt = petal.probe_chol(g, rel_tol, Lz, ndead_cols, route, b, ndead_in, ctx)
    # ---- what is exact
    want_rt = 1 if (device and route != 0 and chol_may_rt(L, Lz)) else 0
    assert rt == want_rt, f"rt = {rt}, expected {want_rt}"
    counted = int(dead[:ndead_cols].sum()) if (ndead_cols > 0 and L <= 140) else int(dead.sum())
    assert nd == max(ndead_in, counted), f"ndead = {nd}, expected max({ndead_in}, {counted})"
    assert np.all(np.isfinite(out)), "NaN / inf in the result (an element no kernel wrote?)"
    dj = np.flatnonzero(dead)
    if route == 2:
        assert np.all(out[L:, :] == 0.0), "padding rows of R^-1 B not exactly zero"
        assert np.all(out[dj, :] == 0.0), "dead rows of R^-1 B not exactly zero"
    else:
        assert np.all(out[:, L:] == 0.0), "padding columns not exactly zero"
        assert np.all(out[:, dj] == 0.0), "dead columns not exactly zero"
        if b is None:
            assert np.all(out[L:, :] == 0.0), "padding rows of T not exactly zero"
            assert np.all(out[dj, :] == 0.0), "dead rows of T not exactly zero"
            assert np.all(np.tril(out, -1) == 0.0), "T not upper triangular"
    # ---- against the long double
    if b is None:
        ref, mod, got = t_ld, t64, out[:L, :L]
    elif route == 1:
        ref, mod, got = b[:, :L].astype(LD) @ t_ld, b[:, :L] @ t64, out[:, :L]
    else:
        ref, mod, got = t_ld @ b[:L, :].astype(LD), t64 @ b[:L, :], out[:L, :]
    floor = U * np.sqrt(L * cond)       # cond(R) = sqrt(cond(G)) on rounding errors that add at random over the L terms of a column
    res = []
    err, model = _colrel(got, ref), _colrel(mod, ref)
    cap = 8 * U * L * cond              # (the sensitivity of the Cholesky factor itself is cond(G), not its root)
    res.append(("chol-fwd", err, model, _bound("chol-fwd", model, floor, cap)))
    if b is None:
        live = np.flatnonzero(~dead)
        gl = g.astype(LD)[np.ix_(live, live)]
        eye = np.eye(len(live), dtype=LD)

        def orth(t):
            tl = t.astype(LD)[np.ix_(live, live)]
            return float(np.abs(tl.T @ gl @ tl - eye).max()) if len(live) else 0.0
        err, model = orth(out[:L, :L]), orth(t64)
        res.append(("chol-orth", err, model, _bound("chol-orth", model, floor, cap)))
    return res


# route 1 orders (k_chol_rt4<NB>, NB = ceil(L / 16) = 1 .. 9; identity B through k_trsm_pack<NB, false>)
CHOL_RT_L = [1, 2, 15, 16, 17, 31, 32, 33, 48, 63, 74, 80, 81, 96, 112, 127, 128, 129, 138, 140]
CHOL_INV2_L = [1, 5, 16, 74, 138, 140]          # route 0, k_chol_inv2
CHOL_BLOCKED_L = [141, 200, 256, 257, 300]      # route 0, chol_inv_blocked: 128-wide blocks (the round-3 defect range; 2, 3 blocks; a 1-wide last block)
CHOL_LEFT_L = [16, 74, 138]                     # route 2, k_trsm_left_pack<NB>
_HOST_MAX_L = 141                               # the reduced table of the host simulation stops here


def _pair(i):
    """condition number and rel_tol of the i-th row of a table: every cond with every rel_tol it may be paired with, in turn"""
    cond = CONDS[i % 4]
    tols = _TOLS_FOR[cond]
    return cond, tols[(i // 4) % len(tols)]


def chol_cases(device):
    cases = []

    def add(name, L, cond, tol, route, form, **kw):
        cases.append(Case(f"chol-r{route}-{name}-L{L}-cond{cond:.0e}-tol{tol:.0e}", form, chol_check, L, cond, tol, route, device=device, **kw))
    for i, L in enumerate(CHOL_RT_L):
        cond, tol = _pair(i)
        nb = (L + 15) // 16
        add("id", L, cond, tol, 1, f"k_chol_rt4<{nb}> + k_trsm_pack<{nb}, false>")
    add("id-Lz144", 74, 1e6, 1e-14, 1, "k_chol_rt4<9> on a 5-block matrix + k_trsm_pack<9, false>", Lz=144)
    for i, (L, rows) in enumerate([(1, 16), (17, 48), (33, 528), (48, 16), (63, 48), (74, 528), (96, 16), (112, 48), (127, 528), (140, 528)]):
        cond, tol = _pair(i + 1)
        nb = (L + 15) // 16
        add(f"B{rows}", L, cond, tol, 1, f"k_chol_rt4<{nb}> + k_trsm_pack<{nb}, false>, {rows // 16} row blocks", brows=rows)
    for i, L in enumerate(CHOL_INV2_L):
        cond, tol = _pair(i + 2)
        add("inv2", L, cond, tol, 0, "k_chol_inv2")
    for i, L in enumerate(CHOL_BLOCKED_L):
        if not device and L > _HOST_MAX_L:
            continue
        cond, tol = _pair(i + 3)
        add("blocked", L, cond, tol, 0, f"chol_inv_blocked, {(L + 127) // 128} blocks (k_chol_inv2 with gd_ref + k_dgemm)")
    for i, L in enumerate(CHOL_LEFT_L):
        cond, tol = _pair(i + 1)
        nb = (L + 15) // 16
        add("left", L, cond, tol, 2, f"k_chol_rt4<{nb}> + k_trsm_left_pack<{nb}> (both GEMM modes)")
    # dependent columns: exact duplicates (one and three), a zero diagonal, ndead_cols between two dead columns, a larger preset
    last = 73
    dup_sets = [("0+1", ((0, 1),)), ("in-block", ((18, 21),)), ("15-16", ((15, 16),)), ("16-17", ((16, 17),)), ("last", ((5, last),)),
                ("three", ((0, 1), (15, 16), (14, 17))), ("three-spread", ((3, 31), (31, 32), (40, last)))]
    for i, (name, dups) in enumerate(dup_sets):
        tol = [1e-6, 1e-12][i % 2]
        for route in (0, 1, 2):
            add(f"dup-{name}", 74, 1e3, tol, route, "dead columns: " + ["k_chol_inv2", "k_chol_rt4<5> + k_trsm_pack", "k_chol_rt4<5> + k_trsm_left_pack"][route], dups=dups)
    for route in (0, 1):
        add("zero-diag", 74, 1e3, 1e-12, route, "G_jj = 0 is dead", zero_col=20)
        add("dup-ndead_cols", 74, 1e3, 1e-12, route, "ndead_cols = 30 between the dead columns 16 and 40", dups=((15, 16), (2, 40)), ndead_cols=30)
        add("dup-preset", 74, 1e3, 1e-12, route, "*ndead = max(preset 5, 1)", dups=((15, 16),), ndead_in=5)
    if device:
        add("dup-across-128", 200, 1e3, 1e-12, 0, "chol_inv_blocked: source in block 0, copy in block 1 (gd_ref)", dups=((100, 130),))
        add("dup-127-128", 200, 1e3, 1e-6, 0, "chol_inv_blocked: copy on the block boundary", dups=((127, 128),))
        add("dup-both-blocks", 257, 1e3, 1e-12, 0, "chol_inv_blocked: dead columns in blocks 0, 1 and the 1-wide block 2: ndead counts them all",
            dups=((3, 50), (60, 140), (7, 256)))
    return cases


# ------------------------------------------------------------------------------------------- op_dgemm
def dgemm_form(ta, tb, M, N, K, alpha, beta, alias, colscale):
    """the kernel op_dgemm's dispatch (csrc/kernels/host_small.inc) takes"""
    if not colscale and ta and not tb and M == N and M % 16 == 0 and M <= 256 and K >= 64 and alpha == 1.0 and beta == 0.0:
        return "k_syrk_f64<true>" if alias else "k_syrk_f64<false>"
    if not colscale and not ta and not tb and M % 16 == 0 and N % 16 == 0 and 64 <= K <= 4096 and alpha == 1.0 and beta == 0.0 and (M // 16) * (N // 16) <= 4096:
        return "k_gemm_nn_f64"
    tiles = -(-N // 16) * -(-M // 16)
    ks = 1
    if K >= 256 and tiles < 256:
        ks = min(16, K // 64, (512 + tiles - 1) // tiles)
    if ks > 1:
        kchunk = (-(-K // ks) + 31) // 32 * 32
        ks = -(-K // kchunk)
        return f"k_dgemm split-K ({ks} slices) + k_dgemm_reduce"
    return "k_dgemm"


def _pow2_rows(rng, n):
    return 2.0 ** rng.integers(-20, 21, n)


def dgemm_check(ctx, ta, tb, M, N, K, alpha, beta, alias=False, colscale=False, pad=0, device=True):
    """real-valued data of mixed signs, the rows of op(A) and the columns of op(B) scaled by powers of two from 2^-20 to 2^20 (exact, so
    the relative errors are those of unscaled data, but no tile and no slice is small against another); pad: every leading dimension
    is that much larger than the row"""
    rng = _rng(77, ta, tb, M, N, K, int(alias), int(colscale), pad)
    opa = rng.standard_normal((M, K)) * _pow2_rows(rng, M)[:, None]
    if alias:
        assert ta and not tb and M == N
        opb = opa.T
    else:
        opb = rng.standard_normal((K, N)) * _pow2_rows(rng, N)[None, :]

    def store(op, trans):
        m = np.ascontiguousarray(op.T if trans else op)
        wide = np.full((m.shape[0], m.shape[1] + pad), 1e300)     # (the probe puts NaN between the rows on the device: a read past a row would show)
        wide[:, :m.shape[1]] = m
        return wide[:, :m.shape[1]]
    a = store(opa, ta)
    b = a if alias else store(opb, tb)
    c0 = rng.standard_normal((M, N)) * np.abs(opa).max(axis=1)[:, None] * np.abs(opb).max(axis=0)[None, :]
    cw = np.full((M, N + pad), -7.25)
    cw[:, :N] = c0
    c = cw[:, :N]
    cs = (rng.standard_normal(N) * 2.0 ** rng.integers(-3, 4, N)) if colscale else None
    petal.probe_dgemm(ta, tb, M, N, K, alpha, a, b, beta, c, cs, ctx)
    assert np.all(cw[:, N:] == -7.25), "the words between the rows of C changed"
    assert np.all(np.isfinite(c)), "NaN / inf in C"
    al, bl = opa.astype(LD), opb.astype(LD)
    ref = LD(alpha) * (al @ bl)
    mag = abs(alpha) * (np.abs(opa) @ np.abs(opb))
    if cs is not None:
        ref = ref * cs.astype(LD)[None, :]
        mag = mag * np.abs(cs)[None, :]
    if beta != 0.0:
        ref = ref + LD(beta) * c0.astype(LD)
        mag = mag + np.abs(beta * c0)
    bnd = 1.01 * (K + 2) * U * mag
    model = alpha * (opa @ opb)
    if cs is not None:
        model = model * cs[None, :]
    if beta != 0.0:
        model = model + beta * c0
    tiny = np.finfo(np.float64).tiny
    err = float((np.abs(c.astype(LD) - ref) / (bnd + tiny)).max())
    mod = float((np.abs(model.astype(LD) - ref) / (bnd + tiny)).max())
    assert float((bnd / (np.abs(mag) + tiny)).max()) <= GUARD
    return [("gemm-frac", err, mod, 1.0)]


def dgemm_cases(device):
    cases = []

    def add(ta, tb, M, N, K, alpha=1.0, beta=0.0, alias=False, colscale=False, pad=0, expect=None):
        """expect: the form the row was WRITTEN for, by hand from op_dgemm's dispatch; dgemm_form restates the dispatch and labels the rest"""
        form = dgemm_form(ta, tb, M, N, K, alpha, beta, alias, colscale)
        assert expect is None or form.split(" (")[0] == expect, (form, expect)
        name = f"gemm-{'t' if ta else 'n'}{'t' if tb else 'n'}-{M}x{N}x{K}" + ("-alias" if alias else "") + \
            (f"-a{alpha:g}b{beta:g}" if (alpha, beta) != (1.0, 0.0) else "") + ("-colscale" if colscale else "") + (f"-ld+{pad}" if pad else "")
        cases.append(Case(name, form, dgemm_check, ta, tb, M, N, K, alpha, beta, alias=alias, colscale=colscale, pad=pad, device=device))
    for m in (16, 80, 144, 256):
        for k in (64, 65, 300):
            add(1, 0, m, m, k, alias=True, expect="k_syrk_f64<true>")
            add(1, 0, m, m, k, expect="k_syrk_f64<false>")
    add(1, 0, 80, 80, 65, alias=True, pad=3, expect="k_syrk_f64<true>")
    for m, n, k in ((16, 16, 64), (512, 80, 80), (528, 144, 138), (16, 16, 4096)):
        add(0, 0, m, n, k, expect="k_gemm_nn_f64")
    add(0, 0, 528, 144, 138, pad=8, expect="k_gemm_nn_f64")
    for m, n, k in ((5, 7, 3), (17, 33, 31), (74, 74, 74), (16, 16, 63), (16, 16, 4097)):
        gen = "k_dgemm" if k < 256 else "k_dgemm split-K"       # (one tile and K >= 256: the long reduction is split)
        for ta in (0, 1):
            for tb in (0, 1):
                add(ta, tb, m, n, k, expect="k_syrk_f64<false>" if (k == 4097 and ta and not tb) else gen)
                add(ta, tb, m, n, k, alpha=-1.0, beta=1.0, expect=gen)
                add(ta, tb, m, n, k, colscale=True, expect=gen)
                add(ta, tb, m, n, k, pad=5, expect="k_syrk_f64<false>" if (k == 4097 and ta and not tb) else gen)
    for m, n, k in ((16, 16, 256), (10, 74, 1000), (74, 74, 4097)):
        for ta, tb in ((0, 0), (0, 1), (1, 0)):
            add(ta, tb, m, n, k, alpha=0.5, expect="k_dgemm split-K")
            add(ta, tb, m, n, k, colscale=True, expect="k_dgemm split-K")
            add(ta, tb, m, n, k, alpha=-1.0, beta=1.0, expect="k_dgemm split-K")
            add(ta, tb, m, n, k, alpha=2.0, beta=-0.5, pad=3, expect="k_dgemm split-K")
    forms = {c.form.split(" (")[0] for c in cases}
    assert forms == {"k_syrk_f64<true>", "k_syrk_f64<false>", "k_gemm_nn_f64", "k_dgemm", "k_dgemm split-K"}, forms
    return cases


# ------------------------------------------------------------------------------------------- op_eigh
def eigh_route(L, clustered, jacobi_opt, verdict=False):
    """the kernels op_eigh's launcher (csrc/kernels/host_pow3_eigh.inc) issues for an order: the two-stage forms, then the Jacobi form
    that runs behind a flagged solve (or at once)"""
    two_stage = not jacobi_opt and not clustered and 3 <= L <= 2048
    parts = []
    if two_stage:
        if L <= 80:
            parts.append("k_tridiag_r")
        elif L <= 138:
            parts.append("k_tridiag_w")
        else:
            parts.append("k_tridiag_mw")
        parts.append("k_trieig_r<4,2>" if L <= 128 else "k_trieig_r<4,3>" if L <= 138 else "k_trieig<4>" if L <= 512 else "k_trieig<1>")
        if verdict and L <= 138:
            return " + ".join(parts)
    parts.append(jacobi_form(L))
    return " + ".join(parts)


def jacobi_form(L):
    """JACA_CASE(mb2, gw) as the launcher derives it; k_eigh<0> beyond the LDS limit.  Of the launcher's eight instantiations only
    (1, 32), (2, 32), (4, 16) and (5, 16) can be reached: 16-lane groups need more than 60 row pairs, which is mb2 >= 4, and
    32-lane groups at most 60, which is mb2 <= 2."""
    half = ((L + 1) & ~1) // 2
    if 8 * (L * (L | 1) + 2 * half + 64) > 160 * 1024 - 256:
        return "k_eigh<0>"
    groups = (half + 1) // 2
    pw = (half + 63) // 64 * 64
    gw = 32 if pw + 32 * groups <= 1024 else 16
    mb2 = max(1, (half - 1 + gw - 1) // gw)
    return f"k_jacobi_a<{min(mb2, 5)},{gw}> + k_apply_rot"


def eig_spectrum(kind, L):
    i = np.arange(L, dtype=LD)
    if kind == "geo":
        return LD(0.97) ** (2 * i)
    if kind == "lin":
        return LD(1) - LD(0.5) * i / LD(L)
    if kind == "mult4":
        return LD(0.9) ** np.floor(i / 4)
    if kind == "rank":
        lam = LD(0.97) ** (2 * i)
        lam[L // 2:] = 0
        return lam
    raise KeyError(kind)


def _gap_tol(tol_rel, override=0.0):
    """the closeness threshold of the two-stage solver as op_eigh's launcher sets it"""
    return override if override > 0 else (1e-8 if tol_rel >= 1e-9 else 1e-5)


def _orth_weights(lam, norm, gap_tol):
    """The two-stage solver computes every eigenvector on its own (one wave per pair, no re-orthogonalisation): each is accurate to
    2^-53 ||A|| / gap, so v_i . v_j carries up to 2 x 2^-53 ||A|| / |lam_i - lam_j| -- by design (ops.h: pairs closer than
    gap_tol ||A|| go to Jacobi, the others 'come out only eps / gap_tol accurate').  Its |V^T V - I| is therefore held to the floor
    2^-53 (L + 2 ||A|| / max(|lam_i - lam_j|, gap_tol ||A||)) ELEMENT BY ELEMENT: the element is weighted by L / (L + 2 / relgap_ij)
    and the weighted maximum keeps the floor 2^-53 L of the Jacobi routes (weights 1: a product of rotations)."""
    L = len(lam)
    l64 = np.asarray(lam, dtype=np.float64)
    rel = np.maximum(np.abs(l64[:, None] - l64[None, :]) / (norm if norm > 0 else 1.0), gap_tol)
    w = L / (L + 2.0 / rel)
    np.fill_diagonal(w, 1.0)
    return w


def _eig_flagged(lam, norm, gap_tol):
    """True where the two-stage solver is CERTAIN to flag the spectrum (and the Jacobi form behind it delivers): A = 0, or two
    neighbours closer than gap_tol / 2 x ||A||.  The solver compares the gap with gap_tol x the Gershgorin bound of the tridiagonal
    matrix, which is at least ||A||; a gap between gap_tol / 2 and a few gap_tol may go either way and keeps the two-stage weights,
    which hold for both results."""
    if not norm > 0:
        return True
    l64 = np.asarray(lam, dtype=np.float64)
    return bool((np.abs(np.diff(l64)) / norm).min() < 0.5 * gap_tol)


def _eig_quantities(a, w, v, lam, norm, wt=None):
    al, vl, wl = a.astype(LD), v.astype(LD), w.astype(LD)
    s = LD(norm) if norm > 0 else LD(1)
    e_w = float(np.abs(wl - lam).max() / s)
    r = al @ vl - vl * wl[None, :]
    res = float(np.sqrt((r * r).sum(axis=0)).max() / s)
    g = np.abs(vl.T @ vl - np.eye(len(w), dtype=LD))
    orth = float((g * wt).max() if wt is not None else g.max())
    return e_w, res, orth


def _eig_floors(L, tol_rel):
    """floors of (eig-w, eig-res, eig-orth, eig-angle).  The Jacobi solvers stop at |a_pq| <= tol_rel sqrt(a_pp a_qq): what is left off
    the diagonal moves an eigenvalue in second order (L tol_rel^2), but column j of the residual is that column of the remainder,
    at most tol_rel sqrt(a_jj trace) <= tol_rel sqrt(L) ||A||, and the angle x gap is bounded by the residual.  V stays a product of
    rotations: orthogonal to 2^-53 L whatever tol_rel."""
    fl = U * L
    return fl + L * tol_rel ** 2, max(fl, tol_rel * np.sqrt(L)), fl, max(fl, tol_rel * np.sqrt(L))


def _eig_model(a):
    def make():
        w, v = np.linalg.eigh(a)
        return w[::-1].copy(), v[:, ::-1].copy()
    return make()


def eig_check(ctx, kind, L, tol_rel, clustered=False, jacobi_opt=False, Lz=0, device=True):
    """planted spectra ("geo", "lin", "mult4", "rank"), an exactly diagonal A ("diag") and A = 0 ("zero"): |w - lam| / ||A||, the largest
    residual ||A v - w v|| / ||A||, |V^T V - I| (floors 2^-53 L: Weyl's 2^-53 sqrt(L) for the rounding of A is inside), descending order,
    the zero padding; for the separated spectra also the angle to the planted vector x gap / ||A|| of the eight leading pairs"""
    def make():
        if kind == "zero":
            return np.zeros((L, L)), None, np.zeros(L, dtype=LD), 0.0
        if kind == "diag":
            lam = eig_spectrum("geo", L)
            perm = _rng(31, L).permutation(L)
            return np.diag(lam.astype(np.float64)[perm]), None, np.sort(lam.astype(np.float64).astype(LD))[::-1], 1.0
        lam = eig_spectrum(kind, L)
        a, q = planted(lam, 3)
        return a, q, lam, float(lam[0])
    a, q, lam, norm = _cached(("eigA", kind, L), make)
    wm, vm = _cached(("eigM", kind, L), lambda: _eig_model(a))
    if jacobi_opt:
        ctx.set_option("eigh_jacobi", 1)
    try:
        w, v, _ = petal.probe_eigh(a, tol_rel, clustered, Lz, ctx=ctx)
    finally:
        if jacobi_opt:
            ctx.set_option("eigh_jacobi", 0)
    assert np.all(np.isfinite(w)) and np.all(np.isfinite(v)), "NaN / inf in the result"
    assert np.all(w[:-1] >= w[1:]), "eigenvalues not in descending order"
    if Lz > L:
        assert v.shape == (Lz, Lz) and np.all(v[L:, :] == 0.0) and np.all(v[:, L:] == 0.0), "padding of V not exactly zero"
    v = v[:L, :L]
    floors = _eig_floors(L, tol_rel)
    # (the two-stage weights only where its result may be the one delivered: behind a flagged solve the Jacobi form delivers a product
    # of rotations, held to the plain 2^-53 L)
    two_stage = device and not clustered and not jacobi_opt and L >= 3 and not _eig_flagged(lam, norm, _gap_tol(tol_rel))
    wt = _orth_weights(lam, norm, _gap_tol(tol_rel)) if two_stage else None
    e = _eig_quantities(a, w, v, lam, norm, wt)
    m = _cached(("eigMq", kind, L, two_stage and _gap_tol(tol_rel)), lambda: _eig_quantities(a, wm, vm, lam, norm, wt))
    res = [(f, e[i], m[i], _bound(f, m[i], floors[i], 32 * U * L)) for i, f in enumerate(("eig-w", "eig-res", "eig-orth"))]
    if kind in ("geo", "lin") and L >= 3:
        nj = min(L, 8)
        lam64 = lam.astype(np.float64)
        gap = np.array([min(abs(lam64[j] - lam64[j - 1]) if j else np.inf, abs(lam64[j] - lam64[j + 1]) if j + 1 < L else np.inf) for j in range(nj)])

        def angle(vv):
            cosv = (vv[:, :nj].astype(LD) * q[:, :nj]).sum(axis=0)
            # sin from the component orthogonal to the planted vector (1 - cos^2 cancels)
            perp = vv[:, :nj].astype(LD) - q[:, :nj] * cosv[None, :]
            return float((np.sqrt((perp * perp).sum(axis=0)).astype(np.float64) * gap / norm).max())
        ea, ma = angle(v), angle(vm)
        res.append(("eig-angle", ea, ma, _bound("eig-angle", ma, floors[3], 32 * U * L)))
    return res


def eig_graded_check(ctx, L, route, device=True):
    """A = fl64(D H D), D over 12 decades, cond(H) <= 10.  route "jacobi" (clustered = true, tol_rel = 1e-15): RELATIVE accuracy of every
    eigenvalue against the long-double Hestenes iteration on the transposed Cholesky factor (D R_H^T: a row-scaled well-conditioned
    matrix), floor 2^-53 L cond(H); the model is the same iteration in float64.  route "two-stage": absolute accuracy only."""
    def make():
        q = orth_ld(L, 9)
        h = (q * (LD(1) + LD(9) * np.arange(L, dtype=LD) / max(L - 1, 1))) @ q.T
        d = LD(10) ** (-LD(12) * np.arange(L, dtype=LD) / max(L - 1, 1))
        a = (h * np.outer(d, d)).astype(np.float64)
        a = (a + a.T) / 2.0
        _, r, dead, _ = chol_drop(a, 0.0, LD)
        assert not dead.any()
        lam = hestenes_ld(r.T)[::-1] ** 2
        l64 = np.linalg.cholesky(a)
        s64, _ = hestenes(l64, np.float64)
        d64 = np.sqrt(np.diag(a))
        return a, lam, (s64[::-1] ** 2), float(np.linalg.cond(a / np.outer(d64, d64)))
    a, lam, lam_model, cond_h = _cached(("graded", L), make)
    assert cond_h <= 11.0, cond_h
    w, v, _ = petal.probe_eigh(a, 1e-15, route == "jacobi", 0, ctx=ctx)
    assert np.all(np.isfinite(w)) and np.all(np.isfinite(v)) and np.all(w[:-1] >= w[1:])
    norm = float(lam[0])
    wm, vm = _cached(("gradedM", L), lambda: _eig_model(a))
    wt = _orth_weights(lam, norm, _gap_tol(1e-15)) if (device and route != "jacobi") else None
    e = _eig_quantities(a, w, v, lam, norm, wt)
    m = _cached(("gradedMq", L, wt is None), lambda: _eig_quantities(a, wm, vm, lam, norm, wt))
    floor = U * L
    res = [(f, e[i], m[i], _bound(f, m[i], floor, 32 * U * L)) for i, f in enumerate(("eig-w", "eig-res", "eig-orth"))]
    if route == "jacobi":
        err = float(np.abs(w.astype(LD) / lam - 1).max())
        model = float(np.abs(lam_model.astype(LD) / lam - 1).max())
        res.append(("eig-rel", err, model, _bound("eig-rel", model, U * L * cond_h, 32 * U * L * cond_h)))
    return res


def eig_pair_check(ctx, L, tol_rel, gap_factor, at, verdict_mode, ncheck=0, override=0.0, verdict_in=0, device=True):
    """the spectrum 1 - i / (2 L) with lam[at + 1] moved to lam[at] - gap_factor x gap_tol (||A|| = 1; gap_tol = what tol_rel or the
    override implies; every other gap is 1 / (2 L) >= 3.6e-3)"""
    gap_tol = _gap_tol(tol_rel, override)

    def make():
        lam = eig_spectrum("lin", L)
        lam[at + 1] = lam[at] - LD(gap_factor * gap_tol)
        a, q = planted(lam, 5)
        return a, q, lam
    a, q, lam = _cached(("pair", L, gap_factor, gap_tol, at), make)
    w, v, word = petal.probe_eigh(a, tol_rel, False, 0, ncheck, verdict_mode, verdict_in, override, ctx=ctx)
    assert np.all(np.isfinite(w)) and np.all(np.isfinite(v)) and np.all(w[:-1] >= w[1:])
    close = gap_factor < 1.0 and (ncheck == 0 or at < ncheck)
    unresolved = verdict_mode == 2 and gap_factor < 1.0 and L <= 138     # (delivered as it is, flagged or below ncheck)
    if verdict_mode == 0:
        assert word == -1
    elif verdict_mode == 1:
        assert word == verdict_in and not close, f"verdict word {word}: a preset {verdict_in} must survive a clean solve"
    elif device and L <= 138:
        assert (word != 0) == close, f"verdict word {word} for a pair {gap_factor} x gap_tol apart (ncheck = {ncheck}, pair at {at})"
    else:
        assert word == 0, f"verdict word {word} where the order ignores the verdict"
    wm, vm = _cached(("pairM", L, gap_factor, gap_tol, at), lambda: _eig_model(a))
    floors = _eig_floors(L, tol_rel)
    # (the two-stage weights only where its result is the one delivered: behind a close pair that counts, the Jacobi form delivers)
    wt = _orth_weights(lam, 1.0, gap_tol) if (device and not close) else None
    e = _eig_quantities(a, w, v, lam, 1.0, wt)
    m = _cached(("pairMq", L, gap_factor, gap_tol, at, wt is None), lambda: _eig_quantities(a, wm, vm, lam, 1.0, wt))
    res = [("eig-w", e[0], m[0], _bound("eig-w", m[0], floors[0], 32 * U * L))]
    if not unresolved:      # (a two-stage result delivered as it is: its close vectors are eps / gap accurate only, not mutually orthogonal)
        res += [(f, e[i], m[i], _bound(f, m[i], floors[i], 32 * U * L)) for i, f in ((1, "eig-res"), (2, "eig-orth"))]

        # the invariant subspace of the pair against the planted one: the part of its vectors outside, x the gap to the rest of the spectrum
        def outside(vv):
            qp = q[:, at:at + 2]
            x = vv[:, at:at + 2].astype(LD)
            x = x - qp @ (qp.T @ x)
            return float(np.sqrt((x * x).sum(axis=0)).max()) * (0.5 / L)
        res.append(("eig-angle", outside(v), outside(vm), _bound("eig-angle", outside(vm), floors[3], 32 * U * L)))
    return res


EIG_SEPARATED_L = [3, 4, 16, 17, 74, 80, 81, 128, 129, 138, 139, 160, 513]
EIG_JACOBI_L = [2, 3, 8, 33, 64, 65, 100, 129, 141, 142, 200]


def eig_cases(device):
    cases = []
    hmax = 100
    for L in EIG_SEPARATED_L:
        if not device and L > hmax:
            continue
        for tol in (1e-15, 1e-8):
            cases.append(Case(f"eig-geo-L{L}-tol{tol:.0e}", eigh_route(L, False, False), eig_check, "geo", L, tol, device=device))
    forms = set()
    for i, L in enumerate(EIG_JACOBI_L):
        if not device and L > hmax:
            continue
        forms.add(jacobi_form(L))
        for tol in (1e-15, 1e-8):
            opt = (i + (tol == 1e-8)) % 2 == 1      # the two ways to the Jacobi route in turn: clustered = true | PETAL_OPT_EIGH_JACOBI
            cases.append(Case(f"eig-jacobi-{'opt' if opt else 'clustered'}-L{L}-tol{tol:.0e}", eigh_route(L, not opt, opt), eig_check,
                              "lin" if L > 100 else "geo", L, tol, clustered=not opt, jacobi_opt=opt, device=device))
    if device:
        assert forms == {"k_jacobi_a<1,32> + k_apply_rot", "k_jacobi_a<2,32> + k_apply_rot", "k_jacobi_a<4,16> + k_apply_rot",
                         "k_jacobi_a<5,16> + k_apply_rot", "k_eigh<0>"}, forms
    for kind in ("mult4", "rank", "diag", "zero"):
        for L, cl in ((16, False), (74, False), (74, True), (139, False)):
            if not device and L > hmax:
                continue
            note = "" if (cl or kind == "diag") else " (flagged: the Jacobi form delivers)"
            cases.append(Case(f"eig-{kind}-L{L}-{'jacobi' if cl else 'two-stage'}", eigh_route(L, cl, False) + note,
                              eig_check, kind, L, 1e-15, clustered=cl, device=device))
    for L, Lz, cl in ((74, 80, False), (74, 80, True), (139, 144, False), (139, 144, True), (3, 16, False)):
        if not device and L > hmax:
            continue
        cases.append(Case(f"eig-pad-L{L}-Lz{Lz}-{'jacobi' if cl else 'two-stage'}", eigh_route(L, cl, False) + ", zero padding of V",
                          eig_check, "lin", L, 1e-15, clustered=cl, Lz=Lz, device=device))
    for L in (16, 48, 96):
        for route in ("jacobi", "two-stage"):
            cases.append(Case(f"eig-graded-L{L}-{route}", eigh_route(L, route == "jacobi", False), eig_graded_check, L, route, device=device))
    # closeness verdict
    for L, tol, ov in ((24, 1e-15, 0.0), (74, 1e-8, 0.0), (138, 1e-15, 0.0), (74, 1e-15, 1e-7)):
        for factor in (0.1, 10.0):
            tag = f"L{L}-tol{tol:.0e}" + (f"-gap{ov:.0e}" if ov else "") + f"-{factor:g}x"
            cases.append(Case(f"eig-pair-mode0-{tag}", eigh_route(L, False, False) + " (close pair: the Jacobi form delivers)", eig_pair_check,
                              L, tol, factor, 6, 0, override=ov, device=device))
            if device or factor > 1:       # (the host simulation has no two-stage solver: it never flags)
                cases.append(Case(f"eig-pair-mode2-{tag}", eigh_route(L, False, False, True) + ", verdict_fresh over a preset 77", eig_pair_check,
                                  L, tol, factor, 6, 2, override=ov, verdict_in=77, device=device))
    cases.append(Case("eig-pair-mode1-L74-10x", eigh_route(74, False, False, True) + ", a preset word survives", eig_pair_check,
                      74, 1e-15, 10.0, 6, 1, verdict_in=4, device=device))
    cases.append(Case("eig-pair-ncheck-L74-0.1x", eigh_route(74, False, False, True) + ", close pair at 10 below ncheck = 5", eig_pair_check,
                      74, 1e-15, 0.1, 10, 2, ncheck=5, verdict_in=77, device=device))
    if device:
        cases.append(Case("eig-pair-mode2-L160-0.1x", eigh_route(160, False, False, True) + ", an order that ignores the verdict", eig_pair_check,
                          160, 1e-15, 0.1, 6, 2, verdict_in=77, device=device))
    return cases


# ------------------------------------------------------------------------------------------- op_jacobi_svd_rows
def svd_form(L):
    """k_jacobi_svd_rows<true> while M and G fit 150 KiB of LDS (the launcher's test), else the global-memory form"""
    return "k_jacobi_svd_rows<true>" if 8 * (L + 2 + 2 * L * (L | 1)) <= 150 * 1024 else "k_jacobi_svd_rows<false>"


assert svd_form(97) == "k_jacobi_svd_rows<true>" and svd_form(98) == "k_jacobi_svd_rows<false>"
SVD_L = [1, 2, 3, 17, 64, 96, 97, 98, 130]      # 97 | 98 is the LDS | global-memory switch; odd L: the dummy player


def svd_input(kind, L):
    def make():
        i = np.arange(L, dtype=LD)
        d = LD(10) ** (-LD(12) * i / max(L - 1, 1))
        perm = _rng(41, L).permutation(L)
        if kind == "DQ":
            return (d[perm, None] * orth_ld(L, 11)).astype(np.float64)
        if kind in ("DB", "zero-row"):
            b = (orth_ld(L, 12) * (LD(1) + LD(9) * i / max(L - 1, 1))) @ orth_ld(L, 13).T
            a = (d[perm, None] * b).astype(np.float64)
            if kind == "zero-row":
                a[L // 3, :] = 0.0
            return a
        if kind == "Rinv":
            t, _ = chol_reference(chol_input(L, 1e6), 1e-15)
            return t.astype(np.float64)
        raise KeyError(kind)
    return _cached(("svdA", kind, L), make)


def svd_check(ctx, kind, L, device=True):
    """relative error of every 1 / s against the long-double Hestenes iteration (floor 2^-53 L cond of the row-scaled matrix; model: the
    same iteration in float64), |U^T U - I| and the row norms of U^T A against s, absolute in ||A|| (floors 2^-53 L; model numpy's SVD)"""
    a = svd_input(kind, L)

    def make():
        s = hestenes_ld(a)
        s64, _ = hestenes(a, np.float64)
        nr = np.sqrt((a * a).sum(axis=1))
        live = nr > 0
        cond_rs = float(np.linalg.cond(a[live] / nr[live, None])) if live.sum() > 1 else 1.0
        um, sm, _ = np.linalg.svd(a)
        return s, s64, cond_rs, um[:, ::-1], sm[::-1]
    s_ld, s64, cond_rs, um, sm = _cached(("svdR", kind, L), make)
    if kind == "DQ":       # the reference against what was planted
        i = np.arange(L, dtype=LD)
        assert float(np.abs(s_ld / np.sort(LD(10) ** (-LD(12) * i / max(L - 1, 1))) - 1).max()) < 1e-13
    u, s_inv, nonconv = petal.probe_jacobi_svd_rows(a, ctx)
    assert nonconv == 0, "nonconv set"
    assert np.all(np.isfinite(u)) and np.all(np.isfinite(s_inv)), "NaN / inf in the result"
    s_dev = np.where(s_inv > 0, 1.0 / np.where(s_inv > 0, s_inv, 1.0), 0.0)
    assert np.all(s_dev[:-1] <= s_dev[1:]), "singular values not ascending"
    nz = s_ld > 0
    assert np.all(s_inv[~nz] == 0.0), "s_inv of a zero singular value is not 0"
    norm = float(s_ld[-1])
    err = float(np.abs(s_inv.astype(LD)[nz] * s_ld[nz] - 1).max())
    model = float(np.abs(s64.astype(LD)[nz] / s_ld[nz] - 1).max())
    res = [("svd-rel", err, model, _bound("svd-rel", model, U * L * cond_rs, 32 * U * L * cond_rs))]
    floor = U * L
    eye = np.eye(L, dtype=LD)
    ul, uml, al = u.astype(LD), um.astype(LD), a.astype(LD)
    e_o, m_o = float(np.abs(ul.T @ ul - eye).max()), float(np.abs(uml.T @ uml - eye).max())
    res.append(("svd-orth", e_o, m_o, _bound("svd-orth", m_o, floor, 32 * U * L)))

    def rows(uu, ss):
        wr = uu.T @ al
        return float(np.abs(np.sqrt((wr * wr).sum(axis=1)) - ss.astype(LD)).max() / norm)
    e_r, m_r = rows(ul, s_dev), rows(uml, sm)
    res.append(("svd-rows", e_r, m_r, _bound("svd-rows", m_r, floor, 32 * U * L)))
    return res


def svd_tie_check(ctx, device=True):
    """rows already orthogonal, norms 2, 1, 2, 1, 3, 1: no rotation, and the order is ascending with the LOWER ROW FIRST among equals"""
    d = np.array([2.0, 1.0, 2.0, 1.0, 3.0, 1.0])
    u, s_inv, nonconv = petal.probe_jacobi_svd_rows(np.diag(d), ctx)
    order = [1, 3, 5, 0, 2, 4]
    want = np.zeros((6, 6))
    want[order, np.arange(6)] = 1.0
    bad = int(np.count_nonzero(u != want)) + int(np.count_nonzero(s_inv != 1.0 / d[order])) + nonconv
    return [("svd-tie", float(bad), 0.0, 0.0)]


def svd_cases(device):
    cases = []
    kinds = ["DQ", "DB", "Rinv", "zero-row"]
    for i, L in enumerate(SVD_L):
        for j, kind in enumerate(kinds):
            if L >= 17 and (i + j) % 2 == 1 and L not in (97, 98):      # the sizes at the switch take every input, the others every second one
                continue
            if kind == "zero-row" and L < 3:
                continue
            cases.append(Case(f"svd-{kind}-L{L}", svd_form(L), svd_check, kind, L, device=device))
    cases.append(Case("svd-tie-rule", svd_form(6), svd_tie_check, device=device))
    return cases


# ------------------------------------------------------------------------------------------- the case tables
class Case:
    """id, the kernel form the row is meant to reach, and the check"""

    def __init__(self, name, form, fn, *args, **kw):
        self.id, self.form, self.fn, self.args, self.kw = name, form, fn, args, kw

    def run(self, ctx):
        return self.fn(ctx, *self.args, **self.kw)

    def both_modes(self):
        """the one route that depends on the GEMM mode: the left solve inside the product launcher"""
        return self.fn is chol_check and self.args[3] == 2

    def __repr__(self):
        return self.id


def all_cases(device=True):
    """device = False: the host simulation's table -- without the orders whose references or whose plain Jacobi solves take long on a
    CPU, and without the rows whose route the simulation does not have (a closeness verdict that flags, the blocked Cholesky's
    per-block count): left out here, never skipped"""
    cases = chol_cases(device) + dgemm_cases(device) + eig_cases(device) + svd_cases(device)
    ids = [c.id for c in cases]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return cases


def main():
    import time
    cases = all_cases()
    print("# case | quantity | error | model error | error / max(model, floor) | bound | kernel form")
    t0 = time.time()
    worst, worst_model = {}, {}
    ctx = petal.Context(0)
    for mode in ("bf16x3", "fp32"):
        ctx.set_gemm_mode(mode)
        for c in cases:
            if mode == "fp32" and not c.both_modes():
                continue
            name = c.id + ("-" + mode if c.both_modes() else "")
            try:
                rows = c.run(ctx)
            except (AssertionError, petal.InvalidInput) as e:
                print(f"{name:52s} FAILED: {e}   [{c.form}]", flush=True)
                continue
            except petal.DeviceError as e:      # the device is in an unknown state: nothing more is started on it
                print(f"{name:52s} DEVICE ERROR, report ends here: {e}   [{c.form}]", flush=True)
                return
            for q, err, model, bound in rows:
                denom = bound / MULT[q] if q in MULT else (bound if bound > 0 else float("nan"))
                ratio = err / denom if denom == denom and denom > 0 else float("nan")
                flag = "" if err <= bound else "   <-- ABOVE THE BOUND"
                print(f"{name:52s} {q:10s} {err:10.3e} {model:10.3e} {ratio:8.3f} {bound:10.3e}   [{c.form}]{flag}")
                if ratio == ratio and ratio > worst.get(q, (0.0, ""))[0]:
                    worst[q] = (ratio, name)
                if ratio == ratio and q in MULT and model / denom > worst_model.get(q, (0.0, ""))[0]:
                    worst_model[q] = (model / denom, name)
    ctx.close()
    for q, (r, cid) in sorted(worst.items()):
        mr, mid = worst_model.get(q, (float("nan"), "-"))
        print(f"# {q}: largest error / max(model, floor) {r:.3f} ({cid}); of the float64 model {mr:.3f} ({mid})")
    print(f"# {len(cases)} cases, wall time {time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
