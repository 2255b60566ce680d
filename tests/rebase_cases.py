"""The composite device operations that STEER the optimistic RandomizedPca fit, each through a probe entry of its own
(include/petal_hip_probe.h: petal_probe_rebase, petal_probe_power_pass_means), called the way rpca_fit calls them:
    op_rebase_xp           k_chol_rt4 + substitution inside K1's packing | k_chol_rt4 + op_trsm_right + op_gemm_xp | explicit inverse
    op_rebase_power_pass   k_chol_rt4<NB>, k_trsm_pack<NB, true> (the two-plane rounded P_out and its operand planes), the fused pass
    op_power_pass_means    k_pow3 / k_pow3f in their MEANS form, k_mean_fix<false>, k_mean_fix<true>
Inside a fit these only steer a self-correcting iteration that is judged at 1e-5 after five passes; here each is held to an exact or
long-double reference of its own statement.  Shared by tests/test_gpu_rebase.py (the HIP library, both GEMM modes) and
tests/test_rebase_hostsim.py (the host simulation oracle/cpu_ops.cpp, a reduced table: it proves the references, certificates and
bounds without a GPU and holds the simulation to the same contract).

TABLE A -- exact-integer re-basing: every output bit for bit.
  R = D (I + N): D a diagonal of powers of two (1, 2, 4), N strictly upper triangular with entries +-1 in (even row, odd column)
  positions only, so N^2 = 0 and R^-1 = (I - N) D^-1 exactly.  G = R^T R in integers.  A = 4 x integers in [-2, 2], so P = A R^-1 is an
  integer matrix; X - mu in {-1, 0, 1} (a quarter non-zero), mu integer or absent.  CERTIFICATE, asserted on the reference before any
  device call: R R^-1 = I and G exact in int64; |P| < 2^16 and |Z| < 2^16 (integers below 2^16 have at most 16 significant bits:
  two_plane() is the identity on them, asserted -- the two-plane roundings of P_out, of Xc and of z in the steering forms are no-ops);
  sum_k |xc_ik| |p_kj| < 2^24 and sum_i |xc_if| |z_ij| < 2^24 (every fp32 partial sum of any slab, in any order, is an integer below
  2^24).  Cholesky of such a G and the substitution touch integers and dyadic fractions only.  A DEPENDENT column j: row j of R is zero,
  so the pivot of column j is exactly 0 -- that column of P_out, Z and Y is zero, the other columns are A_live R_live^-1, and *ndead
  comes back as max(incoming, 1).  Columns L .. M - 1 of A hold non-zero integers; columns L .. M - 1 of P_out, Z and Y must be 0.0.
  The dispatch arm of op_rebase_xp a case reaches is part of its form: [arm 1] RT form with the substitution inside K1's packing (fp32,
  split-product mode, L <= 140), [arm 2] RT form with op_trsm_right and op_gemm_xp (fp32-MFMA mode or fp64 data, L <= 140), [arm 3] the
  explicit inverse with op_gemm_xp_prod (L = 144 > 140).

TABLE B -- re-basing on real iterates: A = Yp (K x L Gaussian, column norms spread over 1e3), G = fl64(Yp^T Yp).
  Reference in long double: R = chol(G), P = A R^-1 by substitution.
  P_out: with p_planes = 2 in the split-product mode two_plane(P_out) == P_out bit for bit (structural), and
         |P_out - P_ld| <= 2^-17 |P_ld| + L 2^-52 cond(R) max |P_ld|     (cond from the reference; without the rounding: the second term alone)
         -- a case of its own beside each case ("-Pbound"), so that a miss does not hide Z and Y.  The first term is what a rounding
         to two bf16 pieces costs when BOTH are rounded from the fp64 value; k_trsm_pack<NB, true> once went through float32 first,
         whose 2^-24 |P| came on top: one element in some 25000 was 1.0005 .. 1.004 times this bound (four device cases, one
         on the host simulation), and the kernel and the simulation now round from the fp64 value.
  Z and Y are judged against products of the RETURNED P_out, with the error classes of tests/plane_cases.py (its functions: planes,
  piece_sums, bounded_class_bound): an element of a product of U on pu planes and V on pv planes is within (3 + T) 2^-24 S of the exact
  product of the operands rounded to those planes.  Z = Xc P_out: (pu, pv) restates the dispatch ((3, 2); (2, 2) for a steering product
  of more than 80 columns; (3, 3) with p_planes = 3; the fp32-MFMA kernel: T = K terms of float32 operands).  Y = Xc^T z of the fused
  pass ((3, 2) then (3, 3); k_pow3f: (2, 2) twice) is taken over the device's own z, which route 1 does not return:
        |Y - Y_ref| <= |Xc|^T E_z + (3 + T2) 2^-24 S2,   E_z = the bound of the first product (+ 2^-17 (|z| + E_z): k_pow3f rounds z),
        S2 <= (1 + 2^-7) |Xc|^T (|z| + E_z),  T2 = the kept piece products of the 32 s rows of ONE workgroup's slab (the slabs
        are added in fp64: 2^-47 S2).
  The references are sums of EXACT float64 products (24 x <= 24 bits) in chunks of 32 terms added in long double: their own error,
  2^-48 S, is added to each bound.

TABLE C -- the means fold.  x (n x K float32, d real columns), P (K x N, L < N real columns), P2 = two_plane(P).
  Reference, long double throughout: mean_f, tv = sum (x - mean)^2, Y = (sum x x^T - n mean mean^T) P2 (the x x^T products are exact
  in float64, summed in chunks in long double).  Every bound is formed from the inputs and the RETURNED provisional centre mu0 (itself
  asserted to be the float32 mean of the strided row sample): xc0 = fl32(x - mu0) as the kernel subtracts, a_f = mean_i |xc0_if|,
  ssq0 = sum xc0^2, delta = mean - mu0.  With s stages of 32 rows per workgroup (ceil(n / 32) stages over min(CUs, stages) workgroups):
    mu64, muT   muT == float32(mu64) exactly.  EXACT class: |mu64_f - mean_f| <= e1_f = 2^-24 (32 s) a_f (fp32 accumulation inside a
                slab; the rounding of the fp32 subtraction, 2^-25 a_f, is the slack between (32 s - 1) and 32 s) + 2^-50 |mean_f|.
                TWO-PLANE class (product 2 reads x - mu0 rounded to two bf16 planes): e2_f = e1_f + 2^-17 a_f.  The contract (ops.h)
                is the two-plane class in the steering form k_pow3f, the exact class in k_pow3<.., MEANS>.  What tells the classes
                apart is not the size of the bounds but that the rounding r = two_plane(xc0) - xc0 is a function of the value: on
                continuous data its column mean is rms(r) / sqrt(n), on columns of few distinct values every equal value carries the
                same r and the column mean B_f = mean_i r_if does not shrink with n.  The families: (i) Gaussian about |mu| = 40
                sigma with one planted direction, (ii) its rows sorted along that direction, (iii) binary {0, 1} columns with
                probabilities 0.01 .. 0.5, (iv) Poisson counts with rates 0.05 .. 3, (v) two arbitrary float32 levels a column, each taken by 30 .. 70 % of the rows.  For
                (iii) and (iv) the classes COINCIDE: mu0 is the mean of 4096 sampled integers, a multiple of 2^-12, so x - mu0 has
                at most 16 significant bits and its two-plane rounding is the identity -- asserted on the reference (r == 0), and
                the means of these families are held to the EXACT class in both forms.  (v) takes their place for what they were
                meant to show: it asserts on the reference alone that B_f != 0 and |B_f| >= 50 rms(r_f) / sqrt(n) in at least half
                the columns, and is held to the two-plane class -- and to the exact class with PETAL_OPT_STEERING off.  In the
                steering form EVERY family is also held to |mu64_f - mean_f - B_f| <= e1_f: the sums are those of the rounded
                values and of nothing else (this is what caught mu64 = fl64(sample mean) + delta, with delta taken about the
                FLOAT32 sample mean the kernel subtracts: an error of up to 2^-25 |mu_f|, 1.4 e1 on family (i)).  The report names the class each case lands in
                (whether mu64 - mean follows B_f).
    tv          |tv - tv_ld| <= ((32 FC / 2) s + 72) 2^-24 ssq0 + 2^-50 ssq0 + n sum_f (2 |delta_f| e_f + e_f^2),   FC = K / 256.
                A lane adds 2 FC values q2 per stage, each from a chain of eight fmas: a term passes 8 + 2 FC s roundings, below the
                16 FC s of a plain serial sum of all the lane's terms; 72 covers the six levels of the wave reduction and the two
                roundings of the fp32 subtraction.  The last term is what the error of the means (e_f: the class bound) does to
                n |delta|^2.  The report also gives the error against the first two terms alone (tv/accum: a regression of the
                accumulation shows there even where delta is large) and against sqrt(16 FC s) 2^-25 ssq0, the random-walk estimate.
    Y           |Y - Y_ld| <= (3 x 2^-17 + 2^-24 (K + 32 s)) |Xc0|^T (|Xc0| |P2|)     (k_pow3f: Xc0 twice and z on two planes;
                k_pow3<.., MEANS>: 6 x 2^-24 in place of 3 x 2^-17, the dropped pieces of weight 2^-24 of two products)
                + n (|e| (|delta|^T |P2|) + |delta| (|e|^T |P2|) + |e| (|e|^T |P2|)) + (K + 8) 2^-52 n |delta| (|delta|^T |P2|)
                (the correction formed with the device's delta, and its fp64 arithmetic) + 2^-44 x the cancellation of the reference.
                Column N - 1 is exact zeros, columns L .. N - 2 are zero.  The SORTED family at n = 12287 (stride 2: the sample
                sees the first 8192 rows only, mu0 is far from the mean) asserts on the reference that the correction
                n delta (delta^T P2) exceeds the bound 100 times in at least half the entries.
    exact       a fold in which every step is exact, all outputs bit for bit (a wrong sign or a missing piece of the correction, the
                unrounded P in it, sums read after they were cleared: each an exact mismatch): n a power of two; x - m in {-1, 0, 1},
                four non-zeros a row, integer m; the sampled rows cancel in pairs, so mu0 = m exactly and delta = (column sums) / n
                is dyadic; P = c (1 + 2^-10 + 2^-20), c in {+-1, +-2}: a float32 number whose two-plane rounding is c (1 + 2^-10)
                != P; z = Xc0 P2 is a multiple of 2^-10 below 2^4 (16 bits: its two-plane rounding in k_pow3f is a no-op), the fp32
                slab sums of Y' are multiples of 2^-10 below 2^14, the column sums and sum (x - mu0)^2 small integers, and the fp64
                correction n delta (delta^T P2) involves dyadic numbers of fewer than 53 bits.  All asserted on the reference.
    refusals    L == N, fp64 data, the fp32-MFMA mode, means_fold_rows < 0, two_plane_omega off, n below fused_pass_min_rows: done == 0
                and every output still NaN.   determinism: two identical calls, identical bytes.

Each check takes a ctx and returns a list of (quantity, error, reference figure, bound) with error <= bound asserted by the runner;
what is exact is reported as a count of differing elements with bound 0.  `python tests/rebase_cases.py` runs every case on
petal.Context(0) in both GEMM modes and prints one line per case and quantity: the report kept in profiles/rebase_errors.txt."""
import math
import os
import sys

import numpy as np

if __name__ == "__main__":      # (run as a script: the package is found from the repository root)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import petal_decomposition_amd as petal
import plane_cases as pc

LD = np.longdouble
SIM_CUS = 256                      # the host simulation has no workgroups: the bounds are formed as for 256 of them
RT_MAXL, RT_MAXM = 140, 144        # where the RT form exists (ops.h)
NS = [8192, 8193, 12001]
_cache = {}


def _cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def two_plane(p):
    """float64 -> the sum of the two leading bf16 pieces of float32(p), as float64 (k_trsm_pack<NB, true>, k_pack_p3, k_mean_fix)"""
    return pc.split2(np.asarray(p, dtype=np.float32)).astype(np.float64)


def cus(device):
    if not device:
        return SIM_CUS
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def ndiff(a, b):
    """elements of a that are not bit-for-bit the values of b (NaN differs from everything)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.count_nonzero(~(a == b)))


def all_nan(*arrs):
    return all(bool(np.isnan(np.asarray(a, dtype=np.float64)).all()) for a in arrs)


def exact_matmul_ld(ut, v, chunk=32):
    """sum_t ut[t, a] v[t, b] in long double from float64 products that are exact (the operands carry <= 24 + 29 bits together),
    chunk terms at a time: error <= chunk 2^-53 sum |terms|"""
    ut, v = np.asarray(ut, dtype=np.float64), np.asarray(v, dtype=np.float64)
    out = np.zeros((ut.shape[1], v.shape[1]), dtype=LD)
    for s in range(0, ut.shape[0], chunk):
        out += (ut[s:s + chunk].T @ v[s:s + chunk]).astype(LD)
    return out


# ------------------------------------------------------------------------------------------- table A: exact integers
def exact_factor(L, seed, dead=None):
    """(R, R_live^-1 padded to L x L with the dead row / column zero, G) -- all float64 holding integers and dyadic fractions"""
    rng = _rng(11, L, seed)
    dg = 2.0 ** rng.integers(0, 3, L)
    nn = np.zeros((L, L))
    for j in range(1, L, 2):
        ev = np.arange(0, j, 2)
        for i in rng.choice(ev, size=min(len(ev), 2), replace=False):
            nn[i, j] = rng.choice([-1.0, 1.0])
    if dead is not None:
        assert dead % 2 == 1 and np.any(nn[:, dead] != 0), "the dependent column needs entries above its pivot"
        dg[dead] = 0.0
    r = dg[:, None] * (np.eye(L) + nn)
    live = np.array([j for j in range(L) if j != dead])
    rinv = np.zeros((L, L))
    rinv[np.ix_(live, live)] = ((np.eye(L) - nn) / np.where(dg > 0, dg, 1.0)[None, :])[np.ix_(live, live)]
    assert np.array_equal(r[np.ix_(live, live)] @ rinv[np.ix_(live, live)], np.eye(len(live))), "certificate: R R^-1 != I"
    g = r.T @ r
    ri = r.astype(np.int64)
    assert np.array_equal(ri.astype(np.float64), r) and np.array_equal((ri.T @ ri).astype(np.float64), g), "certificate: G is not exact"
    if dead is not None:
        assert g[dead, dead] > 0
    return r, rinv, g


def exact_data(n, K, with_mu, dtype, seed):
    def make():
        rng = _rng(12, n, K, seed)
        xc = (rng.integers(-1, 2, (n, K)) * (rng.random((n, K)) < 0.375)).astype(np.float64)
        mu = rng.integers(-5, 6, K).astype(np.float64) if with_mu else None
        x = (xc + (mu if with_mu else 0.0)).astype(dtype)
        if with_mu:
            assert np.array_equal(x - mu.astype(dtype), xc.astype(dtype)), "certificate: x - mu is not exact"
        return x, (mu.astype(dtype) if with_mu else None), xc
    return _cached(("xa", n, K, with_mu, np.dtype(dtype).name, seed), make)


def rebase_arm(split, dtype, L):
    if L > RT_MAXL:
        return "arm 3: explicit inverse + op_gemm_xp_prod"
    if split and dtype == np.float32:
        return "arm 1: RT form, substitution inside K1's packing"
    return "arm 2: RT form, op_trsm_right + op_gemm_xp"


def fused_applies(split, dtype, n, K, M, device):
    return split and dtype == np.float32 and M <= 80 and (K in (256, 512) if device else K % 16 == 0) and n >= (8192 if device else 64)


def exact_check(ctx, route, NB, L, n, K, with_mu, steering, planes, dtype=np.float32, dead=None, ndead_in=0, device=True, split=True):
    M = 16 * NB
    seed = 1000 * route + 10 * NB + (dead or 0)
    _, rinv, g = exact_factor(L, seed, dead)
    rng = _rng(13, seed, K, L)
    a = 4.0 * rng.integers(-2, 3, (K, M))
    a[:, L:] = 4.0 * rng.integers(1, 3, (K, M - L))            # (non-zero: the padding columns of the result must not depend on them)
    x, mu, xc = exact_data(n, K, with_mu, dtype, seed % 3)
    p = np.zeros((K, M))
    p[:, :L] = a[:, :L] @ rinv
    z = xc @ p
    y = xc.T @ z
    # the certificate: the reference alone satisfies every exactness condition
    assert np.array_equal(p, np.rint(p)) and np.abs(p).max() < 2 ** 16 and np.array_equal(two_plane(p), p), "certificate: P"
    assert np.abs(z).max() < 2 ** 16 and np.array_equal(two_plane(z), z), "certificate: Z"
    assert (np.abs(xc) @ np.abs(p)).max() < 2 ** 24, "certificate: the fp32 sums of Z"
    assert (np.abs(xc).T @ np.abs(z)).max() < 2 ** 24, "certificate: the fp32 slab sums of Y"
    if dead is not None:
        assert not p[:, dead].any() and p[:, :L].any(axis=0).sum() == L - 1
    r = petal.probe_rebase(x, mu, g, a, 1e-15, planes, steering, route, ndead_in, ctx=ctx)
    rows = []
    if route > 0 and not fused_applies(split, dtype, n, K, M, device):
        assert r["done"] == 0, "the fused pass has no kernel for this mode / shape"
        assert all_nan(r["p_out"], r["y"]) and (r["z"] is None or all_nan(r["z"])), "a refused call wrote to its outputs"
        assert r["ndead"] == ndead_in
        return [("refused", 0.0, 0.0, 0.0)]
    assert r["done"] == 1
    want_dead = max(ndead_in, 1 if dead is not None else 0)
    rows.append(("ndead", float(abs(r["ndead"] - want_dead)), float(want_dead), 0.0))
    rows.append(("P_out", ndiff(r["p_out"], p), float(np.abs(p).max()), 0.0))
    if route != 1:
        rows.append(("Z", ndiff(r["z"], z), float(np.abs(z).max()), 0.0))
    if route != 0:
        rows.append(("Y", ndiff(r["y"], y), float(np.abs(y).max()), 0.0))
    return rows


# ------------------------------------------------------------------------------------------- table B: real iterates
def chol_ld(g):
    L = g.shape[0]
    g = g.astype(LD)
    r = np.zeros((L, L), dtype=LD)
    for j in range(L):
        s = g[j, j] - (r[:j, j] * r[:j, j]).sum()
        assert s > 0
        r[j, j] = np.sqrt(s)
        if j + 1 < L:
            r[j, j + 1:] = (g[j, j + 1:] - r[:j, j] @ r[:j, j + 1:]) / r[j, j]
    return r


def solve_right_ld(a, r):
    """A R^-1 for upper triangular R, column by column"""
    a = a.astype(LD)
    p = np.zeros_like(a)
    for j in range(r.shape[0]):
        p[:, j] = (a[:, j] - p[:, :j] @ r[:j, j]) / r[j, j]
    return p


def real_data(n, K):
    def make():
        rng = _rng(21, n, K)
        mu = (rng.standard_normal(K) * 3).astype(np.float32)
        x = (rng.standard_normal((n, K)) * (0.5 + rng.random(K)) + mu).astype(np.float32)
        xc = x - mu                                             # float32, as the kernels subtract
        return x, mu, xc
    return _cached(("xb", n, K), make)


def gram_ld(n, K, pu):
    """C = U^T U in long double, U = Xc on pu planes (exact float64 products, chunks of 32 rows)"""
    def make():
        u = real_data(n, K)[2]
        u = pc.split2(u) if pu == 2 else u
        return exact_matmul_ld(u, u)
    return _cached(("cb", n, K, pu), make)


def product_bound(ut, v, pu, pv):
    """(S, bound) of out = U^T V by the kept piece products: plane_cases' bounded class, (3 + T) 2^-24 S, plus the reference's 2^-48 S"""
    up, _ = pc.planes(ut, pu)
    vp, _ = pc.planes(v, pv)
    f8 = np.float64
    au, av = [np.abs(q).astype(f8) for q in up], [np.abs(q).astype(f8) for q in vp]
    nu, nv = [(q != 0).astype(f8) for q in up], [(q != 0).astype(f8) for q in vp]
    S, _, T = pc.piece_sums(au, av, nu, nv)
    return S, pc.bounded_class_bound(S, T) + 2.0 ** -48 * S


def real_check(ctx, route, NB, L, steering, planes, part="products", n=8200, K=256, device=True, split=True):
    M = 16 * NB
    rng = _rng(22, route, NB, L)
    scale = 10.0 ** (3.0 * rng.permutation(L) / max(L - 1, 1))
    yp = rng.standard_normal((K, L)) * scale
    a = np.zeros((K, M))
    a[:, :L] = yp
    g = yp.T @ yp
    x, mu, xc = real_data(n, K)
    r_ld = chol_ld(g)
    p_ld = np.zeros((K, M), dtype=LD)
    p_ld[:, :L] = solve_right_ld(yp, r_ld)
    cond = float(np.linalg.cond(r_ld.astype(np.float64)))
    r = petal.probe_rebase(x, mu, g, a, 1e-15, planes, steering, route, 0, ctx=ctx)
    if route > 0 and not fused_applies(split, np.float32, n, K, M, device):
        assert r["done"] == 0 and all_nan(r["p_out"], r["y"]) and (r["z"] is None or all_nan(r["z"])) and r["ndead"] == 0
        return [("refused", 0.0, 0.0, 0.0)]
    assert r["done"] == 1 and r["ndead"] == 0
    po = r["p_out"]
    # (ops.h: P_out is rounded where the factor is applied in RT form; the explicit-inverse arm, L > 140, keeps it unrounded and
    #  multiplies by float32(P_out) on three planes)
    rounded = split and (planes == 2 or route > 0) and L <= RT_MAXL
    rows = []
    if rounded:
        rows.append(("P=2plane", ndiff(two_plane(po), po), 0.0, 0.0))           # structural: P_out IS its own two-plane rounding
    assert not po[:, L:].any() and not np.isnan(po).any(), "columns L .. M - 1 of P_out are not exact zeros"
    if part == "p_out":
        pb = (2.0 ** -17 * np.abs(p_ld) if rounded else 0) + L * 2.0 ** -52 * cond * np.abs(p_ld).max()
        perr = np.abs(po.astype(LD) - p_ld)
        over = int(np.count_nonzero(perr > pb))
        rows.append(("P_out", float((perr / pb).max()), float(np.abs(p_ld).max()), 1.0))
        rows.append((f"over:{over}", 0.0, 0.0, 0.0))
        return rows
    # the products of the RETURNED P_out
    if route == 0:
        pu, pv = (3, 3) if not split else ((2 if steering and planes == 2 and M > 80 else 3), (2 if rounded else 3))
    else:
        pu, pv = ((2, 2) if route == 1 and steering and ctx.get_option("steering_passes") != 0 else (3, 2))
    v = po.astype(np.float32)                                    # the kernels' operand: float32(P_out) (two planes: P_out itself)
    u = pc.split2(xc) if pu == 2 else xc
    z_ld = exact_matmul_ld(u.T, v)
    if split:
        _, ez = product_bound(u.T, v, pu, pv)
    else:                                                         # the fp32-MFMA kernel: K terms of float32 operands
        S = np.abs(u.astype(np.float64)) @ np.abs(v.astype(np.float64))
        ez = (3.0 + K) * 2.0 ** -24 * S + 2.0 ** -48 * S
    if route != 1:
        z = r["z"]
        assert not z[:, L:].any() and not np.isnan(z).any(), "columns L .. M - 1 of Z are not exact zeros"
        zerr = np.abs(z.astype(LD) - z_ld).astype(np.float64)
        ok = ez > 0
        assert not zerr[~ok].any()
        rows.append(("Z", float((zerr[ok] / ez[ok]).max()), float(np.abs(z_ld).max()), 1.0))
    if route != 0:
        y = r["y"]
        assert not y[:, L:].any() and not np.isnan(y).any(), "columns L .. M - 1 of Y are not exact zeros"
        y_ld = gram_ld(n, K, pu) @ v.astype(LD)
        za = np.abs(z_ld).astype(np.float64)
        ezt = ez + (2.0 ** -17 * (za + ez) if pu == 2 else 0.0)
        ua = np.abs(u.astype(np.float64))
        S2 = (1.0 + 2.0 ** -7) * (ua.T @ (za + ezt))
        stages = -(-n // 32)
        rows_wg = 32 * -(-stages // min(cus(device), stages))       # fp32 sums inside a workgroup's slab, fp64 across slabs
        T2 = float(rows_wg) * (4 if pu == 2 else 6)
        yb = ua.T @ ezt + pc.bounded_class_bound(S2, T2) + 2.0 ** -47 * S2
        yerr = np.abs(y.astype(LD) - y_ld).astype(np.float64)
        ok = yb > 0
        assert not yerr[~ok].any()
        rows.append(("Y", float((yerr[ok] / yb[ok]).max()), float(np.abs(y_ld).max()), 1.0))
    return rows


# ------------------------------------------------------------------------------------------- table C: the means fold
FAMILIES = ["gauss", "sorted", "binary", "counts", "levels"]


def fold_data(n, K, d, family):
    def make():
        rng = _rng(31, n, K, d, FAMILIES.index(family))
        x = np.zeros((n, K), dtype=np.float32)
        if family in ("gauss", "sorted"):
            # (i) Gaussian about |mu| = 40 sigma: unit noise and one planted direction w (a random one); (ii) the same rows sorted along it
            w = rng.standard_normal(d)
            gl = rng.standard_normal(n)
            if family == "sorted":
                gl = np.sort(gl)
            sig = np.sqrt(1.0 + 16.0 * w * w)
            mu = 40.0 * sig * rng.choice([-1.0, 1.0], d)
            x[:, :d] = (rng.standard_normal((n, d)) + 4.0 * gl[:, None] * w[None, :] + mu).astype(np.float32)
        elif family == "binary":
            pr = 10.0 ** rng.uniform(-2.0, math.log10(0.5), d)
            x[:, :d] = (rng.random((n, d)) < pr).astype(np.float32)
        elif family == "counts":
            lam = 10.0 ** rng.uniform(math.log10(0.05), math.log10(3.0), d)
            x[:, :d] = rng.poisson(lam, (n, d)).astype(np.float32)
        else:
            # (v) two LEVELS a column, arbitrary float32 numbers, taken with probabilities 0.3 .. 0.7: binary data that is not {0, 1}
            a = rng.random(d)
            b = a + 0.25 + rng.random(d)
            x[:, :d] = np.where(rng.random((n, d)) < rng.uniform(0.3, 0.7, d), b, a).astype(np.float32)
        return x
    return _cached(("xc", n, K, d, family), make)


def fold_reference(n, K, d, family):
    """long double: (mean, tv, S = sum x x^T) -- the products x x^T are exact in float64, 256 rows at a time"""
    def make():
        x = fold_data(n, K, d, family)
        s1 = np.zeros(K, dtype=LD)
        for s in range(0, n, 4096):
            s1 += x[s:s + 4096].astype(LD).sum(axis=0)
        mean = s1 / LD(n)
        tv = LD(0)
        for s in range(0, n, 4096):
            t = x[s:s + 4096].astype(LD) - mean
            tv += (t * t).sum()
        x8 = x.astype(np.float64)
        return mean, tv, exact_matmul_ld(x8, x8, chunk=256)
    return _cached(("rc", n, K, d, family), make)


def fold_p(K, N, L, d):
    rng = _rng(32, K, N, L, d)
    p = np.zeros((K, N))
    p[:d, :L] = rng.standard_normal((d, L))
    return p


def sample_mean32(x, n):
    ns = min(n, 4096)
    return x[::n // ns][:ns].astype(np.float64).mean(axis=0).astype(np.float32)


def fold_terms(x, mu0, mean, p2, n, K, ncu, steering_form, two_plane_sums=None):
    """every figure the bounds need, from the inputs and the provisional centre alone"""
    xc0 = x - mu0.astype(np.float32)                              # float32, as the kernel subtracts
    a8 = np.abs(xc0).astype(np.float64)
    af = a8.mean(axis=0)
    stages = -(-n // 32)
    s = -(-stages // min(ncu, stages))
    e1 = 2.0 ** -24 * (32 * s) * af + 2.0 ** -50 * np.abs(mean).astype(np.float64)
    e2 = e1 + 2.0 ** -17 * af
    rr = (pc.split2(xc0) - xc0).astype(np.float64)               # (exact: both are float32 numbers 2^-16 apart at most)
    B = rr.mean(axis=0)
    rms = np.sqrt((rr * rr).mean(axis=0))
    ssq0 = float((xc0.astype(np.float64) ** 2).sum())
    delta = (mean - mu0.astype(LD)).astype(np.float64)
    e = e2 if (steering_form if two_plane_sums is None else two_plane_sums) else e1
    ap = np.abs(p2)
    w = a8.T @ (a8 @ ap)
    coef = (3 * 2.0 ** -17 if steering_form else 6 * 2.0 ** -24) + 2.0 ** -24 * (K + 32 * s)
    ad = np.abs(delta)
    corr_err = n * (np.outer(e, ad @ ap) + np.outer(ad, e @ ap) + np.outer(e, e @ ap)) + (K + 8) * 2.0 ** -52 * n * np.outer(ad, ad @ ap)
    FC = K // 256
    tvb0 = ((16 * FC) * s + 72) * 2.0 ** -24 * ssq0 + 2.0 ** -50 * ssq0
    tvb = tvb0 + n * float((2 * ad * e + e * e).sum())
    return {"af": af, "e1": e1, "e2": e2, "B": B, "rms": rms, "ssq0": ssq0, "delta": delta, "s": s, "ybound": coef * w + corr_err,
            "pass_bound": coef * w, "corr": n * np.outer(delta, delta @ p2), "tvb": tvb, "tvb0": tvb0, "rw": math.sqrt(16 * FC * s) * 2.0 ** -25 * ssq0}


def fold_check(ctx, n, K, N, L, d, family, steering_on=True, device=True, split=True):
    x = fold_data(n, K, d, family)
    mean, tv_ld, sxx = fold_reference(n, K, d, family)
    p = fold_p(K, N, L, d)
    p2 = two_plane(p)
    ncu = cus(device)
    # ---- on the reference alone (the provisional centre predicted in numpy)
    tps = steering_on and family not in ("binary", "counts")
    t = fold_terms(x, sample_mean32(x, n), mean, p2, n, K, ncu, steering_on, tps)
    if family in ("binary", "counts"):
        # integers below 16 about mu0 = (an integer) / 4096: x - mu0 has at most 16 significant bits and its two-plane rounding is the
        # identity -- on these families the two classes COINCIDE, and the means are held to the exact class in both forms
        assert not t["rms"].any() and not t["B"].any(), "certificate: x - mu0 is not exactly representable on two planes"
    if family == "levels":
        apart = (t["B"][:d] != 0) & (np.abs(t["B"][:d]) >= 50.0 * t["rms"][:d] / math.sqrt(n))
        assert 2 * np.count_nonzero(apart) >= d, f"certificate: the two-plane bias stands out in {np.count_nonzero(apart)} of {d} columns only"
    if family == "sorted" and 4 * (n // min(n, 4096)) * min(n, 4096) <= 3 * n:      # (the sample misses the tail of the rows: n = 12287)
        big = np.abs(t["corr"][:d, :L]) >= 100.0 * t["ybound"][:d, :L]
        assert 2 * np.count_nonzero(big) >= big.size, f"certificate: the correction exceeds 100 bounds in {np.count_nonzero(big)} of {big.size} entries only"
    y_ld = (sxx - LD(n) * np.outer(mean, mean)) @ p2.astype(LD)
    ref_err = 2.0 ** -44 * ((np.abs(sxx) + LD(n) * np.abs(np.outer(mean, mean))).astype(np.float64) @ np.abs(p2))
    # ---- the call, twice
    before = ctx.get_option("steering_passes")
    ctx.set_option("steering_passes", 1 if steering_on else 0)
    try:
        r = petal.probe_power_pass_means(x, p, L, d, ctx=ctx)
        r2 = petal.probe_power_pass_means(x, p, L, d, ctx=ctx)
    finally:
        ctx.set_option("steering_passes", before)
    assert r["done"] == 1 and r2["done"] == 1
    same = all(np.asarray(r[k]).tobytes() == np.asarray(r2[k]).tobytes() for k in ("y", "mu64", "muT", "mu0", "tv"))
    mu0 = r["mu0"].astype(np.float32)
    assert np.array_equal(mu0.astype(np.float64), r["mu0"])
    pred = sample_mean32(x, n)
    assert np.all(np.abs(mu0 - pred) <= np.spacing(np.abs(pred))), "mu0 is not the float32 mean of the strided row sample"
    if not np.array_equal(mu0, pred):
        t = fold_terms(x, mu0, mean, p2, n, K, ncu, steering_on, tps)
    rows = [("repeat", 0.0 if same else 1.0, 0.0, 0.0)]
    rows.append(("muT", ndiff(r["muT"], r["mu64"].astype(np.float32).astype(np.float64)), 0.0, 0.0))
    merr = (r["mu64"].astype(LD) - mean).astype(np.float64)
    e = t["e2"] if steering_on and family not in ("binary", "counts") else t["e1"]
    assert not merr[e == 0].any(), "a column without spread has a mean that is not exact"
    live = e > 0
    rows.append(("mean/e1", float((np.abs(merr[live]) / t["e1"][live]).max()), 0.0, float("inf")))      # (reported: the exact class)
    rows.append(("mean", float((np.abs(merr[live]) / e[live]).max()), float(np.abs(mean).max()), 1.0))
    follows = float(np.abs(merr - t["B"]).sum()) < 0.25 * float(np.abs(merr).sum())
    plain = float(np.abs(merr).sum()) < 0.25 * float(np.abs(merr - t["B"]).sum())
    cls = "two-plane" if follows else ("exact" if plain or not t["B"].any() else "undetermined")
    if steering_on:      # (every family: the sums ARE those of the rounded values -- on continuous data B_f is merely small)
        rows.append(("mean-B", float((np.abs(merr - t["B"])[live] / t["e1"][live]).max()), float(np.abs(t["B"]).max()), 1.0))
    tverr = abs(float(LD(r["tv"]) - tv_ld))
    rows.append(("tv", tverr / t["tvb"], float(tv_ld), 1.0))
    rows.append(("tv/accum", tverr / t["tvb0"], 0.0, float("inf")))                                  # (reported: the accumulation terms alone)
    rows.append(("tv/rw", tverr / t["rw"], 0.0, float("inf")))                                       # (reported: the random-walk estimate)
    y = r["y"]
    assert not np.isnan(y).any()
    rows.append(("Y[:,N-1]", float(np.count_nonzero(y[:, N - 1])), 0.0, 0.0))
    rows.append(("Y[:,L:]", float(np.count_nonzero(y[:, L:N - 1])), 0.0, 0.0))
    yb = t["ybound"] + ref_err
    yerr = np.abs(y.astype(LD) - y_ld).astype(np.float64)[:, :L]
    ok = yb[:, :L] > 0
    assert not yerr[~ok].any()
    rows.append(("Y", float((yerr[ok] / yb[:, :L][ok]).max()), float(np.abs(y_ld).max()), 1.0))
    rows.append(("class:" + cls, 0.0, 0.0, 0.0))
    return rows


def fold_exact_check(ctx, n, K, N, L, steering_on=True, device=True, split=True):
    """the means fold on data for which EVERY step is exact (see the module docstring): all outputs bit for bit"""
    ns = min(n, 4096)
    stride = n // ns
    assert n & (n - 1) == 0 and stride >= 2
    rng = _rng(33, n, K, N, L)
    xc0 = np.zeros((n, K))
    cols = rng.integers(0, K, (n, 4))
    xc0[np.arange(n)[:, None], cols] = rng.choice([-1.0, 1.0], (n, 4))
    smp = np.arange(0, ns * stride, stride)                       # the sampled rows: consecutive pairs cancel, so their mean is exactly m
    xc0[smp[1::2]] = -xc0[smp[0::2]]
    m = rng.integers(-5, 6, K).astype(np.float64)
    x = (xc0 + m).astype(np.float32)
    c = rng.choice([-2.0, -1.0, 1.0, 2.0], (K, L))
    p = np.zeros((K, N))
    p[:, :L] = c * (1.0 + 2.0 ** -10 + 2.0 ** -20)
    p2 = two_plane(p)
    # the certificate, on the reference alone
    assert np.array_equal(p.astype(np.float32).astype(np.float64), p) and np.array_equal(p2[:, :L], c * (1.0 + 2.0 ** -10)), "certificate: P2"
    assert np.array_equal(sample_mean32(x, n).astype(np.float64), m) and np.array_equal((x - m.astype(np.float32)).astype(np.float64), xc0), "certificate: mu0, xc0"
    z = xc0 @ p2
    assert np.array_equal(two_plane(z), z) and np.array_equal(np.rint(z * 1024), z * 1024), "certificate: z on two planes"
    assert (np.abs(xc0).T @ np.abs(z)).max() * 1024 < 2 ** 24 and np.abs(xc0).sum(axis=0).max() < 2 ** 24, "certificate: the fp32 slab sums"
    sums = xc0.sum(axis=0)
    delta = sums / n
    assert np.count_nonzero(delta) > K // 2
    y = xc0.T @ z - n * np.outer(delta, delta @ p2)
    y_unrounded = xc0.T @ z - n * np.outer(delta, delta @ p)
    y[:, L:] = 0.0
    assert np.count_nonzero(y[:, :L] != y_unrounded[:, :L]) > K * L // 2, "certificate: a correction with the unrounded P would not show"
    assert np.count_nonzero(np.outer(delta, delta @ p2)[:, :L]) > K * L // 2
    mean = m + delta
    tv = float((xc0 * xc0).sum()) - n * float((delta * delta).sum())
    before = ctx.get_option("steering_passes")
    ctx.set_option("steering_passes", 1 if steering_on else 0)
    try:
        r = petal.probe_power_pass_means(x, p, L, K, ctx=ctx)
    finally:
        ctx.set_option("steering_passes", before)
    assert r["done"] == 1
    return [("mu0", ndiff(r["mu0"], m), 5.0, 0.0), ("mu64", ndiff(r["mu64"], mean), float(np.abs(mean).max()), 0.0),
            ("muT", ndiff(r["muT"], mean.astype(np.float32).astype(np.float64)), 0.0, 0.0), ("tv", float(abs(r["tv"] - tv)), tv, 0.0),
            ("Y", ndiff(r["y"], y), float(np.abs(y).max()), 0.0)]


REFUSALS = ["L==N", "fp64", "fp32-mode", "means_fold_rows<0", "two_plane_omega-off", "few-rows"]


def refusal_check(ctx, kind, device=True, split=True):
    n, K, N, L = 8192, 256, 16, 15
    dtype = np.float32
    if kind == "L==N":
        L = N
    if kind == "fp64":
        dtype = np.float64
    if kind == "few-rows":
        n = 8191 if device else 63
    x = fold_data(8192, K, K, "gauss")[:n].astype(dtype)
    p = fold_p(K, N, L, K)
    undo = []
    if kind == "fp32-mode":
        ctx.set_gemm_mode("fp32")
        undo.append(lambda: ctx.set_gemm_mode("bf16x3" if split else "fp32"))
    for name, opt, val in (("means_fold_rows<0", "means_fold_rows", -1), ("two_plane_omega-off", "two_plane_omega", 0)):
        if kind == name:
            old = ctx.get_option(opt)
            ctx.set_option(opt, val)
            undo.append(lambda opt=opt, old=old: ctx.set_option(opt, old))
    try:
        r = petal.probe_power_pass_means(x, p, L, K, ctx=ctx)
    finally:
        for f in undo:
            f()
    assert r["done"] == 0, f"{kind}: the operation ran"
    assert all_nan(r["y"], r["mu64"], r["muT"], [r["tv"]]), f"{kind}: a refused call wrote to its outputs"
    return [("refused", 0.0, 0.0, 0.0)]


def invalid_check(ctx, device=True, split=True):
    """a shape the probes cannot stage is PETAL_INVALID_INPUT (nothing is launched: the entry returns before it stages anything)"""
    x = np.zeros((64, 48), dtype=np.float32)
    g, bad = np.eye(16), 0
    calls = [lambda: petal.probe_rebase(x[:, :40], None, g, np.zeros((40, 16)), ctx=ctx),                    # K not a multiple of 16
             lambda: petal.probe_rebase(x, None, np.eye(24), np.zeros((48, 16)), ctx=ctx),                   # L > M
             lambda: petal.probe_rebase(x, None, g, np.zeros((48, 16)), route=3, ctx=ctx),
             lambda: petal.probe_rebase(x, None, g, np.zeros((48, 16)), p_planes=1, ctx=ctx),
             lambda: petal.probe_power_pass_means(x, np.zeros((48, 24)), 15, ctx=ctx),                      # N not a multiple of 16
             lambda: petal.probe_power_pass_means(x, np.zeros((48, 16)), 17, ctx=ctx),                      # L > N
             lambda: petal.probe_power_pass_means(x, np.zeros((48, 16)), 15, d=49, ctx=ctx)]
    for f in calls:
        try:
            f()
        except petal.InvalidInput:
            bad += 1
    return [("invalid", float(len(calls) - bad), float(len(calls)), 0.0)]


# ------------------------------------------------------------------------------------------- the tables
class Case:
    """one check with its arguments; form(split) names the kernels the case reaches"""
    def __init__(self, name, fn, *args, form=None, modes=("bf16x3", "fp32"), **kw):
        self.id, self.fn, self.args, self.kw, self._form, self.modes = name, fn, args, kw, form, modes

    def run(self, ctx, mode, device=True):
        """the check in the GEMM mode `mode` ("bf16x3" | "fp32"); the ctx is left in the split-product mode"""
        ctx.set_gemm_mode(mode)
        try:
            return self.fn(ctx, *self.args, device=device, split=mode == "bf16x3", **self.kw)
        finally:
            ctx.set_gemm_mode("bf16x3")

    def form(self, split=True):
        return self._form(split) if callable(self._form) else (self._form or "")

    def __repr__(self):
        return self.id


def exact_cases(device):
    out = []
    i = 0
    for NB in range(1, 10):                                    # route 0: every block count, L in {M, M - 6, 1}
        M = 16 * NB
        for L in (M, M - 6, 1):
            if not device and not (NB in (2, 5) and L != 1):
                i += 1
                continue
            n, K = NS[i % 3], (256, 512)[(i // 3) % 2]
            with_mu, steering, planes = i % 2 == 0, (i // 2) % 2 == 1, 2 + (i // 4) % 2
            # [arm 1 in the split-product mode, arm 2 in the fp32-MFMA mode; L = 144: arm 3 in both]
            out.append(Case(f"A-r0-NB{NB}-L{L}-n{n}-K{K}" + ("-mu" if with_mu else "") + ("-steer" if steering else "") + f"-p{planes}",
                            exact_check, 0, NB, L, n, K, with_mu, steering, planes,
                            form=lambda split, L=L: rebase_arm(split, np.float32, L)))
            i += 1
    for NB, L in ((2, 32), (5, 74), (9, 144)) if device else ():   # fp64 data: [arm 2; L = 144: arm 3]
        out.append(Case(f"A-r0-f64-NB{NB}-L{L}", exact_check, 0, NB, L, NS[NB % 3], 256, True, False, 2, dtype=np.float64, modes=("bf16x3",),
                        form=lambda split, L=L: rebase_arm(split, np.float64, L)))
    i = 0
    for NB in range(1, 6):                                     # routes 1, 2: k_chol_rt4<NB>, k_trsm_pack<NB, true>, the fused pass
        M = 16 * NB
        for K in (256, 512):
            for route in (1, 2):
                if not device and not (route == 1 and NB in (2, 5) and K == 256):
                    i += 1
                    continue
                L = (M, M - 6, M, 1)[i % 4] if NB < 5 else (M, M - 6)[i % 2]
                n, with_mu, steering = NS[(i + NB) % 3], i % 3 != 0, (i // 2) % 2 == 0
                out.append(Case(f"A-r{route}-NB{NB}-L{L}-n{n}-K{K}" + ("-mu" if with_mu else "") + ("-steer" if steering else ""),
                                exact_check, route, NB, L, n, K, with_mu, steering, 2,
                                form=lambda split, route=route, steering=steering: ("k_chol_rt4 + k_trsm_pack<NB, true> + " +
                                     ("k_pow3f" if route == 1 and steering else "k_pow3")) if split else "refused: no fused pass in the fp32-MFMA mode"))
                i += 1
    # one dependent column (the pivot of column `dead` is exactly 0), and *ndead entering at 3 / 1
    var = [(0, 3, 42, 8193, 256, 5, 0), (0, 9, 144, 8192, 256, 71, 0), (1, 5, 80, 8193, 512, 33, 0), (2, 2, 32, 12001, 256, 7, 0),
           (1, 4, 58, 8192, 256, 21, 1), (0, 4, 64, 8192, 256, None, 3), (1, 3, 48, 8193, 256, None, 3)]
    for route, NB, L, n, K, dead, nin in var if device else var[:1] + var[4:6]:
        out.append(Case(f"A-r{route}-NB{NB}-L{L}-" + (f"dead{dead}" if dead is not None else "nodead") + f"-in{nin}", exact_check, route, NB, L, n, K,
                        True, route == 1, 2, dead=dead, ndead_in=nin,
                        form=lambda split, route=route, L=L: rebase_arm(split, np.float32, L) if route == 0 else
                        ("k_chol_rt4 + k_trsm_pack<NB, true> + fused pass" if split else "refused")))
    return out


def real_cases(device):
    out = []
    for NB in range(1, 10) if device else (2, 6):              # one size per block count
        M = 16 * NB
        L = M if NB in (3, 9) else M - 6
        steering, planes = NB % 2 == 0, (3 if NB in (4, 7) else 2)
        out.append(Case(f"B-r0-NB{NB}-L{L}" + ("-steer" if steering else "") + f"-p{planes}", real_check, 0, NB, L, steering, planes,
                        form=lambda split, L=L: rebase_arm(split, np.float32, L)))
    for NB in range(1, 6) if device else (3,):
        M = 16 * NB
        route = 1 + NB % 2 if device else 1
        L = M if NB == 2 else M - 6
        out.append(Case(f"B-r{route}-NB{NB}-L{L}" + ("-steer" if route == 1 else ""), real_check, route, NB, L, route == 1, 2,
                        form=lambda split, route=route: ("k_trsm_pack<NB, true> + " + ("k_pow3f" if route == 1 else "k_pow3, Z stored")) if split else "refused"))
    if device:
        out.append(Case("B-r1-NB5-L79-nosteer", real_check, 1, 5, 79, False, 2, form=lambda split: "k_trsm_pack<5, true> + k_pow3" if split else "refused"))
    # the bound of P_out itself is a case of its own beside each of the above (so that a miss there does not hide Z and Y)
    return [c for b in out for c in (b, Case(b.id + "-Pbound", real_check, *b.args, part="p_out", form=b._form))]


def fold_cases(device):
    # n = 12287: stride = n / 4096 = 2, the sample sees the first 8192 rows only; (N, L) = (80, 79): the all-ones column sits
    # directly behind the last real one.  Trimmed to about twenty cases: every n, K, (N, L), d and family several times.
    table = [
        (8192, 256, 16, 15, 0, "gauss"), (8192, 512, 80, 79, 6, "binary"), (8192, 256, 48, 42, 6, "counts"), (8192, 512, 80, 74, 0, "sorted"),
        (8192, 256, 80, 79, 0, "binary"), (8192, 512, 16, 15, 0, "counts"),
        (12287, 256, 80, 79, 0, "sorted"), (12287, 512, 48, 42, 6, "sorted"), (12287, 256, 16, 15, 6, "binary"), (12287, 512, 80, 74, 0, "counts"),
        (12287, 256, 48, 42, 0, "gauss"), (12287, 512, 80, 79, 6, "gauss"), (12287, 256, 80, 74, 6, "sorted"),
        (65573, 256, 80, 79, 6, "binary"), (65573, 512, 48, 42, 0, "counts"), (65573, 256, 16, 15, 0, "sorted"), (65573, 512, 80, 74, 6, "gauss"),
        (65573, 256, 80, 74, 0, "counts"),
        (8192, 256, 48, 42, 0, "levels"), (12287, 512, 80, 79, 6, "levels"), (65573, 256, 80, 74, 6, "levels"),
    ]
    if not device:
        table = [table[0], table[2], table[6], table[8], table[18]]
    out = []
    for n, K, N, L, cut, fam in table:
        out.append(Case(f"C-{n}x{K}-N{N}-L{L}-d{K - cut}-{fam}", fold_check, n, K, N, L, K - cut, fam, modes=("bf16x3",),
                        form="k_pow3f<.., MEANS> + k_mean_fix"))
    # the non-steering form k_pow3<.., MEANS>: the three-plane analogue, the exact class of the means
    for n, K, N, L, cut, fam in ([(8192, 256, 80, 79, 0, "binary"), (12287, 512, 48, 42, 6, "sorted"), (12287, 256, 80, 74, 0, "levels")] if device
                                 else [(8192, 256, 16, 15, 0, "levels")]):
        out.append(Case(f"C-{n}x{K}-N{N}-L{L}-d{K - cut}-{fam}-nosteer", fold_check, n, K, N, L, K - cut, fam, steering_on=False, modes=("bf16x3",),
                        form="k_pow3<.., MEANS> + k_mean_fix"))
    # everything exact: the fold bit for bit, in both forms
    for n, K, N, L, steer in ([(8192, 256, 16, 15, True), (16384, 512, 80, 79, True), (8192, 512, 48, 42, False), (16384, 256, 80, 74, True)] if device
                              else [(8192, 256, 16, 15, True), (8192, 256, 48, 42, False)]):
        out.append(Case(f"C-exact-{n}x{K}-N{N}-L{L}" + ("" if steer else "-nosteer"), fold_exact_check, n, K, N, L, steering_on=steer, modes=("bf16x3",),
                        form=("k_pow3f" if steer else "k_pow3") + "<.., MEANS> + k_mean_fix"))
    for kind in REFUSALS:
        out.append(Case(f"C-refuse-{kind}", refusal_check, kind, modes=("bf16x3",), form="refused"))
    out.append(Case("probe-invalid-shapes", invalid_check, modes=("bf16x3",), form="PETAL_INVALID_INPUT"))
    return out


TABLES = {"A": exact_cases, "B": real_cases, "C": fold_cases}


def all_cases(device=True):
    cases = [c for name in TABLES for c in TABLES[name](device)]
    ids = [c.id for c in cases]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return cases


def params(device=True):
    """(case, mode) pairs of a runner"""
    return [(c, m) for c in all_cases(device) for m in c.modes]


def check_rows(case, mode, rows):
    for q, err, ref, bound in rows:
        print(f"{case.id}-{mode} [{case.form(mode == 'bf16x3')}] {q}: error {err:.3e}, reference {ref:.3e}, bound {bound:.3e}")
    for q, err, ref, bound in rows:
        assert err <= bound, (case.id, mode, q, err, bound)


def main():
    import time
    print("# case-mode | quantity | error (exact quantities: differing elements; bounded ones: error / bound) | largest reference value | bound | kernels")
    t0 = time.time()
    ctx = petal.Context(0)
    failed = 0
    for case, mode in params(True):
        name = f"{case.id}-{mode}"
        try:
            rows = case.run(ctx, mode, device=True)
        except (AssertionError, petal.InvalidInput) as e:
            failed += 1
            print(f"{name:58s} FAILED: {e}   [{case.form(mode == 'bf16x3')}]", flush=True)
            continue
        except petal.DeviceError as e:      # the device is in an unknown state: nothing more is started on it
            print(f"{name:58s} DEVICE ERROR, report ends here: {e}", flush=True)
            return 1
        for q, err, ref, bound in rows:
            flag = "" if err <= bound else "   <-- ABOVE THE BOUND"
            failed += bool(flag)
            print(f"{name:58s} {q:16s} {err:10.3e} {ref:10.3e} {bound:8.1f}   [{case.form(mode == 'bf16x3')}]{flag}", flush=True)
    ctx.close()
    print(f"# {failed} rows or cases failed; wall time {time.time() - t0:.0f} s")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
