"""Exact tests of the LOWER bf16 planes of every split-product kernel: k_xp3 (K1), k_atb3 (K2), the fused pass k_pow3 / k_pow3f,
the Gram kernel k_gram5 and the score kernel -- and of their steering forms, reached through PETAL_OPT_STEERING_HOOK.  Shared by
tests/test_gpu_planes.py (the HIP library, both GEMM modes) and tests/test_planes_host.py (the numpy model of the piece products, its
mutants, and the host simulation).

Every fp32 operand of these kernels is split by round-to-nearest-even into bf16 pieces x = h + m + l, and a product keeps the pieces
of weight >= 2^-16: u_i v_j with i + j <= 2 (h = 0, m = 1, l = 2) -- six of them for three-plane operands, five when the second
operand is DEFINED as its two leading pieces, four when both are (the steering forms).  The exact-integer tests of
tests/test_gpu_parity.py draw operands that are single bf16 numbers: their m and l planes are zero.  Here the operands carry a BIT
BUDGET instead: a float of <= 8 significant bits has an h plane only, <= 16 bits h and m, <= 24 bits all three.  An output element is
EXACT -- in fp32 accumulation of the kept piece products in any order -- when every dropped piece product of it is exactly zero, all
its terms are multiples of one granularity q, and sum |terms| < 2^24 q (every partial sum is then a multiple of q below 2^24 q: a
float32 number).  The plain float64 product of the operands is then the reference TO THE LAST BIT, and a wrong lane, chunk or LDS
address of a lower plane, a dropped or doubled piece product, swapped m / l planes or an aliased plane is an exact mismatch.

The CERTIFICATE (Product.analyse, on the CPU, per call, before any device is touched) classifies every output element from the
operands' actual pieces: the pieces re-add exactly to the operand, x - mu is exact in float32 where a centre is used, and
   exact class:   no non-zero dropped piece product,  sum |kept piece products| (+ |bias|) < 2^24 q,
                  q = the smallest (lowest set bit of u) x (lowest set bit of v) among the element's non-zero terms (and the bias's)
   bounded class: everything else, held to the DERIVED bound |out - ref_longdouble| <= (3 + T) 2^-24 sum |terms|
                  (3: the three dropped pieces of weight 2^-24; T: the non-zero piece products of the element, worst-case fp32 accumulation).
At least half of every call's output elements must be in the exact class (asserted).  In the steering forms the reference is the
statement with the operands rounded to two planes by the numpy split (ops.h: that rounding is their definition); a case with operands
wider than 16 bits also asserts that this reference DIFFERS from the three-plane one in an eighth or more of the non-zero elements of the
exact class, so an exact match is itself the proof that k_pow3f / k_xp3<.., X2> / k_atb3<.., P4> ran.

Plane designs (bits of the first operand x bits of the second; what an exact match proves):
   x24   24 (20 under a centre) x +-2^s     m h', l h'                  single term per element
   p24   +-2^s x 24                         h m', h l'                  single term
   d12   12 x 12                            h m', m h', m m'            single term
   multi 16 x +-1, up to 64 terms of equal exponent (K1, K2, score) | classes 20 / 1 / 10 / 1 bits, 8 terms (fused pass, Gram)
   mixed (fused pass, Gram): the features of X rotate through 24-, 1-, 12- and 1-bit classes, so y[f, j] covers three x one, one x
         three and two x two planes; p16 (fused pass): power-of-two X, 16-bit P.
Multi-term cases use terms of EQUAL exponent per output column (a per-feature exponent): the order independence of the certificate
needs nothing else, and the per-call certificate is asserted, never assumed.

Rotation.  K1 and the score kernel take a dense X (every row, ragged tails included, carries all three planes in every call) and a
P with its non-zeros moving over the calls until EVERY k index has carried one (so every k mod 32, every 32-deep chunk).  K2, the
fused pass and the Gram kernel take a row-sparse operand: at most 8 non-zero rows per call (64 in K2's multi design), placed so that
over the calls every row position of a 32-row stage, the first and the last stage and every ragged tail row carry one; the fused
pass's P rotates until every k mod 32, every 32-deep chunk and every 64-feature wave slice has carried a non-zero.  At most 24 calls
per case; Case.run asserts the coverage is complete.

The steering forms' dispatch (csrc/kernels/host_gemm.inc), which the expected forms below restate: under the hook K1 runs P on two
planes always and X on two planes in panels of six column tiles or more (more than 80 columns in this table); K2 runs both operands on
two planes in the eight-wave 32-column form (not in the narrow-workgroup form of <= 128 features, not with a centred B); the fused pass
runs k_pow3f when no z is wanted.  The host simulation (oracle/cpu_ops.cpp) steers K2 by `more than 80 columns` alone -- it differs from
the device at 512 features x 80 columns, where the device takes the eight-wave form.  The tests assume the default build
(PETAL_STEER_PIECES = 4).

`python tests/plane_cases.py` runs every case on petal.Context(0) in both GEMM modes and prints one line per case: the report kept in
profiles/plane_probe_errors.txt."""
import os
import sys

import numpy as np

if __name__ == "__main__":      # (run as a script: the package is found from the repository root)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LD = np.longdouble
KEPT = [(0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0)]      # i + j <= 2
LOWER = KEPT[1:]
PLANE = "hml"
MAX_CALLS = 24


# ------------------------------------------------------------------------------------------- planes, granularity, b-bit numbers
def bf16(x):
    """float32 -> the nearest bf16 (ties to even), as a float32"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + (np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1)))) & np.uint32(0xffff0000)).view(np.float32)


def planes(x, npl=3):
    """([h, m, l], value): split3 / split2 of csrc/kernels/k_gemm_split_k1.inc; npl = 2: l = 0 and value = h + m, the two-plane rounding"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    h = bf16(x)
    r = x - h
    m = bf16(r)
    l = bf16(r - m) if npl == 3 else np.zeros_like(x)
    val = (h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64)).astype(np.float32)
    assert np.array_equal(val.astype(np.float64), h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64))
    if npl == 3:
        assert np.array_equal(val, x), "certificate: the three pieces do not re-add to the operand"
    return [h, m, l], val


def split2(x):
    return planes(x, 2)[1]


def gran(x):
    """value of the lowest set bit of every element (inf for zero)"""
    a = np.abs(np.asarray(x, dtype=np.float64))
    m, e = np.frexp(a)
    mi = np.ldexp(m, 53).astype(np.int64)
    g = np.ldexp((mi & -mi).astype(np.float64), e - 53)
    return np.where(a == 0, np.inf, g)


def bbit(rng, shape, bits, exps, no_carry=False):
    """b-bit float32 numbers: sign x an integer in [2^(b-1), 2^b) x 2^exps (exps broadcasts; bits too).  no_carry: the integers stop at
    2^b - 2^(b-8) (b > 8), so that the h piece never rounds up into the next binade and |h| + |m| + |l| < 2^b: a product of such a
    number with a power of two is in the exact class whatever its bits (the fused pass's z has to be, element for element)"""
    bits = np.broadcast_to(np.asarray(bits, dtype=np.int64), shape)
    lo = np.left_shift(np.int64(1), bits - 1)
    span = lo - np.where(bits > 8, np.left_shift(np.int64(1), np.maximum(bits - 8, 0)), 0) if no_carry else lo
    m = lo + (rng.random(shape) * span).astype(np.int64)
    assert np.all((m >= lo) & (m < lo + span))
    s = rng.integers(0, 2, shape) * 2 - 1
    out = np.ldexp((s * m).astype(np.float64), np.broadcast_to(np.asarray(exps, dtype=np.int64), shape))
    assert np.array_equal(out.astype(np.float32).astype(np.float64), out)
    return out.astype(np.float32)


def centred_input(xc, mu):
    """x = xc + mu with the certificate that the kernels' float32 x - mu gives xc back exactly"""
    if mu is None:
        return xc
    x64 = xc.astype(np.float64) + mu.astype(np.float64)
    x = x64.astype(np.float32)
    assert np.array_equal(x.astype(np.float64), x64), "certificate: xc + mu is not a float32 number"
    assert np.array_equal(x - mu.astype(np.float32), xc), "certificate: x - mu is not exact in float32"
    return x


# ------------------------------------------------------------------------------------------- mutants of the piece-product model
class Mutant:
    """what a subtly wrong kernel would compute: a change of the model's planes or of its list of piece products"""
    def __init__(self, name, fn):
        self.name, self.fn = name, fn

    def __repr__(self):
        return self.name


def _drop(i, j):
    def fn(up, vp, pairs, prod):
        return up, vp, [p for p in pairs if p != (i, j)]
    return Mutant(f"drop-{PLANE[i]}{PLANE[j]}'", fn)


def _swap_ml(side):
    def fn(up, vp, pairs, prod):
        if side == 0:
            return [up[0], up[2], up[1]], vp, pairs
        return up, [vp[0], vp[2], vp[1]], pairs
    return Mutant(f"swap-m-l-{'uv'[side]}", fn)


def _l_is_m(side):
    def fn(up, vp, pairs, prod):
        if side == 0:
            return [up[0], up[1], up[1]], vp, pairs
        return up, [vp[0], vp[1], vp[1]], pairs
    return Mutant(f"l-aliases-m-{'uv'[side]}", fn)


def _rot8(side, plane):
    """the plane read one lane group of 8 further within its 32-deep chunk, along the operand's k / feature axis"""
    def fn(up, vp, pairs, prod):
        ops = [list(up), list(vp)]
        axis = prod.kaxis[side]
        a = ops[side][plane]
        kk = a.shape[axis]
        idx = np.arange(kk)
        src = (idx // 32) * 32 + (idx % 32 + 8) % 32
        ok = src < kk
        b = np.take(a, np.where(ok, src, 0), axis=axis)
        shape = [1, 1]
        shape[axis] = kk
        ops[side][plane] = b * ok.reshape(shape).astype(np.float32)
        return ops[0], ops[1], pairs
    return Mutant(f"rot8-{'uv'[side]}-{PLANE[plane]}", fn)


MUTANTS = [_drop(i, j) for i, j in LOWER] + [_swap_ml(0), _swap_ml(1), _l_is_m(0), _l_is_m(1), _rot8(0, 1), _rot8(0, 2), _rot8(1, 1)]
_ELEMENT_MUTANTS = MUTANTS[:9]      # (those that act on one element's terms alone: the mismatch report tries them)


# ------------------------------------------------------------------------------------------- one product and its certificate
def piece_sums(au, av, nu, nv):
    """(S, D, T) of out = U^T V from the magnitudes au / av and the non-zero indicators nu / nv of the operands' three pieces (float64,
    t x a and t x b each): S = sum |kept piece products|, D = sum |dropped piece products|, T = the number of non-zero kept ones"""
    S = au[0].T @ (av[0] + av[1] + av[2]) + au[1].T @ (av[0] + av[1]) + au[2].T @ av[0]
    D = au[1].T @ av[2] + au[2].T @ (av[1] + av[2])
    T = nu[0].T @ (nv[0] + nv[1] + nv[2]) + nu[1].T @ (nv[0] + nv[1]) + nu[2].T @ nv[0]
    return S, D, T


def bounded_class_bound(S, T):
    """the derived bound of the bounded class: the three dropped pieces of weight 2^-24 and T terms of worst-case fp32 accumulation"""
    return (3.0 + T) * 2.0 ** -24 * S


class Product:
    """out[a, b] = sum_t U[t, a] V[t, b] (+ bias[b]) by the kept piece products of U on pu planes and V on pv planes.  U (T x A) and
    V (T x B) hold only the t that matter (tlab: their original indices; alab: the original indices of the a axis).  kaxis: the axis of
    (U, V) that is a k / feature axis of the kernel's fragments, and whether it is complete (the rot8 mutants need it complete)."""
    def __init__(self, name, U, V, pu=3, pv=3, bias=None, tlab=None, alab=None, kaxis=(0, 0), tname="k"):
        self.name = name
        self.U, self.V = np.ascontiguousarray(U, dtype=np.float32), np.ascontiguousarray(V, dtype=np.float32)
        assert self.U.shape[0] == self.V.shape[0]
        self.pu, self.pv = pu, pv
        self.bias = None if bias is None else np.asarray(bias, dtype=np.float32)
        self.tlab = np.arange(self.U.shape[0]) if tlab is None else np.asarray(tlab)
        self.alab = np.arange(self.U.shape[1]) if alab is None else np.asarray(alab)
        self.kaxis, self.tname = kaxis, tname
        self._a = None

    def analyse(self):
        if self._a is not None:
            return self._a
        up, ur = planes(self.U, self.pu)
        vp, vr = planes(self.V, self.pv)
        f8 = np.float64
        au, av = [np.abs(p).astype(f8) for p in up], [np.abs(p).astype(f8) for p in vp]
        nu, nv = [(p != 0).astype(f8) for p in up], [(p != 0).astype(f8) for p in vp]
        ref = ur.astype(f8).T @ vr.astype(f8)
        S, D, T = piece_sums(au, av, nu, nv)
        # q[a, b] = the smallest granularity among the element's non-zero terms (every piece of an operand is a multiple of the
        # operand's own lowest set bit): a (min, x) product, one t at a time over the columns that t reaches
        gu, gv = gran(ur), gran(vr)
        q = np.full(ref.shape, np.inf)
        for t in range(ur.shape[0]):
            cols = np.nonzero(np.isfinite(gv[t]))[0]
            if len(cols):
                q[:, cols] = np.minimum(q[:, cols], gu[t][:, None] * gv[t, cols][None, :])
        if self.bias is not None:
            b = self.bias.astype(f8)
            ref = ref + b
            S = S + np.abs(b)
            T = T + (b != 0)
            q = np.minimum(q, gran(b)[None, :])
        exact = (D == 0) & (S * (1 + 1e-12) < 2.0 ** 24 * q)
        assert 2 * np.count_nonzero(exact) >= exact.size, f"{self.name}: fewer than half of the elements are in the exact class"
        self._a = {"ref": ref, "S": S, "T": T, "q": q, "exact": exact, "bound": bounded_class_bound(S, T), "up": up, "vp": vp, "ur": ur, "vr": vr}
        return self._a

    def ref_longdouble(self, ai, bi):
        a = self.analyse()
        out = np.zeros(len(ai), dtype=LD)
        for s in range(0, len(ai), 1 << 16):
            e = slice(s, s + (1 << 16))
            out[e] = (a["ur"][:, ai[e]].astype(LD) * a["vr"][:, bi[e]].astype(LD)).sum(axis=0)
        if self.bias is not None:
            out += self.bias.astype(LD)[bi]
        return out

    def model(self, mutant=None, seed=0):
        """the kept piece products, accumulated in float32 in a shuffled order"""
        rng = np.random.default_rng(seed)
        up, _ = planes(self.U, self.pu)
        vp, _ = planes(self.V, self.pv)
        pairs = list(KEPT)
        if mutant is not None:
            up, vp, pairs = mutant.fn(up, vp, pairs, self)
        perm = rng.permutation(self.U.shape[0])
        acc = np.zeros((self.U.shape[1], self.V.shape[1]), dtype=np.float32)
        for k in rng.permutation(len(pairs)):
            i, j = pairs[k]
            if up[i].any() and vp[j].any():
                acc = acc + np.ascontiguousarray(up[i][perm].T) @ vp[j][perm]
        if self.bias is not None:
            acc = acc + self.bias[None, :]
        assert acc.dtype == np.float32
        return acc

    def check(self, out, where):
        """THE assertion: exact class equal to the float64 product, bounded class within (3 + T) 2^-24 sum |terms| of the long double.
        Returns (elements in the exact class, mismatches = 0, elements in the bounded class, largest error / bound)."""
        a = self.analyse()
        out = np.asarray(out)
        assert out.shape == a["ref"].shape, (where, self.name, out.shape, a["ref"].shape)
        o = out.astype(np.float64)
        bad = a["exact"] & ~(o == a["ref"])
        ratio = 0.0
        ai, bi = np.nonzero(~a["exact"])
        if len(ai):
            err = np.abs(o[ai, bi].astype(LD) - self.ref_longdouble(ai, bi))
            r = (err / a["bound"][ai, bi].astype(LD)).astype(np.float64)
            ratio = float(np.nan_to_num(r, nan=np.inf).max())
        nbad = int(np.count_nonzero(bad))
        if nbad:
            raise AssertionError(f"{where} {self.name}: {nbad} of {int(a['exact'].sum())} certified-exact elements differ\n" + self.describe(bad, o))
        if ratio > 1.0:
            w = int(np.argmax(r))
            raise AssertionError(f"{where} {self.name}: bounded-class element ({self.alab[ai[w]]}, {bi[w]}) is {ratio:.3f} x its bound "
                                 f"(3 + {int(a['T'][ai[w], bi[w]])}) 2^-24 {a['S'][ai[w], bi[w]]:.6g}")
        return int(a["exact"].sum()), nbad, int(len(ai)), ratio

    def describe(self, bad, o):
        """the first mismatches by fragment position, contributing terms and the plane mutants that reproduce the wrong value"""
        a = self.analyse()
        lines = []
        for ea, eb in np.argwhere(bad)[:6]:
            u = [p[:, ea].astype(np.float64) for p in a["up"]]
            v = [p[:, eb].astype(np.float64) for p in a["vp"]]
            ts = np.nonzero((a["ur"][:, ea] != 0) & (a["vr"][:, eb] != 0))[0]
            terms = ", ".join(f"{self.tname} {int(self.tlab[t])} (mod 32: {int(self.tlab[t]) % 32}, chunk {int(self.tlab[t]) // 32})" for t in ts[:4])
            hits = []
            for mt in _ELEMENT_MUTANTS:
                up, vp, pairs = mt.fn(u, v, list(KEPT), self)
                val = sum(float((up[i] * vp[j]).sum()) for i, j in pairs) + (float(self.bias[eb]) if self.bias is not None else 0.0)
                if val == o[ea, eb]:
                    hits.append(mt.name)
            lines.append(f"  out[{int(self.alab[ea])}, {int(eb)}] (a mod 32: {int(self.alab[ea]) % 32}, column tile {int(eb) // 16}) = {o[ea, eb]!r}, expected "
                         f"{a['ref'][ea, eb]!r}: off by {(o[ea, eb] - a['ref'][ea, eb]) / a['q'][ea, eb]:.6g} q; terms at {terms or 'none'}; "
                         f"reproduced by {hits or 'no single-plane mutant'}")
        return "\n".join(lines)


# ------------------------------------------------------------------------------------------- runners: who computes the outputs
class DeviceRunner:
    """a petal.Context: the HIP library, or the host simulation (sim = True: its own steering rules)"""
    def __init__(self, ctx, split, sim=False):
        self.ctx, self.split, self.sim = ctx, split, sim
        self.label = "sim" if sim else ("bf16x3" if split else "fp32")

    def set_hook(self, on):
        self.ctx.set_option("steering_hook", 1 if on else 0)

    def forms(self, call, hook):
        """(pu, pv) of every product of the call, restating the dispatch of host_gemm.inc / host_pow3_eigh.inc / cpu_ops.cpp"""
        k, steer = call.kernel, hook and self.split
        if k == "k1":
            return [(2 if steer and call.NP > 80 else 3, 2 if steer else 3)]
        if k == "k2":
            p4 = steer and not call.b_centred and (call.NP > 80 if self.sim else call.p4_shape)
            return [(2, 2) if p4 else (3, 3)]
        if k == "fused":
            if not self.split:
                return [(3, 3), (3, 3)]
            return [(2, 2), (2, 2)] if steer and not call.want_z else [(3, 2), (3, 3)]
        return [(3, 3)]

    def execute(self, call, products):
        import petal_decomposition_amd as petal
        a, ctx = call.args, self.ctx
        if call.kernel == "k1":
            return {"z": petal.gemm_xp(a["x"], a["p"], a["mu"], a["bias"], ctx=ctx)}
        if call.kernel == "score":
            _, y = petal.score_rows(a["x"], a["comp"], a["mu"], None, centering=a["mu"] is not None, want_y=True, ctx=ctx)
            return {"z": y}
        if call.kernel == "k2":
            return {"c": petal.gemm_atb(a["a"], a["b"], a["mu_a"], a["mu_b"], ctx=ctx)}
        if call.kernel == "gram":
            ctx.set_option("gram_split_hook", 1)
            try:
                return {"c": petal.gemm_atb(a["x"], None, a["mu"], a["mu"], ctx=ctx)}
            finally:
                ctx.set_option("gram_split_hook", 0)
        if call.kernel == "fused":
            before = ctx.get_option("fused_pass_min_rows")
            ctx.set_option("fused_pass_min_rows", 64)
            try:
                y, z, fused = petal.power_pass(a["x"], a["p"], a["mu"], want_z=call.want_z, ctx=ctx)
            finally:
                ctx.set_option("fused_pass_min_rows", before)
            assert bool(fused) == bool(self.split), f"power_pass: fused = {fused} in {self.label} mode"
            return {"y": y, "z": z}
        raise KeyError(call.kernel)


class ModelRunner:
    """the numpy model of the piece products (split-product forms), optionally mutated"""
    split, sim, label = True, False, "model"

    def __init__(self, mutant=None):
        self.mutant = mutant

    def set_hook(self, on):
        pass

    forms = DeviceRunner.forms

    def execute(self, call, products):
        mt = self.mutant
        if call.kernel in ("k1", "score"):
            z = np.zeros((call.n, products[0].V.shape[1]), dtype=np.float32)
            z[products[0].alab] = products[0].model(mt)
            return {"z": z}
        if call.kernel in ("k2", "gram"):
            return {"c": products[0].model(mt).astype(np.float64)}
        p1, p2 = products
        zr = p1.model(mt)                                   # (R x N: the non-zero rows of z)
        y = Product("y", p2.U, zr, p2.pu, p2.pv, kaxis=p2.kaxis).model(mt).astype(np.float64)   # (a wrong z reaches y, as on the device)
        z = None
        if call.want_z:
            z = np.zeros((call.n, zr.shape[1]), dtype=np.float32)
            z[p1.alab] = zr
        return {"y": y, "z": z}


# ------------------------------------------------------------------------------------------- row and column rotation
def rows_for_call(n, c, R):
    """at most R distinct rows of call c: R - 2 spread over the stages at rotating positions within a 32-row stage, one in the first
    stage, one walking through the ragged tail (the last stage where there is none)"""
    nst = (n + 31) // 32
    tail = n % 32 if n % 32 else min(32, n)
    rows = [c % min(32, n), n - 1 - (c % tail)]
    for k in range(max(R - 2, 0)):
        st = ((c * 7 + k * 13 + 1) * max(1, nst // 29) + k) % nst
        r = st * 32 + (5 * c + 11 * k + 24) % 32
        rows.append(r if r < n else (r - 32 if r >= 32 else r % n))
    out = []
    for r in rows:
        if r not in out:
            out.append(int(r))
    return sorted(out[:R])


class RowCoverage:
    def __init__(self, n):
        self.n, self.pos, self.stages, self.tail = n, set(), set(), set()

    def add(self, rows):
        for r in rows:
            self.pos.add(r % 32)
            self.stages.add(r // 32)
            if r >= self.n - self.n % 32:
                self.tail.add(r)

    def missing(self):
        n = self.n
        m = []
        if len(self.pos) < min(32, n):
            m.append(f"row positions {sorted(set(range(min(32, n))) - self.pos)}")
        if 0 not in self.stages or (n - 1) // 32 not in self.stages:
            m.append("first / last stage")
        if len(self.tail) < n % 32:
            m.append(f"tail rows {sorted(set(range(n - n % 32, n)) - self.tail)}")
        return m


def pi_for_call(K, N, c):
    """the k index of column j's non-zero in call c"""
    j = np.arange(N)
    return ((c * N + j) % K * 37) % K


# ------------------------------------------------------------------------------------------- the cases
class Call:
    pass


class Case:
    """one (kernel, shape, plane design, variant): a rotation of at most MAX_CALLS calls.  run(runner) executes them on the runner and
    gives every output to Product.check; returns the totals (calls, exact elements, mismatches, bounded elements, largest error / bound)."""
    kernel = ""

    def __init__(self, design, hook=False, small=False):
        self.design, self.hook, self.small = design, hook, small
        self.seed = 0

    def __repr__(self):
        return self.id

    def rng(self, salt=0):
        return np.random.default_rng([self.seed, salt])

    def run(self, runner, max_calls=MAX_CALLS):
        self.setup()
        tot = [0, 0, 0, 0, 0.0]
        runner.set_hook(self.hook)
        try:
            for c in range(max_calls):
                call = self.call(c)
                forms = runner.forms(call, self.hook)
                products = self.products(call, forms)
                for p in products:
                    p.analyse()
                if c == 0 and self.proves_steering(forms):
                    self.assert_forms_differ(call, forms)
                outs = runner.execute(call, products)
                for st in self.check(call, products, outs, f"{self.id} [{runner.label}] call {c}:"):
                    tot[1] += st[0]
                    tot[2] += st[1]
                    tot[3] += st[2]
                    tot[4] = max(tot[4], st[3])
                tot[0] += 1
                if not self.missing():
                    break
        finally:
            runner.set_hook(False)
        assert not self.missing(), f"{self.id}: coverage incomplete after {tot[0]} calls: {self.missing()}"
        return tuple(tot)

    def proves_steering(self, forms):
        return False

    def assert_forms_differ(self, call, forms):
        """the two-plane reference differs from the three-plane one in an eighth or more of the non-zero elements of the exact class:
        matching it exactly proves that the steering kernel ran"""
        two = self.products(call, forms)[-1].analyse()
        three = self.products(call, self.exact_forms)[-1].analyse()
        live = two["exact"] & (three["ref"] != 0)
        diff = np.count_nonzero((two["ref"] != three["ref"]) & live)
        assert 8 * diff >= np.count_nonzero(live) > 0, f"{self.id}: the steering form would not be told from the exact one ({diff} of {np.count_nonzero(live)})"


def _exps(rng, count, centred):
    return rng.integers(-3, 4, count) if centred else rng.integers(-6, 7, count)


class K1Case(Case):
    """z = (x - mu) P + bias through petal_gemm_xp (kernel 'k1'), or y = (x - mu) C^T through petal_score_rows ('score'): X dense and
    constant over the calls, P with one non-zero per column (64 rows of +-1 in the multi design) at rotating k"""
    exact_forms = [(3, 3)]

    def __init__(self, kernel, n, K, N, design, centred=False, bias=False, hook=False):
        super().__init__(design, hook, small=n * K * N <= (1 << 22))
        self.kernel, self.n, self.K, self.N, self.centred, self.with_bias = kernel, n, K, N, centred, bias
        self.id = f"{kernel}-{n}x{K}x{N}-{design}" + ("-centred" if centred else "") + ("-bias" if bias else "") + ("-hook" if hook else "")
        self.seed = (31 * n + 17 * K + 7 * N + 3 * centred + hook) % 1000 + {"x24": 1, "p24": 2, "d12": 3, "multi": 4}[design] * 1000

    def setup(self):
        rng = self.rng()
        n, K = self.n, self.K
        cap = 20 if self.centred else 24
        self.xbits = {"x24": cap, "p24": 1, "d12": 12, "multi": 16}[self.design]
        self.ex = np.full(K, int(rng.integers(-3, 4))) if self.design == "multi" else _exps(rng, K, self.centred)
        self.xc = bbit(rng, (n, K), self.xbits, self.ex[None, :])
        self.mu = rng.integers(-2, 3, K).astype(np.float32) if self.centred else None
        self.x = centred_input(self.xc, self.mu)
        self.covered = set()

    def missing(self):
        left = set(range(self.K)) - self.covered
        return [f"k indices {sorted(left)[:8]}..."] if left else []

    def proves_steering(self, forms):
        (pu, pv), = forms      # (x24: 20 bits or more of X, proves X2; p24: 24 bits of P, proves the two-plane P)
        return (self.design == "x24" and pu == 2) or (self.design == "p24" and pv == 2)

    def call(self, c):
        rng = self.rng(c + 1)
        K, N = self.K, self.N
        p = np.zeros((K, N), dtype=np.float32)
        if self.design == "multi":
            ks = np.unique((c * 64 + np.arange(min(64, K))) % K)
            p[ks] = (rng.integers(0, 2, (len(ks), N)) * 2 - 1).astype(np.float32)
            unit = np.full(N, 2.0 ** float(self.ex[0]))
        else:
            pi = pi_for_call(K, N, c)
            s = rng.integers(-4, 5, N)
            pbits = {"x24": 1, "p24": 24, "d12": 12}[self.design]
            p[pi, np.arange(N)] = bbit(rng, (N,), pbits, s)
            ks = np.unique(pi)
            unit = np.ldexp(1.0, self.ex[pi] + s)
        self.covered.update(int(k) for k in ks)
        call = Call()
        call.kernel, call.n, call.NP, call.want_z = self.kernel, self.n, (N + 15) // 16 * 16, False
        call.ks, call.p = ks, p
        call.bias = (rng.integers(-8, 9, N) * unit).astype(np.float32) if self.with_bias else None
        if self.kernel == "score":
            call.args = {"x": self.x, "comp": np.ascontiguousarray(p.T), "mu": self.mu}
        else:
            call.args = {"x": self.x, "p": p, "mu": self.mu, "bias": call.bias}
        return call

    def products(self, call, forms):
        ks = np.arange(self.K) if self.small else call.ks      # (small shapes keep the whole k axis: the rot8 mutants need it)
        (pu, pv), = forms
        return [Product("z", self.xc[:, ks].T, call.p[ks], pu, pv, bias=call.bias, tlab=ks, kaxis=(0, 0), tname="k")]

    def check(self, call, products, outs, where):
        return [products[0].check(outs["z"], where)]


def _row_sparse(case, c, R, single, centred, classes, rng):
    """the non-zero rows of call c of a row-sparse X (n x K): (rows, xc_rows).  single: the rows' feature supports are disjoint -- row r of
    the call owns the features f with (f // 8 + c) % R == r -- so that every y / C element has ONE term; the feature classes (bits) rotate with c."""
    K = case.K
    rows = rows_for_call(case.n, c, R)
    f = np.arange(K)
    bits = np.asarray(classes)[(f + f // 32 + c) % len(classes)]
    if centred:
        bits = np.minimum(bits, 20)
    xr = bbit(rng, (len(rows), K), bits[None, :], case.ex[None, :], no_carry=True)
    if single:
        own = (f // 8 + c) % len(rows)
        xr = xr * (own[None, :] == np.arange(len(rows))[:, None]).astype(np.float32)
    return rows, xr


class K2Case(Case):
    """C = (A - muA)^T (B - muB) through petal_gemm_atb: A dense and constant, B row-sparse.  Single-term designs: 8 non-zero rows per
    call, row r of the call non-zero in the columns j = r (mod 8); multi: 64 rows of +-2^s, equal exponent per column."""
    kernel = "k2"
    exact_forms = [(3, 3)]

    def __init__(self, n, M, N, design, centre="none", hook=False, p4_shape=False):
        super().__init__(design, hook, small=True)
        self.n, self.M, self.K, self.N, self.centre, self.p4_shape = n, M, M, N, centre, p4_shape
        self.id = f"k2-{n}x{M}x{N}-{design}-centre-{centre}" + ("-hook" if hook else "")
        self.seed = (31 * n + 17 * M + 7 * N + 3 * len(centre) + hook) % 1000 + {"x24": 11, "p24": 12, "d12": 13, "multi": 14}[design] * 1000

    def setup(self):
        rng = self.rng()
        n, M, N = self.n, self.M, self.N
        ca, cb = self.centre in ("a", "both"), self.centre == "both"
        self.abits = {"x24": 20 if ca else 24, "p24": 1, "d12": 12, "multi": 16}[self.design]
        self.bbits = {"x24": 1, "p24": 20 if cb else 24, "d12": 12, "multi": 1}[self.design]
        self.ex = _exps(rng, M, ca)
        self.ac = bbit(rng, (n, M), self.abits, self.ex[None, :])
        self.mu_a = rng.integers(-2, 3, M).astype(np.float32) if ca else None
        self.a = centred_input(self.ac, self.mu_a)
        self.mu_b = rng.integers(-2, 3, N).astype(np.float32) if cb else None
        self.sb = _exps(rng, N, cb)
        self.cov = RowCoverage(n)

    def missing(self):
        return self.cov.missing()

    def proves_steering(self, forms):
        return forms != self.exact_forms and self.design in ("x24", "p24")

    def call(self, c):
        rng = self.rng(c + 1)
        n, N = self.n, self.N
        R = min(64, n) if self.design == "multi" else 8
        rows = rows_for_call(n, c, R)
        br = bbit(rng, (len(rows), N), self.bbits, self.sb[None, :])
        if self.design != "multi":
            br = br * ((np.arange(N)[None, :] % len(rows)) == np.arange(len(rows))[:, None]).astype(np.float32)
        bc = np.zeros((n, N), dtype=np.float32)
        bc[rows] = br
        self.cov.add(rows)
        call = Call()
        call.kernel, call.n, call.NP, call.want_z = "k2", n, (N + 15) // 16 * 16, False
        call.b_centred, call.p4_shape = self.mu_b is not None, self.p4_shape
        call.rows, call.br = np.asarray(rows), br
        call.args = {"a": self.a, "b": centred_input(bc, self.mu_b), "mu_a": self.mu_a, "mu_b": self.mu_b}
        return call

    def products(self, call, forms):
        (pu, pv), = forms
        return [Product("c", self.ac[call.rows], call.br, pu, pv, tlab=call.rows, kaxis=(1, 1), tname="row")]

    def check(self, call, products, outs, where):
        return [products[0].check(outs["c"], where)]


MIXED = [24, 1, 12, 1]          # the feature classes of the single-term designs of the fused pass and the Gram kernel
MULTI = [20, 1, 10, 1]          # ... of their multi-term design: 8 terms of equal exponent stay below 2^24 q for 20 x 1 and 10 x 10


class GramCase(Case):
    """C = (X - mu)^T (X - mu) through petal_gemm_atb(x) under PETAL_OPT_GRAM_SPLIT_HOOK: X row-sparse, at most 8 non-zero rows"""
    kernel = "gram"

    def __init__(self, n, d, design, centred=False, max_calls=MAX_CALLS):
        super().__init__(design, False, small=d <= 256)
        self.n, self.K, self.centred, self.max_calls = n, d, centred, max_calls
        self.id = f"gram-{n}x{d}-{design}" + ("-centred" if centred else "")
        self.seed = (31 * n + 17 * d + 3 * centred) % 1000 + {"mixed": 5, "multi": 6}[design] * 1000

    def setup(self):
        rng = self.rng()
        self.ex = _exps(rng, self.K, self.centred)
        self.mu = rng.integers(-2, 3, self.K).astype(np.float32) if self.centred else None
        self.x = np.zeros((self.n, self.K), dtype=np.float32)
        if self.centred:
            self.x[:] = self.mu[None, :]
        self.cov, self.last = RowCoverage(self.n), []

    def missing(self):
        return [] if self.max_calls == 1 else self.cov.missing()      # (the widest shape: one call per design, no rotation)

    def call(self, c):
        rows, xr = _row_sparse(self, c, 8, self.design == "mixed", self.centred, MIXED if self.design == "mixed" else MULTI, self.rng(c + 1))
        self.x[self.last] = self.mu[None, :] if self.centred else 0.0
        self.x[rows] = centred_input(xr, self.mu)
        self.last = rows
        self.cov.add(rows)
        call = Call()
        call.kernel, call.n, call.want_z = "gram", self.n, False
        call.rows, call.xr = np.asarray(rows), xr
        call.args = {"x": self.x, "mu": self.mu}
        return call

    def products(self, call, forms):
        return [Product("c", call.xr, call.xr, 3, 3, tlab=call.rows, kaxis=(1, 1), tname="row")]

    def check(self, call, products, outs, where):
        return [products[0].check(outs["c"], where)]

    def run(self, runner, max_calls=MAX_CALLS):
        return super().run(runner, min(max_calls, self.max_calls))


class FusedCase(Case):
    """y = (X - mu)^T ((X - mu) P) and z = (X - mu) P through petal_power_pass with PETAL_OPT_FUSED_PASS_MIN_ROWS lowered to 64: X
    row-sparse (at most 8 non-zero rows), P with one non-zero per column at rotating k.  z has one term per element and is exact BY
    DESIGN (asserted): the second product's reference stands on it.  designs: mixed, p16 (power-of-two X, 16-bit P), multi."""
    kernel = "fused"
    exact_forms = [(3, 2), (3, 3)]

    def __init__(self, n, K, N, design, centred=False, want_z=False, hook=False):
        super().__init__(design, hook, small=n <= 96)
        self.n, self.K, self.N, self.centred, self.want_z = n, K, N, centred, want_z
        self.id = f"fused-{n}x{K}x{N}-{design}" + ("-centred" if centred else "") + ("-z" if want_z else "") + ("-hook" if hook else "")
        self.seed = (31 * n + 17 * K + 7 * N + 3 * centred + 2 * want_z + hook) % 1000 + {"mixed": 7, "p16": 8, "multi": 9}[design] * 1000

    def setup(self):
        GramCase.setup(self)
        self.kcov = set()

    def missing(self):
        m = self.cov.missing()
        K = self.K
        if len({k % 32 for k in self.kcov}) < 32 or len({k // 32 for k in self.kcov}) < K // 32 or len({k // 64 for k in self.kcov}) < K // 64:
            m.append("k mod 32 / 32-deep chunks / 64-feature wave slices of P")
        return m

    def proves_steering(self, forms):
        return forms == [(2, 2), (2, 2)] and self.design == "mixed"

    def call(self, c):
        rng = self.rng(c + 1)
        K, N = self.K, self.N
        classes = {"mixed": MIXED, "p16": [1], "multi": MULTI}[self.design]
        rows, xr = _row_sparse(self, c, 8, self.design != "multi", self.centred, classes, rng)
        self.x[self.last] = self.mu[None, :] if self.centred else 0.0
        self.x[rows] = centred_input(xr, self.mu)
        self.last = rows
        self.cov.add(rows)
        pi = pi_for_call(K, N, c)
        p = np.zeros((K, N), dtype=np.float32)
        p[pi, np.arange(N)] = bbit(rng, (N,), 16 if self.design == "p16" else 1, rng.integers(-4, 5, N))
        self.kcov.update(int(k) for k in pi)
        call = Call()
        call.kernel, call.n, call.want_z = "fused", self.n, self.want_z
        call.rows, call.xr, call.p, call.ks = np.asarray(rows), xr, p, np.unique(pi)
        call.args = {"x": self.x, "p": p, "mu": self.mu}
        return call

    def products(self, call, forms):
        (pu1, pv1), (pu2, pv2) = forms
        ks = np.arange(self.K) if self.small else call.ks
        p1 = Product("z", call.xr[:, ks].T, call.p[ks], pu1, pv1, tlab=ks, alab=call.rows, kaxis=(0, 0), tname="k")
        a1 = p1.analyse()
        assert a1["exact"].all(), f"{self.id}: z is not exact by design"
        zr = a1["ref"].astype(np.float32)
        assert np.array_equal(zr.astype(np.float64), a1["ref"])
        return [p1, Product("y", call.xr, zr, pu2, pv2, tlab=call.rows, kaxis=(1, 1), tname="row")]

    def check(self, call, products, outs, where):
        st = [products[1].check(outs["y"], where)]
        if call.want_z:
            z = np.asarray(outs["z"])
            st.append(products[0].check(z[call.rows], where))
            rest = np.ones(self.n, dtype=bool)
            rest[call.rows] = False
            assert not z[rest].any(), f"{where} z: rows of zero input are not zero: {np.unique(np.argwhere(z[rest] != 0)[:, 0])[:8].tolist()} (of the other rows)"
        return st


# ------------------------------------------------------------------------------------------- the tables
K1_SHAPES = [(64, 32, 16), (333, 48, 74), (4099, 512, 74), (777, 80, 138), (1000, 208, 200)]
# (n, M, N, the device runs the eight-wave 32-column form -- P4 under the hook)
K2_SHAPES = [(256, 64, 80, False), (1000, 48, 74, False), (4099, 512, 74, True), (777, 32, 138, True), (2048, 208, 200, True)]
FUSED_NS, FUSED_KS, FUSED_COLS = [96, 8200, 20011], [256, 512], [16, 48, 74]
GRAM_SHAPES = [(64, 64, MAX_CALLS), (5000, 200, MAX_CALLS), (8192, 256, MAX_CALLS), (4100, 1024, 1)]
SCORE_SHAPES = [(64, 32, 16), (4099, 512, 64)]
SINGLE = ["x24", "p24", "d12"]


def k1_cases():
    out = []
    for n, K, N in K1_SHAPES:
        for d in SINGLE + ["multi"]:
            out += [K1Case("k1", n, K, N, d), K1Case("k1", n, K, N, d, centred=True, bias=True), K1Case("k1", n, K, N, d, centred=True, bias=True, hook=True)]
    return out


def k2_cases():
    out = []
    for n, M, N, p4 in K2_SHAPES:
        for d in SINGLE + ["multi"]:
            out += [K2Case(n, M, N, d, "none"), K2Case(n, M, N, d, "a"), K2Case(n, M, N, d, "both"), K2Case(n, M, N, d, "a", hook=True, p4_shape=p4)]
    return out


def fused_cases():
    out = []
    for K in FUSED_KS:
        for N in FUSED_COLS:
            for n in FUSED_NS:
                for d in ["mixed", "p16", "multi"]:
                    out += [FusedCase(n, K, N, d), FusedCase(n, K, N, d, centred=True, want_z=True), FusedCase(n, K, N, d, centred=True, hook=True)]
    return out


def gram_cases():
    return [GramCase(n, d, design, centred, mc) for n, d, mc in GRAM_SHAPES for design in ["mixed", "multi"] for centred in (False, True)]


def score_cases():
    return [K1Case("score", n, d, k, design, centred=cen) for n, d, k in SCORE_SHAPES for design in SINGLE for cen in (True, False)]


TABLES = {"k1": k1_cases, "k2": k2_cases, "fused": fused_cases, "gram": gram_cases, "score": score_cases}


def all_cases():
    return [c for name in TABLES for c in TABLES[name]()]


def main():
    import time
    import petal_decomposition_amd as petal
    print("# case | GEMM mode | calls | elements in the exact class | mismatches among them | elements in the bounded class | largest error / bound there")
    t0 = time.time()
    failed = 0
    for mode in ("bf16x3", "fp32"):
        ctx = petal.Context(0)
        ctx.set_gemm_mode(mode)
        runner = DeviceRunner(ctx, split=mode == "bf16x3")
        for case in all_cases():
            try:
                calls, ne, nbad, nb, ratio = case.run(runner)
                print(f"{case.id:46s} {mode:7s} {calls:3d} {ne:10d} {nbad:4d} {nb:9d} {ratio:8.4f}")
            except AssertionError as e:
                failed += 1
                print(f"{case.id:46s} {mode:7s} FAILED: {e}")
        ctx.close()
    print(f"# {failed} cases failed; wall time {time.time() - t0:.0f} s")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
