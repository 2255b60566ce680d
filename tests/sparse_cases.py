"""RandomizedPca on sparse CSR data (include/petal_hip_sparse.h): the test generator, a numpy model of the sparse pipeline, the parity case
table with its bars, the exact-integer matrices of the product tests, and the checks the GPU suite and the host suite share.  numpy
only: scipy is imported nowhere.

Run as a script on a machine with the GPU it writes profiles/sparse_errors.txt: per case the largest error over its bar."""
import functools
import os
import sys
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import petal_oracle as po  # noqa: E402
import petal_decomposition_amd as petal  # noqa: E402
from parity_cases import decided_signs, rowwise_rel  # noqa: E402

ITEM_NNZ = petal.CSR_ITEM_NNZ
N_OVERSAMPLE = 10


# ------------------------------------------------------------------------------------------- the generator
def synth_sparse(n, d, k, seed, du=0.05, dv=0.05, noise=0.01, dn=0.01):
    """A dense float64 array that is mostly zeros: the sum over r = 2 k factors of 100 rho^j u_j v_j^T, rho = 10^(-3 / k), u_j and v_j with
    Bernoulli(du) / Bernoulli(dv) support and N(0.5, 1) values, plus N(0, noise^2) entries on a Bernoulli(dn) mask."""
    rng = np.random.default_rng(seed)
    rho = 10.0 ** (-3.0 / k)
    x = np.zeros((n, d))
    for j in range(2 * k):
        u = (rng.random(n) < du) * rng.normal(0.5, 1.0, n)
        v = (rng.random(d) < dv) * rng.normal(0.5, 1.0, d)
        x += 100.0 * rho ** j * np.outer(u, v)
    x += (rng.random((n, d)) < dn) * rng.normal(0.0, noise, (n, d))
    return x


def to_csr(x):
    """(data, indices, indptr) of the nonzero entries of a dense array, in its dtype."""
    r, c = np.nonzero(x)
    indptr = np.zeros(x.shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=x.shape[0]), out=indptr[1:])
    return x[r, c].copy(), c.astype(np.int32), indptr


def densify(data, indices, indptr, shape, dtype=None):
    """The dense array of a CSR triple, duplicates added in position order in the data's own type (what the library's fall-back forms)."""
    out = np.zeros(shape, dtype=data.dtype if dtype is None else dtype)
    rows = np.repeat(np.arange(shape[0]), np.diff(indptr))
    np.add.at(out, (rows, indices), data.astype(out.dtype))
    return out


class Duck:
    """the least a sparse input needs: .data / .indices / .indptr / .shape"""

    def __init__(self, data, indices, indptr, shape):
        self.data, self.indices, self.indptr, self.shape = data, indices, indptr, shape


# ------------------------------------------------------------------------------------------- the parity cases and their bars
Case = namedtuple("Case", "n d k n_iter dt centering du dv seed")
CASES = [
    Case(3000, 400, 8, 7, "f32", True, 0.05, 0.05, 11),
    Case(3000, 400, 8, 2, "f64", True, 0.05, 0.05, 12),
    Case(2000, 1000, 12, 5, "f32", True, 0.05, 0.05, 13),
    Case(257, 130, 4, 0, "f32", False, 0.05, 0.05, 14),
    Case(130, 257, 4, 7, "f64", True, 0.05, 0.05, 15),          # n < d
    Case(1500, 3000, 16, 7, "f32", True, 0.03, 0.03, 16),
    Case(1200, 300, 70, 5, "f32", True, 0.02, 0.02, 17),        # l = 80: more than 64 columns, the kernel walks column panels
]


def case_id(c):
    return f"{c.n}x{c.d}-k{c.k}-it{c.n_iter}-{c.dt}-{'c' if c.centering else 'nc'}"


def bar(c):
    """the project's parity bar (tests/parity_cases.py::rpca_parity): component rows and singular values, relative"""
    return 1e-5 if c.dt == "f32" else 1e-9


def np_dtype(c):
    return np.float32 if c.dt == "f32" else np.float64


@functools.lru_cache(maxsize=None)
def inputs(c):
    """x (dense, the case's dtype), its CSR triple, and Omega (float64, exactly representable in the case's dtype)"""
    x = synth_sparse(c.n, c.d, c.k, c.seed, du=c.du, dv=c.dv).astype(np_dtype(c))
    om = np.random.default_rng(c.seed + 1000).standard_normal((c.d, c.k + N_OVERSAMPLE)).astype(np_dtype(c)).astype(np.float64)
    for a in (x, om):
        a.setflags(write=False)
    return x, to_csr(x), om


@functools.lru_cache(maxsize=None)
def reference(c):
    """the oracle on the densified float64 matrix with the same Omega and n_iter: (oracle, its U, its y)"""
    x, _, om = inputs(c)
    o = po.RandomizedPcaOracle(c.k, centering=c.centering, n_iter=c.n_iter, n_oversample=N_OVERSAMPLE)
    uo = o._inner_fit(x.astype(np.float64), omega=om)
    return o, uo, po.transform_with_u(uo, o.singular, c.k)


# ------------------------------------------------------------------------------------------- the numpy model of the pipeline
def model_fit(x, om, k, n_iter, centering, storage, accumulate=np.float64):
    """The sparse pipeline in numpy: implicit centring, every iterate stored in `storage`, products accumulated in `accumulate`,
    Cholesky-QR re-basing on fp64 Gram matrices on both sides, Cholesky-QR2 for Q, the Gram route for the SVD of B.
    Returns (components, singular values)."""
    x64 = x.astype(np.float64)
    n = x.shape[0]
    mu = x64.mean(axis=0) if centering else np.zeros(x.shape[1])

    def st(a):
        return a.astype(storage).astype(np.float64)

    def prod(a, b):
        return (a.astype(accumulate) @ b.astype(accumulate)).astype(np.float64)

    def xp(p):      # Xc P = X P - 1 (mu^T P)
        return st(prod(x64, p) - np.outer(np.ones(n), mu @ p))

    def xtz(z):     # Xc^T Z = X^T Z - mu (1^T Z)
        return st(prod(x64.T, z) - np.outer(mu, z.sum(axis=0)))

    def rebase(a):
        r = np.linalg.cholesky(a.T @ a).T
        return st(np.linalg.solve(r.T, a.T).T)

    L = min(om.shape[1], *x.shape)
    z = xp(st(om[:, :L]))
    for _ in range(n_iter):
        z = xp(rebase(xtz(rebase(z))))
    q = rebase(rebase(z))
    bt = xtz(q)
    lam, uh = np.linalg.eigh(bt.T @ bt)
    lam, uh = lam[::-1][:k], uh[:, ::-1][:, :k]
    sig = np.sqrt(np.maximum(lam, 0.0))
    return st((bt @ uh / sig).T), sig


def model_errors(c):
    """the model's distance from the oracle: (largest component row error, largest singular value error), both relative"""
    x, _, om = inputs(c)
    o, _, _ = reference(c)
    comp, sig = model_fit(x, om, c.k, c.n_iter, c.centering, np_dtype(c))
    return float(rowwise_rel(comp, o.components).max()), float(np.abs(sig / o.singular - 1).max())


# ------------------------------------------------------------------------------------------- the parity check both suites run
def check_parity(ctx, c, expect_kernel):
    """The sparse fit of a case against the oracle with the accuracy contract's bars; returns {quantity: error / bar}.  Every figure is
    printed before it is asserted."""
    x, (data, indices, indptr), om = inputs(c)
    o, uo, yo = reference(c)
    tol = bar(c)
    sx = petal.CsrMatrix(data, indices, indptr, x.shape, ctx=ctx)
    try:
        m = petal.RandomizedPca(c.k, centering=c.centering, ctx=ctx, n_iter=c.n_iter, n_oversample=N_OVERSAMPLE)
        y = m.fit_transform(sx, omega=om.astype(np_dtype(c)))
        path = m.kernel_path
        t = m.transform(sx)
        path_t = m.kernel_path
    finally:
        sx.close()
    comp = m.components().astype(np.float64)
    sgn = np.sign(np.sum(comp * o.components, axis=1))
    s = np.sign(np.sum(y.astype(np.float64) * yo, axis=0))
    s[s == 0] = 1
    to = o.transform(x.astype(np.float64))
    err = {
        "comp": float(rowwise_rel(comp, o.components).max()) / tol,
        "sing": float(np.abs(m.singular_values().astype(np.float64) / o.singular - 1).max()) / tol,
        "evr": float(np.abs(m.explained_variance_ratio().astype(np.float64) / o.explained_variance_ratio() - 1).max()) / (4 * tol),
        "mean": float(np.abs(m.mean() - o.means).max()) / (1e-6 * max(1.0, float(np.abs(o.means).max()))),
        "y": float(np.abs(y * s - yo).max() / np.abs(yo).max()) / (20 * tol),
        "transform": float(np.abs(t * s - to).max() / np.abs(to).max()) / (20 * tol),
    }
    print(f"{case_id(c)}: kernel_path {path}/{path_t}  " + "  ".join(f"{q} {v:.3f}" for q, v in err.items()) + "  (error / bar)")
    assert path == int(expect_kernel) and path_t == int(expect_kernel), (path, path_t)
    assert y.dtype == np_dtype(c) and m.components().dtype == np_dtype(c)
    for q, v in err.items():
        assert v <= 1.0, (case_id(c), q, v)
    dec = decided_signs(uo, c.k, margin=min(0.5, max(1e-3, 100 * tol)))
    assert np.all(sgn[dec] == 1), f"svd_flip signs differ from the oracle's on decided components {np.nonzero(dec & (sgn != 1))[0]}"
    return err, m


# ------------------------------------------------------------------------------------------- exact-integer matrices for the product
def int_matrix(n, d, seed, long_by):
    """An integer-valued CSR triple (|x| <= 8) with empty rows and columns, unsorted indices, a duplicated entry, an explicit zero, and one
    row and one column of 2 ITEM_NNZ + 3 stored entries: `long_by` "dense" enlarges the other dimension so that the row / column is
    fully dense, "dup" keeps the shape and reaches the length with duplicates.  Returns (data float64, indices, indptr, shape)."""
    rng = np.random.default_rng(seed)
    long = 2 * ITEM_NNZ + 3
    if long_by == "dense":
        n, d = max(n, long + 2), max(d, long + 2)                # (two empty rows / columns stay empty)
    rows = [[] for _ in range(n)]           # lists of (column, value)
    empty_r, empty_c = {1, n - 2}, {0, d - 3}
    long_r, long_c = 3, 5
    for i in range(n):
        if i in empty_r or i == long_r:
            continue
        cols = np.nonzero(rng.random(d) < 0.08)[0]
        rows[i] = [(int(j), int(v)) for j, v in zip(cols, rng.integers(-8, 9, cols.size)) if j not in empty_c and j != long_c]
    ok_c = [j for j in range(d) if j not in empty_c]
    rows[long_r] = [(ok_c[q % len(ok_c)], int(rng.integers(-8, 9))) for q in range(long)]          # the long row ("dup": every column again and again)
    placed, q = sum(1 for e in rows[long_r] if e[0] == long_c), 0
    ok_r = [i for i in range(n) if i not in empty_r and i != long_r]
    while placed < long:                                                                             # the long column
        rows[ok_r[q % len(ok_r)]].append((long_c, int(rng.integers(-8, 9))))
        placed, q = placed + 1, q + 1
    rows[7].append(rows[7][0])                                   # a duplicated entry
    rows[8].append((4, 0))                                       # an explicit zero
    data, indices, indptr = [], [], [0]
    for i in range(n):
        order = rng.permutation(len(rows[i]))                    # unsorted inside the row
        indices += [rows[i][q][0] for q in order]
        data += [rows[i][q][1] for q in order]
        indptr.append(len(indices))
    data, indices, indptr = np.asarray(data, dtype=np.float64), np.asarray(indices, dtype=np.int32), np.asarray(indptr, dtype=np.int64)
    dense = densify(data, indices, indptr, (n, d))
    assert np.diff(indptr)[long_r] == long and np.bincount(indices, minlength=d)[long_c] == long
    assert not dense[sorted(empty_r)].any() and not dense[:, sorted(empty_c)].any() and np.abs(data).max() <= 8
    assert any(np.any(np.diff(indices[indptr[r]:indptr[r + 1]]) < 0) for r in range(n))
    return data, indices, indptr, (n, d)


GEMM_WIDTHS = (1, 14, 16, 17, 64, 74, 80, 138)
INT_SHAPES = [(257, 130, "dup"), (130, 257, "dup"), (257, 130, "dense"), (130, 257, "dense")]


def check_gemm_exact(ctx, n, d, long_by, dt, widths=GEMM_WIDTHS):
    """petal_csr_gemm on an integer matrix with integer P, a, s: every product and sum is exact in fp64 and in fp32 storage, so the result
    equals the numpy integer result bit for bit -- both images, with and without the epilogue.  Returns the handle's info."""
    data, indices, indptr, shape = int_matrix(n, d, seed=n + 7 * d, long_by=long_by)
    dense = densify(data, indices, indptr, shape).astype(np.int64)
    rng = np.random.default_rng(5)
    sx = petal.CsrMatrix(data.astype(dt), indices, indptr, shape, ctx=ctx)
    try:
        info = sx.info()
        for N in widths:
            for transposed in (False, True):
                xm = dense.T if transposed else dense
                p = rng.integers(-8, 9, (xm.shape[1], N))
                a, s = rng.integers(-8, 9, xm.shape[0]), rng.integers(-8, 9, N)
                for ref, kw in ((xm @ p, {}), (xm @ p - np.outer(a, s), {"a": a, "s": s}), (xm @ p - s[None, :], {"s": s})):
                    assert np.abs(ref).max() < 2 ** 24
                    out = petal.csr_gemm(sx, p, transposed=transposed, **kw)
                    bad = np.argwhere(out != ref)
                    assert bad.size == 0, (f"csr_gemm {shape} {long_by} {np.dtype(dt).name} N={N} transposed={transposed} {sorted(kw)}: "
                                           f"{bad.shape[0]} wrong, first at {bad[:4].tolist()}")
    finally:
        sx.close()
    return info


# ------------------------------------------------------------------------------------------- profiles/sparse_errors.txt
def main():
    ctx = petal.Context(0)
    lines = ["# tests/sparse_cases.py on one MI355X (petal_rpca_fit_csr through RandomizedPca on a resident CsrMatrix, kernel_path = 1): per case",
             "# the error of every quantity of the accuracy contract over its bar (components and singular values 1e-5 float32 / 1e-9 float64,",
             "# explained_variance_ratio 4x, means 1e-6 max(1, |mu|), y and transform 20x of their largest entry), against the oracle on the",
             "# densified float64 matrix with the same Omega and n_iter; `model`: the numpy model of the pipeline (component, singular value error)."]
    worst = (0.0, "", "")
    for c in CASES:
        err, _ = check_parity(ctx, c, expect_kernel=True)
        me = model_errors(c)
        lines.append(f"{case_id(c)}: " + "  ".join(f"{q} {v:.4f}" for q, v in err.items()) + f"  model comp {me[0]:.2e} sing {me[1]:.2e}")
        for q, v in err.items():
            if v > worst[0]:
                worst = (v, q, case_id(c))
    lines.insert(4, f"# Largest error over bar: {worst[0]:.4f} ({worst[1]}, {worst[2]}).")
    out = os.path.join(ROOT, "profiles", "sparse_errors.txt")
    if len(sys.argv) > 1:
        out = sys.argv[1]
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    ctx.close()


if __name__ == "__main__":
    main()
