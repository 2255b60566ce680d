"""Times RandomizedPca.fit (k = 64, n_iter = 5) on a resident CsrMatrix of 200000 x 20000 at densities 0.2 %, 1 % and 5 % against the dense
fit of the same matrix densified in HBM (16 GB in float32: what a user with sparse data had to do before): same process, alternating
runs, wall time of the whole call.  A second, profiled run (event brackets on every tagged launch) gives the time per sparse product
launch against the bytes it must move, nnz (8 + 4 LP).  Writes profiles/sparse_bench.json unless --out says otherwise.
usage: python dev/sparse_bench.py [--calls 5] [--warmup 2] [--rows 200000] [--cols 20000] [--out FILE.json] [--no-dense]"""
import argparse
import json
import os
import platform
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import petal_decomposition_amd as petal

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--rows", type=int, default=200000)
ap.add_argument("--cols", type=int, default=20000)
ap.add_argument("--densities", default="0.002,0.01,0.05")
ap.add_argument("--no-dense", action="store_true")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sparse_bench.json"))
a = ap.parse_args()

K, N_ITER, N_OVERSAMPLE = 64, 5, 10
LP = (K + N_OVERSAMPLE + 15) // 16 * 16
n, d = a.rows, a.cols
ctx = petal.Context(0)
rng = np.random.default_rng(1)
omega = rng.standard_normal((d, K + N_OVERSAMPLE)).astype(np.float32)
rows_out = []


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


for density in [float(v) for v in a.densities.split(",")]:
    m = max(1, int(round(density * d)))                       # stored entries per row (a duplicate now and then: legal, they add up)
    t0 = time.perf_counter()
    indices = rng.integers(0, d, (n, m), dtype=np.int32)
    # a planted low-rank part so that the spectrum is not flat, plus noise: row i weighs factor f by u[i, f], column j by v[j, f]
    u, v = rng.standard_normal((n, 8)).astype(np.float32), rng.standard_normal((d, 8)).astype(np.float32) * np.linspace(3, 0.5, 8, dtype=np.float32)
    data = np.empty((n, m), dtype=np.float32)
    for lo in range(0, n, 20000):                              # in slabs: the gathered factors of a slab are m x 8 floats a row
        hi = min(n, lo + 20000)
        data[lo:hi] = np.einsum("if,imf->im", u[lo:hi], v[indices[lo:hi]]) + 0.3 * rng.standard_normal((hi - lo, m)).astype(np.float32)
    indptr = np.arange(n + 1, dtype=np.int64) * m
    t_gen = time.perf_counter() - t0
    t0 = time.perf_counter()
    sx = petal.CsrMatrix(data.ravel(), indices.ravel(), indptr, (n, d), ctx=ctx)
    t_create = time.perf_counter() - t0
    assert sx.resident
    nnz = sx.nnz
    xd = None
    if not a.no_dense:
        xd = torch.zeros((n, d), dtype=torch.float32, device="cuda")
        for lo in range(0, n, 20000):
            hi = min(n, lo + 20000)
            r = torch.arange(lo, hi, device="cuda").repeat_interleave(m)
            xd.index_put_((r, torch.from_numpy(indices[lo:hi].ravel().astype(np.int64)).cuda()), torch.from_numpy(data[lo:hi].ravel()).cuda(),
                          accumulate=True)
    sparse, dense = petal.RandomizedPca(K, ctx=ctx, n_iter=N_ITER), petal.RandomizedPca(K, ctx=ctx, n_iter=N_ITER)
    ts, td = [], []
    for it in range(a.warmup + a.calls):                       # alternating
        t = wall(lambda: sparse.fit(sx, omega=omega))
        if it >= a.warmup:
            ts.append(t)
        if xd is not None:
            t = wall(lambda: dense.fit(xd, omega=omega))
            if it >= a.warmup:
                td.append(t)
    assert sparse.kernel_path == 1
    agree = None
    if xd is not None:
        agree = float(np.abs(sparse.singular_values().astype(np.float64) / dense.singular_values() - 1).max())
    ctx.set_profiling(2)                                       # a run of its own: the brackets cost launches
    sparse.fit(sx, omega=omega)
    st = ctx.stats()
    ctx.set_profiling(0)
    bytes_launch = nnz * (8 + 4 * LP)
    per = {}
    for tag, what in (("xp", "X . P"), ("atb", "X^T . Z")):
        ms = st[f"{tag}_ms"] / max(1, st[f"{tag}_launches"])
        per[what] = {"launches": int(st[f"{tag}_launches"]), "ms_per_launch": ms, "bytes_per_launch": bytes_launch,
                     "TB_per_s": bytes_launch / (ms * 1e-3) / 1e12 if ms > 0 else None}
    ms_, md_ = float(np.median(ts)), float(np.median(td)) if td else None
    row = {"rows": n, "cols": d, "density": density, "nnz": int(nnz), "k": K, "n_iter": N_ITER, "LP": LP, "dtype": "float32",
           "csr_bytes": int(nnz * 8 + (n + 1) * 8), "dense_bytes": int(n * d * 4),
           "sparse_fit_ms": {"median": ms_, "min": float(min(ts)), "max": float(max(ts)), "calls": len(ts)},
           "dense_fit_ms": None if not td else {"median": md_, "min": float(min(td)), "max": float(max(td)), "calls": len(td)},
           "dense_over_sparse": None if not td else md_ / ms_, "max_sigma_difference_rel": agree,
           "spmm": per, "profiled_fit_ms": st["fit_ms"], "generate_s": t_gen, "csr_create_s": t_create}
    print(json.dumps(row), flush=True)
    rows_out.append(row)
    sx.close()
    del xd, data, indices
    torch.cuda.empty_cache()

res = {"box": platform.node(), "device": torch.cuda.get_device_name(0),
       "note": "wall time of the whole fit call (results land in host arrays: every call ends synchronised), medians of alternating runs after "
               "warm-up; the dense fit runs on the same matrix densified and resident in HBM; spmm: event-bracketed launches of one profiled fit, "
               "bytes_per_launch = nnz (8 + 4 LP) -- index, value and one gathered row of the dense operand per nonzero",
       "results": rows_out}
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
ctx.close()
