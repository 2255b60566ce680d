"""Times Nmf on a resident CsrMatrix (include/petal_hip_nmf_sparse.h).  The project's protocol: medians of --calls alternating calls after
--warmup warm-up calls, device-resident input, every window ending in a device synchronise.

  fit        per iteration of Nmf.fit = (fit of 21 iterations - fit of 1) / 20, float32 data, k = 16 and 64, at each --densities of a
             --rows x --cols matrix (200000 x 20000: the shapes of dev/sparse_bench.py); one profiled fit gives the mean time of a sweep
             launch (row and column sweeps alike, the split-row launch included) beside the gather's bytes nnz (12 + 8 kp)
  gemm       the same gather without the rule: the X . P launches of a profiled RandomizedPca.fit on a float64 handle of the same pattern
             with kp columns (k + n_oversample = kp), alternating with the Nmf fit -- the ratio says what the sweep's epilogue costs
  fallback   the forced densifying fit (nmf_fallback = 1) where the dense image fits the library's 2^32-byte limit
  transform  20 and 200 updates at k = 16 and 64: one pass over the matrix, the rule in the epilogue is what this prices
  cross      --cross: at 1000000 x 512 (the dense kernel's envelope) the sparse fit against dense Nmf.fit of the densified matrix at
             1 %, 5 % and 20 %

torch's float64 sparse_csr product is not timed here (the cell stays "unmeasured").  Writes profiles/nmf_sparse_bench.json unless --out
says otherwise.
usage: python dev/nmf_sparse_bench.py [--calls 5] [--warmup 2] [--rows 200000] [--cols 20000] [--densities 0.002,0.01,0.05] [--cross] [--cross-densities 0.01,0.05,0.2] [--out FILE]"""
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
ap.add_argument("--ks", default="16,64")
ap.add_argument("--cross", action="store_true")
ap.add_argument("--cross-densities", default="0.01,0.05,0.2")
ap.add_argument("--no-gemm", action="store_true")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "nmf_sparse_bench.json"))
a = ap.parse_args()
ctx = petal.Context(0)
rng = np.random.default_rng(1)
KS = [int(v) for v in a.ks.split(",")]


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def medians(fns):
    """{name: median ms} of the callables, alternating"""
    ts = {name: [] for name in fns}
    for it in range(a.warmup + a.calls):
        for name, fn in fns.items():
            t = wall(fn)
            if it >= a.warmup:
                ts[name].append(t)
    return {name: float(np.median(v)) for name, v in ts.items()}


def pattern(n, d, density):
    """m stored entries per row at random columns (a duplicate now and then: legal), non-negative planted values"""
    m = max(1, int(round(density * d)))
    indices = rng.integers(0, d, (n, m), dtype=np.int32)
    u, v = rng.random((n, 8), dtype=np.float32), rng.random((d, 8), dtype=np.float32)
    data = np.empty((n, m), dtype=np.float32)
    for lo in range(0, n, 20000):
        hi = min(n, lo + 20000)
        data[lo:hi] = np.einsum("if,imf->im", u[lo:hi], v[indices[lo:hi]]) + 0.05 * rng.random((hi - lo, m), dtype=np.float32)
    return data.ravel(), indices.ravel(), np.arange(n + 1, dtype=np.int64) * m


def padded(k):
    return 16 if k <= 16 else 32 if k <= 32 else 64


def fit_rows(n, d, density, cross=False):
    data, indices, indptr = pattern(n, d, density)
    sx = petal.CsrMatrix(data, indices, indptr, (n, d), ctx=ctx)
    assert sx.resident
    nnz, out = sx.nnz, []
    s64 = None
    if not a.no_gemm and not cross:
        s64 = petal.CsrMatrix(data.astype(np.float64), indices, indptr, (n, d), ctx=ctx)
    xd = None
    if cross:
        xd = torch.zeros((n, d), dtype=torch.float32, device="cuda")
        r = torch.arange(n, device="cuda").repeat_interleave(len(indices) // n)
        xd.index_put_((r, torch.from_numpy(indices.astype(np.int64)).cuda()), torch.from_numpy(data).cuda(), accumulate=True)
    for k in KS:
        kp = padded(k)
        mk = lambda it: petal.Nmf(k, max_iter=it, tol=0.0, init="random", seed=3, ctx=ctx)   # noqa: E731
        fns = {"fit1": lambda: mk(1).fit(sx), "fit21": lambda: mk(21).fit(sx)}
        if xd is not None:
            fns.update({"dense1": lambda: mk(1).fit(xd), "dense21": lambda: mk(21).fit(xd)})
        t = medians(fns)
        row = {"rows": n, "cols": d, "density": density, "nnz": int(nnz), "k": k, "kp": kp, "dtype": "float32",
               "fit_1_ms": t["fit1"], "fit_21_ms": t["fit21"], "per_iteration_ms": (t["fit21"] - t["fit1"]) / 20.0,
               "gather_bytes_per_sweep": int(nnz * (12 + 8 * kp))}
        if xd is not None:
            row.update({"dense_fit_1_ms": t["dense1"], "dense_fit_21_ms": t["dense21"], "dense_per_iteration_ms": (t["dense21"] - t["dense1"]) / 20.0})
        ctx.set_profiling(2)                                   # a run of its own: the brackets cost launches
        m = mk(5).fit(sx)
        st = ctx.stats()
        ctx.set_profiling(0)
        assert m.kernel_path == 1
        ms = st["pow_ms"] / max(1, st["pow_launches"])
        row.update({"sweep_launches": int(st["pow_launches"]), "sweep_ms": ms,
                    "sweep_TB_per_s": row["gather_bytes_per_sweep"] / (ms * 1e-3) / 1e12 if ms > 0 else None})
        if s64 is not None:                                     # the same gather without the rule: X . P of float64 data, kp columns
            om = rng.standard_normal((d, kp))
            rp = petal.RandomizedPca(kp - 10, ctx=ctx, n_iter=2, n_oversample=10)
            ctx.set_profiling(2)
            rp.fit(s64, omega=om)
            sg = ctx.stats()
            ctx.set_profiling(0)
            gm = sg["xp_ms"] / max(1, sg["xp_launches"])
            row.update({"csr_gemm_f64_ms": gm, "sweep_over_gemm": ms / gm if gm > 0 else None,
                        "note_gemm": "float64 values: 16 bytes per stored entry against the sweep's 12 on float32 data"})
        if not cross and float(n) * d * 4 <= 2.0 ** 32:
            ctx.set_option("nmf_fallback", 1)
            tf = medians({"fb1": lambda: mk(1).fit(sx), "fb3": lambda: mk(3).fit(sx)})
            ctx.set_option("nmf_fallback", 0)
            row.update({"fallback_fit_1_ms": tf["fb1"], "fallback_per_iteration_ms": (tf["fb3"] - tf["fb1"]) / 2.0})
        else:
            row["fallback_per_iteration_ms"] = "unmeasured: the dense image exceeds the 2^32-byte limit" if not cross else "unmeasured"
        if not cross:
            for upd in (20, 200):
                mt = petal.Nmf(k, max_iter=upd, tol=1e6, init="random", seed=3, ctx=ctx).fit(sx)   # (the fit stops at its first check)
                row[f"transform_{upd}_ms"] = medians({"t": lambda: mt.transform(sx)})["t"]
                mt.close()
        row["torch_sparse_csr_f64_ms"] = "unmeasured"
        print(json.dumps(row), flush=True)
        out.append(row)
    sx.close()
    if s64 is not None:
        s64.close()
    del xd
    torch.cuda.empty_cache()
    return out


rows_out = []
for density in [float(v) for v in a.densities.split(",")]:
    rows_out += fit_rows(a.rows, a.cols, density)
cross_out = []
if a.cross:
    for density in [float(v) for v in a.cross_densities.split(",")]:
        cross_out += fit_rows(1000000, 512, density, cross=True)
res = {"box": platform.node(), "device": torch.cuda.get_device_name(0),
       "note": "wall time of whole calls between device synchronises, medians of alternating calls after warm-up; per_iteration = (fit of 21 "
               "iterations - fit of 1) / 20; sweep_ms: event-bracketed launches of one profiled fit, the mean over row and column sweeps; "
               "gather_bytes_per_sweep = nnz (12 + 8 kp) -- index, value and one gathered fp64 row of the other factor per stored entry",
       "results": rows_out, "dense_crossing_1000000x512": cross_out if a.cross else "unmeasured"}
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
ctx.close()
