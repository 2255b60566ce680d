"""Times Nmf(beta_loss="kullback-leibler") on a resident CsrMatrix (include/petal_hip_nmf_kl.h).  The project's protocol: medians of
--calls alternating calls after --warmup warm-up calls, a resident handle, every window ending in a device synchronise.

  fit        per iteration of Nmf.fit = (fit of 21 iterations - fit of 1) / 20, float32 data, k = 16 and 64, Kullback-Leibler and
             Frobenius fits alternating on the SAME handle, at the sparse-Nmf table's shapes: 200000 x 20000 at 0.2 % and 1 %, and
             1000000 x 512 at 1 % and 5 %
  sweep      the mean time of a sweep launch of one profiled fit of 10 iterations (event brackets; row and column sweeps alike, the
             split-row launch included): k_nmf_kl_sweep (20 update sweeps and the 2 sweeps of the loss) and, in the same session,
             k_nmf_sweep (Frobenius), beside the gather's bytes nnz (12 + 8 kp); their ratio is what the inner product, the division and
             the second use of every gathered row cost
  transform  20 updates: a handle without split rows loops in the kernel (one launch), re-reading its gathered rows from the caches

The host-loop fall-back (nmf_fallback = 1) is not timed here (the cell stays "unmeasured").  Writes profiles/nmf_kl_bench.json unless
--out says otherwise.
usage: python dev/nmf_kl_bench.py [--calls 5] [--warmup 2] [--shapes 200000x20000x0.002,...] [--ks 16,64] [--out FILE]"""
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
ap.add_argument("--shapes", default="200000x20000x0.002,200000x20000x0.01,1000000x512x0.01,1000000x512x0.05")
ap.add_argument("--ks", default="16,64")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "nmf_kl_bench.json"))
a = ap.parse_args()
ctx = petal.Context(0)
rng = np.random.default_rng(1)
KS = [int(v) for v in a.ks.split(",")]
KL = "kullback-leibler"


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
    """m stored entries per row at random columns (a duplicate now and then: legal), positive planted values"""
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


def profiled_sweep_ms(make):
    ctx.set_profiling(2)                                       # a run of its own: the brackets cost launches
    m = make(10).fit(sx)
    st = ctx.stats()
    ctx.set_profiling(0)
    assert m.kernel_path == 1
    m.close()
    return st["pow_ms"] / max(1, st["pow_launches"]), int(st["pow_launches"])


rows_out = []
for shape in a.shapes.split(","):
    n, d, density = shape.split("x")
    n, d, density = int(n), int(d), float(density)
    data, indices, indptr = pattern(n, d, density)
    sx = petal.CsrMatrix(data, indices, indptr, (n, d), ctx=ctx)
    assert sx.resident
    info = sx.info()
    for k in KS:
        kp = padded(k)
        kl = lambda it: petal.Nmf(k, max_iter=it, tol=0.0, init="random", seed=3, ctx=ctx, beta_loss=KL)   # noqa: E731
        fro = lambda it: petal.Nmf(k, max_iter=it, tol=0.0, init="random", seed=3, ctx=ctx)                 # noqa: E731
        t = medians({"kl1": lambda: kl(1).fit(sx), "kl21": lambda: kl(21).fit(sx), "fro1": lambda: fro(1).fit(sx), "fro21": lambda: fro(21).fit(sx)})
        gather = int(sx.nnz * (12 + 8 * kp))
        row = {"rows": n, "cols": d, "density": density, "nnz": int(sx.nnz), "k": k, "kp": kp, "dtype": "float32",
               "items": info["items"], "items_transposed": info["items_transposed"],
               "kl_fit_1_ms": t["kl1"], "kl_fit_21_ms": t["kl21"], "kl_per_iteration_ms": (t["kl21"] - t["kl1"]) / 20.0,
               "frobenius_per_iteration_ms": (t["fro21"] - t["fro1"]) / 20.0, "gather_bytes_per_sweep": gather}
        kms, kn = profiled_sweep_ms(kl)
        fms, fn_ = profiled_sweep_ms(fro)
        row.update({"kl_sweep_launches": kn, "kl_sweep_ms": kms, "frobenius_sweep_launches": fn_, "frobenius_sweep_ms": fms,
                    "kl_sweep_over_frobenius_sweep": kms / fms if fms > 0 else None,
                    "kl_sweep_TB_per_s_of_gather_bytes": gather / (kms * 1e-3) / 1e12 if kms > 0 else None,
                    "frobenius_sweep_TB_per_s_of_gather_bytes": gather / (fms * 1e-3) / 1e12 if fms > 0 else None})
        mt = petal.Nmf(k, max_iter=20, tol=1e6, init="random", seed=3, ctx=ctx, beta_loss=KL).fit(sx)   # (the fit stops at its first check)
        mf = petal.Nmf(k, max_iter=20, tol=1e6, init="random", seed=3, ctx=ctx).fit(sx)
        tt = medians({"kl": lambda: mt.transform(sx), "fro": lambda: mf.transform(sx)})
        row.update({"kl_transform_20_ms": tt["kl"], "frobenius_transform_20_ms": tt["fro"], "host_loop_fallback_per_iteration_ms": "unmeasured"})
        mt.close()
        mf.close()
        print(json.dumps(row), flush=True)
        rows_out.append(row)
    sx.close()
res = {"box": platform.node(), "device": torch.cuda.get_device_name(0),
       "note": "wall time of whole calls between device synchronises, medians of alternating calls after warm-up; per_iteration = (fit of 21 "
               "iterations - fit of 1) / 20; sweep_ms: event-bracketed launches of one profiled fit of 10 iterations, the mean over row and "
               "column sweeps (the Kullback-Leibler figure includes the 2 sweeps of the loss); gather_bytes_per_sweep = nnz (12 + 8 kp) -- "
               "index, value and one gathered fp64 row of the other factor per stored entry",
       "results": rows_out}
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
ctx.close()
