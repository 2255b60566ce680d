"""Times IncrementalPca on a matrix resident in HBM fed as B device batches: total partial_fit time (ending in a device synchronise),
finalize, the same batches on the forced two-pass path (PETAL_OPT_IPCA_FALLBACK), and Pca.fit of the whole matrix in the same process
(pca_fit's kernels and launch sequence are what they were before IncrementalPca was added).  Medians of five alternating calls after
two warm-ups.  The one expectation checked: the kernel path is not slower than the two-pass path at any point.
Writes profiles/ipca_bench.json unless --out says otherwise.
usage: python dev/ipca_bench.py [--calls 5] [--warmup 2] [--out FILE.json] [--small]"""
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
ap.add_argument("--small", action="store_true", help="a thousandth of the rows: a rehearsal of the script, not a measurement")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ipca_bench.json"))
a = ap.parse_args()

SHAPES = [(1000000, 64, torch.float32), (500000, 512, torch.float32), (200000, 256, torch.float32), (200000, 64, torch.float64)]
BATCHES = (1, 8, 64)
K = 16
ctx = petal.Context(0)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def med(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "calls": len(v)}


rows_out, slower = [], []
for n, d, dt in SHAPES:
    if a.small:
        n //= 1000
    gen = torch.Generator(device="cuda").manual_seed(n + d)
    x = torch.randn((n, d), dtype=dt, device="cuda", generator=gen) * torch.linspace(4.0, 0.5, d, dtype=dt, device="cuda") + 1.5
    whole = petal.Pca(K, ctx=ctx)
    for B in BATCHES:
        step = -(-n // B)
        parts = [x[r:r + step] for r in range(0, n, step)]
        inc = {0: petal.IncrementalPca(K, ctx=ctx), 1: petal.IncrementalPca(K, ctx=ctx)}

        def feed(fallback):
            m = inc[fallback]
            m.reset()
            ctx.set_option("ipca_fallback", fallback)
            for p in parts:
                m.partial_fit(p)
            ctx.set_option("ipca_fallback", 0)

        t = {0: [], 1: [], "finalize": [], "pca": []}
        for it in range(a.warmup + a.calls):                   # alternating
            for fallback in (0, 1):
                v = wall(lambda: feed(fallback))
                if it >= a.warmup:
                    t[fallback].append(v)
            v = wall(lambda: inc[0].finalize())
            w = wall(lambda: whole.fit(x)) if B == BATCHES[0] else None
            if it >= a.warmup:
                t["finalize"].append(v)
                if w is not None:
                    t["pca"].append(w)
        assert inc[0].info()["kernel_batches"] == len(parts) and inc[1].info()["kernel_batches"] == 0
        agree = float(np.abs(inc[0].singular_values().astype(np.float64) / inc[1].singular_values() - 1).max())
        row = {"rows": n, "cols": d, "dtype": str(dt).replace("torch.", ""), "batches": len(parts), "k": K,
               "partial_fit_total_ms": med(t[0]), "two_pass_total_ms": med(t[1]), "finalize_ms": med(t["finalize"]),
               "pca_fit_whole_ms": med(t["pca"]) if t["pca"] else None, "two_pass_over_kernel": float(np.median(t[1]) / np.median(t[0])),
               "max_sigma_difference_rel": agree if np.isfinite(agree) else None}
        if row["two_pass_over_kernel"] < 1.0:
            slower.append((n, d, row["dtype"], len(parts)))
        print(json.dumps(row), flush=True)
        rows_out.append(row)
        for m in inc.values():
            m.close()
    del x
    torch.cuda.empty_cache()

res = {"box": platform.node(), "device": torch.cuda.get_device_name(0), "rehearsal": bool(a.small),
       "note": "wall time around the calls, each window ending in a device synchronise; device-resident input (zero copy); medians of alternating "
               "calls after warm-up; two_pass: the same batches with PETAL_OPT_IPCA_FALLBACK set; pca_fit_whole: Pca.fit of the whole matrix, same "
               "process (its code path is unchanged by IncrementalPca)",
       "kernel_path_slower_at": slower, "results": rows_out}
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
ctx.close()
