"""Exact Pca on wide data (include/petal_hip_wide.h): the dual route against the primal route forced with pca_dual = -1 (the behaviour
before the dual route existed) where both can run, the dual route alone where the primal one cannot, and k_row_gram by itself (the
launch under TAG_ATB with profiling on: stats atb_ms) beside the two floors it can be priced against.  Writes profiles/pca_wide_bench.json: medians of five alternating calls after two
warm-up calls, wall time around the calls, each window ending in a device synchronise; device-resident input (zero copy)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import petal_decomposition_amd as petal  # noqa: E402

HBM_GBS = 6000.0      # the measured streaming rate the project prices passes against (about 6 TB/s)
FP64_TFLOPS = 78.6    # MI355X matrix fp64 peak
K = 16
BOTH = [(512, 4096, torch.float32), (1024, 8192, torch.float32), (2048, 8192, torch.float32), (512, 4096, torch.float64)]
DUAL_ONLY = [(1000, 100000, torch.float32), (2000, 50000, torch.float32)]


def data(n, d, dt):
    g = torch.Generator(device="cuda").manual_seed(n + d)
    s = 10.0 * 0.8 ** torch.arange(2 * K, device="cuda", dtype=torch.float64)
    x = (torch.randn((n, 2 * K), generator=g, device="cuda", dtype=torch.float64) * s) @ torch.randn((2 * K, d), generator=g, device="cuda", dtype=torch.float64)
    x += 0.01 * torch.randn((n, d), generator=g, device="cuda", dtype=torch.float64) + 1.0
    return x.to(dt).contiguous()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(fns, warm=2, reps=5):
    for _ in range(warm):
        for f in fns:
            f()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            ts[i].append(timed(f))
    return [statistics.median(t) for t in ts]


def main():
    ctx = petal.Context(0)
    rows = []

    def fit(x, dual):
        def run():
            ctx.set_option("pca_dual", dual)
            petal.Pca.new(K, ctx).fit(x)
            ctx.set_option("pca_dual", 0)
        return run

    for n, d, dt in BOTH + DUAL_ONLY:
        x = data(n, d, dt)
        esz = x.element_size()
        both = (n, d, dt) in BOTH
        fns = [fit(x, 0)] + ([fit(x, -1)] if both else [])
        med = alternate(fns)
        # the kernel alone: event brackets around the one tagged launch of a dual fit, in fits of their own (profiling costs time)
        ctx.set_profiling(2)
        kern = []
        for i in range(7):
            petal.Pca.new(K, ctx).fit(x)
            st = ctx.stats()
            assert st["atb_launches"] == 1, st
            if i >= 2:
                kern.append(st["atb_ms"])
        ctx.set_profiling(0)
        route = petal.Pca.new(K, ctx).last_route()
        row = {"n": n, "d": d, "dtype": str(dt).split(".")[-1], "k": K, "auto_route": route, "fit_auto_ms": med[0],
               "fit_primal_forced_ms": med[1] if both else None, "k_row_gram_ms": statistics.median(kern),
               "floor_read_once_ms": n * d * esz / (HBM_GBS * 1e9) * 1e3, "floor_fp64_upper_triangle_ms": n * n * d / (FP64_TFLOPS * 1e12) * 1e3}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del x
    out = {"device": torch.cuda.get_device_name(0),
           "note": "wall time around the calls, each window ending in a device synchronise; device-resident input (zero copy); medians of five "
                   "alternating calls after two warm-up calls; fit_auto: the default options (the auto rule: dual when n < d and d > 2048); "
                   "fit_primal_forced: pca_dual = -1, the d x d Gram route; k_row_gram: stream time between events around the kernel's launch "
                   "(profiling level 2, median of five fits after two; the slab sum that follows it is not included); floors: n d esz bytes at %g GB/s, n^2 d fp64 flops at %g TFLOP/s" % (HBM_GBS, FP64_TFLOPS),
           "rows": rows}
    dst = os.path.join(ROOT, sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "pca_wide_bench.json"))
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
