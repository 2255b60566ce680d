"""Nmf (include/petal_hip_nmf.h): time per iteration of `fit` (tol = 0, custom initialisation) and `transform` (20 updates) at
100000 x 512 and 1000000 x 512 with k = 16 and 64, float32 device-resident input, beside the composed path (nmf_fallback = 1), the same
updates written in torch on the same GPU in float64 (X widened once, outside the timed window) and in float32, and the stream time of
k_nmf_pass by itself (the launches under TAG_POW with profiling on: stats pow_ms) beside its two floors -- n d esz + 16 n k bytes at
6 TB/s and 2 n d k + 2 n k^2 fp64 multiply-adds at the matrix fp64 peak.  Writes profiles/nmf_bench.json: medians of five alternating
calls after two warm-up calls, wall time around the calls, each window ending in a device synchronise.  Time per iteration = (a fit of
21 iterations - a fit of 1 iteration) / 20, so that the ingest, the scan and the start-up pass cancel.  The composed path is timed from
single calls of 3 and 1 iterations: it moves W through the host every iteration."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import petal_decomposition_amd as petal  # noqa: E402

FP64_TFLOPS = 78.6    # MI355X matrix fp64 peak
HBM_TBS = 6.0
SHAPES = [(100000, 512, 16), (100000, 512, 64), (1000000, 512, 16), (1000000, 512, 64)]
ITERS = 20
EPS = 2.0 ** -23


def data(n, d, k, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.rand((n, k + 2), generator=g, device="cuda") @ torch.rand((k + 2, d), generator=g, device="cuda")
    x += 0.01 * x.mean() * torch.randn((n, d), generator=g, device="cuda").abs()
    avg = float((x.mean() / k).sqrt())
    w0 = avg * torch.randn((n, k), generator=g, device="cuda").abs()
    h0 = avg * torch.randn((k, d), generator=g, device="cuda").abs()
    return x.contiguous(), w0.contiguous(), h0.contiguous()


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


def torch_fit(x, w0, h0, iters):
    """the same updates in torch, in x's dtype"""
    w, h = w0.to(x.dtype).clone(), h0.to(x.dtype).clone()
    for _ in range(iters):
        den = w @ (h @ h.T)
        den[den == 0] = EPS
        w = w * ((x @ h.T) / den)
        den = (w.T @ w) @ h
        den[den == 0] = EPS
        h = h * ((w.T @ x) / den)
    return w, h


def torch_transform(x, h, k, iters):
    h = h.to(x.dtype)
    w = torch.full((x.shape[0], k), float((x.mean() / k).sqrt()), dtype=x.dtype, device="cuda")
    z, hht = x @ h.T, h @ h.T
    for _ in range(iters):
        den = w @ hht
        den[den == 0] = EPS
        w = w * (z / den)
    return w


def main():
    ctx = petal.Context(0)
    out = {"device": torch.cuda.get_device_name(0),
           "note": "wall time around the calls, each window ending in a device synchronise; device-resident float32 input; medians of five "
                   "alternating calls after two warm-up calls; per iteration = (fit of %d iterations - fit of 1) / %d; composed: "
                   "nmf_fallback = 1, single calls of 3 and 1 iterations; torch: the same updates in float64 (X widened once, outside the "
                   "window) and in float32; k_nmf_pass: stream time between events around the kernel's launches (profiling level 2), mean "
                   "over the launches of one fit; floors: n d esz + 16 n k bytes at %g TB/s, 2 n d k + 2 n k^2 fp64 multiply-adds at %g "
                   "TFLOP/s" % (ITERS + 1, ITERS, HBM_TBS, FP64_TFLOPS),
           "rows": []}
    dst = os.path.join(ROOT, sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "nmf_bench.json"))

    def save():
        with open(dst, "w") as f:
            json.dump(out, f, indent=1)

    for n, d, k in SHAPES:
        x, w0, h0 = data(n, d, k, n + d + k)
        x64 = x.double()

        def fit(iters):
            return petal.Nmf(k, max_iter=iters, tol=0.0, init="custom", ctx=ctx).fit(x, W=w0, H=h0)
        med = alternate([lambda: fit(ITERS + 1), lambda: fit(1), lambda: torch_fit(x64, w0, h0, ITERS), lambda: torch_fit(x, w0, h0, ITERS)])
        model = fit(ITERS)
        assert model.info()["fit_kernel"] == 1
        tmed = alternate([lambda: model.transform(x), lambda: torch_transform(x64, torch.from_numpy(model.components).cuda(), k, ITERS),
                          lambda: torch_transform(x, torch.from_numpy(model.components).cuda(), k, ITERS)])
        assert model.info()["transform_kernel"] == 1
        ctx.set_profiling(2)
        fit(ITERS)
        st = ctx.stats()
        kms = st["pow_ms"] / st["pow_launches"]
        model.transform(x)
        st2 = ctx.stats()
        ctx.set_profiling(0)
        ctx.set_option("nmf_fallback", 1)
        try:
            fit(1)
            c3, c1 = timed(lambda: fit(3)), timed(lambda: fit(1))
        finally:
            ctx.set_option("nmf_fallback", 0)
        floor_hbm = (n * d * 4 + 16 * n * k) / (HBM_TBS * 1e12) * 1e3
        floor_mfma = (2.0 * n * d * k + 2.0 * n * k * k) * 2.0 / (FP64_TFLOPS * 1e12) * 1e3
        row = {"n": n, "d": d, "k": k, "fit_per_iteration_ms": (med[0] - med[1]) / ITERS, "fit_21_ms": med[0], "fit_1_ms": med[1],
               "composed_per_iteration_ms": (c3 - c1) / 2.0, "torch_fp64_per_iteration_ms": med[2] / ITERS,
               "torch_fp32_per_iteration_ms": med[3] / ITERS, "transform_20_updates_ms": tmed[0], "torch_fp64_transform_ms": tmed[1],
               "torch_fp32_transform_ms": tmed[2], "k_nmf_pass_ms": kms, "k_nmf_pass_launches": st["pow_launches"],
               "k_nmf_pass_transform_ms": st2["pow_ms"], "floor_hbm_ms": floor_hbm, "floor_fp64_mfma_ms": floor_mfma,
               "fraction_of_floor": max(floor_hbm, floor_mfma) / kms}
        print(json.dumps(row), flush=True)
        out["rows"].append(row)
        save()
        model.close()
        del x, x64, w0, h0
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
