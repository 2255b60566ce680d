"""Nmf with the Kullback-Leibler loss on dense data (include/petal_hip_nmf_kl_dense.h): time per iteration of `fit` (tol = 0, custom
initialisation) through dense_path="fused" (k_nmf_kl_pass) and through the compressed route (the CSR of the whole matrix, k_nmf_kl_sweep)
on the same fully dense float32 device-resident matrix, d = 512, n = 100000 and 1000000, k = 16 and 64, beside the same updates written
in torch in float64 (X widened once, outside the timed window) and in float32, the stream time of k_nmf_kl_pass by itself (the launches
under TAG_POW with profiling on: stats pow_ms) and its two floors -- n dp 4 bytes at 6 TB/s and 4 n dp kp fp64 multiply-adds at the
matrix fp64 peak -- and `transform` at 20 and 200 updates on both routes.  Writes profiles/nmf_kl_dense_bench.json: medians of five
alternating calls after two warm-up calls, wall time around the calls, each window ending in a device synchronise.  Time per iteration
= (a fit of 21 iterations - a fit of 1 iteration) / 20, so that the ingest, the scan and the loss passes cancel.

The compressed route is timed on a CsrMatrix built once, outside the timed window (the Python facade's dense_path="compress" would
compress on the host inside every call); above COMPRESS_MAX_NNZ stored entries its two resident images and their construction do not fit
this script's time budget and the entries say "unmeasured"."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import petal_decomposition_amd as petal  # noqa: E402

FP64_TFLOPS = 78.6    # MI355X matrix fp64 peak
HBM_TBS = 6.0
SHAPES = [(100000, 512, 16), (100000, 512, 64), (1000000, 512, 16), (1000000, 512, 64)]
ITERS = 20
EPS = 2.0 ** -23
KL = "kullback-leibler"
COMPRESS_MAX_NNZ = 1 << 27
UNMEASURED = "unmeasured"


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
        den = h.sum(dim=1)
        den[den == 0] = EPS
        w = w * (((x / (w @ h).clamp_min_(EPS)) @ h.T) / den)
        den = w.sum(dim=0)
        den[den == 0] = EPS
        h = h * ((w.T @ (x / (w @ h).clamp_min_(EPS))) / den[:, None])
    return w, h


def torch_transform(x, h, k, iters):
    h = h.to(x.dtype)
    w = torch.full((x.shape[0], k), float((x.mean() / k).sqrt()), dtype=x.dtype, device="cuda")
    den = h.sum(dim=1)
    den[den == 0] = EPS
    for _ in range(iters):
        w = w * (((x / (w @ h).clamp_min_(EPS)) @ h.T) / den)
    return w


def whole_csr(x, ctx):
    """the CSR of every entry of a dense device matrix (fully dense data: every entry is stored)"""
    n, d = x.shape
    indptr = np.arange(n + 1, dtype=np.int64) * d
    indices = np.tile(np.arange(d, dtype=np.int32), n)
    return petal.CsrMatrix(x.cpu().numpy().reshape(-1), indices, indptr, (n, d), ctx=ctx)


def main():
    ctx = petal.Context(0)
    out = {"device": torch.cuda.get_device_name(0),
           "note": "wall time around the calls, each window ending in a device synchronise; device-resident fully dense float32 input; "
                   "medians of five alternating calls after two warm-up calls; per iteration = (fit of %d iterations - fit of 1) / %d; "
                   "fused: dense_path='fused'; compress: the same fit on the CsrMatrix of every entry, built once outside the window "
                   "(the facade's dense_path='compress' also compresses on the host inside every call: not timed here); torch: the same "
                   "updates in float64 (X widened once, outside the window) and in float32; k_nmf_kl_pass: stream time between events "
                   "around the kernel's launches (profiling level 2), (a fit of %d - a fit of 1) / %d; floors: n dp 4 bytes at %g TB/s, "
                   "4 n dp kp fp64 multiply-adds at %g TFLOP/s; 'unmeasured': more than %d stored entries on the compressed route"
                   % (ITERS + 1, ITERS, ITERS + 1, ITERS, HBM_TBS, FP64_TFLOPS, COMPRESS_MAX_NNZ),
           "rows": []}
    dst = os.path.join(ROOT, sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "nmf_kl_dense_bench.json"))

    def save():
        with open(dst, "w") as f:
            json.dump(out, f, indent=1)

    for n, d, k in SHAPES:
        x, w0, h0 = data(n, d, k, n + d + k)
        assert float(x.min()) > 0.0
        x64 = x.double()
        kp = 16 if k <= 16 else (32 if k <= 32 else 64)
        sx = whole_csr(x, ctx) if n * d <= COMPRESS_MAX_NNZ else None

        def fit(iters, xin=x, path="fused"):
            return petal.Nmf(k, max_iter=iters, tol=0.0, init="custom", ctx=ctx, beta_loss=KL, dense_path=path).fit(xin, W=w0, H=h0)
        fns = [lambda: fit(ITERS + 1), lambda: fit(1), lambda: torch_fit(x64, w0, h0, ITERS), lambda: torch_fit(x, w0, h0, ITERS)]
        if sx is not None:
            fns += [lambda: fit(ITERS + 1, sx), lambda: fit(1, sx)]
        med = alternate(fns)
        row = {"n": n, "d": d, "k": k, "fused_fit_per_iteration_ms": (med[0] - med[1]) / ITERS, "fused_fit_21_ms": med[0], "fused_fit_1_ms": med[1],
               "torch_fp64_per_iteration_ms": med[2] / ITERS, "torch_fp32_per_iteration_ms": med[3] / ITERS,
               "compress_fit_per_iteration_ms": (med[4] - med[5]) / ITERS if sx is not None else UNMEASURED}
        ctx.set_profiling(2)
        pow_ms = []
        for iters in (ITERS + 1, 1):
            m = fit(iters)
            assert m.kernel_path == 1
            pow_ms.append(ctx.stats()["pow_ms"])
            m.close()
        ctx.set_profiling(0)
        row["k_nmf_kl_pass_per_iteration_ms"] = (pow_ms[0] - pow_ms[1]) / ITERS
        row["floor_hbm_ms"] = n * d * 4 / (HBM_TBS * 1e12) * 1e3
        row["floor_fp64_mfma_ms"] = 4.0 * n * d * kp * 2.0 / (FP64_TFLOPS * 1e12) * 1e3
        row["fraction_of_floor"] = max(row["floor_hbm_ms"], row["floor_fp64_mfma_ms"]) / row["k_nmf_kl_pass_per_iteration_ms"]
        for updates in (20, 200):
            model = fit(updates)
            hc = torch.from_numpy(model.components).cuda()
            fns = [lambda: model.transform(x), lambda: torch_transform(x64, hc, k, updates)]
            if sx is not None:
                fns.append(lambda: model.transform(sx))
            tmed = alternate(fns)
            assert model.info()["transform_kernel"] == 1 or sx is not None
            row[f"fused_transform_{updates}_updates_ms"] = tmed[0]
            row[f"torch_fp64_transform_{updates}_updates_ms"] = tmed[1]
            row[f"compress_transform_{updates}_updates_ms"] = tmed[2] if sx is not None else UNMEASURED
            model.close()
        print(json.dumps(row), flush=True)
        out["rows"].append(row)
        save()
        if sx is not None:
            sx.close()
        del x, x64, w0, h0
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
