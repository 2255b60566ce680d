"""KernelPca (include/petal_hip_kpca.h): `fit` at n = 2048, 4096, 8192 with d = 64 and 512 (float32, rbf, k = 16); `transform` of m = 1e5 and
1e6 rows of width 64 against n = 2048 and 4096; k_kapply by itself (the launch under TAG_XP with profiling on: stats xp_ms) beside its
floor of m n (d + k + 1) fp64 multiply-adds at the matrix fp64 peak; and the same transform written in torch on the same GPU in float64
(matmul, exp, matmul), row-blocked to fit memory -- what a user would otherwise write.  Writes profiles/kpca_bench.json: medians of
five alternating calls after two warm-up calls, wall time around the calls, each window ending in a device synchronise; device-resident
input.  A fit whose first call takes longer than SLOW_S is recorded from that one call, and the larger n of the same width are not run."""
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
K = 16
FIT_N = (2048, 4096, 8192)
FIT_D = (64, 512)
TRANSFORM = [(100000, 2048), (100000, 4096), (1000000, 2048), (1000000, 4096)]
TRANSFORM_D = 64
SLOW_S = 15.0
TORCH_BLOCK = 8192


def data(n, d, seed):
    """planted rows in the manner of tests/kpca_cases.py: 2 k graded directions, small noise, a sign pattern 5 off zero"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    s = 3.0 * 0.85 ** torch.arange(2 * K, device="cuda", dtype=torch.float64)
    q, _ = torch.linalg.qr(torch.randn((d, 2 * K), generator=g, device="cuda", dtype=torch.float64))
    x = (torch.randn((n, 2 * K), generator=g, device="cuda", dtype=torch.float64) * s) @ q.T
    x += 0.05 * torch.randn((n, d), generator=g, device="cuda", dtype=torch.float64)
    x += 5.0 * torch.sign(torch.randn(d, generator=g, device="cuda", dtype=torch.float64))
    return x.to(torch.float32).contiguous()


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


def torch_transform(xq, xt, c, a, gamma):
    """phi(Xq Xt^T) A' in float64 torch, row-blocked: matmul, exp, matmul"""
    t = xt.double() - c
    nt = (t * t).sum(dim=1)
    out = torch.empty((xq.shape[0], a.shape[1]), dtype=torch.float64, device="cuda")
    for r0 in range(0, xq.shape[0], TORCH_BLOCK):
        q = xq[r0:r0 + TORCH_BLOCK].double() - c
        d2 = (q * q).sum(dim=1)[:, None] + nt[None, :] - 2.0 * (q @ t.T)
        out[r0:r0 + TORCH_BLOCK] = torch.exp(-gamma * d2.clamp_(min=0.0)) @ a
    return out


def main():
    ctx = petal.Context(0)
    out = {"device": torch.cuda.get_device_name(0),
           "note": "wall time around the calls, each window ending in a device synchronise; device-resident float32 input; medians of five "
                   "alternating calls after two warm-up calls; rbf, gamma = 1 / d, k = %d; k_kapply: stream time between events around the "
                   "kernel's launch (profiling level 2, median of five transforms after two); floor: m n (d + k + 1) fp64 multiply-adds "
                   "at %g TFLOP/s; torch: the same phi(Xq Xt^T) A' in float64 torch (matmul, exp, matmul) in blocks of %d rows"
                   % (K, FP64_TFLOPS, TORCH_BLOCK),
           "fit": [], "transform": []}
    dst = os.path.join(ROOT, sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "kpca_bench.json"))

    def save():
        with open(dst, "w") as f:
            json.dump(out, f, indent=1)

    d = TRANSFORM_D
    for m, n in TRANSFORM:
        xt, xq = data(n, d, n + d), data(m, d, m + n + d)
        model = petal.KernelPca(K, "rbf", ctx=ctx).fit(xt)
        c = xt.double().mean(dim=0)
        a = torch.cat([torch.from_numpy(model.scaled_eigenvectors()).cuda(), torch.ones((n, 1), dtype=torch.float64, device="cuda")], dim=1)
        med = alternate([lambda: model.transform(xq), lambda: torch_transform(xq, xt, c, a, 1.0 / d)])
        assert model.info()["transform_kernel"] == 1
        ctx.set_profiling(2)
        kern = []
        for i in range(7):
            model.transform(xq)
            st = ctx.stats()
            assert st["xp_launches"] == 1, st
            if i >= 2:
                kern.append(st["xp_ms"])
        ctx.set_profiling(0)
        floor = m * n * (d + K + 1) * 2.0 / (FP64_TFLOPS * 1e12) * 1e3
        kms = statistics.median(kern)
        row = {"m": m, "n": n, "d": d, "k": K, "transform_ms": med[0], "torch_fp64_ms": med[1], "k_kapply_ms": kms, "floor_fp64_mfma_ms": floor,
               "fraction_of_floor": floor / kms}
        print(json.dumps(row), flush=True)
        out["transform"].append(row)
        save()
        model.close()
        del xt, xq, a
    for d in FIT_D:
        slow = False
        for n in FIT_N:
            if slow:
                row = {"n": n, "d": d, "fit_ms": None, "note": "not run: the next smaller n of this width already took longer than %g s" % SLOW_S}
            else:
                x = data(n, d, n + d)
                first = timed(lambda: petal.KernelPca(K, "rbf", ctx=ctx).fit(x))
                if first > SLOW_S * 1e3:
                    slow = True
                    row = {"n": n, "d": d, "fit_ms": first, "note": "one call (the first, allocations included): not repeated"}
                else:
                    row = {"n": n, "d": d, "fit_ms": alternate([lambda: petal.KernelPca(K, "rbf", ctx=ctx).fit(x)])[0], "first_call_ms": first,
                           "topk_solver": petal.KernelPca(K, "rbf", ctx=ctx).fit(x).info()["topk_solver"]}
                del x
            print(json.dumps(row), flush=True)
            out["fit"].append(row)
            save()

    ctx.close()


if __name__ == "__main__":
    main()
