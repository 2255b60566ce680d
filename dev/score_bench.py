"""Times petal_score_rows against petal_transform writing in place into a device matrix, and the composition the scores replace
(transform + inverse_transform + a subtract-square-reduce in torch).  Same process, alternating calls, warm clocks; each call is
bracketed by a pair of events on the stream the ctx launches on, so a figure is the whole call's device time (operand upload, operand
pack, the product kernel).
usage: python dev/score_bench.py [--rows 1000000] [--d 512] [--k 64] [--calls 30] [--gemm bf16x3|fp32] [--out FILE.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import petal_decomposition_amd as petal

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1000000)
ap.add_argument("--d", type=int, default=512)
ap.add_argument("--k", type=int, default=64)
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--gemm", default="bf16x3")
ap.add_argument("--out", default=None)
a = ap.parse_args()

stream = torch.cuda.current_stream()
ctx = petal.Context(0, stream=stream.cuda_stream)
ctx.set_gemm_mode(a.gemm)
g = torch.Generator(device="cuda")
g.manual_seed(1)
x = torch.randn((a.rows, a.d), generator=g, device="cuda") * 2 + 0.5
rng = np.random.default_rng(7)
comp = np.linalg.qr(rng.standard_normal((a.d, a.k)))[0].T.astype(np.float32)
mu = x[:4096].mean(0).cpu().numpy().astype(np.float32)
w = (1.0 / np.linspace(4.0, 1.0, a.k)).astype(np.float32)
m = petal.Pca(a.k, ctx=ctx)
m._store(comp, mu, np.ones(a.k, dtype=np.float32), np.ones(1, dtype=np.float32), a.rows)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    r = fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), r


def composition():
    xr = m.inverse_transform(m.transform(x))
    return ((x - xr) ** 2).sum(dim=1)


runs = {"score_rows": lambda: petal.score_rows(x, comp, mu, weights=w, ctx=ctx)[0], "transform": lambda: m.transform(x), "composition": composition}
ms = {k: [] for k in runs}
for it in range(a.warmup + a.calls):
    for name, fn in runs.items():       # alternating: each round runs every variant once
        t, r = timed(fn)
        if it >= a.warmup:
            ms[name].append(t)
        del r
res = {"rows": a.rows, "d": a.d, "k": a.k, "dtype": "float32", "gemm": a.gemm, "calls": a.calls}
for name, v in ms.items():
    v = np.asarray(v)
    res[name + "_ms"] = {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}
res["score_over_transform_median"] = res["score_rows_ms"]["median"] / res["transform_ms"]["median"]
res["composition_over_score_median"] = res["composition_ms"]["median"] / res["score_rows_ms"]["median"]
# what came out agrees with the composition it replaces (float32 cancellation floor: a few eps q)
sc = petal.score_rows(x[:4096], comp, mu, ctx=ctx)[0][:, 0]
xc = x[:4096].double() - torch.from_numpy(mu).cuda().double()
v = torch.from_numpy(comp).cuda().double()
want = (xc * xc).sum(1) - ((xc @ v.T) ** 2).sum(1)
res["max_residual_error_over_q"] = float(((sc.double() - want).abs() / (xc * xc).sum(1)).max())
print(json.dumps(res))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
ctx.close()
