"""Times petal_pca_fit_segments (SegmentedPca.fit) on B equal segments resident in HBM against the Python loop over Pca.fit on the same
slices: same process, same tree, alternating runs, wall time of the whole call (results land in host arrays, so every call ends
synchronised).  Writes profiles/segments_bench.json unless --out says otherwise.
usage: python dev/segments_bench.py [--calls 7] [--loop-calls 3] [--out FILE.json] [--quick]"""
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
ap.add_argument("--calls", type=int, default=7)
ap.add_argument("--loop-calls", type=int, default=3)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--quick", action="store_true", help="B <= 1024 only")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "segments_bench.json"))
a = ap.parse_args()

HBM_BYTES_PER_S = 8e12
CONFIGS = [(1, 1000, 16, 4, torch.float64), (64, 1000, 16, 4, torch.float64), (1024, 1000, 16, 4, torch.float64),
           (8192, 1000, 16, 4, torch.float64), (4096, 256, 64, 8, torch.float32)]
if a.quick:
    CONFIGS = [c for c in CONFIGS if c[0] <= 1024]

ctx = petal.Context(0)
g = torch.Generator(device="cuda")
g.manual_seed(1)
rows_out = []
for B, n, d, k, dt in CONFIGS:
    x = torch.randn((B * n, d), generator=g, device="cuda", dtype=dt) * torch.linspace(3.0, 0.3, d, device="cuda", dtype=dt) + 0.5
    off = np.arange(B + 1, dtype=np.int64) * n
    seg = petal.SegmentedPca(k, ctx=ctx)
    one = petal.Pca(k, ctx=ctx)

    def batched():
        seg.fit(x, off)
        return seg.singular_values

    def looped():
        out = np.empty((B, k), dtype=seg.singular_values.dtype if seg.singular_values.size else np.float64)
        for b in range(B):
            one.fit(x[b * n:(b + 1) * n])
            out[b] = one.singular_values()
        return out

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t0) * 1e3, r

    tb, tl, sb, sl = [], [], None, None
    rounds = a.warmup + a.calls
    for it in range(rounds):              # alternating: the loop takes its turn in the first `loop_calls` timed rounds
        t, sb = wall(batched)
        if it >= a.warmup:
            tb.append(t)
        if it < a.warmup + a.loop_calls:
            t, sl = wall(looped)
            if it >= a.warmup:
                tl.append(t)
    assert seg.kernel_segments == B, seg.kernel_segments
    agree = float(np.abs(sb.astype(np.float64) - sl).max() / np.abs(sl).max())
    mb, ml = float(np.median(tb)), float(np.median(tl))
    xbytes = B * n * d * x.element_size()
    row = {"segments": B, "rows_per_segment": n, "d": d, "k": k, "dtype": str(dt).replace("torch.", ""),
           "batched_ms": {"median": mb, "min": float(min(tb)), "max": float(max(tb)), "calls": len(tb)},
           "loop_ms": {"median": ml, "min": float(min(tl)), "max": float(max(tl)), "calls": len(tl)},
           "segments_per_s": B / (mb * 1e-3), "loop_over_batched": ml / mb, "x_bytes": xbytes,
           "fraction_of_8TBps": xbytes / (mb * 1e-3) / HBM_BYTES_PER_S, "max_sigma_difference_rel": agree,
           "per_phase_share": None}
    print(json.dumps(row))
    rows_out.append(row)
    del x
res = {"box": platform.node(), "device": torch.cuda.get_device_name(0), "note": "wall time of the whole call, device-resident X; "
       "per_phase_share is not measured: the phases are inside one kernel", "results": rows_out}
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
ctx.close()
