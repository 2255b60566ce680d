"""Nmf with the coordinate-descent solver (include/petal_hip_nmf_cd.h) beside the multiplicative-update solver, dev/nmf_bench.py's
protocol: time per iteration of `fit` (tol = 0, custom initialisation) and `transform` (20 updates) at 100000 x 512 and 1000000 x 512
with k = 16 and 64, float32 device-resident input, solver="cd" and solver="mu" alternating in the same process; the stream time of
k_nmf_cd_pass and of k_nmf_pass by themselves (the launches under TAG_POW with profiling level 2: stats pow_ms over pow_launches); and a
quality line at the two smaller shapes: from the same custom start, the first number of coordinate-descent iterations whose
reconstruction_err is below the one the multiplicative updates report after 200 iterations, and the wall time of that fit.  Writes
profiles/nmf_cd_bench.json: medians of five alternating calls after two warm-up calls, wall time around the calls, each window ending
in a device synchronise.  Time per iteration = (a fit of 21 iterations - a fit of 1 iteration) / 20.  The per-iteration read-back of
the violation that tol > 0 adds is not measured here."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import petal_decomposition_amd as petal  # noqa: E402

SHAPES = [(100000, 512, 16), (100000, 512, 64), (1000000, 512, 16), (1000000, 512, 64)]
QUALITY_ROWS = 100000
ITERS = 20
MU_ITERS = 200


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


def main():
    ctx = petal.Context(0)
    out = {"device": torch.cuda.get_device_name(0),
           "note": "wall time around the calls, each window ending in a device synchronise; device-resident float32 input; medians of five "
                   "alternating calls after two warm-up calls, solver cd and solver mu alternating in one process; per iteration = (fit of "
                   "%d iterations - fit of 1) / %d at tol = 0; pass alone: stream time between events around the kernel's launches "
                   "(profiling level 2), mean over the launches of one fit; quality: the first number of cd iterations (bisection, the loss "
                   "decreases with the iterations) whose reconstruction_err is below mu's after %d iterations from the same start, and the "
                   "wall time of that cd fit; null where 200 cd iterations do not reach it; the read-back of tol > 0 is unmeasured"
                   % (ITERS + 1, ITERS, MU_ITERS),
           "rows": []}
    dst = os.path.join(ROOT, sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "nmf_cd_bench.json"))

    def save():
        with open(dst, "w") as f:
            json.dump(out, f, indent=1)

    for n, d, k in SHAPES:
        x, w0, h0 = data(n, d, k, n + d + k)

        def fit(solver, iters):
            return petal.Nmf(k, max_iter=iters, tol=0.0, init="custom", ctx=ctx, solver=solver).fit(x, W=w0, H=h0)
        med = alternate([lambda: fit("cd", ITERS + 1), lambda: fit("cd", 1), lambda: fit("mu", ITERS + 1), lambda: fit("mu", 1)])
        cd, mu = fit("cd", ITERS), fit("mu", ITERS)
        assert cd.info()["fit_kernel"] == 1 and mu.info()["fit_kernel"] == 1
        tmed = alternate([lambda: cd.transform(x), lambda: mu.transform(x)])
        assert cd.info()["transform_kernel"] == 1 and mu.info()["transform_kernel"] == 1
        alone = {}
        ctx.set_profiling(2)
        for solver in ("cd", "mu"):
            fit(solver, ITERS)
            st = ctx.stats()
            alone[solver] = st["pow_ms"] / st["pow_launches"]
        ctx.set_profiling(0)
        row = {"n": n, "d": d, "k": k, "cd_fit_per_iteration_ms": (med[0] - med[1]) / ITERS, "mu_fit_per_iteration_ms": (med[2] - med[3]) / ITERS,
               "cd_fit_21_ms": med[0], "cd_fit_1_ms": med[1], "mu_fit_21_ms": med[2], "mu_fit_1_ms": med[3],
               "cd_transform_20_updates_ms": tmed[0], "mu_transform_20_updates_ms": tmed[1],
               "k_nmf_cd_pass_ms": alone["cd"], "k_nmf_pass_ms": alone["mu"], "pass_alone_cd_over_mu": alone["cd"] / alone["mu"]}
        if n == QUALITY_ROWS:
            t_mu = timed(lambda: fit("mu", MU_ITERS))
            target = fit("mu", MU_ITERS).reconstruction_err
            lo, hi = 0, MU_ITERS            # the loss after lo iterations is above the target (0: the start), after hi below -- if at all
            if fit("cd", hi).reconstruction_err >= target:
                hi = None
            while hi is not None and hi - lo > 1:
                mid = (lo + hi) // 2
                if fit("cd", mid).reconstruction_err < target:
                    hi = mid
                else:
                    lo = mid
            row.update({"mu_200_iterations_err": target, "mu_200_iterations_ms": t_mu, "cd_iterations_to_mu_200_err": hi,
                        "cd_ms_to_mu_200_err": timed(lambda: fit("cd", hi)) if hi is not None else None,
                        "cd_err_there": fit("cd", hi).reconstruction_err if hi is not None else fit("cd", MU_ITERS).reconstruction_err})
        print(json.dumps(row), flush=True)
        out["rows"].append(row)
        save()
        cd.close()
        mu.close()
        del x, w0, h0
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
