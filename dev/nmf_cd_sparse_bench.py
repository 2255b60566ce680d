"""Nmf with the coordinate-descent solver on sparse CSR data (include/petal_hip_nmf_cd_sparse.h) beside the multiplicative-update
solver on the same resident handle, dev/nmf_cd_bench.py's protocol: time per iteration of `fit` (tol = 0, custom initialisation) and
`transform` (20 updates) at 1000000 x 512 (1 % and 5 % stored) and 200000 x 20000 (0.2 % and 1 %), each with k = 16 and 64, float32
values, solver="cd" (sparse_path="sweep") and solver="mu" alternating in the same process; the stream time of one sweep launch of
k_nmf_cd_sweep and of k_nmf_sweep (the launches under TAG_POW with profiling level 2: stats pow_ms over pow_launches); at
1000000 x 512 the dense solver="cd" (k_nmf_cd_pass) on the densified matrix; and a quality line at 1000000 x 512, 1 %: from the same
custom start, the first number of coordinate-descent iterations whose reconstruction_err is below the one the multiplicative updates
report after 200 iterations, and the wall time of that fit.  Writes profiles/nmf_cd_sparse_bench.json after every row: medians of five
alternating calls after two warm-up calls, wall time around the calls, each window ending in a device synchronise.  Time per iteration
= (a fit of 21 iterations - a fit of 1 iteration) / 20.  The per-iteration read-back of the violation that tol > 0 adds is not measured
here.  `--rows a,b,...` runs a subset of CONFIGS (their indices), `--no-quality` leaves the quality line out."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import petal_decomposition_amd as petal  # noqa: E402

# (rows, columns, stored share, k), the cheaper shapes first
CONFIGS = [(1000000, 512, 0.01, 16), (1000000, 512, 0.01, 64), (1000000, 512, 0.05, 16), (1000000, 512, 0.05, 64),
           (200000, 20000, 0.002, 16), (200000, 20000, 0.002, 64), (200000, 20000, 0.01, 16), (200000, 20000, 0.01, 64)]
DENSE_COLS = 512                 # the dense solver is measured where the densified matrix is small enough (2 GB as float32)
QUALITY = (1000000, 512, 0.01)
ITERS = 20
MU_ITERS = 200


def data(n, d, share, k, seed):
    """(data, indices, indptr) float32 / int32 / int64 with d * share stored entries in every row, columns drawn without repetition
    inside a row by a random stride walk; values: a planted product of rank k + 2 plus 1 % noise; and W0, H0 as float32"""
    rng = np.random.default_rng(seed)
    m = max(1, int(round(d * share)))
    u, v = rng.random((n, k + 2), dtype=np.float32), rng.random((d, k + 2), dtype=np.float32)
    start = rng.integers(0, d, size=(n, 1))
    stride = d // m
    indices = ((start + stride * np.arange(m)[None, :] + rng.integers(0, stride, size=(n, m))) % d).astype(np.int32)
    values = np.empty((n, m), dtype=np.float32)
    step = max(1, (1 << 24) // (m * (k + 2)))
    for r0 in range(0, n, step):
        r1 = min(n, r0 + step)
        values[r0:r1] = np.einsum("ir,ijr->ij", u[r0:r1], v[indices[r0:r1]])
    values *= 1.0 + 0.01 * np.abs(rng.standard_normal((n, m), dtype=np.float32))
    indptr = (np.arange(n + 1, dtype=np.int64) * m)
    avg = float(np.sqrt(values.sum() / (float(n) * d) / k))
    w0 = (avg * np.abs(rng.standard_normal((n, k), dtype=np.float32)))
    h0 = (avg * np.abs(rng.standard_normal((k, d), dtype=np.float32)))
    return values.reshape(-1), indices.reshape(-1), indptr, w0, h0


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
    args = sys.argv[1:]
    which = list(range(len(CONFIGS)))
    if "--rows" in args:
        which = [int(v) for v in args[args.index("--rows") + 1].split(",")]
    quality = "--no-quality" not in args
    names = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] != "--rows")]
    dst = os.path.join(ROOT, names[0] if names else os.path.join("profiles", "nmf_cd_sparse_bench.json"))
    ctx = petal.Context(0)
    out = {"device": torch.cuda.get_device_name(0),
           "note": "wall time around the calls, each window ending in a device synchronise; float32 values on one resident CsrMatrix per "
                   "row of this table; medians of five alternating calls after two warm-up calls, solver cd (sparse_path sweep) and solver "
                   "mu alternating in one process; per iteration = (fit of %d iterations - fit of 1) / %d at tol = 0; sweep alone: stream "
                   "time between events around one sweep's launches (profiling level 2), mean over the sweeps of one fit; dense cd: "
                   "Nmf(solver='cd') on the densified device-resident matrix; quality: the first number of cd iterations (bisection) whose "
                   "reconstruction_err is below mu's after %d iterations from the same start, and the wall time of that cd fit; null "
                   "where 200 cd iterations do not reach it; a key that is absent was not measured; the read-back of tol > 0 is unmeasured"
                   % (ITERS + 1, ITERS, MU_ITERS),
           "rows": []}
    if os.path.exists(dst) and "--rows" in args:   # (a later call adds its rows to an earlier call's)
        with open(dst) as f:
            out["rows"] = json.load(f)["rows"]

    def save():
        with open(dst, "w") as f:
            json.dump(out, f, indent=1)

    for ci in which:
        n, d, share, k = CONFIGS[ci]
        values, indices, indptr, w0, h0 = data(n, d, share, k, n + d + k)
        sx = petal.CsrMatrix(values, indices, indptr, (n, d), ctx=ctx)

        def fit(solver, iters, x=sx):
            return petal.Nmf(k, max_iter=iters, tol=0.0, init="custom", ctx=ctx, solver=solver, sparse_path="sweep").fit(x, W=w0, H=h0)
        med = alternate([lambda: fit("cd", ITERS + 1), lambda: fit("cd", 1), lambda: fit("mu", ITERS + 1), lambda: fit("mu", 1)])
        cd, mu = fit("cd", ITERS), fit("mu", ITERS)
        assert cd.kernel_path == 1 and mu.kernel_path == 1
        tmed = alternate([lambda: cd.transform(sx), lambda: mu.transform(sx)])
        assert cd.kernel_path == 1 and mu.kernel_path == 1
        alone = {}
        ctx.set_profiling(2)
        for solver in ("cd", "mu"):
            fit(solver, ITERS)
            st = ctx.stats()
            alone[solver] = st["pow_ms"] / st["pow_launches"]
        ctx.set_profiling(0)
        row = {"n": n, "d": d, "stored_share": share, "nnz": int(values.size), "k": k,
               "cd_fit_per_iteration_ms": (med[0] - med[1]) / ITERS, "mu_fit_per_iteration_ms": (med[2] - med[3]) / ITERS,
               "cd_fit_21_ms": med[0], "cd_fit_1_ms": med[1], "mu_fit_21_ms": med[2], "mu_fit_1_ms": med[3],
               "cd_transform_20_updates_ms": tmed[0], "mu_transform_20_updates_ms": tmed[1],
               "k_nmf_cd_sweep_ms": alone["cd"], "k_nmf_sweep_ms": alone["mu"], "sweep_alone_cd_over_mu": alone["cd"] / alone["mu"],
               "final_err_cd_20": cd.reconstruction_err, "final_err_mu_20": mu.reconstruction_err}
        if d == DENSE_COLS:
            rows = torch.from_numpy(np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))).cuda()
            xd = torch.zeros((n, d), dtype=torch.float32, device="cuda")
            xd.index_put_((rows, torch.from_numpy(indices.astype(np.int64)).cuda()), torch.from_numpy(values).cuda(), accumulate=True)
            del rows
            w0d, h0d = torch.from_numpy(w0).cuda(), torch.from_numpy(h0).cuda()

            def fit_dense(iters):
                return petal.Nmf(k, max_iter=iters, tol=0.0, init="custom", ctx=ctx, solver="cd").fit(xd, W=w0d, H=h0d)
            dmed = alternate([lambda: fit_dense(ITERS + 1), lambda: fit_dense(1)])
            assert fit_dense(1).info()["fit_kernel"] == 1
            row.update({"dense_cd_fit_per_iteration_ms": (dmed[0] - dmed[1]) / ITERS, "dense_cd_fit_21_ms": dmed[0], "dense_cd_fit_1_ms": dmed[1]})
            del xd, w0d, h0d
            torch.cuda.empty_cache()
        if quality and (n, d, share) == QUALITY:
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
        out["rows"] = [r for r in out["rows"] if (r["n"], r["d"], r["stored_share"], r["k"]) != (n, d, share, k)] + [row]
        save()
        cd.close()
        mu.close()
        sx.close()
    ctx.close()


if __name__ == "__main__":
    main()
