"""bench.py's output contract: stdout carries exactly one line, the JSON record, with the keys the driver reads and the
`roofline` / `cpu_baseline` objects; the sharded code path (one-rank process group, built-in RCCL after the child-process
probe) prints the same record."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQUIRED = ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config", "roofline"]
# what only `--full` measures (runs of its own beside the timed steps)
FULL_ONLY = ["cpu_baseline", "serial_chain", "predicted_scaling", "host_in", "x_padded_pitch", "fp32_mfma_mode", "exact_mode", "redo_case",
             "northstar_gemm", "northstar_fit", "fastica_cfg3", "pca_cfg1", "one_gpu_same_matrix"]


def _run(*extra, launcher_env=True, n_gpus=1, steps=3):
    env = dict(os.environ)
    if launcher_env:
        env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29577", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    else:  # as the driver runs it at N = 1 / as a user runs `python bench.py --gpus N`: no launcher variables at all
        for key in ("MASTER_ADDR", "MASTER_PORT", "RANK", "WORLD_SIZE", "LOCAL_RANK"):
            env.pop(key, None)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps), "--warmup", "1", "--no-northstar", *extra],
                         capture_output=True, text=True, timeout=420, env=env, cwd=ROOT)   # (a run takes 10 - 60 s)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.split("\n") if ln.strip()]
    assert len(lines) == 1, f"stdout must be the JSON line only, got {len(lines)} lines: {res.stdout[:500]}"
    rec = json.loads(lines[0])
    for key in REQUIRED:
        assert key in rec, key
    assert rec["steps"] == steps and rec["warmup"] == 1 and rec["n_gpus"] == n_gpus
    assert rec["value"] > 0 and rec["higher_is_better"] is True and rec["vs_baseline"] is None
    assert set(["bound", "achieved", "peak", "unit", "frac", "traffic"]) <= set(rec["roofline"])
    assert abs(rec["roofline"]["frac"] - rec["roofline"]["achieved"] / rec["roofline"]["peak"]) < 1e-3
    assert "workload" in rec["config"]
    return rec


def test_clock_ramp_follows_rank_zero():
    """bench.py's untimed clock ramp repeats sharded fits for a quarter of a second: on each rank's OWN clock two ranks can disagree about
    the number of fits by one, and then one waits in a fit's all-reduce while the other waits in the barrier behind the loop (a hung
    `--gpus N` job; round 6).  The decision is rank 0's, broadcast before every repetition: a rank whose own clock says "go on" for
    ever stops when the broadcast says stop, and one whose clock says "stop" at once goes on while the broadcast says go."""
    sys.path.insert(0, ROOT)
    import bench
    import torch

    class FakeDist:                     # the broadcast delivers rank 0's decisions: go, go, go, stop
        def __init__(self):
            self.decisions = [1, 1, 1, 0]
        def broadcast(self, flag, src=0):
            assert src == 0
            flag[0] = self.decisions.pop(0)

    for seconds in (3600.0, 0.0):       # this rank's own clock: never done / done before it starts
        calls = []
        bench.ramp(lambda: calls.append(1), seconds, FakeDist(), torch, "cpu")
        assert len(calls) == 3, (seconds, len(calls))
    calls = []
    bench.ramp(lambda: calls.append(1), 0.0)     # no process group: the local clock decides
    assert calls == []


def test_roofline_bound_is_computed_from_the_shape():
    """bench.py picks the binding roofline per shape: at l = 74 (configs[1]) the X stream binds the split-product kernels
    ("hbm"); at l = 138 (configs[3]) the six bf16 piece products take longer than the bytes ("mfma" on the bf16 pipe:
    0.17 ms vs 0.145 ms per pass at 250000 x 1024); the fp32-MFMA mode is bound by the fp32 pipe at both."""
    sys.path.insert(0, ROOT)
    import bench
    for (n, d, l, mode, bound, pipe) in [(100000, 512, 74, "bf16x3", "hbm", "hbm"), (250000, 1024, 138, "bf16x3", "mfma", "mfma-bf16"),
                                         (1000000, 512, 74, "bf16x3", "hbm", "hbm"),
                                         (100000, 512, 74, "fp32", "mfma", "mfma-fp32"), (250000, 1024, 138, "fp32", "mfma", "mfma-fp32")]:
        flops, nbytes = 2.0 * n * d * l, 4.0 * (n * d + n * l + d * l)
        b = bench.pass_bound(flops, nbytes, mode)
        assert (b["bound"], b["pipe"]) == (bound, pipe), (n, d, l, mode, b)
        assert b["floor_s"] == max(b["times_s"].values())
    # the entry itself: cfg4's K1 at 0.42 ms is 0.40 of the bf16 pipe with SIX piece products -- and 0.34 with the FIVE it issues
    # behind a two-plane operand (round-4 verdict: the line charged six to both kernels and overstated K1)
    kinds6 = bench.kind_table(250000, 1024, 138, "bf16x3", two_plane=False)
    e = bench.roofline_entry("K1 (Z = Xc.P)", {"K1 (Z = Xc.P)": 0.42, "K2 (Y = Xc^T.Z)": 0.41}, kinds6, "bf16x3", 0.0, 250000, 1024, 138)
    assert e["bound"] == "mfma" and e["pipe"] == "mfma-bf16" and abs(e["frac"] - 0.404) < 0.002, e
    assert abs(e["frac"] - e["achieved"] / e["peak"]) < 1e-3
    kinds5 = bench.kind_table(250000, 1024, 138, "bf16x3", two_plane=True)
    e = bench.roofline_entry("K1 (Z = Xc.P)", {"K1 (Z = Xc.P)": 0.351, "K2 (Y = Xc^T.Z)": 0.40}, kinds5, "bf16x3", 0.0, 250000, 1024, 138)
    assert e["piece_products"] == 5.0 and e["pipe"] == "hbm" and abs(e["frac"] - 0.413) < 0.003, e   # five products: the X stream binds (145 us)
    assert e["other_kernel"]["K2 (Y = Xc^T.Z)"]["piece_products"] == 6.0
    kinds = bench.kind_table(100000, 512, 74, "bf16x3", two_plane=True)
    e = bench.roofline_entry("K2 (Y = Xc^T.Z)", {"K1 (Z = Xc.P)": 0.055, "K2 (Y = Xc^T.Z)": 0.0565, "K3 (Y' = Xc^T.(Xc.P), fused)": 0.0}, kinds, "bf16x3", 0.0, 100000, 512, 74)
    assert e["bound"] == "hbm" and abs(e["frac"] - 0.519) < 0.002 and "fp32_equivalent_frac_of_fp32_mfma_peak" not in e
    # the fused pass: one read of X, 5 + 6 piece products -- at l = 74 the matrix pipe binds it (33 us against 26 us of bytes)
    e = bench.roofline_entry("K3 (Y' = Xc^T.(Xc.P), fused)", {"K1 (Z = Xc.P)": 0.0, "K2 (Y = Xc^T.Z)": 0.0, "K3 (Y' = Xc^T.(Xc.P), fused)": 0.1}, kinds, "bf16x3", 0.0, 100000, 512, 74)
    assert e["bound"] == "mfma" and e["piece_products"] == 5.5 and abs(e["frac"] - 0.333) < 0.003, e
    assert e["bytes_per_launch"] == 4.0 * (100000 * 512 + 2 * 512 * 74)
    f = bench.fit_roofline(100000, 512, 74, 5, 4, "bf16x3", 1.39)
    assert f["passes"] == 6 and f["pass_pipe"] == "mfma-bf16" and 0.1 < f["frac"] < 0.35, f
    f = bench.fit_roofline(250000, 1024, 138, 7, 4, "bf16x3", 7.5)
    assert f["passes"] == 16, f


def test_default_workload_per_gpu_count():
    """N = 1: configs[1], the configuration the metric is quoted on (weak-scaling label as before).  N > 1 without --config:
    configs[3] as north_star scales it -- ONE 2000000 x 1024 matrix, k = 128, 7 power iterations (src/pca.rs:679-680), its rows
    split over the ranks: strong scaling, rows_per_gpu = 2000000 / N."""
    sys.path.insert(0, ROOT)
    import bench
    assert bench.default_config(1) == "cfg2" and bench.CONFIGS["cfg2"]["n"] == 100000 and not bench.CONFIGS["cfg2"].get("strong")
    for n_gpus in (2, 4, 8):
        name = bench.default_config(n_gpus)
        cfg = bench.CONFIGS[name]
        assert name == "cfg4s" and cfg["strong"] and (cfg["n"], cfg["d"], cfg["k"], cfg["n_iter"]) == (2000000, 1024, 128, 7)
        blocks = [bench.shard_rows(cfg["n"], n_gpus, r) for r in range(n_gpus)]
        assert blocks[0][0] == 0 and blocks[-1][1] == cfg["n"] and all(a[1] == b[0] for a, b in zip(blocks, blocks[1:]))
        assert all(e - b == cfg["n"] // n_gpus for b, e in blocks)
    assert bench.shard_rows(10, 3, 0) == (0, 4) and bench.shard_rows(10, 3, 1) == (4, 7) and bench.shard_rows(10, 3, 2) == (7, 10)
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert '"scaling": "strong" if strong else "weak"' in src and '"northstar_fit"' in src


def test_help_runs_without_a_gpu():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "--gpus" in res.stdout and "--steps" in res.stdout and "--warmup" in res.stdout


@pytest.mark.gpu
def test_single_gpu_record():
    rec = _run("--full")
    cb = rec["cpu_baseline"]
    assert set(["value", "unit", "cores", "kind", "sample"]) <= set(cb) and cb["kind"] in ("port", "reference") and cb["value"] > 0
    assert rec["config"]["collective"] == "none"


@pytest.mark.gpu
def test_sharded_path_record_one_rank_group():
    rec = _run("--single-rank-group", "--no-cpu-baseline")
    assert rec["config"]["collective"].startswith("built-in RCCL"), rec["config"]["collective"]


def test_gpus_flag_disagreeing_with_the_launcher_is_refused():
    """--gpus N must equal WORLD_SIZE when a launcher set it: never a one-GPU measurement labelled otherwise"""
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8"], capture_output=True, text=True, timeout=120, env=env)
    assert res.returncode != 0 and res.stdout.strip() == "" and "WORLD_SIZE" in res.stderr


def test_self_launch_refuses_when_gpus_are_missing():
    """`python bench.py --gpus N` with no launcher starts the ranks itself -- and refuses, before touching any GPU, when the node
    shows fewer than N devices (this container: 0; the one-GPU box: 1)."""
    import torch
    want = torch.cuda.device_count() + 1
    if want < 2:
        want = 2
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(want)], capture_output=True, text=True,
                         timeout=300, env=env)
    assert res.returncode != 0 and res.stdout.strip() == "" and "refusing" in res.stderr


@pytest.mark.gpu
def test_self_launch_single_gpu_without_launcher_variables():
    rec = _run("--no-cpu-baseline", launcher_env=False)
    assert rec["config"]["collective"] == "none" and rec["roofline"]["traffic_measured_at"]


@pytest.mark.gpu
@pytest.mark.parametrize("config", ["cfg2", "cfg5"])
def test_weak_scaling_line_with_two_ranks_sharing_the_gpu(config):
    """`--config cfg2 / cfg5 --gpus 2`: per-GPU workloads (weak scaling).  The replicated-chain measurement behind `serial_chain` is a few more
    SHARDED fits: until round 6 rank 0 ran them alone, beside ranks already waiting at the last barrier -- a hung job.
    serial_chain_ms is time per fit minus the medians of the bracketed kernels and all-reduce waits, which on two ranks time-sharing one
    GPU swing by a millisecond from run to run: a time per fit averaged over 3 fits (3.2 - 5.2 ms between runs) made it negative in
    one of seven runs, so the time per fit here is averaged over 30."""
    rec = _run("--config", config, "--gpus", "2", "--share-gpu", "--no-cpu-baseline", "--full", launcher_env=False, n_gpus=2, steps=30)
    assert rec["scaling"] == "weak" and rec["config"]["parallelism"] == "sample-sharded x2" and "speedup_vs_one_gpu_same_matrix" in rec
    if config == "cfg2":
        assert rec["serial_chain"]["serial_chain_ms"] > 0 and rec["collective"]["allreduce_calls_per_fit"] == 5 + 3


@pytest.mark.gpu
def test_self_launch_two_ranks_sharing_the_gpu():
    """The launcher path end to end with N = 2 on the one-GPU box: bench.py starts two rank processes itself (fresh children,
    before any GPU call), they share GPU 0 and all-reduce over gloo; rank 0 prints the one record with n_gpus = 2."""
    rec = _run("--gpus", "2", "--share-gpu", "--no-cpu-baseline", "--full", launcher_env=False, n_gpus=2)
    assert "SHARE GPU 0" in rec["config"]["collective"] and rec["config"]["parallelism"] == "sample-sharded x2"
    # no --config at N = 2: configs[3] split two ways, strong scaling, total samples per second
    assert rec["scaling"] == "strong" and rec["config"]["rows_per_gpu"] == 1000000 and rec["config"]["rows_total"] == 2000000
    assert rec["config"]["n_components"] == 128 and rec["config"]["n_iter"] == 7 and rec["config"]["features"] == 1024
    assert abs(rec["value"] - 2000000 / (rec["ms_per_step"] * 1e-3)) <= 1e-3 * rec["value"]
    co = rec["collective"]
    assert co["allreduce_calls_per_fit"] == 7 + 3 and co["allreduce_bytes_per_fit"] > 0 and co["allreduce_ms_per_fit"] > 0
    assert rec["one_gpu_same_matrix"]["ms_per_step"] > 0


@pytest.mark.gpu
def test_single_gpu_record_has_the_northstar_fit():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--full"],
                         capture_output=True, text=True, timeout=420, env=env, cwd=ROOT)   # (a run takes 10 - 60 s)
    assert res.returncode == 0, res.stderr[-2000:]
    rec = json.loads(res.stdout.strip().split("\n")[-1])
    assert rec["scaling"] == "weak" and rec["config"]["rows_per_gpu"] == 100000
    nf = rec["northstar_fit"]
    for key in ("n_iter_5", "n_iter_7"):
        assert nf[key]["ms_per_fit"] > 0 and 0 < nf[key]["fit_roofline"]["frac"] <= 1.0
    assert nf["n_iter_7"]["fit_roofline"]["passes"] == 8 and nf["n_iter_7"]["fit_roofline"]["pass_kind"].startswith("fused")
    assert rec["fused_pass"]["launches_per_fit"] == 6 and rec["roofline"]["kernel"].startswith("K3")
    assert rec["serial_chain"]["serial_chain_ms"] > 0
    assert rec["host_in"]["row_pitch_bytes"] == 2048 + 128


def test_dump_outputs_writes_float_arrays_and_samples_large_ones(tmp_path):
    """--dump-outputs: one <name>.npy per array in float32 / float64; an array past its share of the byte budget is replaced by a fixed,
    seeded sample of its elements -- the same elements in every run, so two builds compare output for output."""
    sys.path.insert(0, ROOT)
    import bench
    arrays = {"components": np.arange(12, dtype=np.float32).reshape(3, 4), "singular": np.ones(3), "n_iter": np.array([7]),
              "big": np.arange(4096, dtype=np.float64)}
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), arrays, max_bytes=4 * 8192)
    assert sorted(os.listdir(tmp_path / "a")) == ["big.npy", "components.npy", "n_iter.npy", "singular.npy"]
    c = np.load(tmp_path / "a" / "components.npy")
    assert c.dtype == np.float32 and np.array_equal(c, arrays["components"])
    n_iter = np.load(tmp_path / "a" / "n_iter.npy")
    assert n_iter.dtype == np.float64 and n_iter.tolist() == [7.0]
    big = np.load(tmp_path / "a" / "big.npy")
    assert big.dtype == np.float64 and big.size == 8192 // 8 and np.all(np.diff(big) > 0)   # a sorted sample of the elements
    assert np.array_equal(big, np.load(tmp_path / "b" / "big.npy"))


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_timed_outputs(tmp_path):
    """A plain run (no --full) carries only what its timed steps measured; --dump-outputs writes the outputs of the last timed fit.  With the
    same arguments the inputs are the same from run to run, so the outputs are too, whatever the number of steps."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    names = ["components", "explained_variance_ratio", "mean", "singular_values"]
    dumps = []
    for steps in (2, 3):
        out = tmp_path / f"steps{steps}"
        res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                              "--dump-outputs", str(out)], capture_output=True, text=True, timeout=420, env=env, cwd=ROOT)
        assert res.returncode == 0, res.stderr[-2000:]
        lines = [ln for ln in res.stdout.split("\n") if ln.strip()]
        assert len(lines) == 1, res.stdout[:500]
        rec = json.loads(lines[0])
        assert rec["steps"] == steps and rec["ms_per_step"] > 0 and rec["value"] > 0 and "roofline" in rec
        assert not [key for key in FULL_ONLY if key in rec], [key for key in FULL_ONLY if key in rec]
        assert sorted(os.listdir(out)) == [f"{name}.npy" for name in names]
        dumps.append({name: np.load(out / f"{name}.npy") for name in names})
    c = dumps[0]["components"]
    assert c.shape == (64, 512) and c.dtype in (np.float32, np.float64) and np.all(np.isfinite(c))
    assert dumps[0]["singular_values"].shape == (64,) and dumps[0]["mean"].shape == (512,)
    for name in names:
        assert np.array_equal(dumps[0][name], dumps[1][name]), name
