"""bench.py as the driver's SCALE run starts it -- under `python -m torch.distributed.run`, one rank per GPU, RCCL process
group, the REAL solver handle -- on the one GPU a test box has (VERDICT r4 "Next round" 7): the first execution of
`dist.all_gather_into_tensor(gathered, dU)` + `h.last_kernel_ms()` + the MAX-reduced timing together must not be the
driver's. tests/test_bench_ranks_gloo.py covers the rank logic at world_size 2 over gloo with a stand-in handle; this is
the other half: the real handle over the real backend at world_size 1, and the N = 1 value of the SCALE series agreeing
with the plain BENCH invocation of the same workload."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "8192", "--no-secondary", "--no-cpu-baseline",
        "--no-accuracy"]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(cmd):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines            # exactly ONE line on stdout, whatever RCCL / the launcher print elsewhere
    return json.loads(lines[0])


def test_bench_under_the_launcher_on_one_gpu_agrees_with_the_plain_run():
    launched = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr",
                     "127.0.0.1", "--master-port", str(_free_port())] + ARGS)
    plain = _run([sys.executable] + ARGS)
    for rec in (launched, plain):
        assert rec["n_gpus"] == 1 and rec["steps"] == 3 and rec["warmup"] == 1 and rec["scaling"] == "weak"
        assert rec["unit"] == "solves/s" and rec["dtype"] == "f32" and rec["higher_is_better"] is True
        assert rec["config"]["batch_per_gpu"] == 8192 and rec["config"]["max_active_dynobs"] == 40
        r = rec["roofline"]
        assert r["bound"] == "hbm" and r["achieved"] > 0 and 0 < r["frac"] < 1 and r["kernel_ms"] > 0 and r["valu_frac"] > 0
        # the kernel's HIP-event time is inside the wall time of a step, and most of it
        assert 0.5 * rec["ms_per_step"] < r["kernel_ms"] <= rec["ms_per_step"] * 1.001, (r["kernel_ms"], rec["ms_per_step"])
        assert abs(rec["value"] - 8192 / (rec["ms_per_step"] * 1e-3)) < 1e-3 * rec["value"]
    assert "single GPU" in plain["config"]["sharding"] and "single GPU" in launched["config"]["sharding"]
    # same workload, same kernels: the launcher adds the process group, one all_gather of 1.3 MB and one all_reduce
    if abs(launched["value"] - plain["value"]) > 0.05 * plain["value"]:
        # (three timed steps of ~120 ms each: one repeat of the plain run before a box hiccup counts as a failure)
        plain = _run([sys.executable] + ARGS)
    assert abs(launched["value"] - plain["value"]) <= 0.05 * plain["value"], (launched["value"], plain["value"])
    assert launched["roofline"]["psi_evals_per_solve"] == plain["roofline"]["psi_evals_per_solve"]     # bit-identical solves


def test_plain_run_is_the_headline_alone_and_dumps_the_same_outputs_every_run(tmp_path):
    """A plain run (no --full) prints the headline without the secondary rows, the CPU baseline or the accuracy digest;
    --steps sets the timed steps; --dump-outputs writes the last step's outputs, float32 / float64 only, the same arrays
    from two runs of the same arguments (seeded inputs; the number of steps does not change the results)."""
    import numpy as np
    base = [sys.executable, "bench.py", "--gpus", "1", "--warmup", "1", "--batch", "8192"]
    recs = [_run(base + ["--steps", str(k), "--dump-outputs", str(tmp_path / str(k))]) for k in (2, 3)]
    for k, rec in zip((2, 3), recs):
        assert rec["steps"] == k and rec["ms_per_step"] > 0
        assert abs(rec["value"] - 8192 / (rec["ms_per_step"] * 1e-3)) < 1e-3 * rec["value"]
        assert not {"secondary_solves_per_s", "cpu_baseline", "accuracy_summary"} & set(rec)
    names = {"U", "cost", "status", "iters", "info"}
    for k in (2, 3):
        assert sorted(os.listdir(tmp_path / str(k))) == sorted(n + ".npy" for n in names)
    shapes = {"U": (8192, 40), "cost": (8192,), "status": (8192,), "iters": (8192, 2), "info": (8192, 6)}
    for n in names:
        a, b = np.load(tmp_path / "2" / (n + ".npy")), np.load(tmp_path / "3" / (n + ".npy"))
        assert a.dtype == np.float32 if n in ("U", "cost", "info") else a.dtype == np.float64, (n, a.dtype)
        assert a.shape == shapes[n] and np.array_equal(a, b), n
    assert np.isfinite(np.load(tmp_path / "2" / "U.npy")).all()
