#!/usr/bin/env python3
"""Headline benchmark: batched NMPC solves/sec on MI355X (BASELINE.json metric).

  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
  (N > 1: python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... bench.py ...)

A plain run sets up the headline workload, runs W untimed and K timed steps and prints the line; `ms_per_step` is the
wall time of one timed step. `--dump-outputs DIR` then writes what the last timed step returned to its caller (U, cost,
status, iters, info[:, :6] of rank 0's shard; under torch.distributed.run also the gathered U) as DIR/<name>.npy in float32 /
float64, at most 64 MB in all (a fixed, seeded sample of rows beyond that). The inputs are seeded: the same arguments
give the same inputs on every run, so two builds can be compared output for output. `--full` adds what the headline
does not need (N = 1 only): `secondary_solves_per_s`, `cpu_baseline` and `accuracy_summary` below.

A "step" is one pass of the hot path over one batch: every rank solves its own shard of B independent MPC
problems (weak scaling: B per GPU is fixed) with the parameter batch already resident in HBM, then (N > 1) the
control sequences are all-gathered over RCCL -- the only collective on this path. Workload: BASELINE.json
configs[2] (batch=65536 main_eva.py scenarios, N=20, 4 obstacles x 10 hypotheses, fp32) -- the per-GPU shard of
configs[3] (8 x 65536, seeds 1..8), so the N = 1, 2, 4, 8 series of the metric is one family.

Rank 0 prints ONE COMPACT JSON line (< 4 KB aimed at, < 8 KB asserted: round 3's 21.7 KB line was not parsed by the
driver) with the driver's keys plus
  roofline               : HBM roofline of the solve kernel (algorithmic bytes / HIP-event kernel time) -- this path is
                           VALU/latency bound, so the HBM fraction is tiny by construction; the fp32 vector-ALU figure
                           that actually bounds it sits next to it as roofline.valu_tflops / valu_frac / psi_evals_per_solve
  converged_frac         : share of the timed instances that end Converged
  secondary_solves_per_s : (--full, N = 1) flat {name: solves/s} of the other BASELINE configurations, the `passing`
                           scenario family (where the solver converges), fp64, polish and dispatch-hint rows
  cpu_baseline           : (--full) the CPU oracle (plain-C restatement of the reference's OpEn algorithm, kind "port")
                           timed on this box's host cores on a bounded sample of the same batch (N = 1, rank 0 only)
  accuracy_summary       : (--full, N = 1) flat {name: number} digest of the SURVEY.md 8(d) accuracy protocol
                           (tests/accuracy_protocol.py) on small seeded samples of the configs[1] / [2] / [4] generators
and writes everything it measured, un-abridged (solver statistics, every secondary row, the whole accuracy table, the
CPU-baseline notes), to `bench_detail.json` next to this file and to stderr.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WORKLOADS = {
    # name -> (BASELINE.json description, scenario key)
    "cfg1": ("batch=1024 random init states, N=20, 2 obstacles x 5 WTA hypotheses, fp32, 1 MI355X",
             "cfg1_b1024_n20_2x5"),
    "cfg2": ("batch=65536 main_eva.py scenarios, mpc_fast.yaml N=20, 4 obs x 10 hypotheses, 1 MI355X",
             "cfg2_b65536_n20_4x10"),
    "cfg4": ("long horizon N=40, 8 obs x 20 hypotheses, batch=8192, 1 MI355X",
             "cfg4_b8192_n40_8x20"),
}
CLOSED_LOOP_STEPS = (1, 8, 20)   # time steps at which the corridor closed-loop family captures its parameter vectors
REFSCEN_STEPS = (2, 14, 26)      # ... and the reference-scenario family (runs of 45-95 steps: all scenarios still running; the
                                 # scenario's own pedestrian meets the robot around steps 22-32, tools/bench_evaluate.py)
HARVEST_STEPS = {"closed_loop": CLOSED_LOOP_STEPS, "refscen": REFSCEN_STEPS}
HARVEST_FAMILY = {"closed_loop": "corridor", "refscen": "reference"}
REFERENCE_TIME_CAP_US = 100_000  # config/mpc_fast.yaml max_solver_time (mpc_builder.py:189): the `_budget` rows
HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
VALU_PEAK_TFLOPS = 157.3     # MI355X_MICROARCH.md: peak FP32 vector


def measured_traffic(workload, dtype, batch, family="toward_robot", axis_aligned=0):
    """HBM bytes per launch from the committed rocprofv3 PMC passes of this same command (FETCH_SIZE and
    WRITE_SIZE collected in separate passes, gfx950 correction applied; profiles/rNN_<workload>_traffic.json).
    A counter pass cannot run inside the timed process, so the latest committed measurement that matches the
    workload is reported; None if there is none."""
    import glob
    best = None
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_traffic.json"))):
        try:
            rec = json.load(open(path))
        except (OSError, ValueError):
            continue
        if rec.get("workload") == workload and rec.get("dtype") == dtype and rec.get("batch") == batch and \
                rec.get("family", "toward_robot") == family:
            best = rec
    if best is None:
        return None
    # (profiles/rNN_cfg4_f64_traffic.json holds both members of the streamed-table kernel pair: the compressed table is the
    #  one the reference's axis-aligned inputs take)
    # (an --axis-aligned -1 run streams the GENERAL table)
    member = "general" if axis_aligned < 0 else "compressed"
    val = best.get("hbm_bytes_per_launch", (best.get(member) or {}).get("hbm_bytes_per_launch"))
    return None if val is None else float(val)


def flops_forward(N, Nother, Nstc, Ndyn):
    """Algorithmic flops of one psi evaluation; cost+gradient is counted as 3x."""
    return N * (33 + 8 * (2 * Nother - 1) + 28 * Nstc + 62 * Ndyn) + 10 * N * (N + 1) + 12 * N


class Env:
    """torch / distributed context shared by the timed workloads.

    `backend` / `device` / `handle_factory` exist for ONE reason: tests/test_bench_ranks_gloo.py drives the rank logic of
    this file (seed per rank, gathered shape, MAX-reduced time, one JSON line from rank 0) at world_size 2 over gloo on a
    GPU-less box with a stand-in for the solver handle. The bench itself always runs with the defaults: RCCL, cuda, the
    real handle -- and refuses to start without a GPU."""

    def __init__(self, args, backend="nccl", device="cuda", handle_factory=None):
        import torch
        import torch.distributed as dist
        import dyobav_mpcnwta_warehouse_amd as nm
        self.torch, self.dist, self.nm = torch, dist, nm
        self.device = device
        self.handle_factory = handle_factory or nm.Handle
        self.rank = int(os.environ.get("RANK", "0"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        if self.world != args.gpus:
            if self.world == 1 and args.gpus > 1:
                raise SystemExit("--gpus N > 1 must be launched with torch.distributed.run (one process per GPU)")
            args.gpus = self.world
        if device == "cuda":
            if not torch.cuda.is_available():
                raise SystemExit("bench.py needs an MI355X: the solver has no CPU path")
            torch.cuda.set_device(self.local_rank)
        self.use_dist = self.world > 1 or "RANK" in os.environ   # under torch.distributed.run the same path runs for N = 1
        if self.use_dist:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29500")
            if device == "cuda":
                dist.init_process_group(backend, rank=self.rank, world_size=self.world,     # "nccl" is RCCL on ROCm
                                        device_id=torch.device("cuda", self.local_rank))
            else:
                dist.init_process_group(backend, rank=self.rank, world_size=self.world)

    def sync(self):
        if self.device == "cuda":
            self.torch.cuda.synchronize()

    def fence(self):
        self.sync()
        if self.use_dist:
            self.dist.barrier()
        self.sync()


def harvested_batch(env: Env, cfg, family: str, B: int, spec: dict, np_dtype):
    """Parameter vectors harvested from the closed loop (scenarios.harvest_closed_loop), on the device; cached per
    (family, B, dtype) so that the rows that time the same batch under other options (budget, polish) share one harvest."""
    key = (family, B, np.dtype(np_dtype).name)
    cache = env.__dict__.setdefault("harvest_cache", {})
    if key not in cache:
        t_h = time.perf_counter()
        dP_h, step_of = env.nm.scenarios.harvest_closed_loop(cfg, B, steps=HARVEST_STEPS[family], seed=13 + env.rank,
                                                             n_ped=spec["n_ped"], n_hyp=spec["n_hyp"], dtype=np_dtype,
                                                             return_device=True, family=HARVEST_FAMILY[family])
        cache[key] = (dP_h, {"capture_steps": {int(s_): int((step_of == s_).sum().item()) for s_ in env.torch.unique(step_of)},
                             "seconds": time.perf_counter() - t_h, "scenarios": HARVEST_FAMILY[family]})
    return cache[key]


def run_workload(env: Env, workload: str, family: str, dtype: str, steps: int, warmup: int, batch=None,
                 latency_waves: int = 0, reg_table: int = 0, coop_waves: int = 0, dispatch_hint: bool = False,
                 polish: bool = False, staged: int = 0, axis_aligned: int = 0, capacity_hint: bool = True,
                 budget: bool = False) -> dict:
    """Time `steps` passes of one workload (after `warmup` untimed ones); returns the measurements of this rank with
    the whole-job rate (max over ranks of the elapsed time)."""
    torch, dist, nm = env.torch, env.dist, env.nm
    desc, key = WORKLOADS[workload]
    np_dtype = np.float32 if dtype == "f32" else np.float64
    t_dtype = torch.float32 if dtype == "f32" else torch.float64
    spec = dict(nm.scenarios.BENCH_CONFIGS[key])
    layout = spec.pop("layout")
    B = batch or spec.pop("B")
    spec.pop("B", None)
    spec["seed"] = spec["seed"] + env.rank           # every rank solves a different shard
    N = layout.N

    cfg = nm.default_config_struct()
    cfg.device_id = env.local_rank
    cfg.N_hor, cfg.Nother, cfg.Nstcobs, cfg.Ndynobs = layout.N, layout.Nother, layout.Nstc, layout.Ndyn
    # capacity hint (stated in the line: config.max_active_dynobs): the workload has n_ped x n_hyp predicted-obstacle
    # hypotheses, the remaining Ndynobs slots are the reference's zero padding (mpc_interface.py:82-88) -- what a caller like
    # MpcInterface knows (it counts the rows it fills); fewer provisioned rows -> smaller tables per instance.
    # capacity_hint = False: Ndynobs rows provisioned (the `_nohint` secondary row)
    cfg.max_active_dynobs = spec["n_ped"] * spec["n_hyp"] if capacity_hint else 0
    harvest = None
    if family in HARVEST_STEPS:
        # BASELINE configs[2] literally: "main_eva.py scenarios" -- parameter vectors harvested from the batched closed-loop
        # evaluator (row f3) at these dimensions, a third each from three time steps of the runs. `refscen`: the reference's
        # own scenario_0..2 on its warehouse map (scenarios.make_reference_scenarios); `closed_loop`: round 5's corridor
        # family (tests/test_gpu_closed_loop.py runs the parity protocol on both distributions)
        dP_h, harvest = harvested_batch(env, cfg, family, B, spec, np_dtype)
        P_host = dP_h[:4096].cpu().numpy()       # (what the CPU baseline / checksum of a --family closed_loop run sample)
    else:
        P_host = nm.scenarios.make_batch_chunked(B, layout, ped_mode=family, dtype=np_dtype, **spec)   # bounded host memory
    cfg.latency_waves = latency_waves
    cfg.reg_table = reg_table
    cfg.coop_waves = coop_waves
    cfg.polish = int(polish)
    cfg.staged = staged
    cfg.axis_aligned = axis_aligned
    if budget:
        # the reference's max_solver_time (0.1 s of ITS solver on a host core) as the deterministic evaluation budget
        # (nmpc_config.max_evaluations; solver.evaluation_budget): a SECONDARY row, never the headline
        from dyobav_mpcnwta_warehouse_amd.solver import evaluation_budget
        cfg.max_evaluations = evaluation_budget(REFERENCE_TIME_CAP_US, layout.N, layout.Nother, layout.Nstc, layout.Ndyn)
    h = env.handle_factory(cfg)
    dev = env.device
    if dev == "cuda":
        h.set_stream(torch.cuda.current_stream().cuda_stream)

    # inputs and outputs resident in HBM before the timed region
    dP = dP_h.contiguous() if harvest is not None else torch.from_numpy(P_host.astype(np_dtype)).to(dev)
    dU = torch.empty(B, 2 * N, dtype=t_dtype, device=dev)
    dcost = torch.empty(B, dtype=t_dtype, device=dev)
    dstatus = torch.empty(B, dtype=torch.int32, device=dev)
    diters = torch.empty(B, 2, dtype=torch.int32, device=dev)
    dinfo = torch.empty(B, 8, dtype=t_dtype, device=dev)
    gathered = torch.empty(env.world * B, 2 * N, dtype=t_dtype, device=dev) if env.use_dist else None
    kernel_ms = []

    gather_ms = []
    cuda = dev == "cuda"
    ev_g = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) if (cuda and env.use_dist) else None

    def step(record):
        h.solve_raw(np_dtype, dP, B, dU, dcost, dstatus, diters, None, None, False, None, dinfo, sync=False)
        if env.use_dist:
            # RCCL over xGMI: gather the results, nothing else. Timed by HIP events on the stream the solve was enqueued on
            # (torch's current stream = the handle's stream): what the gather itself costs, next to each rank's own time
            t_g = time.perf_counter()
            if ev_g and record:
                ev_g[0].record()
            dist.all_gather_into_tensor(gathered, dU)
            if ev_g and record:
                ev_g[1].record()
        if record:
            kernel_ms.append(h.last_kernel_ms())           # HIP events on the launch stream (syncs that stream)
            if env.use_dist:
                if ev_g:
                    ev_g[1].synchronize()
                    gather_ms.append(float(ev_g[0].elapsed_time(ev_g[1])))
                else:                                      # (gloo stand-in of tests/test_bench_ranks_gloo.py: host clock)
                    gather_ms.append((time.perf_counter() - t_g) * 1e3)

    if dispatch_hint:
        # nmpc_set_dispatch_order: longest first, ranked by the evaluation counts of an (untimed) earlier pass over the
        # same batch -- the information a receding-horizon loop has from its previous time step. Never used for the
        # headline: there every pass sees its batch for the first time.
        step(False)
        h.set_dispatch_order(torch.argsort(dinfo[:, 4], descending=True, stable=True).to(torch.int32))
    for _ in range(warmup):
        step(False)
    env.fence()
    t0 = time.perf_counter()
    for _ in range(steps):
        step(True)
    env.fence()
    elapsed = time.perf_counter() - t0
    scale_diag = None
    if env.use_dist:
        # SCALE diagnostics (one glance at the first multi-GPU run): how many ranks RCCL saw, every rank's OWN time per step
        # (imbalance between the shards -- SURVEY 8e's named risk -- shows here), its kernel time, and the gather
        mine = torch.tensor([elapsed / steps * 1e3, float(np.mean(kernel_ms)), float(np.mean(gather_ms))], dtype=torch.float64, device=dev)
        every = [torch.zeros_like(mine) for _ in range(env.world)]
        dist.all_gather(every, mine)
        every = torch.stack(every).cpu().numpy()
        scale_diag = {"ranks": int(dist.get_world_size()), "per_rank_ms": [float(v) for v in every[:, 0]],
                      "per_rank_kernel_ms": [float(v) for v in every[:, 1]], "gather_ms": float(every[:, 2].max()),
                      "gather_bytes_per_rank": int(dU.numel() * dU.element_size())}
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    status = dstatus.cpu().numpy()
    iters = diters.cpu().numpy()
    info_t = dinfo.cpu().numpy()
    info = info_t.astype(np.float64)
    U = dU.cpu().numpy()
    # what the caller of the last timed step received (bench.py --dump-outputs). info[:, 6:8] say which kernel family solved
    # an instance -- the tail hand-off picks its instances at run time -- so only the solver statistics info[:, :6] go along
    outputs = {"U": U, "cost": dcost.cpu().numpy(), "status": status, "iters": iters, "info": info_t[:, :6]}
    if gathered is not None:
        outputs["U_gathered"] = gathered          # (a device tensor: copied to the host only when dumped)
    kinfo = h.kernel_info()
    launch = h.last_launch_info()
    h.close()

    w = np.dtype(np_dtype).itemsize
    bytes_per_solve = w * (layout.np_ + 2 * N + 4)
    k_ms = float(np.mean(kernel_ms))
    achieved_gbs = bytes_per_solve * B / (k_ms * 1e-3) / 1e9
    ff = flops_forward(layout.N, layout.Nother, layout.Nstc, layout.Ndyn)
    n_psi, n_grad = info[:, 4], info[:, 5]
    # 0: throughput kernel; > 0: latency kernel with that many wavefronts per instance; < 0: cooperative. (By the launch's family:
    # under the tail hand-off a throughput launch has a few rows with info[7] = 4 -- the instances the latency family solved.)
    fam_l = launch.get("family", "throughput")
    waves = 0 if fam_l == "throughput" else int(info[:, 7].max()) if fam_l == "latency" else int(info[:, 7].min())
    tname = "float" if dtype == "f32" else "double"
    lps = kinfo["lanes_per_step"]
    # short name for the line: the rocprofv3 kernel-trace name (register-table kernels are pairs: <.., slots, 1> = the
    # axis-aligned member, <.., 2> = the general one); prose in bench_detail.json
    li = nm.layout_info(cfg) if hasattr(nm, "layout_info") and not isinstance(cfg, type(None)) else None
    try:
        rs = int(li.reg_slots_f32) if (li is not None and dtype == "f32") else 0
    except Exception:
        rs = 0
    member = {2: 1, 1: 1, 0: 2}.get(launch["axis_aligned"], 0)
    tail = f",false,{rs},{member}" if (rs and lps == 3 and waves >= 0 and member) else ""
    try:
        glb = bool(li.global_table_f32 if dtype == "f32" else li.global_table_f64) if li is not None else False
    except Exception:
        glb = False
    # (cooperative kernels on the global table are pairs too: <.., true, 1> streams the compressed table of axis-aligned ellipses)
    ctail = f",true,{member}" if (glb and member and waves == -4) else ""
    if dtype == "f64" and not tail and lps == 3 and waves == 0 and member and launch["axis_aligned"] >= 0:
        tail = f",false,14,{member}"                 # (the fp64 register-table kernel: one wavefront per SIMD, 14 slots)
    kernel_name = (f"solve_spec_kernel<{tname},{lps}{tail or ',false,0,0'},true> W={waves}" if waves > 0
                   else f"solve_coop_reg_kernel<{'true' if 33 <= layout.N <= 42 else 'false'}> W=8" if waves == -8
                   else f"solve_coop_kernel<{tname},{lps}{ctail}> W={-waves}" if waves < 0
                   else f"solve_kernel<{tname},{lps}{tail}>")
    kernel_desc = ("latency mode: several wavefronts per instance, speculative line search" if waves > 0
                   else "cooperative: the wavefronts of a workgroup share each evaluation" if waves < 0
                   else "one wavefront per instance")
    flops_launch = float(np.sum((n_psi - n_grad) * ff + n_grad * 3 * ff))
    achieved_tf = flops_launch / (k_ms * 1e-3) / 1e12
    conv = status == 0
    if launch["axis_aligned"] == 2:
        kernel_desc += "; axis-aligned member of the kernel pair chosen on the device (the general twin returns at once)"
    if launch.get("tail_handed_off"):
        kernel_desc += f"; tail hand-off: the {launch['tail_handed_off']} instances ranked longest solved by the latency family's tail member (same bits) next to it"
    if launch["staged_outer_iterations"]:
        kernel_name += " x2 launches"
        kernel_desc += f"; two launches: pilot of {launch['staged_outer_iterations']} outer iteration(s), rest ranked by ||F2||"
    polished = None
    if polish:
        kernel_name += " +polish64"
        kernel_desc += "; fp64 polish of the converged instances"
        polished = {"selected": launch["polish_selected"], "replaced": int((info[:, 6] == 1).sum()),
                    "kept_main_result": int((info[:, 6] == 2).sum())}

    def part(mask):
        if not mask.any():
            return {"frac": 0.0}
        return {"frac": float(mask.mean()), "outer_iters_mean": float(iters[mask, 0].mean()),
                "inner_iters_mean": float(iters[mask, 1].mean()), "psi_evals_mean": float(n_psi[mask].mean()),
                "share_of_psi_evals": float(n_psi[mask].sum() / n_psi.sum())}

    return {
        "value": env.world * B * steps / elapsed, "ms_per_step": elapsed / steps * 1e3, "steps": steps, "warmup": warmup,
        "config": {"workload": f"{workload}: {desc}", "family": family, "batch_per_gpu": B, "N_hor": layout.N,
                   "Ndynobs": layout.Ndyn, "Nstcobs": layout.Nstc, "Nother": layout.Nother, "np": layout.np_,
                   "max_active_dynobs": int(cfg.max_active_dynobs), "latency_waves": int(cfg.latency_waves),
                   "max_evaluations": int(getattr(cfg, "max_evaluations", 0)), "tail_handed_off": int(launch.get("tail_handed_off", 0)),
                   "dispatch": ("longest first by the evaluation counts of a previous pass over the same batch"
                                if dispatch_hint else "index order"),
                   "lds_bytes_per_instance": int(kinfo["lds_bytes_" + dtype]),
                   "sharding": f"{env.world} x independent shards (seeds {spec['seed'] - env.rank}..), all_gather of U"
                   if env.world > 1 else "single GPU"},
        # HBM roofline as the contract asks; this path is bound by fp32 vector-ALU issue, not by HBM: that
        # roofline is the valu_* keys (algorithmic flops of the psi / grad-psi evaluations the kernel counted / kernel time
        # / peak fp32 vector rate), flat so that they survive any consumer that keeps scalars only
        "roofline": {"bound": "hbm", "achieved": achieved_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": achieved_gbs / HBM_PEAK_GBS, "traffic": measured_traffic(workload, dtype, B, family, axis_aligned),
                     "kernel": kernel_name, "kernel_description": kernel_desc, "kernel_ms": k_ms, "algorithmic_bytes_per_launch": bytes_per_solve * B,
                     "binding_roofline": "fp32 VALU issue (see valu_*), HBM fraction is tiny by construction",
                     "valu_tflops": achieved_tf, "valu_peak_tflops": VALU_PEAK_TFLOPS,
                     "valu_frac": achieved_tf / VALU_PEAK_TFLOPS, "flops_per_psi_eval": ff,
                     "psi_evals_per_solve": float(n_psi.mean()), "grad_evals_per_solve": float(n_grad.mean())},
        "polish": polished,
        "scale": scale_diag,
        "harvest": harvest,
        "solver": {"converged_frac": float(conv.mean()), "out_of_time_frac": float((status == 2).mean()),
                   "outer_iters_mean": float(iters[:, 0].mean()),
                   "inner_iters_mean": float(iters[:, 1].mean()), "inner_iters_max": int(iters[:, 1].max()),
                   "converged": part(conv), "not_converged": part(~conv),
                   "converged_solves_per_s": float(conv.mean() * env.world * B * steps / elapsed)},
        "_host": (layout, P_host, U, status),
        "_gathered": gathered,
        "_outputs": outputs,
    }


def main(argv=None, env_factory=Env):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="cfg2")
    ap.add_argument("--family", choices=("toward_robot", "oncoming", "passing", "closed_loop", "refscen"), default="toward_robot",
                    help="scenario family of the generator (SURVEY.md 8d prescribes toward_robot); refscen / closed_loop: "
                         "parameter vectors harvested from the closed loop on the reference's scenarios / the corridor family")
    ap.add_argument("--batch", type=int, default=None, help="override the per-GPU batch (default: BASELINE's)")
    ap.add_argument("--dtype", choices=("f32", "f64"), default="f32")
    ap.add_argument("--full", action="store_true",
                    help="also run the secondary workloads, the CPU baseline and the accuracy protocol (N = 1 only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the outputs of the last timed step as DIR/<name>.npy (float32 / float64, <= 64 MB)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-secondary", action="store_true", help="with --full: skip the secondary workloads")
    ap.add_argument("--no-accuracy", action="store_true", help="with --full: skip the accuracy protocol")
    ap.add_argument("--latency-waves", type=int, default=0,
                    help="nmpc_config.latency_waves: 0 = automatic (library default), 1 = one wavefront per instance, "
                         "2..4 = latency mode")
    ap.add_argument("--reg-table", type=int, default=0, help="nmpc_config.reg_table: 0 = automatic, -1 = LDS / global table")
    ap.add_argument("--coop-waves", type=int, default=0, help="nmpc_config.coop_waves: 0 = automatic, 1 = off, 2..4")
    ap.add_argument("--axis-aligned", type=int, default=0, help="nmpc_config.axis_aligned: 0 = scan of the batch on the device, "
                    "1 = promised, -1 = the general kernels (diagnostic: the other member of a kernel pair)")
    args = ap.parse_args(argv)

    # stdout must carry exactly ONE JSON line: RCCL / HIP libraries print banners and warnings on fd 1, so keep a
    # private copy of the real stdout for the result and point fd 1 at stderr for everything else.
    sys.stdout.flush()
    result_out = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)

    env = env_factory(args)
    m = run_workload(env, args.workload, args.family, args.dtype, args.steps, args.warmup, args.batch,
                     args.latency_waves, args.reg_table, args.coop_waves, axis_aligned=args.axis_aligned)
    layout, P_host, U, status = m.pop("_host")
    gathered = m.pop("_gathered")
    outputs = m.pop("_outputs")

    if env.rank == 0:
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, outputs)
        detail = {
            "metric": f"MPC solves/sec (N={layout.N}, batched)",
            "value": m["value"],
            "unit": "solves/s",
            "n_gpus": env.world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": m["ms_per_step"],
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": args.dtype,
            "data": "synthetic",
            "config": m["config"],
            "roofline": m["roofline"],
            # share of the timed instances that end Converged: on the contract family (pedestrians walk INTO
            # the robot) the hard constraint is infeasible for almost all of them -- see the `passing` rows of `secondary`
            "converged_frac": m["solver"]["converged_frac"],
            "converged_solves_per_s": m["solver"]["converged_solves_per_s"],
            "solver": m["solver"],
        }
        if m.get("scale"):      # launched under torch.distributed.run: ranks / per-rank times / gather time at the top level
            detail.update(m["scale"])
        full = args.full and env.world == 1
        if full and not args.no_secondary:
            detail["secondary"] = secondary_workloads(env, args)
        if full and not args.no_cpu_baseline:
            detail["cpu_baseline"] = cpu_baseline(layout, P_host)
        if full and not args.no_accuracy:
            detail["accuracy"] = accuracy_table(env)
        line = compact_line(detail)
        try:                                       # the un-abridged record: a side file + stderr, never stdout
            with open(os.path.join(ROOT, "bench_detail.json"), "w") as f:
                json.dump(detail, f, indent=1)
        except OSError as exc:
            print(f"[bench] bench_detail.json not written: {exc!r}", file=sys.stderr)
        print("[bench detail] " + json.dumps(detail), file=sys.stderr)
        result_out.write(line + "\n")
        result_out.flush()

    if env.use_dist:
        env.dist.destroy_process_group()
    return {"U": U, "gathered": gathered, "P_checksum": float(np.abs(P_host).sum())}


DUMP_LIMIT_BYTES = 64 * 10 ** 6


def dump_outputs(out_dir: str, outputs: dict) -> None:
    """DIR/<name>.npy for every output of the last timed step: float arrays in their own precision, integer ones as
    float64 (exact). Above DUMP_LIMIT_BYTES in all, every array keeps the same fixed share of its rows, chosen by a
    seeded generator (the same rows on every run), and DIR/<name>_rows.npy holds the row indices kept."""
    arrays = {}
    for name, a in outputs.items():
        a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
        arrays[name] = a if a.dtype in (np.float32, np.float64) else a.astype(np.float64)
    total = sum(a.nbytes for a in arrays.values())
    # (when sampled: 8 bytes of index per kept row, and room for the .npy headers)
    keep = 1.0 if total <= 0.99 * DUMP_LIMIT_BYTES else \
        0.95 * DUMP_LIMIT_BYTES / (total + 8 * sum(a.shape[0] for a in arrays.values()))
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        if keep < 1.0:
            n = a.shape[0]
            rows = np.sort(np.random.default_rng(0).choice(n, max(1, int(n * keep)), replace=False))
            a = a[rows]
            np.save(os.path.join(out_dir, f"{name}_rows.npy"), rows.astype(np.float64))
        np.save(os.path.join(out_dir, f"{name}.npy"), np.ascontiguousarray(a))


LINE_TARGET_BYTES, LINE_LIMIT_BYTES = 4096, 8192


def _r(x, sig=5):
    """floats to `sig` significant digits (the line is a digest; bench_detail.json keeps full precision)"""
    if isinstance(x, (bool, np.bool_)):
        return bool(x)
    if isinstance(x, (int, np.integer)):
        return int(x)
    if isinstance(x, (float, np.floating)):
        x = float(x)
        if x != x or x in (float("inf"), float("-inf")):
            return None                      # strict JSON only
        return float(f"{x:.{sig}g}")
    return x


def secondary_key(row) -> str:
    """flat name of a secondary row: workload[_b<batch override>]_family_dtype[_polish][_hint]"""
    w = row["workload"].split(":")[0]
    fam = "" if row["family"] == "toward_robot" else "_" + row["family"]
    b = f"_b{row['batch']}" if row.get("batch_override") else ""
    return f"{w}{b}{fam}_{row['dtype']}" + ("_polish" if row.get("polish") else "") + ("_budget" if row.get("budget") else "") + \
        ("_hint" if row["dispatch"] != "index order" else "") + ("_nohint" if row.get("nohint") else "")


def accuracy_digest(acc) -> dict:
    """{workload_family: {comparison: {..}}}: the comparisons that carry the parity / accuracy statement, short keys.
      def_*   default tolerance: share of the pairs converged on both sides within the north star's 1e-4, max, same-status
              share -- HIP fp64 vs the oracle next to the oracle vs its re-associated twin (the noise floor);
      audit   first-divergence audit of the pairs > 1e-4 apart: how many, how many unexplained (HIP side / twin side);
      tight_* tolerance 1e-8: pairs converged on both sides (n), of which both end points are KKT points by the independent
              evaluator (kkt) and the largest |du| among THOSE; pairs > 1e-4 apart by kind: not_kkt (an end point is not
              stationary: penalty escalation), second_min (another local minimum, different cost), unexpl (must be 0);
      f32_fix / f32pol_fix   fp32 / fp32 + polish against the fp64 fixed point (tolerance 1e-8), converged instances;
      ret_f32pol             ALL returned instances (converged or not, same status) of fp32 + polish against fp64 + polish."""
    out = {}
    for row in acc.get("rows", []):
        d = {}
        for cmp_, short in (("hip64_vs_oracle64", "def_hip_orc"), ("oracle64_vs_reassociated", "def_orc_twin")):
            st = row.get(cmp_)
            if st and st.get("both_converged"):
                d[short] = {"n": st["both_converged"], "lt1e-4": _r(st["frac_lt_1e-4_both_converged"], 3),
                            "max": _r(st["max_abs_du_both_converged"], 2), "same_st": _r(st["same_status_frac"], 3)}
        if row.get("divergence_audit"):
            a = row["divergence_audit"]
            d["audit"] = {"far": a.get("n_far", a["n_pairs"]), "audited": a["n_pairs"], "unexpl": a["n_unexplained"],
                          "twin_unexpl": a["oracle_vs_reassociated"]["n_unexplained"]}
        for cmp_, short in (("tight_kkt_hip64_vs_oracle64", "tight_hip_orc"), ("tight_kkt_oracle64_vs_reassociated", "tight_orc_twin")):
            k = row.get(cmp_)
            if k and k["n_pairs"]:
                d[short] = {"n": k["n_pairs"], "kkt": k["n_both_kkt"], "kkt_max_du": _r(k["max_abs_du_both_kkt"], 2),
                            "not_kkt": k["n_not_kkt"], "second_min": k["n_second_kkt_point"], "unexpl": k["n_unexplained"]}
        for cmp_, short in (("hip32_vs_hip64_tight", "f32_fix"), ("hip32polish_vs_hip64_tight", "f32pol_fix")):
            st = row.get(cmp_)
            if st and st.get("n"):
                d[short] = {"n": st["n"], "lt1e-4": _r(st["frac_lt_1e-4"], 3), "med": _r(st["median_abs_du"], 2), "max": _r(st["max_abs_du"], 2)}
        st = row.get("all_returned_hip32polish_vs_hip64polish")
        if st and st["all"].get("n"):
            d["ret_f32pol"] = {"n": st["all"]["n"], "lt1e-4": _r(st["all"]["frac_lt_1e-4"], 3), "lt1e-3": _r(st["all"]["frac_lt_1e-3"], 3),
                               "conv_lt1e-4": _r(st["converged"].get("frac_lt_1e-4"), 3)}
        # (the line carries the families where a comparison is well posed: a good share converges; bench_detail.json has all)
        if d and row["family"] != "toward_robot":
            out[f"{row['workload']}_{row['family']}"] = d
    return out


def compact_line(detail: dict) -> str:
    """The ONE stdout line: driver keys, `roofline`, `cpu_baseline` and flat digests -- numbers, no prose. Optional parts
    are dropped (largest first) should the line ever exceed LINE_TARGET_BYTES; above LINE_LIMIT_BYTES is an error."""
    keep_cfg = ("workload", "family", "batch_per_gpu", "N_hor", "Ndynobs", "max_active_dynobs", "tail_handed_off", "Nstcobs", "Nother", "np", "dispatch",
                "sharding")
    keep_roof = ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "kernel_ms", "algorithmic_bytes_per_launch",
                 "valu_tflops", "valu_peak_tflops", "valu_frac", "psi_evals_per_solve", "flops_per_psi_eval")
    out = {k: _r(detail[k], 9) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
                                         "higher_is_better", "scaling", "vs_baseline", "dtype", "data")}
    out["config"] = {k: detail["config"][k] for k in keep_cfg if k in detail["config"]}
    out["roofline"] = {k: _r(detail["roofline"][k], 6) for k in keep_roof if k in detail["roofline"]}
    out["converged_frac"] = _r(detail["converged_frac"])
    out["converged_solves_per_s"] = _r(detail["converged_solves_per_s"])
    if "ranks" in detail:
        out["ranks"] = detail["ranks"]
        out["per_rank_ms"] = [_r(v, 6) for v in detail["per_rank_ms"]]
        out["per_rank_kernel_ms"] = [_r(v, 6) for v in detail["per_rank_kernel_ms"]]
        out["gather_ms"] = _r(detail["gather_ms"], 4)
        out["gather_bytes_per_rank"] = detail["gather_bytes_per_rank"]
    if "cpu_baseline" in detail:
        cb = detail["cpu_baseline"]
        out["cpu_baseline"] = {k: _r(cb[k]) for k in ("value", "unit", "cores", "kind", "sample", "single_core_value", "value_trig_hoisted",
                                                      "value_with_reference_time_cap", "value_with_evaluation_budget", "evals_per_s_per_core", "converged_frac",
                                                      "closed_loop_value", "open_probe")
                               if k in cb}
    if "secondary" in detail:
        out["secondary_solves_per_s"] = {secondary_key(r): _r(r["value"], 4) for r in detail["secondary"]}
        # the closed-loop distribution at the headline dimensions: which side of the north star's 1e5 it falls on, and how
        # much of it converges (the parity protocol on the same distribution: accuracy_summary.cfg2_closed_loop)
        for fam, key in (("refscen", "reference_scenarios"), ("closed_loop", "closed_loop")):
            cl = [r for r in detail["secondary"] if r["family"] == fam and not r.get("polish") and not r.get("budget")]
            bd = [r for r in detail["secondary"] if r["family"] == fam and r.get("budget")]
            if cl:
                out[key] = {"solves_per_s": _r(cl[0]["value"], 4), "converged_frac": _r(cl[0]["converged_frac"], 3),
                            "psi_evals_per_solve": _r(cl[0]["psi_evals_per_solve"], 4), "kernel_ms": _r(cl[0]["kernel_ms"], 4),
                            "capture_steps": list(HARVEST_STEPS[fam])}
                if bd:      # the same batch under the reference's time cap as an evaluation budget
                    out[key]["budget"] = {"max_evaluations": bd[0]["max_evaluations"], "solves_per_s": _r(bd[0]["value"], 4),
                                          "out_of_time_frac": _r(bd[0]["out_of_time_frac"], 3),
                                          "converged_frac": _r(bd[0]["converged_frac"], 3)}
    if "accuracy" in detail:
        out["accuracy_summary"] = accuracy_digest(detail["accuracy"])
    out["detail"] = "bench_detail.json"
    line = json.dumps(out, separators=(",", ":"), allow_nan=False)
    for victim in ("accuracy_summary", "secondary_solves_per_s"):
        if len(line) <= LINE_TARGET_BYTES or victim not in out:
            continue
        if victim == "accuracy_summary":        # first thin it out: the families where something converges, parity keys only
            out[victim] = {k: {q: v for q, v in d.items() if q in ("def_hip_orc", "def_orc_twin", "audit", "tight_hip_orc", "tight_orc_twin")}
                           for k, d in out[victim].items() if "toward_robot" not in k}
        else:
            del out[victim]
        line = json.dumps(out, separators=(",", ":"), allow_nan=False)
    if len(line) > LINE_LIMIT_BYTES:
        raise RuntimeError(f"bench line is {len(line)} bytes (> {LINE_LIMIT_BYTES}): the driver would not parse it")
    return line


def secondary_workloads(env: Env, args) -> list:
    """The other BASELINE configurations and the converging scenario family, one short timed run each."""
    # (workload, family, dtype, steps, warmup, dispatch hint, batch override, polish, note); note "budget" = the row runs with the
    # reference's 0.1 s time cap as an evaluation budget (nmpc_config.max_evaluations) -- secondary rows only
    runs = [("cfg2", "refscen", "f32", 2, 1, False, None, False,
             "BASELINE configs[2] as written -- main_eva.py scenarios: the reference's scenario_0..2 on its 55-polygon warehouse "
             "map (scenarios.make_reference_scenarios), 4 pedestrians x 10 hypotheses, parameter vectors harvested from the "
             "closed loop (row f3), a third each from time steps %s" % (REFSCEN_STEPS,)),
            ("cfg2", "refscen", "f32", 2, 0, False, None, False, "budget"),
            ("cfg2", "refscen", "f32", 2, 0, False, None, True, None),
            ("cfg2", "refscen", "f32", 5, 1, False, 6000, False,
             "the same family at three device fills: what a closed-loop evaluation sends once most of its scenarios have finished "
             "(resumable solve + tail hand-off from one fill on since round 6, profiles/r06_exp_mid_batches.txt)"),
            ("cfg2", "closed_loop", "f32", 2, 1, False, None, False,
             "round 5's builder-designed corridor family, harvested the same way at time steps %s" % (CLOSED_LOOP_STEPS,)),
            ("cfg2", "closed_loop", "f32", 2, 0, False, None, False, "budget"),
            ("cfg2", "toward_robot", "f32", 2, 0, False, None, False, "budget"),
            ("cfg2", "passing", "f32", 2, 1, False, None, False, None),
            ("cfg1", "toward_robot", "f32", 5, 1, False, None, False, None),
            ("cfg1", "toward_robot", "f32", 5, 1, False, None, False, "nohint"),
            ("cfg1", "passing", "f32", 5, 1, False, None, False, None),
            ("cfg1", "toward_robot", "f32", 2, 1, False, 65536, False,
             "the reference's shipped yaml dimensions (Ndynobs = 15, 2 x 5 hypotheses) at the batch size of configs[2]"),
            ("cfg4", "toward_robot", "f32", 1, 1, False, None, False, None),
            ("cfg4", "toward_robot", "f64", 1, 0, False, None, False, None),
            ("cfg2", "toward_robot", "f64", 1, 0, False, 16384, False, "configs[2] in fp64, a quarter of its batch"),
            # fp64 continuation of the converged instances (nmpc_config.polish): the throughput cost of fp64-grade answers
            ("cfg2", "passing", "f32", 2, 0, False, None, True, None),
            ("cfg1", "passing", "f32", 3, 0, False, None, True, None),
            # steady state of a receding-horizon loop: dispatch order from a previous pass (see run_workload)
            ("cfg2", "toward_robot", "f32", 2, 0, True, None, False, None),
            ("cfg2", "passing", "f32", 2, 0, True, None, False, None),
            ("cfg1", "toward_robot", "f32", 5, 0, True, None, False, None),
            ("cfg4", "toward_robot", "f32", 1, 0, True, None, False, None)]
    res = []
    for workload, family, dtype, steps, warmup, hint, batch, polish, note in runs:
        nohint, budget = note == "nohint", note == "budget"
        if workload == args.workload and family == args.family and dtype == args.dtype and not hint and not batch and not polish \
                and not budget:
            continue
        if nohint:
            note = "configs[1] WITHOUT the capacity hint: all 15 obstacle rows of the shipped yaml provisioned (6-slot register table since round 5; the 14-slot one before)"
        if budget:
            note = ("the same batch with the reference's time cap (max_solver_time = 0.1 s of its CPU solver) as the deterministic "
                    "evaluation budget nmpc_config.max_evaluations (solver.evaluation_budget): instances that use it up end "
                    "NotConvergedOutOfTime with the point they reached, as the reference's do -- never the headline")
        r = run_workload(env, workload, family, dtype, steps, warmup, batch=batch, dispatch_hint=hint, polish=polish,
                         capacity_hint=not nohint, budget=budget)
        r.pop("_host")
        r.pop("_gathered")
        res.append({"workload": r["config"]["workload"], "family": family, "dtype": dtype, "note": note,
                    "batch_override": bool(batch), "nohint": nohint, "budget": budget, "harvest": r["harvest"],
                    "max_evaluations": r["config"]["max_evaluations"], "out_of_time_frac": r["solver"]["out_of_time_frac"],
                    "max_active_dynobs": r["config"]["max_active_dynobs"],
                    "polish": r["polish"],
                    "psi_evals_per_solve": r["roofline"]["psi_evals_per_solve"],
                    "dispatch": r["config"]["dispatch"], "value": r["value"],
                    "unit": "solves/s", "ms_per_step": r["ms_per_step"], "steps": steps,
                    "batch": r["config"]["batch_per_gpu"], "kernel": r["roofline"]["kernel"],
                    "kernel_ms": r["roofline"]["kernel_ms"], "hbm_frac": r["roofline"]["frac"],
                    # measured HBM-side traffic of this workload's committed PMC passes (profiles/rNN_*_traffic.json) over
                    # this run's kernel time: the obstacle table of configs[4] is re-streamed on every evaluation, which
                    # makes that configuration -- and only that one -- memory bound
                    "traffic": r["roofline"]["traffic"],
                    "traffic_GBps": (r["roofline"]["traffic"] / (r["roofline"]["kernel_ms"] * 1e-3) / 1e9
                                     if r["roofline"]["traffic"] else None),
                    "valu_frac": r["roofline"]["valu_frac"], "converged_frac": r["solver"]["converged_frac"],
                    "converged_solves_per_s": r["solver"]["converged_solves_per_s"],
                    "inner_iters_mean": r["solver"]["inner_iters_mean"]})
    return res


def usable_cores() -> int:
    """Host cores this process may actually use: CPU affinity capped by the cgroup CPU quota."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    try:  # cgroup v2
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(float(quota) / float(period) + 0.5)))
    except (OSError, ValueError):
        try:  # cgroup v1
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            p = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                n = min(n, max(1, int(q / p + 0.5)))
        except (OSError, ValueError):
            pass
    return n


def probe_open() -> dict:
    """Is a genuine OpEn toolchain on this box (SURVEY.md 8c last row)? The reference's solver is
    generated by opengen (Python) + casadi and compiled by cargo; with all three present `tests/opengen_problem.py`
    builds the same problem with OpEn and the baseline below would be the real thing. Recorded either way."""
    import importlib.util
    import shutil
    found = {"cargo": shutil.which("cargo"), "rustc": shutil.which("rustc"),
             "opengen": importlib.util.find_spec("opengen") is not None,
             "casadi": importlib.util.find_spec("casadi") is not None}
    ok = bool(found["cargo"]) and found["opengen"] and found["casadi"]
    return {"available": ok, "found": found}


def cpu_baseline(layout, P_host):
    """The CPU oracle (kind "port": C restatement of the OpEn algorithm, fp64) on this box's host cores, on a bounded
    sample of the timed batch, all cores via OpenMP over instances. Reported, not tuned. If the box had cargo +
    opengen + casadi the genuine OpEn solver would be built and timed instead (kind "opengen")."""
    import oracle
    pr = oracle.Problem(layout.N, layout.Nother, layout.Nstc, layout.Ndyn)
    cores = usable_cores()
    probe = probe_open()
    if probe["available"]:
        try:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import opengen_problem
            return opengen_problem.time_genuine_open(layout, P_host, cores, probe)
        except Exception as exc:   # an OpEn build that fails must not take the bench line with it
            probe["build_error"] = repr(exc)[:300]
    sample = min(P_host.shape[0], 64 * cores)
    Ps = P_host[:sample]
    oracle.solve_batch(pr, oracle.Options(), Ps[:min(sample, cores)], nthreads=cores)   # warm the threads
    t0 = time.perf_counter()
    _, ro = oracle.solve_batch(pr, oracle.Options(), Ps, nthreads=cores)
    t_all = time.perf_counter() - t0
    n1 = min(sample, 16)
    t0 = time.perf_counter()
    _, r_one = oracle.solve_batch(pr, oracle.Options(), Ps[:n1], nthreads=1)
    t_one = time.perf_counter() - t0
    # the constant behind max_solver_time -> max_evaluations (solver.evaluation_budget): evaluated points per second of this
    # generated-code-equivalent CPU path on ONE core of this box, and the same in SURVEY 8(d)'s forward flops
    from dyobav_mpcnwta_warehouse_amd.solver import CPU_FORWARD_FLOPS_PER_S, evaluation_budget, forward_flops
    evals_per_s_core = float(r_one["n_points"].sum()) / t_one
    ff = forward_flops(layout.N, layout.Nother, layout.Nstc, layout.Ndyn)
    # the same sample with the ellipses' cos / sin hoisted out of the evaluations (orc_options.hoist_trig: once per solve, same
    # bits). The default recomputes them on every evaluation, as the reference's CasADi-generated code does; a hand-tuned CPU
    # solver would not -- VERDICT r3 called the plain figure pessimistic, so both are reported.
    t0 = time.perf_counter()
    oracle.solve_batch(pr, oracle.Options(hoist_trig=1), Ps, nthreads=cores)
    t_hoist = time.perf_counter() - t0
    # the same sample with the reference's own wall-clock cap per solve (max_solver_time = 0.1 s, mpc_builder.py:189)
    cap_s = 0.1
    t0 = time.perf_counter()
    _, rc = oracle.solve_batch(pr, oracle.Options(max_time_s=cap_s), Ps, nthreads=cores)
    t_cap = time.perf_counter() - t0
    # ... and with that cap in its deterministic form (orc_options.max_evals = nmpc_config.max_evaluations of the `_budget` rows)
    n_budget = evaluation_budget(REFERENCE_TIME_CAP_US, layout.N, layout.Nother, layout.Nstc, layout.Ndyn)
    t0 = time.perf_counter()
    _, rb = oracle.solve_batch(pr, oracle.Options(max_evals=n_budget), Ps, nthreads=cores)
    t_bud = time.perf_counter() - t0
    # ... and on the closed-loop distribution of the same dimensions (configs[2] only: BASELINE's "main_eva.py scenarios",
    # scenarios.harvest_closed_loop -- the GPU row next to it is secondary_solves_per_s.cfg2_closed_loop_f32)
    closed = None
    if layout.N == 20 and layout.Ndyn == 40:
        try:
            import dyobav_mpcnwta_warehouse_amd as nm
            cfg = nm.default_config_struct()
            cfg.Ndynobs, cfg.max_active_dynobs = layout.Ndyn, 40
            # (round 6: the reference's own scenarios -- the GPU row next to it is secondary_solves_per_s.cfg2_refscen_f32)
            Pc, _ = nm.scenarios.harvest_closed_loop(cfg, max(3 * sample // 2, 96), steps=REFSCEN_STEPS, seed=13, n_ped=4, n_hyp=10,
                                                     dtype=np.float32, family="reference")
            Pc = np.ascontiguousarray(Pc[:sample], dtype=np.float64)
            t0 = time.perf_counter()
            _, rcl = oracle.solve_batch(pr, oracle.Options(), Pc, nthreads=cores)
            t_cl = time.perf_counter() - t0
            closed = {"value": len(Pc) / t_cl, "scenarios": "reference (scenario_0..2 on the warehouse map)",
                      "sample": f"{len(Pc)} harvested instances, fp64, {t_cl:.1f} s wall",
                      "converged_frac": float(np.mean(rcl["status"] == 0))}
        except Exception as exc:      # (the harvest needs the device; the baseline of the timed batch above must survive without)
            closed = {"error": repr(exc)[:200]}
    return {"value": sample / t_all, "unit": "solves/s", "cores": cores, "kind": "port", "closed_loop": closed,
            "closed_loop_value": None if not closed else closed.get("value"),
            "note": "fp64 restatement run to its iteration caps: the reference's own solver would be cut off at its "
                    "max_solver_time (0.1 s per solve, mpc_builder.py:189) -- at %.0f ms per solve on one core most of "
                    "these solves would end NotConvergedOutOfTime there. Reported, not a target." % (1e3 * t_one / n1),
            "sample": f"first {sample} instances of the timed batch, fp64, {t_all:.1f} s wall",
            "single_core_value": n1 / t_one, "single_core_sample": f"first {n1} instances, 1 thread",
            "value_trig_hoisted": sample / t_hoist,
            "value_with_reference_time_cap": sample / t_cap,
            "evals_per_s_per_core": evals_per_s_core, "forward_flops_per_s_per_core": evals_per_s_core * ff,
            "budget_constant_forward_flops_per_s": CPU_FORWARD_FLOPS_PER_S,
            "value_with_evaluation_budget": sample / t_bud,
            "evaluation_budget": {"max_evals": n_budget, "wall_s": t_bud, "out_of_time_frac": float(np.mean(rb["status"] == 2)),
                                  "converged_frac": float(np.mean(rb["status"] == 0))},
            "reference_time_cap": {"max_solver_time_s": cap_s, "wall_s": t_cap,
                                   "out_of_time_frac": float(np.mean(rc["status"] == 2)),
                                   "converged_frac": float(np.mean(rc["status"] == 0))},
            "converged_frac": float(np.mean(ro["status"] == 0)),
            "open_probe": "unavailable" if not probe["available"] else "build failed", "open_probe_detail": probe}


def accuracy_table(env: Env) -> dict:
    """SURVEY.md 8(d) accuracy protocol on small seeded samples (tests/accuracy_protocol.py; the oracle is the checker).
    The -m gpu test tests/test_gpu_accuracy.py runs the same protocol on larger samples and asserts on it."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import accuracy_protocol
    import oracle
    cores = usable_cores()
    t0 = time.perf_counter()
    rows, skipped = [], []
    # the tightened-tolerance leg runs on the family where the solver converges (`passing`); on the contract family
    # almost every instance is infeasible and would burn the raised caps (2000 x 15 iterations) on the CPU side
    for workload in ("cfg2", "cfg1", "cfg4"):
        for family in ("passing", "toward_robot"):
            if time.perf_counter() - t0 > 110.0:            # keep the default bench run within minutes
                skipped.append(f"{workload}/{family}")
                continue
            full = family == "passing" and workload != "cfg4"
            rows.append(accuracy_protocol.run_case(env.nm, oracle, workload, family, nthreads=cores, tight=full, audit=full,
                                                   audit_max=12, tight_audit=False, n_tight=16 if workload == "cfg2" else 24))
            if workload == "cfg2" and family == "passing":
                # the same protocol on the closed-loop distribution at these dimensions (tests/test_gpu_closed_loop.py asserts
                # on a larger sample)
                lay = env.nm.scenarios.BENCH_CONFIGS["cfg2_b65536_n20_4x10"]["layout"]
                cfg = env.nm.default_config_struct()
                cfg.Ndynobs, cfg.max_active_dynobs = lay.Ndyn, 40
                Pc, _ = env.nm.scenarios.harvest_closed_loop(cfg, 96, steps=REFSCEN_STEPS, seed=13, n_ped=4, n_hyp=10, dtype=np.float32,
                                                             family="reference")
                rows.append(accuracy_protocol.run_case_on(env.nm, oracle, Pc[:32].astype(np.float64), lay, 40, "cfg2", "refscen",
                                                          nthreads=cores, tight=True, audit=True, audit_max=12, tight_audit=False,
                                                          n_tight=16))
    return {"protocol": "oracle64_vs_reassociated = the oracle's own noise floor (same fp64 algorithm, sums associated differently); "
                        "divergence_audit = iteration traces of every pair > 1e-4 apart laid side by side; "
                        "HIP fp64 vs oracle fp64 with the same Lipschitz-estimator step (1e-4) at default tolerance / caps "
                        "and (family `passing`, configs[1] and [2]; configs[4] in tests/test_gpu_accuracy.py) at tolerance 1e-8 with caps 2000 x 15; HIP fp32 vs HIP fp64; "
                        "|du| = max_i |u_i - u_ref_i| per instance", "rows": rows, "skipped_for_time": skipped,
            "seconds": time.perf_counter() - t0}


if __name__ == "__main__":
    main()
