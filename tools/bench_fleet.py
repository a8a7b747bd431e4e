#!/usr/bin/env python3
"""What the fleet stage costs beside the solve, and what coupling does to the robot-robot collisions: the closed loop on
reference-scenario fleets (``scenarios.make_fleet_scenarios``) with ``BatchEvaluator(fleet=R)``, HIP events around every
``nmpc_fleet_exchange_*`` and ``nmpc_fleet_post_*`` call (``time_fleet``) next to the solve's own kernel time of the same step.

Per (G, R) two runs with the same seeds: coupled and ``fleet_coupling=False`` (the epilogue only). Reported per run: wall time,
per step the two kernels' milliseconds against the solve's, their totals and share of the wall time, and how many of the
collisions are robot-robot. The yardstick is the project's own for a stage beside the solve (the Kalman stage: 5 % of the run).

   usage: bench_fleet.py OUT.json [B] [max_steps] [f32|f64] [GxR ...]        (defaults 65536 120 f32 8192x8 1024x64)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dyobav_mpcnwta_warehouse_amd as nm  # noqa: E402
from dyobav_mpcnwta_warehouse_amd.evaluate import BatchEvaluator  # noqa: E402


def one_run(G, R, dtype, max_steps, coupling, n_ped=4):
    import torch
    sc = nm.scenarios.make_fleet_scenarios(G, R, seed=13, n_ped=n_ped)
    sc.pop("scenario_index")
    sc.pop("group")
    ev = BatchEvaluator(nm.default_config_struct(), dtype=dtype, predictor="cvmp", human_stagger=nm.scenarios.HUMAN_STAGGER, seed=13,
                        fleet=R, fleet_coupling=coupling, **sc)
    ev.time_fleet = True
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = ev.run(max_steps=max_steps)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    ms = ev.fleet_ms
    ev.close()
    ex, po, so = ms.get("exchange", []), ms["post"], res.solve_ms
    steps = len(so)
    rec = {"G": G, "R": R, "B": G * R, "coupled": bool(coupling), "lockstep_steps": steps, "wall_s": wall,
           "solve_kernel_ms_total": float(sum(so)), "exchange_ms_total": float(sum(ex)), "post_ms_total": float(sum(po)),
           "exchange_share_of_wall_time": float(sum(ex)) * 1e-3 / wall, "post_share_of_wall_time": float(sum(po)) * 1e-3 / wall,
           "exchange_ms_first_step": ex[0] if ex else None, "exchange_ms_max": max(ex) if ex else None,
           "exchange_over_solve_max": max(e / s for e, s in zip(ex, so)) if ex else None,
           "post_ms_first_step": po[0], "post_ms_max": max(po), "post_over_solve_max": max(p / s for p, s in zip(po, so)),
           "collisions": int(res.collision.sum()), "collisions_robot_robot": int(res.collision_fleet.sum()),
           "complete": int(res.complete.sum()), "mean_steps": float(res.steps.mean()),
           "clearance_fleet_median": float(np.median(res.clearance_fleet[np.isfinite(res.clearance_fleet)])),
           "per_step": [{"step": k, "solve_ms": so[k], "exchange_ms": ex[k] if ex else None, "post_ms": po[k]} for k in range(steps)]}
    return rec


def main():
    out = sys.argv[1]
    B, steps, dt = (sys.argv[2:5] + ["65536", "120", "f32"][len(sys.argv[2:5]):])
    shapes = [tuple(int(v) for v in s.split("x")) for s in sys.argv[5:]] or [(int(B) // 8, 8), (int(B) // 64, 64)]
    dtype = np.float32 if dt == "f32" else np.float64
    runs = []
    for G, R in shapes:
        for coupling in (True, False):
            r = one_run(G, R, dtype, int(steps), coupling)
            print(json.dumps({k: v for k, v in r.items() if k != "per_step"}), flush=True)
            runs.append(r)
    rec = {"what": "closed loop on reference-scenario fleets: the fleet exchange and epilogue beside the solve, coupled against uncoupled",
           "workload": f"B = G x R fleets of make_fleet_scenarios(seed 13, 4 pedestrians per group), <= {steps} steps, default configuration "
                       f"(mpc_fast.yaml dimensions), predictor cvmp, stagger 0.5", "dtype": dt, "runs": runs}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
