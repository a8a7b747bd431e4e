#!/usr/bin/env python3
"""The closed loop on the reference scenarios with both predictors the reference can run without network weights, one after
the other with the same seeds: tools/bench_evaluate.py --predictor cvmp and --predictor kfmp (a fresh process each), and
one record of what the Kalman-filter stage (nmpc_kf_predict_*) costs -- HIP events around every call: per-step
milliseconds at the first and the last lock-step, its share of the step and of the run -- next to solves/s, exit-status
counts and the four main_pre metrics of both runs.
   usage: kf_evaluate_profile.py OUT.json [B] [max_steps] [f32|f64] [n_ped]        (defaults 65536 120 f32 4)"""
import json, os, subprocess, sys

HERE = os.path.dirname(os.path.abspath(__file__))
out = sys.argv[1]
B, steps, dt, n_ped = (sys.argv[2:] + ["65536", "120", "f32", "4"][len(sys.argv) - 2:])[:4]
runs = {}
for predictor in ("cvmp", "kfmp"):
    p = subprocess.run([sys.executable, os.path.join(HERE, "bench_evaluate.py"), "--predictor", predictor, B, steps, dt, n_ped, "1"],
                       capture_output=True, text=True, env=dict(os.environ, FAMILY="reference"))
    if p.returncode != 0:
        sys.exit(f"bench_evaluate.py --predictor {predictor} failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    runs[predictor] = json.loads(p.stdout.strip().splitlines()[-1])


def summary(r):
    ps = r["per_step"]
    tot = {k: sum(s[k] for s in ps) for k in ("converged", "out_of_iterations", "out_of_time")}
    solves = sum(s["running"] for s in ps)
    return {"scenario_steps_per_s": r["value"], "wall_s": r["wall_s"], "lockstep_steps": r["lockstep_steps"],
            "solves": solves, "solves_per_s_in_the_solve_kernels": solves / (r["solve_kernel_ms_total"] * 1e-3),
            "solve_kernel_ms_total": r["solve_kernel_ms_total"], "solve_ms_first_step": ps[0]["solve_ms"], "solve_ms_last_step": ps[-1]["solve_ms"],
            "exit_status_counts": tot, "complete_rate": r["complete_rate"], "collision_rate": r["collision_rate"], "mean_steps": r["mean_steps"],
            "metrics_of_successful_runs": r["metrics_of_successful_runs"]}


st = runs["kfmp"]["predictor_stage"]
kf_ps, ms = runs["kfmp"]["per_step"], st["ms_per_step"]
rec = {"what": "closed loop (row f3) on the reference scenarios, constant-velocity against Kalman-filter predictor, same seeds",
       "workload": runs["kfmp"]["config"]["workload"], "dtype": runs["kfmp"]["dtype"], "B": int(B), "max_steps": int(steps), "n_ped": int(n_ped),
       "kf_stage": {k: st[k] for k in st if k != "ms_per_step"},
       "kf_stage_per_step": [{"step": s["step"], "running": s["running"], "kf_ms": m, "solve_ms": s["solve_ms"]} for s, m in zip(kf_ps, ms)],
       "cvmp": summary(runs["cvmp"]), "kfmp": summary(runs["kfmp"])}
with open(out, "w") as f:
    json.dump(rec, f, indent=1)
print(json.dumps({k: rec[k] for k in ("workload", "kf_stage")}))
