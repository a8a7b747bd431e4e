#!/usr/bin/env python3
"""The closed loop on the reference scenarios with the dynamic-window baseline tracker (tools/bench_evaluate.py --tracker dwa,
a fresh process per predictor) and one record of what its stage (nmpc_dwa_step_*) costs -- HIP events around every call: ms
per lock-step, scenario-steps/s -- next to the outcome rates and the four main_pre metrics, with the MPC rows of
profiles/kf_evaluate_refscen.json (same scenarios, seeds and batch size) beside them.
   usage: dwa_evaluate_profile.py OUT.json [B] [max_steps] [f32|f64] [n_ped] [predictors]     (defaults 65536 120 f32 4 cvmp)"""
import json, os, subprocess, sys

HERE = os.path.dirname(os.path.abspath(__file__))
out = sys.argv[1]
B, steps, dt, n_ped, preds = (sys.argv[2:] + ["65536", "120", "f32", "4", "cvmp"][len(sys.argv) - 2:])[:5]
rec = {"what": "closed loop (row f3) on the reference scenarios, dynamic-window baseline tracker", "B": int(B), "max_steps": int(steps), "dtype": dt,
       "n_ped": int(n_ped), "dwa": {}}
for predictor in preds.split(","):
    p = subprocess.run([sys.executable, os.path.join(HERE, "bench_evaluate.py"), "--tracker", "dwa", "--predictor", predictor, B, steps, dt, n_ped, "1"],
                       capture_output=True, text=True, env=dict(os.environ, FAMILY="reference"))
    if p.returncode != 0:
        sys.exit(f"bench_evaluate.py --tracker dwa --predictor {predictor} failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    r = json.loads(p.stdout.strip().splitlines()[-1])
    rec["workload"] = r["config"]["workload"]
    rec["dwa"][predictor] = {"scenario_steps_per_s": r["value"], "wall_s": r["wall_s"], "lockstep_steps": r["lockstep_steps"], "dwa_stage": r["tracker_stage"],
                             "complete_rate": r["complete_rate"], "collision_rate": r["collision_rate"], "mean_steps": r["mean_steps"],
                             "metrics_of_successful_runs": r["metrics_of_successful_runs"], "by_scenario": r["by_scenario"]}
kf = os.path.join(os.path.dirname(HERE), "profiles", "kf_evaluate_refscen.json")
if os.path.exists(kf):
    with open(kf) as f:
        k = json.load(f)
    rec["mpc_rows_of_kf_evaluate_refscen"] = {"workload": k.get("workload"), "B": k.get("B"), "max_steps": k.get("max_steps"), "cvmp": k.get("cvmp"), "kfmp": k.get("kfmp")}
with open(out, "w") as f:
    json.dump(rec, f, indent=1)
print(json.dumps({p: {k: v for k, v in rec["dwa"][p]["dwa_stage"].items() if k != "per_step"} for p in rec["dwa"]}))
