#!/usr/bin/env python3
"""What one dynamic-window step costs on the device, rectangular rows against per-offset lists: HIP events around the call, the start
states, goals and node paths of the reference scenarios on the 55-rectangle warehouse map, pedestrians 1 .. 5 m around the robot.
   mode 2, H = 4                 nmpc_dwa_step_*        (rows read from global memory inside the point loop)
   lists, R = 4, full counts     nmpc_dwa_step_lists_*  (the same rows and results, staged in LDS)
   lists, R = 15 and R = 40      counts drawn from 0 .. R per offset (offset 0: 4 current positions)
Every figure is the median over `calls` calls; `repeats` repeats give the run-to-run spread.
   usage: bench_dwa_lists.py OUT.json [B] [f32|f64] [calls] [repeats]          (defaults 4096 f32 20 3)"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import dyobav_mpcnwta_warehouse_amd as nm
from dyobav_mpcnwta_warehouse_amd import _capi
from dyobav_mpcnwta_warehouse_amd.configs import DwaConfiguration

out_path = sys.argv[1]
B, dt, calls, repeats = (sys.argv[2:] + ["4096", "f32", "20", "3"][len(sys.argv) - 2:])[:4]
B, calls, repeats = int(B), int(calls), int(repeats)
dtype = np.float32 if dt == "f32" else np.float64
tdt = torch.float32 if dt == "f32" else torch.float64
N, CAP = 20, 55
rng = np.random.default_rng(7)
sc = nm.scenarios.make_reference_scenarios(B, seed=13, n_ped=4)
up = lambda x, t=tdt: torch.as_tensor(np.ascontiguousarray(x), dtype=t, device="cuda")
state = np.asarray(sc["robot_starts"], dtype=float)
paths = sc["robot_paths"]
pmax = max(len(p) for p in paths)
path = np.stack([np.array([tuple(q)[:2] for q in p] + [tuple(p[-1])[:2]] * (pmax - len(p)), dtype=float) for p in paths])
cfg = nm.default_config_struct()
h = nm.Handle(cfg)
h.set_stream(torch.cuda.current_stream().cuda_stream)
common = dict(state_c=up(state), last_u_c=up(np.stack([rng.uniform(0.1, 1.2, B), rng.uniform(-0.3, 0.3, B)], axis=1)),
              goal=up(np.array([p[-1][:2] for p in paths], dtype=float)), path=up(path), path_len=up([len(p) for p in paths], torch.long),
              polys=up(sc["map_polygons"]), U_c=torch.zeros(B, 2 * N, dtype=tdt, device="cuda"), min_cost=torch.zeros(B, dtype=tdt, device="cuda"),
              choice=torch.zeros(B, dtype=torch.int32, device="cuda"), counts=torch.zeros(B, 2, dtype=torch.int32, device="cuda"))


def rows(R):
    """[B, R, N+1, 6]: means that start 1 .. 5 m from the robot and drift at up to 1 m/s."""
    a = rng.uniform(0, 2 * np.pi, (B, R, 1))
    p0 = state[:, None, None, :2] + rng.uniform(1.0, 5.0, (B, R, 1, 1)) * np.stack([np.cos(a), np.sin(a)], axis=-1)
    d = np.zeros((B, R, N + 1, 6))
    d[..., :2] = p0 + 0.2 * np.arange(N + 1)[None, None, :, None] * rng.uniform(-1, 1, (B, R, 1, 2))
    return d


def measure(args, call):
    for k, v in common.items():
        setattr(args, k, v.data_ptr())
    args.B, args.n_run, args.M, args.Pmax, args.cap = B, B, int(sc["map_polygons"].shape[0]), pmax, CAP
    for _ in range(3):
        call(dtype, args)
    torch.cuda.synchronize()
    med = []
    for _ in range(repeats):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
        for e0, e1 in ev:
            e0.record()
            call(dtype, args)
            e1.record()
        torch.cuda.synchronize()
        med.append(float(np.median([e0.elapsed_time(e1) for e0, e1 in ev])))
    return dict(ms_median_per_repeat=med, ms=float(np.median(med)), spread_ms=max(med) - min(med), finite_choices=int((common["choice"] >= 0).sum()))


rec = {"what": "one dynamic-window step, HIP events around the call", "B": B, "dtype": dt, "calls_per_repeat": calls, "repeats": repeats,
       "device": torch.cuda.get_device_name(0), "map_rectangles": int(sc["map_polygons"].shape[0]), "candidates_cap": CAP}
d4 = up(rows(4))
a = _capi.NmpcDwaArgs().set_config(DwaConfiguration(), 0.8)
a.H, a.dyn_mode, a.dyn_c = 4, 2, d4.data_ptr()
rec["mode2_H4"] = measure(a, h.dwa_step)
keep = common["U_c"].clone()
for name, R, full in (("lists_R4_full", 4, True), ("lists_R15_unequal", 15, False), ("lists_R40_unequal", 40, False)):
    d = d4 if full else up(rows(R))
    cnt = np.full((B, N + 1), R) if full else rng.integers(0, R + 1, (B, N + 1))
    cnt[:, 0] = 4
    cnt = up(cnt, torch.int32)
    a = _capi.NmpcDwaListsArgs().set_config(DwaConfiguration(), 0.8)
    a.R, a.dyn_c, a.dyn_count = R, d.data_ptr(), cnt.data_ptr()
    rec[name] = measure(a, h.dwa_step_lists)
    rec[name]["mean_count_per_offset"] = float(cnt[:, 1:].float().mean())
    if full:
        rec[name]["same_controls_as_mode2"] = bool(torch.equal(keep, common["U_c"]))
h.close()
with open(out_path, "w") as f:
    json.dump(rec, f, indent=1)
print(json.dumps({k: (v["ms"], v["spread_ms"]) for k, v in rec.items() if isinstance(v, dict)}))
