#!/usr/bin/env python3
"""Measurement of the snap kernel (predictor hypotheses in pixels -> world points, csrc/nmpc_snap.h) on the warehouse map of
tests/golden/snap_map.npz: one JSON line with, for a batch with a third of the points in occupied cells and for the
reference-like share (uniform over the map, ~9 %): kernel milliseconds by HIP events, in-point x edge-pixel pairs per
second, the share of the fp64 VALU issue bound that is (static instruction count of the pair loop x pairs over the issue
rate: a MODEL, the count is read off the ISA), and the f2 kernel's time on the snapped tensor beside it. With HOSTHOP=<B>
also the host hop the stage replaces at that batch: .cpu(), tests/snap_reference.py, .cuda().

usage: bench_snap.py [B=65536] [steps=10] [n_ped=4] [n_hyp=10] [f32|f64]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import dyobav_mpcnwta_warehouse_amd as nm
from dyobav_mpcnwta_warehouse_amd.snap import WorldTransform

B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
n_ped, K = (int(v) for v in sys.argv[3:5]) if len(sys.argv) > 4 else (4, 10)
dt = np.float64 if (len(sys.argv) > 5 and sys.argv[5] == "f64") else np.float32
tdt = torch.float64 if dt == np.float64 else torch.float32
N, Ndyn = 20, 15
# VALU instructions per (in-point, edge pixel) in the pair loop of snap_walk<4> (gfx950 ISA of this build: 2 subtract,
# 2 multiply, 1 add, the IEEE division = 2 v_div_scale + v_rcp_f64 + 6 fma/mul + v_div_fmas + v_div_fixup, 2 compares,
# 3 v_cndmask, and a quarter of the pixel's unpack + 2 conversions) and the fp64 issue rate: one wave instruction per 4
# cycles per SIMD (78.6 TFLOPS fp64 vector spec = 256 CUs x 4 SIMDs x 16 lanes x 2 x 2.4 GHz); v_rcp_f64 takes 4 slots
INSTR_PER_PAIR = 5 + 11 + 3 + 5 + 1
PEAK_WAVE_INSTR = 256 * 4 * 2.4e9 / 4

z = np.load(os.path.join(ROOT, "tests", "golden", "snap_map.npz"))
H, W = (int(v) for v in z["shape"])
occupied = np.unpackbits(z["occupied_bits"])[:H * W].reshape(H, W).astype(bool)
edge = np.unpackbits(z["edge_bits"])[:H * W].reshape(H, W).astype(bool)
tf = WorldTransform(0.1, -15.0, -15.0, False, True, 0.0, float(H))
cfg = nm.default_config_struct(); cfg.N_hor, cfg.Ndynobs = N, Ndyn
h = nm.Handle(cfg); h.set_stream(torch.cuda.current_stream().cuda_stream)
h.set_map(occupied, edge)
g = torch.Generator(device="cuda").manual_seed(0)
occ_rc = torch.from_numpy(np.argwhere(occupied)).cuda()


def batch(Bn, share_from_occupied):
    """points uniform over the map, a share of them redrawn from occupied cells"""
    shape = (Bn, N, n_ped * K)
    col = torch.rand(shape, generator=g, device="cuda", dtype=torch.float64) * W
    row = torch.rand(shape, generator=g, device="cuda", dtype=torch.float64) * H
    if share_from_occupied > 0:
        pick = torch.rand(shape, generator=g, device="cuda") < share_from_occupied
        j = torch.randint(len(occ_rc), shape, generator=g, device="cuda")
        frac = torch.rand(shape + (2,), generator=g, device="cuda", dtype=torch.float64)
        col = torch.where(pick, occ_rc[j, 1] + frac[..., 0], col)
        row = torch.where(pick, occ_rc[j, 0] + frac[..., 1], row)
    return torch.stack([col, row], dim=-1).to(tdt).contiguous()


def measure(name, share_from_occupied):
    raw = batch(B, share_from_occupied)
    out = torch.empty_like(raw)
    n_sn = torch.empty(B, N, n_ped, dtype=torch.int32, device="cuda")
    snap = lambda: h.snap_hypotheses(dt, raw, out, n_ped, K, tf, 1.0, n_sn)
    for _ in range(2): snap()
    torch.cuda.synchronize(); ms = []
    for _ in range(steps):
        snap(); torch.cuda.synchronize(); ms.append(h.last_kernel_ms())
    n_in = int(n_sn.sum())
    pairs = n_in * int(edge.sum())
    k_ms = float(np.mean(ms))
    cur = out[:, 0].reshape(B, n_ped, K, 2).mean(dim=2).contiguous()
    dyn = torch.empty(B, Ndyn, N + 1, 6, dtype=tdt, device="cuda")
    f2 = lambda: h.hypotheses_to_ellipses(dt, out, cur, dyn)
    for _ in range(2): f2()
    torch.cuda.synchronize(); f2ms = []
    for _ in range(steps):
        f2(); torch.cuda.synchronize(); f2ms.append(h.last_kernel_ms())
    rate = pairs / (k_ms * 1e-3)
    return {"case": name, "share_in": n_in / (B * N * n_ped * K), "kernel_ms": k_ms, "kernel_ms_min": float(np.min(ms)),
            "kernel_ms_max": float(np.max(ms)), "pairs": pairs, "pairs_per_s": rate,
            "bound": {"name": "fp64 VALU issue (model: static instruction count x pairs / issue rate)",
                      "instr_per_pair": INSTR_PER_PAIR, "peak_wave_instr_per_s": PEAK_WAVE_INSTR,
                      "frac": rate / 64 * INSTR_PER_PAIR / PEAK_WAVE_INSTR},
            "f2_kernel_ms": float(np.mean(f2ms))}


res = {"metric": "snap kernel (pixels -> world points, device-side)", "n_gpus": 1, "steps": steps, "dtype": "f64" if dt == np.float64 else "f32",
       "config": {"workload": f"B={B}, N={N}, {n_ped} pedestrians x {K} hypotheses, warehouse map {H}x{W}, {int(edge.sum())} edge pixels"},
       "variant": "plain IEEE division per pair (the near-tie shortcut is not built)",
       "cases": [measure("third_in", 1.0 / 3.0), measure("reference_like", 0.0)]}
hop = int(os.environ.get("HOSTHOP", "0"))
if hop:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import snap_reference as sr
    raw = batch(hop, 1.0 / 3.0)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    host = raw.cpu().numpy()
    t1 = time.perf_counter()
    world, _, _ = sr.snap(host, n_ped, K, occupied, edge, tf)
    t2 = time.perf_counter()
    back = torch.from_numpy(world.astype(dt)).cuda(); torch.cuda.synchronize()
    t3 = time.perf_counter()
    out = torch.empty_like(raw)
    h.snap_hypotheses(dt, raw, out, n_ped, K, tf); torch.cuda.synchronize()
    h.snap_hypotheses(dt, raw, out, n_ped, K, tf); torch.cuda.synchronize()
    res["host_hop"] = {"B": hop, "to_host_ms": (t1 - t0) * 1e3, "numpy_restatement_ms": (t2 - t1) * 1e3, "to_device_ms": (t3 - t2) * 1e3,
                       "device_kernel_ms_same_batch": h.last_kernel_ms(), "same_result": bool(torch.equal(back, out))}
print(json.dumps(res))
