#!/usr/bin/env python3
"""The closed loop on the reference scenarios with the multi-hypothesis predictor (``BatchEvaluator(predictor="mmp")``) and a
record of what its stage costs: HIP events around the whole stage, around each of its parts (input stack, network, snap, f2)
and the solve kernel's own time, per lock-step; and the input kernel (nmpc_mmp_input_*) alone on one full chunk, as achieved
write bandwidth next to the two rates it can be held against -- the float4 copy rate of the device (6.29 TB/s) and what f1,
the other store-bound kernel of the time step, was recorded at (5.6 TB/s).

The network is a randomly initialised module with the layer shapes of the reference's ``ConvMultiHypoNet(lite=True)`` (7 x 7
stem with 64 channels, 3 x 3 max-pool, residual stages of 3 / 4 / 6 / 3 basic blocks with 16 / 32 / 64 / 128 channels, 2 x 2
average pool, 3200 -> 128 -> 2 K), written here: the trained weights are not available, so its hypotheses mean nothing and
only its cost is of interest. The map is the warehouse label image of tests/golden/snap_map.npz.
   usage: mmp_evaluate_profile.py OUT.json [B] [steps] [f32|f64] [n_ped] [n_hyp]        (defaults 256 3 f32 4 20)"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

import dyobav_mpcnwta_warehouse_amd as nm  # noqa: E402
from dyobav_mpcnwta_warehouse_amd.evaluate import MMP_SIGMA, BatchEvaluator  # noqa: E402
from dyobav_mpcnwta_warehouse_amd.snap import WorldTransform  # noqa: E402

COPY_TBS, F1_TBS = 6.29, 5.6


def conv(cin, cout, k, stride, pad, act=True):
    layers = [torch.nn.Conv2d(cin, cout, k, stride, pad, bias=False), torch.nn.BatchNorm2d(cout)]
    return torch.nn.Sequential(*(layers + ([torch.nn.LeakyReLU(0.1, inplace=True)] if act else [])))


class Block(torch.nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.a, self.b = conv(cin, cout, 3, stride, 1), conv(cout, cout, 3, 1, 1, act=False)
        self.skip = None if stride == 1 and cin == cout else torch.nn.Sequential(torch.nn.Conv2d(cin, cout, 1, stride, bias=False),
                                                                                 torch.nn.BatchNorm2d(cout))
        self.act = torch.nn.LeakyReLU(inplace=True)

    def forward(self, x):
        return self.act(self.b(self.a(x)) + (x if self.skip is None else self.skip(x)))


def make_network(K, fc_input=3200):
    layers, cin = [conv(7, 64, 7, 2, 3), torch.nn.MaxPool2d(3, 2, 1)], 64
    for n, c, s in ((3, 16, 1), (4, 32, 2), (6, 64, 2), (3, 128, 2)):
        for i in range(n):
            layers.append(Block(cin, c, s if i == 0 else 1))
            cin = c
    layers += [torch.nn.AvgPool2d(2, 2), torch.nn.Flatten(), torch.nn.Linear(fc_input, 128), torch.nn.LeakyReLU(inplace=True),
               torch.nn.Linear(128, 2 * K)]
    return torch.nn.Sequential(*layers)


def input_kernel_rate(ev, n_item, reps=20):
    """ms and GB/s of nmpc_mmp_input_* alone on ``n_item`` pedestrians of the evaluator's start state."""
    out = torch.empty(n_item, ev.N, 7, ev.mmp_Hm, ev.mmp_Wm, dtype=torch.float32, device=ev.dev)
    a = nm._capi.NmpcMmpArgs().set_transform(ev.mmp_tf, ev.mmp_rescale, MMP_SIGMA)
    a.B, a.H, a.n_item, a.n_off, a.Hm, a.Wm = ev.B, ev.H, n_item, ev.N, ev.mmp_Hm, ev.mmp_Wm
    hist, hcount = ev.hist.contiguous(), ev.hcount.contiguous()
    a.hist, a.hcount, a.ref_image, a.out = hist.data_ptr(), hcount.data_ptr(), ev.mmp_ref.data_ptr(), out.data_ptr()
    ms = []
    for i in range(5 + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ev.h.mmp_input(ev.dt, a)
        e1.record()
        torch.cuda.synchronize()
        if i >= 5:
            ms.append(e0.elapsed_time(e1))
    nbytes = out.numel() * 4
    med = float(np.median(ms))
    return {"items": n_item, "bytes_written": nbytes, "ms_median": med, "ms_min": float(min(ms)), "write_GBps_median": nbytes / med * 1e-6,
            "write_GBps_best": nbytes / min(ms) * 1e-6, "share_of_copy_rate": nbytes / med * 1e-9 / COPY_TBS, "share_of_f1_rate": nbytes / med * 1e-9 / F1_TBS}


def main():
    out_path = sys.argv[1]
    B, steps, dt, n_ped, K = (sys.argv[2:] + ["256", "3", "f32", "4", "20"][len(sys.argv) - 2:])[:5]
    B, steps, n_ped, K = int(B), int(steps), int(n_ped), int(K)
    z = np.load(os.path.join(ROOT, "tests", "golden", "snap_map.npz"))
    Hm, Wm = (int(v) for v in z["shape"])
    occupied = np.unpackbits(z["occupied_bits"])[:Hm * Wm].reshape(Hm, Wm).astype(bool)
    ref = np.where(occupied, 0.0, 255.0).astype(np.float32)
    tf = WorldTransform(scale=0.1, offsetx_after=-15.0, offsety_after=-15.0, y_reverse=True, y_max_before=float(Hm))
    sc = nm.scenarios.make_reference_scenarios(B, n_ped=n_ped)
    sc.pop("scenario_index")
    torch.manual_seed(0)
    net = make_network(K).cuda().eval()
    ev = BatchEvaluator(nm.default_config_struct(), dtype=np.float32 if dt == "f32" else np.float64, predictor="mmp",
                        network=lambda x: net(x) + 150.0, mmp_hyp=K, ref_image=ref, transform=tf, **sc)
    rec = {"what": "closed loop (row f3) on the reference scenarios with the multi-hypothesis predictor stage; random network of the "
                   "reference's layer shapes", "B": B, "n_ped": n_ped, "n_hyp": K, "dtype": dt, "max_steps": steps, "map": [Hm, Wm],
           "chunk_pedestrians": ev.mmp_chunk, "network_parameters": sum(p.numel() for p in net.parameters()),
           "compared_with": {"float4_copy_TBps": COPY_TBS, "f1_recorded_TBps": F1_TBS}}
    rec["input_kernel"] = input_kernel_rate(ev, min(ev.mmp_chunk, B * n_ped))
    print(json.dumps(rec["input_kernel"]), flush=True)
    with open(out_path, "w") as f:                          # (kept even if the run below does not finish)
        json.dump(rec, f, indent=1)
    ev.time_predictor = ev.time_predictor_parts = True
    try:
        res = ev.run(max_steps=steps)
    finally:
        ev.close()
    parts = ev.predictor_part_ms
    rec["per_step"] = [dict(step=t, stage_ms=ev.predictor_ms[t], solve_ms=res.solve_ms[t], **{k: v[t] for k, v in parts.items()})
                       for t in range(len(ev.predictor_ms))]
    rec["n_obs_max"], rec["n_outside_total"] = int(res.n_obs.max()), int(res.n_outside[res.n_outside > 0].sum())
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec["per_step"]))


if __name__ == "__main__":
    main()
