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

``--fused-stem``: the same network split by hand into its first layer (``mmp_stem.fold_stem``: convolution, norm, LeakyReLU,
max-pool -> ``nmpc_mmp_stem_*``) and the trunk behind it; the parent path (input stack + whole network) and the fused path
(fused first layer + trunk) run in the same process on the same device, alternately, with HIP events around ``input``,
``network`` and the whole stage of every lock-step; the medians over the alternated repetitions are compared. Beside them: the
fused kernel alone on one chunk as bytes stored per second against the float4 copy rate, and torch's own first layer alone on
one chunk of the parent path -- the share of the network's time that the first layer is.

``--fused-layer1``: one step further. The parent path is the fused first layer with the whole trunk in torch (the fused path of
``--fused-stem``); the new path hands the first residual stage (three blocks at 16 channels, ``mmp_stem.fold_block`` ->
``nmpc_mmp_block_f32``) to the device stage as well and keeps the trunk from the second stage on. Alternated as above, with HIP
events around ``input``, ``layer1``, ``network`` and the whole stage. Beside them: torch's own layer1, eager, alone on one chunk
of the parent path's stem output (the time the three block launches have to beat, and its share of the parent's network time),
and the block kernels alone on one chunk as fma per second against the fp32 peak and bytes per second against the copy rate.

``--fused-layer2``: one step further again. The parent path is the new path of ``--fused-layer1`` (fused first layer and layer1,
trunk from layer2 on in torch); the new path hands the second residual stage (four blocks at 32 channels, the first at stride 2,
``mmp_stem.fold_block2`` -> ``nmpc_mmp_block2_f32``) to the device stage as well and keeps the trunk from layer3 on. Alternated as
above, with HIP events around ``input``, ``layer1``, ``layer2``, ``network`` and the whole stage. Beside them: torch's own layer2,
eager, alone on one chunk of the parent path's layer1 output, and the four launches alone on one chunk as fma per second against
the fp32 peak and bytes per second against the copy rate, next to the model of csrc/nmpc_mmp_block2.h.

``--fused-layer3``: and once more. The parent path is the new path of ``--fused-layer2`` (trunk from layer3 on in torch); the new
path hands the third residual stage (six blocks at 64 channels, the first at stride 2, ``mmp_stem.fold_block3`` ->
``nmpc_mmp_block3_f32``) to the device stage as well and keeps the trunk from layer4 on. Alternated as above, with HIP events
around ``input``, ``layer1``, ``layer2``, ``layer3``, ``network`` and the whole stage. Measured first: torch's own layer3, eager,
alone on one chunk of the parent path's layer2 output; then the six launches alone on that chunk, next to the model of
csrc/nmpc_mmp_block3.h.

``--fused-layer4``: the last step. The parent path is the new path of ``--fused-layer3`` (trunk from layer4 on in torch); the new
path is ``mmp_stem.split_network_whole``: the fourth residual stage (three blocks at 128 channels, ``nmpc_mmp_block4_f32``) and
the pool with both linear layers (``nmpc_mmp_head_f32``) on the device as well, and NO torch module in the stage. Alternated as
above, with HIP events around ``input``, ``layer1`` .. ``layer4``, ``head`` / ``network`` and the whole stage. Measured first:
torch's own layer4 and its pool and linear layers, eager, each alone on one chunk of the parent path's layer3 output; then the
three block launches and the head launch alone on that chunk, next to the model of csrc/nmpc_mmp_block4.h.

``--half-layer4``: the protocol of ``--half-layer3`` for layer4 on binary16 operands (``nmpc_mmp_block4_f16``). Both arms run layer3
on binary16 operands, which this option does not touch: ``mmp_half=("layer3",)`` -- layer4 by the float32 launches -- against
``mmp_half=("layer3", "layer4")``, alternated in one process: the three launches alone on one chunk, then the closed loop.
``--half-layer2``: the same protocol for layer2 on binary16 operands (``nmpc_mmp_block2_f16``), both arms with layer3 and layer4 on
them: ``mmp_half=("layer3", "layer4")`` against the same with ``mmp_operands={"layer2": "f16"}``; the four launches alone, then the loop.
``--activations-f16``: the same protocol for binary16 activations in memory (``nmpc_mmp_block{2,3,4}_f16_io``), both arms with layer2,
layer3 and layer4 on binary16 operands: ``mmp_activations="f32"`` (the parent's path) against ``"f16"``; the 13 launches alone per run
and per block, then the loop; the record holds both arms' run-to-run spreads and whether the f16 arm is faster by more than the
larger of them in every run.
``--half-layer1``: the same protocol for layer1 on binary16 operands (``nmpc_mmp_block_f16``): ``parent`` -- layer2 .. layer4 on binary16
operands with ``mmp_activations="f16"``, layer1 on float32 -- against ``mmp_precision="f16"``; the 16 launches alone per run and per block,
then the loop; the record holds layer1's three launches and the stage of each run, the spreads and both merge conditions.
``--fill-f16``: the same protocol for the fused first layer writing binary16 (``nmpc_mmp_stem_io_*``): ``parent`` -- ``mmp_precision="f16"``
-- against the same with ``mmp_fill="f16"``; the fill's launch and the 16 block launches alone per run, then the loop; the record holds
every part, every block of layer1 and the stage of each run, the stage's spreads and both merge conditions.
   usage: mmp_evaluate_profile.py OUT.json [B] [steps] [f32|f64] [n_ped] [n_hyp]
          [--fused-stem [REPS] | --fused-layer1 [REPS] | --fused-layer2 [REPS] | --fused-layer3 [REPS] | --fused-layer4 [REPS] | --half-layer3 [REPS]
           | --half-layer4 [REPS] | --half-layer2 [REPS] | --activations-f16 [REPS] | --half-layer1 [REPS] | --fill-f16 [REPS]]
          (defaults 256 3 f32 4 20; 3)"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

import dyobav_mpcnwta_warehouse_amd as nm  # noqa: E402
from dyobav_mpcnwta_warehouse_amd.evaluate import BatchEvaluator  # noqa: E402
from dyobav_mpcnwta_warehouse_amd.snap import WorldTransform  # noqa: E402

COPY_TBS, F1_TBS = 6.29, 5.6
PEAK_TFMAS = 78.6            # fp32 fma per second of the device (vector and v_mfma_f32_16x16x4_f32 alike), in 1e12


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


def _world(B, n_ped):
    """The warehouse label image with its size and transform, and the reference scenarios: (Hm, Wm, ref, tf, sc)."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "snap_map.npz"))
    Hm, Wm = (int(v) for v in z["shape"])
    occupied = np.unpackbits(z["occupied_bits"])[:Hm * Wm].reshape(Hm, Wm).astype(bool)
    ref = np.where(occupied, 0.0, 255.0).astype(np.float32)
    tf = WorldTransform(scale=0.1, offsetx_after=-15.0, offsety_after=-15.0, y_reverse=True, y_max_before=float(Hm))
    sc = nm.scenarios.make_reference_scenarios(B, n_ped=n_ped)
    sc.pop("scenario_index")
    return Hm, Wm, ref, tf, sc


def _timed(call, reps, warm=2):
    ms = []
    for i in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        y = call()
        e1.record()
        torch.cuda.synchronize()
        del y
        if i >= warm:
            ms.append(e0.elapsed_time(e1))
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms))}


def _fill(ev, n_item):
    """A call that launches the fill kernel of the evaluator's front end alone (nmpc_mmp_input_* or nmpc_mmp_stem_*) on the first
    ``n_item`` pedestrians of its start state and returns the kernel's output [n_item * N, *fill_row]."""
    fe = ev.mmp_front
    fe.allocate(n_item)
    hist, hcount = ev.hist.contiguous(), ev.hcount.contiguous()
    return lambda: fe.fill(hist.data_ptr(), hcount.data_ptr(), ev.B, ev.H, None, n_item)


def input_kernel_rate(ev, n_item, reps=20):
    """ms and GB/s of nmpc_mmp_input_* alone on ``n_item`` pedestrians of the evaluator's start state."""
    t = _timed(_fill(ev, n_item), reps, warm=5)
    nbytes, med = n_item * ev.N * int(np.prod(ev.mmp_front.fill_row)) * 4, t["ms_median"]
    return {"items": n_item, "bytes_written": nbytes, **t, "write_GBps_median": nbytes / med * 1e-6,
            "write_GBps_best": nbytes / t["ms_min"] * 1e-6, "share_of_copy_rate": nbytes / med * 1e-9 / COPY_TBS, "share_of_f1_rate": nbytes / med * 1e-9 / F1_TBS}


def stem_kernel_rate(ev, n_item, reps=20):
    """ms and GB/s stored of nmpc_mmp_stem_* alone on ``n_item`` pedestrians of the evaluator's start state."""
    t = _timed(_fill(ev, n_item), reps, warm=5)
    C = ev.mmp_front.fill_row[0]
    nbytes, med = n_item * ev.N * int(np.prod(ev.mmp_front.fill_row)) * 4, t["ms_median"]
    fma = n_item * C * ((ev.mmp_Hm - 1) // 2 + 1) * ((ev.mmp_Wm - 1) // 2 + 1) * 343        # base and E, once per pedestrian
    return {"items": n_item, "bytes_stored": nbytes, **t, "store_GBps_median": nbytes / med * 1e-6,
            "share_of_copy_rate": nbytes / med * 1e-9 / COPY_TBS, "conv_fma": fma, "conv_TFMAps_median": fma / med * 1e-9}


def torch_stem_alone(ev, stem_modules, n_item, reps=5):
    """ms of torch's own first layer (the four modules, eager) on the input stack of ``n_item`` pedestrians: one chunk of the parent path."""
    x = _fill(ev, n_item)()
    with torch.no_grad():
        t = _timed(lambda: stem_modules(x), reps)
    return dict(items=n_item, samples=n_item * ev.N, **t)


def fused_stem_main(out_path, B, steps, dt, n_ped, K, reps):
    from dyobav_mpcnwta_warehouse_amd.mmp_stem import fold_stem
    Hm, Wm, ref, tf, sc = _world(B, n_ped)
    torch.manual_seed(0)
    net = make_network(K).cuda().eval()
    # the split, by hand: net[0] = Sequential(Conv2d, BatchNorm2d, LeakyReLU), net[1] = MaxPool2d, the rest is the trunk
    spec = fold_stem(net[0][0], net[0][1], net[0][2], net[1])
    stem_modules, trunk = torch.nn.Sequential(net[0], net[1]), torch.nn.Sequential(*list(net)[2:])
    paths = {"parent": dict(network=lambda x: net(x) + 150.0), "fused": dict(network=lambda x: trunk(x) + 150.0, mmp_stem=spec)}

    def evaluator(path):
        return BatchEvaluator(nm.default_config_struct(), dtype=np.float32 if dt == "f32" else np.float64, predictor="mmp", mmp_hyp=K,
                              ref_image=ref, transform=tf, **paths[path], **sc)
    rec = {"what": "closed loop (row f3) on the reference scenarios, multi-hypothesis predictor stage: the parent path (input stack + whole "
                   "network) and the fused first layer + trunk, alternated in one process; random network of the reference's layer shapes",
           "B": B, "n_ped": n_ped, "n_hyp": K, "dtype": dt, "max_steps": steps, "map": [Hm, Wm], "repetitions": reps,
           "compared_with": {"float4_copy_TBps": COPY_TBS}, "chunk_pedestrians": {}, "runs": {"parent": [], "fused": []}}
    for path in paths:                                      # warm-up: code objects, library algorithm choice, allocator
        ev = evaluator(path)
        rec["chunk_pedestrians"][path] = ev.mmp_chunk
        try:
            if path == "fused":
                rec["stem_kernel"] = stem_kernel_rate(ev, min(ev.mmp_chunk, B * n_ped))
            else:
                rec["torch_stem_alone"] = torch_stem_alone(ev, stem_modules, min(ev.mmp_chunk, B * n_ped))
            ev.run(max_steps=1)
        finally:
            ev.close()
        print(json.dumps({k: rec[k] for k in ("stem_kernel", "torch_stem_alone") if k in rec}), flush=True)
    for _ in range(reps):
        for path in paths:
            ev = evaluator(path)
            ev.time_predictor = ev.time_predictor_parts = True
            try:
                res = ev.run(max_steps=steps)
            finally:
                ev.close()
            parts = ev.predictor_part_ms
            rec["runs"][path].append([dict(step=t, stage_ms=ev.predictor_ms[t], solve_ms=res.solve_ms[t], **{k: v[t] for k, v in parts.items()})
                                      for t in range(len(ev.predictor_ms))])
            print(path, json.dumps(rec["runs"][path][-1]), flush=True)
            with open(out_path, "w") as f:                  # (kept even if a later run does not finish)
                json.dump(rec, f, indent=1)
    med = lambda path, key: float(np.median([key(s) for run in rec["runs"][path] for s in run]))
    both = lambda s: s["input"] + s["network"]
    rec["median_per_lock_step_ms"] = {p: {"input": med(p, lambda s: s["input"]), "network": med(p, lambda s: s["network"]),
                                          "input_plus_network": med(p, both), "stage": med(p, lambda s: s["stage_ms"])} for p in paths}
    m = rec["median_per_lock_step_ms"]
    rec["fused_over_parent"] = m["fused"]["input_plus_network"] / m["parent"]["input_plus_network"]
    # torch's first layer alone on one chunk, scaled to the pedestrians of a lock-step: its share of the parent's network time
    ts = rec["torch_stem_alone"]
    rec["torch_stem_share_of_parent_network"] = ts["ms_median"] * (B * n_ped / ts["items"]) / m["parent"]["network"]
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: rec[k] for k in ("median_per_lock_step_ms", "fused_over_parent", "torch_stem_share_of_parent_network")}))


def torch_layer1_alone(ev, layer1, n_item, reps=5):
    """ms of torch's own layer1 (three blocks, eager) on the stem output of ``n_item`` pedestrians: one chunk of the parent path."""
    x = _fill(ev, n_item)()
    with torch.no_grad():
        t = _timed(lambda: layer1(x), reps)
    return dict(items=n_item, samples=n_item * ev.N, **t)


def block_kernel_rate(ev, n_item, reps=10):
    """The three nmpc_mmp_block_f32 launches alone on the stem output of ``n_item`` pedestrians: ms each and together, useful fma
    per second (9 Cin 16 + 9 16 16 (+ Cin 16) per pixel) and bytes per second (x read once, out written once)."""
    fe = ev.mmp_front
    rows, (_, Hp, Wp) = _fill(ev, n_item)().shape[0], fe.row
    rec = {"items": n_item, "rows": rows, "blocks": []}
    fma_all = bytes_all = 0
    for i, b in enumerate(fe.blocks):
        Cin, proj = int(b.w1.shape[1]), b.wd is not None
        fma = rows * Hp * Wp * 16 * (9 * Cin + 9 * 16 + (Cin if proj else 0))
        nbytes = rows * Hp * Wp * 4 * (Cin + 16)
        t = _timed(lambda: fe.run_block(i, rows), reps, warm=3)
        rec["blocks"].append(dict(Cin=Cin, projection=proj, fma=fma, bytes=nbytes, TFMAps_median=fma / t["ms_median"] * 1e-9,
                                  share_of_fp32_peak=fma / t["ms_median"] * 1e-9 / PEAK_TFMAS, GBps_median=nbytes / t["ms_median"] * 1e-6,
                                  share_of_copy_rate=nbytes / t["ms_median"] * 1e-9 / COPY_TBS, **t))
        fma_all, bytes_all = fma_all + fma, bytes_all + nbytes
    t = _timed(lambda: fe.run_blocks(rows), reps, warm=3)
    rec.update(fma=fma_all, bytes=bytes_all, TFMAps_median=fma_all / t["ms_median"] * 1e-9, share_of_fp32_peak=fma_all / t["ms_median"] * 1e-9 / PEAK_TFMAS,
               GBps_median=bytes_all / t["ms_median"] * 1e-6, share_of_copy_rate=bytes_all / t["ms_median"] * 1e-9 / COPY_TBS, **t)
    return rec


def fused_layer1_main(out_path, B, steps, dt, n_ped, K, reps):
    from types import SimpleNamespace

    from dyobav_mpcnwta_warehouse_amd.mmp_stem import fold_block, fold_stem
    Hm, Wm, ref, tf, sc = _world(B, n_ped)
    torch.manual_seed(0)
    net = make_network(K).cuda().eval()
    # the split, by hand: net[0], net[1] = the first layer; net[2 .. 4] = layer1 (Block: a, b, skip, act); the rest is the trunk
    spec = fold_stem(net[0][0], net[0][1], net[0][2], net[1])
    blocks = tuple(fold_block(SimpleNamespace(conv1=b.a, conv2=b.b, downsample=b.skip, leaky=b.act)) for b in list(net)[2:5])
    layer1, trunk1, trunk2 = torch.nn.Sequential(*list(net)[2:5]), torch.nn.Sequential(*list(net)[2:]), torch.nn.Sequential(*list(net)[5:])
    paths = {"parent": dict(network=lambda x: trunk1(x) + 150.0, mmp_stem=spec),
             "fused": dict(network=lambda x: trunk2(x) + 150.0, mmp_stem=spec, mmp_blocks=blocks)}

    def evaluator(path):
        return BatchEvaluator(nm.default_config_struct(), dtype=np.float32 if dt == "f32" else np.float64, predictor="mmp", mmp_hyp=K,
                              ref_image=ref, transform=tf, **paths[path], **sc)
    rec = {"what": "closed loop (row f3) on the reference scenarios, multi-hypothesis predictor stage: the parent path (fused first layer + "
                   "whole trunk in torch) and the fused first layer + fused layer1 + trunk from layer2 on, alternated in one process; random "
                   "network of the reference's layer shapes",
           "B": B, "n_ped": n_ped, "n_hyp": K, "dtype": dt, "max_steps": steps, "map": [Hm, Wm], "repetitions": reps,
           "compared_with": {"float4_copy_TBps": COPY_TBS, "fp32_peak_TFMAps": PEAK_TFMAS}, "chunk_pedestrians": {}, "runs": {"parent": [], "fused": []}}
    for path in paths:                                      # warm-up: code objects, library algorithm choice, allocator
        ev = evaluator(path)
        rec["chunk_pedestrians"][path] = ev.mmp_chunk
        try:
            if path == "fused":
                rec["block_kernels"] = block_kernel_rate(ev, min(ev.mmp_chunk, B * n_ped))
            else:
                rec["torch_layer1_alone"] = torch_layer1_alone(ev, layer1, min(ev.mmp_chunk, B * n_ped))
            ev.run(max_steps=1)
        finally:
            ev.close()
        print(json.dumps({k: rec[k] for k in ("block_kernels", "torch_layer1_alone") if k in rec}), flush=True)
        with open(out_path, "w") as f:
            json.dump(rec, f, indent=1)
    for _ in range(reps):
        for path in paths:
            ev = evaluator(path)
            ev.time_predictor = ev.time_predictor_parts = True
            try:
                res = ev.run(max_steps=steps)
            finally:
                ev.close()
            parts = ev.predictor_part_ms
            rec["runs"][path].append([dict(step=t, stage_ms=ev.predictor_ms[t], solve_ms=res.solve_ms[t], **{k: v[t] for k, v in parts.items()})
                                      for t in range(len(ev.predictor_ms))])
            print(path, json.dumps(rec["runs"][path][-1]), flush=True)
            with open(out_path, "w") as f:                  # (kept even if a later run does not finish)
                json.dump(rec, f, indent=1)
    med = lambda path, key: float(np.median([key(s) for run in rec["runs"][path] for s in run]))
    names = {"parent": ("input", "network"), "fused": ("input", "layer1", "network")}
    rec["median_per_lock_step_ms"] = {p: dict({k: med(p, lambda s, k=k: s[k]) for k in names[p]},
                                              behind_input=med(p, lambda s, p=p: sum(s[k] for k in names[p][1:])),
                                              stage=med(p, lambda s: s["stage_ms"])) for p in paths}
    m = rec["median_per_lock_step_ms"]
    rec["fused_layer1_over_parent"] = m["fused"]["stage"] / m["parent"]["stage"]
    # torch's layer1 alone on one chunk, scaled to the pedestrians of a lock-step: its share of the parent's network time; and
    # the three block launches alone, scaled alike
    tl, bk = rec["torch_layer1_alone"], rec["block_kernels"]
    rec["torch_layer1_per_lock_step_ms"] = tl["ms_median"] * (B * n_ped / tl["items"])
    rec["torch_layer1_share_of_parent_network"] = rec["torch_layer1_per_lock_step_ms"] / m["parent"]["network"]
    rec["block_kernels_per_lock_step_ms"] = bk["ms_median"] * (B * n_ped / bk["items"])
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: rec[k] for k in ("median_per_lock_step_ms", "fused_layer1_over_parent", "torch_layer1_per_lock_step_ms",
                                          "torch_layer1_share_of_parent_network", "block_kernels_per_lock_step_ms")}))


def torch_layer2_alone(ev, layer2, n_item, reps=5):
    """ms of torch's own layer2 (four blocks, eager) on the layer1 output of ``n_item`` pedestrians: one chunk of the parent path."""
    fe = ev.mmp_front
    rows = _fill(ev, n_item)().shape[0]
    x = fe.run_blocks(rows)
    with torch.no_grad():
        t = _timed(lambda: layer2(x), reps)
    return dict(items=n_item, samples=rows, **t)


def _strided_kernel_rate(fe, rows, reps, blocks, C, first, plane, run_all, cins=None):
    """The launches of one strided stage (``blocks`` at ``C`` output channels, ``run_block(first ..)``, input plane ``plane``) alone
    on ``rows`` rows of what the stage in front left: ms each and together, useful fma per second (C (9 Cin + 9 C (+ Cin)) per
    output pixel) and bytes per second (x read once, out written once)."""
    H, W = plane
    rec = {"rows": rows, "blocks": []}
    fma_all = bytes_all = 0
    for i, b in enumerate(blocks):
        Cin, proj, s = (cins[i] if cins else int(b.w1.shape[1])), b.wd is not None, int(b.stride)      # (cins: packed weights do not show Cin)
        H2, W2 = (H - 1) // s + 1, (W - 1) // s + 1
        fma = rows * H2 * W2 * C * (9 * Cin + 9 * C + (Cin if proj else 0))
        nbytes = rows * 4 * (Cin * H * W + C * H2 * W2)
        t = _timed(lambda: fe.run_block(first + i, rows), reps, warm=3)
        rec["blocks"].append(dict(Cin=Cin, stride=s, projection=proj, plane_in=[H, W], plane_out=[H2, W2], fma=fma, bytes=nbytes,
                                  TFMAps_median=fma / t["ms_median"] * 1e-9, share_of_fp32_peak=fma / t["ms_median"] * 1e-9 / PEAK_TFMAS,
                                  GBps_median=nbytes / t["ms_median"] * 1e-6, share_of_copy_rate=nbytes / t["ms_median"] * 1e-9 / COPY_TBS, **t))
        fma_all, bytes_all, H, W = fma_all + fma, bytes_all + nbytes, H2, W2
    t = _timed(lambda: run_all(rows), reps, warm=3)
    rec.update(fma=fma_all, bytes=bytes_all, TFMAps_median=fma_all / t["ms_median"] * 1e-9, share_of_fp32_peak=fma_all / t["ms_median"] * 1e-9 / PEAK_TFMAS,
               GBps_median=bytes_all / t["ms_median"] * 1e-6, share_of_copy_rate=bytes_all / t["ms_median"] * 1e-9 / COPY_TBS, **t)
    return rec


def block2_kernel_rate(ev, n_item, reps=10):
    """The four layer2 launches of the evaluator's front end (float32 or binary16 operands) alone on the layer1 output of ``n_item``
    pedestrians (``_strided_kernel_rate``)."""
    fe = ev.mmp_front
    rows = _fill(ev, n_item)().shape[0]
    fe.run_blocks(rows)
    return {"items": n_item, **_strided_kernel_rate(fe, rows, reps, fe.blocks2, 32, len(fe.blocks), fe.fill_row[1:], fe.run_blocks2,
                                                    cins=fe.stage("layer2").cins)}


def torch_layer3_alone(ev, layer3, n_item, reps=5):
    """ms of torch's own layer3 (six blocks, eager) on the layer2 output of ``n_item`` pedestrians: one chunk of the parent path."""
    fe = ev.mmp_front
    rows = _fill(ev, n_item)().shape[0]
    fe.run_blocks(rows)
    x = fe.run_blocks2(rows)
    with torch.no_grad():
        t = _timed(lambda: layer3(x), reps)
    return dict(items=n_item, samples=rows, **t)


def block3_kernel_rate(ev, n_item, reps=10):
    """The six nmpc_mmp_block3_f32 launches alone on the layer2 output of ``n_item`` pedestrians (``_strided_kernel_rate``)."""
    fe = ev.mmp_front
    rows = _fill(ev, n_item)().shape[0]
    fe.run_blocks(rows)
    plane = tuple(fe.run_blocks2(rows).shape[2:])
    return {"items": n_item, **_strided_kernel_rate(fe, rows, reps, fe.blocks3, 64, len(fe.blocks) + len(fe.blocks2), plane, fe.run_blocks3,
                                                    cins=fe.stage("layer3").cins)}


def fused_layer2_main(out_path, B, steps, dt, n_ped, K, reps):
    from types import SimpleNamespace

    from dyobav_mpcnwta_warehouse_amd.mmp_stem import fold_block, fold_block2, fold_stem
    Hm, Wm, ref, tf, sc = _world(B, n_ped)
    torch.manual_seed(0)
    net = make_network(K).cuda().eval()
    # the split, by hand (the module here is a plain Sequential, not of the shape split_network_layer2 takes): net[0], net[1] = the
    # first layer; net[2 .. 4] = layer1, net[5 .. 8] = layer2 (Block: a, b, skip, act); the rest is the trunk
    spec = fold_stem(net[0][0], net[0][1], net[0][2], net[1])
    as_block = lambda b: SimpleNamespace(conv1=b.a, conv2=b.b, downsample=b.skip, leaky=b.act)
    blocks = tuple(fold_block(as_block(b)) for b in list(net)[2:5])
    blocks2 = tuple(fold_block2(as_block(b)) for b in list(net)[5:9])
    layer2, trunk2, trunk3 = torch.nn.Sequential(*list(net)[5:9]), torch.nn.Sequential(*list(net)[5:]), torch.nn.Sequential(*list(net)[9:])
    paths = {"parent": dict(network=lambda x: trunk2(x) + 150.0, mmp_stem=spec, mmp_blocks=blocks),
             "fused": dict(network=lambda x: trunk3(x) + 150.0, mmp_stem=spec, mmp_blocks=blocks, mmp_blocks2=blocks2)}

    def evaluator(path):
        return BatchEvaluator(nm.default_config_struct(), dtype=np.float32 if dt == "f32" else np.float64, predictor="mmp", mmp_hyp=K,
                              ref_image=ref, transform=tf, **paths[path], **sc)
    rows_step = B * n_ped * nm.default_config_struct().N_hor
    rec = {"what": "closed loop (row f3) on the reference scenarios, multi-hypothesis predictor stage: the parent path (fused first layer + "
                   "fused layer1 + trunk from layer2 on in torch) and the same with layer2 fused as well + trunk from layer3 on, alternated in "
                   "one process; random network of the reference's layer shapes",
           "B": B, "n_ped": n_ped, "n_hyp": K, "dtype": dt, "max_steps": steps, "map": [Hm, Wm], "repetitions": reps,
           "compared_with": {"float4_copy_TBps": COPY_TBS, "fp32_peak_TFMAps": PEAK_TFMAS},
           "model_of_the_header_per_lock_step_ms": {"rows": 20480, "mfma_pipe_never_waits": 40.2, "useful_fma_at_fp32_peak": 28.2, "bytes_at_copy_rate": 5.8},
           "chunk_pedestrians": {}, "runs": {"parent": [], "fused": []}}
    for path in paths:                                      # warm-up: code objects, library algorithm choice, allocator
        ev = evaluator(path)
        rec["chunk_pedestrians"][path] = ev.mmp_chunk
        try:
            if path == "fused":
                rec["block2_kernels"] = block2_kernel_rate(ev, min(ev.mmp_chunk, B * n_ped))
            else:
                rec["torch_layer2_alone"] = torch_layer2_alone(ev, layer2, min(ev.mmp_chunk, B * n_ped))
            ev.run(max_steps=1)
        finally:
            ev.close()
        print(json.dumps({k: rec[k] for k in ("block2_kernels", "torch_layer2_alone") if k in rec}), flush=True)
        with open(out_path, "w") as f:
            json.dump(rec, f, indent=1)
    for _ in range(reps):
        for path in paths:
            ev = evaluator(path)
            ev.time_predictor = ev.time_predictor_parts = True
            try:
                res = ev.run(max_steps=steps)
            finally:
                ev.close()
            parts = ev.predictor_part_ms
            rec["runs"][path].append([dict(step=t, stage_ms=ev.predictor_ms[t], solve_ms=res.solve_ms[t], **{k: v[t] for k, v in parts.items()})
                                      for t in range(len(ev.predictor_ms))])
            print(path, json.dumps(rec["runs"][path][-1]), flush=True)
            with open(out_path, "w") as f:                  # (kept even if a later run does not finish)
                json.dump(rec, f, indent=1)
    med = lambda path, key: float(np.median([key(s) for run in rec["runs"][path] for s in run]))
    names = {"parent": ("input", "layer1", "network"), "fused": ("input", "layer1", "layer2", "network")}
    rec["median_per_lock_step_ms"] = {p: dict({k: med(p, lambda s, k=k: s[k]) for k in names[p]},
                                              behind_layer1=med(p, lambda s, p=p: sum(s[k] for k in names[p][2:])),
                                              stage=med(p, lambda s: s["stage_ms"])) for p in paths}
    m = rec["median_per_lock_step_ms"]
    rec["fused_layer2_over_parent"] = m["fused"]["stage"] / m["parent"]["stage"]
    # torch's layer2 alone on one chunk, scaled to the rows of a lock-step: its share of the parent's network time; and the four
    # block launches alone, scaled alike, against the header's model
    tl, bk = rec["torch_layer2_alone"], rec["block2_kernels"]
    rec["torch_layer2_per_lock_step_ms"] = tl["ms_median"] * (rows_step / tl["samples"])
    rec["torch_layer2_share_of_parent_network"] = rec["torch_layer2_per_lock_step_ms"] / m["parent"]["network"]
    rec["block2_kernels_per_lock_step_ms"] = bk["ms_median"] * (rows_step / bk["rows"])
    rec["block2_kernels_over_torch_layer2"] = rec["block2_kernels_per_lock_step_ms"] / rec["torch_layer2_per_lock_step_ms"]
    rec["block2_kernels_over_model"] = rec["block2_kernels_per_lock_step_ms"] * (20480 / rows_step) / 40.2
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: rec[k] for k in ("median_per_lock_step_ms", "fused_layer2_over_parent", "torch_layer2_per_lock_step_ms",
                                          "torch_layer2_share_of_parent_network", "block2_kernels_per_lock_step_ms",
                                          "block2_kernels_over_torch_layer2", "block2_kernels_over_model")}))


MODEL3 = {"rows": 20480, "mfma_pipe_never_waits": 69.0, "useful_fma_at_fp32_peak": 44.3, "bytes_at_copy_rate": 4.3}   # csrc/nmpc_mmp_block3.h


def fused_layer3_main(out_path, B, steps, dt, n_ped, K, reps):
    from types import SimpleNamespace

    from dyobav_mpcnwta_warehouse_amd.mmp_stem import fold_block, fold_block2, fold_block3, fold_stem
    Hm, Wm, ref, tf, sc = _world(B, n_ped)
    torch.manual_seed(0)
    net = make_network(K).cuda().eval()
    # the split, by hand, as in fused_layer2_main: net[2 .. 4] = layer1, net[5 .. 8] = layer2, net[9 .. 14] = layer3; the rest is the trunk
    spec = fold_stem(net[0][0], net[0][1], net[0][2], net[1])
    as_block = lambda b: SimpleNamespace(conv1=b.a, conv2=b.b, downsample=b.skip, leaky=b.act)
    blocks = tuple(fold_block(as_block(b)) for b in list(net)[2:5])
    blocks2 = tuple(fold_block2(as_block(b)) for b in list(net)[5:9])
    blocks3 = tuple(fold_block3(as_block(b)) for b in list(net)[9:15])
    layer3, trunk3, trunk4 = torch.nn.Sequential(*list(net)[9:15]), torch.nn.Sequential(*list(net)[9:]), torch.nn.Sequential(*list(net)[15:])
    paths = {"parent": dict(network=lambda x: trunk3(x) + 150.0, mmp_stem=spec, mmp_blocks=blocks, mmp_blocks2=blocks2),
             "fused": dict(network=lambda x: trunk4(x) + 150.0, mmp_stem=spec, mmp_blocks=blocks, mmp_blocks2=blocks2, mmp_blocks3=blocks3)}

    def evaluator(path):
        return BatchEvaluator(nm.default_config_struct(), dtype=np.float32 if dt == "f32" else np.float64, predictor="mmp", mmp_hyp=K,
                              ref_image=ref, transform=tf, **paths[path], **sc)
    rows_step = B * n_ped * nm.default_config_struct().N_hor
    rec = {"what": "closed loop (row f3) on the reference scenarios, multi-hypothesis predictor stage: the parent path (fused first layer + "
                   "fused layer1 + fused layer2 + trunk from layer3 on in torch) and the same with layer3 fused as well + trunk from layer4 on, "
                   "alternated in one process; random network of the reference's layer shapes",
           "B": B, "n_ped": n_ped, "n_hyp": K, "dtype": dt, "max_steps": steps, "map": [Hm, Wm], "repetitions": reps,
           "compared_with": {"float4_copy_TBps": COPY_TBS, "fp32_peak_TFMAps": PEAK_TFMAS},
           "model_of_the_header_per_lock_step_ms": MODEL3, "chunk_pedestrians": {}, "runs": {"parent": [], "fused": []}}
    for path in paths:                                      # warm-up; torch's layer3 alone (the parent path) comes first
        ev = evaluator(path)
        rec["chunk_pedestrians"][path] = ev.mmp_chunk
        try:
            if path == "fused":
                rec["block3_kernels"] = block3_kernel_rate(ev, min(ev.mmp_chunk, B * n_ped))
            else:
                rec["torch_layer3_alone"] = torch_layer3_alone(ev, layer3, min(ev.mmp_chunk, B * n_ped))
            ev.run(max_steps=1)
        finally:
            ev.close()
        print(json.dumps({k: rec[k] for k in ("block3_kernels", "torch_layer3_alone") if k in rec}), flush=True)
        with open(out_path, "w") as f:
            json.dump(rec, f, indent=1)
    for _ in range(reps):
        for path in paths:
            ev = evaluator(path)
            ev.time_predictor = ev.time_predictor_parts = True
            try:
                res = ev.run(max_steps=steps)
            finally:
                ev.close()
            parts = ev.predictor_part_ms
            rec["runs"][path].append([dict(step=t, stage_ms=ev.predictor_ms[t], solve_ms=res.solve_ms[t], **{k: v[t] for k, v in parts.items()})
                                      for t in range(len(ev.predictor_ms))])
            print(path, json.dumps(rec["runs"][path][-1]), flush=True)
            with open(out_path, "w") as f:                  # (kept even if a later run does not finish)
                json.dump(rec, f, indent=1)
    med = lambda path, key: float(np.median([key(s) for run in rec["runs"][path] for s in run]))
    names = {"parent": ("input", "layer1", "layer2", "network"), "fused": ("input", "layer1", "layer2", "layer3", "network")}
    rec["median_per_lock_step_ms"] = {p: dict({k: med(p, lambda s, k=k: s[k]) for k in names[p]},
                                              behind_layer2=med(p, lambda s, p=p: sum(s[k] for k in names[p][3:])),
                                              stage=med(p, lambda s: s["stage_ms"])) for p in paths}
    m = rec["median_per_lock_step_ms"]
    rec["fused_layer3_over_parent"] = m["fused"]["stage"] / m["parent"]["stage"]
    # torch's layer3 alone on one chunk, scaled to the rows of a lock-step: its share of the parent's network time; and the six
    # block launches alone, scaled alike, against the header's model
    tl, bk = rec["torch_layer3_alone"], rec["block3_kernels"]
    rec["torch_layer3_per_lock_step_ms"] = tl["ms_median"] * (rows_step / tl["samples"])
    rec["torch_layer3_share_of_parent_network"] = rec["torch_layer3_per_lock_step_ms"] / m["parent"]["network"]
    rec["block3_kernels_per_lock_step_ms"] = bk["ms_median"] * (rows_step / bk["rows"])
    rec["block3_kernels_over_torch_layer3"] = rec["block3_kernels_per_lock_step_ms"] / rec["torch_layer3_per_lock_step_ms"]
    rec["block3_kernels_over_model"] = rec["block3_kernels_per_lock_step_ms"] * (20480 / rows_step) / MODEL3["mfma_pipe_never_waits"]
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: rec[k] for k in ("median_per_lock_step_ms", "fused_layer3_over_parent", "torch_layer3_per_lock_step_ms",
                                          "torch_layer3_share_of_parent_network", "block3_kernels_per_lock_step_ms",
                                          "block3_kernels_over_torch_layer3", "block3_kernels_over_model")}))


MODEL4 = {"rows": 20480, "mfma_pipe_never_waits": 27.3, "useful_fma_at_fp32_peak": 23.5, "bytes_at_copy_rate": 1.3,
          "head_vector_memory_instructions": 0.64}    # csrc/nmpc_mmp_block4.h; the head: the FIRST model of nmpc_mmp_head.h


def _layer3_output(ev, n_item):
    fe = ev.mmp_front
    rows = _fill(ev, n_item)().shape[0]
    fe.run_blocks(rows)
    fe.run_blocks2(rows)
    return rows, fe.run_blocks3(rows)


def torch_layer4_and_head_alone(ev, layer4, end, n_item, reps=5):
    """ms of torch's own layer4 (three blocks, eager) on the layer3 output of ``n_item`` pedestrians -- one chunk of the parent path --
    and of its pool, flatten and linear layers on what layer4 gives."""
    rows, x = _layer3_output(ev, n_item)
    with torch.no_grad():
        t4 = _timed(lambda: layer4(x), reps)
        y = layer4(x)
        te = _timed(lambda: end(y), reps)
    return dict(items=n_item, samples=rows, **t4), dict(items=n_item, samples=rows, **te)


def block4_and_head_kernel_rate(ev, n_item, reps=10):
    """The three nmpc_mmp_block4_f32 launches alone on the layer3 output of ``n_item`` pedestrians (``_strided_kernel_rate``), then the
    nmpc_mmp_head_f32 launch alone on what they leave: ms, useful fma per second (F x 128 + 128 x O per row) and bytes per second
    (x read once, W1 and W2 once per group of 16 rows -- from L2 --, out written once)."""
    fe = ev.mmp_front
    rows, x = _layer3_output(ev, n_item)
    first = len(fe.blocks) + len(fe.blocks2) + len(fe.blocks3)
    blocks = {"items": n_item, **_strided_kernel_rate(fe, rows, reps, fe.blocks4, 128, first, tuple(x.shape[2:]), fe.run_blocks4)}
    y = fe.run_blocks4(rows)
    F, O = int(fe.head.w1.shape[1]), int(fe.head.w2.shape[0])
    t = _timed(lambda: fe.run_head(rows), reps, warm=3)
    fma, groups = rows * (F * 128 + 128 * O), -(-rows // 16)
    nbytes = 4 * (rows * int(np.prod(y.shape[1:])) + groups * (F * 128 + 128 * O) + rows * O)
    head = dict(items=n_item, rows=rows, F=F, O=O, fma=fma, bytes=nbytes, TFMAps_median=fma / t["ms_median"] * 1e-9,
                GBps_median=nbytes / t["ms_median"] * 1e-6, **t)
    return blocks, head


def fused_layer4_main(out_path, B, steps, dt, n_ped, K, reps):
    from types import SimpleNamespace

    from dyobav_mpcnwta_warehouse_amd.mmp_stem import split_network_whole
    Hm, Wm, ref, tf, sc = _world(B, n_ped)
    torch.manual_seed(0)
    net = make_network(K).cuda().eval()
    # the module here is a plain Sequential: net[0], net[1] = the first layer, net[2 .. 4] = layer1, net[5 .. 8] = layer2, net[9 .. 14]
    # = layer3, net[15 .. 17] = layer4, net[18] = the pool, net[20 .. 22] = fc1, leaky, the hypothesis layer. Named as
    # split_network_whole wants it (Block: a, b, skip, act)
    as_block = lambda b: SimpleNamespace(conv1=b.a, conv2=b.b, downsample=b.skip, leaky=b.act)
    L = list(net)
    shaped = SimpleNamespace(resnet34=SimpleNamespace(stem=SimpleNamespace(conv1=L[0], pooling=L[1]), layer1=[as_block(b) for b in L[2:5]],
                                                      layer2=[as_block(b) for b in L[5:9]], layer3=[as_block(b) for b in L[9:15]],
                                                      layer4=[as_block(b) for b in L[15:18]], apool=L[18]), fc1=L[20], leaky=L[21], swarm=L[22])
    spec, blocks, blocks2, blocks3, blocks4, head = split_network_whole(shaped)
    head = head._replace(c2=head.c2 + np.float32(150.0))   # (the "+ 150" that puts the random network's hypotheses on the map)
    layer4, end, trunk4 = torch.nn.Sequential(*L[15:18]), torch.nn.Sequential(*L[18:]), torch.nn.Sequential(*L[15:])
    front = dict(mmp_stem=spec, mmp_blocks=blocks, mmp_blocks2=blocks2, mmp_blocks3=blocks3)
    paths = {"parent": dict(network=lambda x: trunk4(x) + 150.0, **front), "fused": dict(network=None, mmp_blocks4=blocks4, mmp_head=head, **front)}

    def evaluator(path):
        return BatchEvaluator(nm.default_config_struct(), dtype=np.float32 if dt == "f32" else np.float64, predictor="mmp", mmp_hyp=K,
                              ref_image=ref, transform=tf, **paths[path], **sc)
    rows_step = B * n_ped * nm.default_config_struct().N_hor
    rec = {"what": "closed loop (row f3) on the reference scenarios, multi-hypothesis predictor stage: the parent path (fused first layer + "
                   "fused layer1 .. layer3 + trunk from layer4 on in torch) and the whole network on the device (layer4 and the head fused as "
                   "well, no torch module), alternated in one process; random network of the reference's layer shapes",
           "B": B, "n_ped": n_ped, "n_hyp": K, "dtype": dt, "max_steps": steps, "map": [Hm, Wm], "repetitions": reps,
           "compared_with": {"float4_copy_TBps": COPY_TBS, "fp32_peak_TFMAps": PEAK_TFMAS},
           "model_of_the_headers_per_lock_step_ms": MODEL4, "chunk_pedestrians": {}, "runs": {"parent": [], "fused": []}}
    for path in paths:                                      # warm-up; torch's layer4 and end alone (the parent path) come first
        ev = evaluator(path)
        rec["chunk_pedestrians"][path] = ev.mmp_chunk
        try:
            if path == "fused":
                rec["block4_kernels"], rec["head_kernel"] = block4_and_head_kernel_rate(ev, min(ev.mmp_chunk, B * n_ped))
            else:
                rec["torch_layer4_alone"], rec["torch_pool_and_head_alone"] = torch_layer4_and_head_alone(ev, layer4, end, min(ev.mmp_chunk, B * n_ped))
            ev.run(max_steps=1)
        finally:
            ev.close()
        print(json.dumps({k: rec[k] for k in ("block4_kernels", "head_kernel", "torch_layer4_alone", "torch_pool_and_head_alone") if k in rec}), flush=True)
        with open(out_path, "w") as f:
            json.dump(rec, f, indent=1)
    for _ in range(reps):
        for path in paths:
            ev = evaluator(path)
            ev.time_predictor = ev.time_predictor_parts = True
            try:
                res = ev.run(max_steps=steps)
            finally:
                ev.close()
            parts = ev.predictor_part_ms
            rec["runs"][path].append([dict(step=t, stage_ms=ev.predictor_ms[t], solve_ms=res.solve_ms[t], **{k: v[t] for k, v in parts.items()})
                                      for t in range(len(ev.predictor_ms))])
            print(path, json.dumps(rec["runs"][path][-1]), flush=True)
            with open(out_path, "w") as f:                  # (kept even if a later run does not finish)
                json.dump(rec, f, indent=1)
    med = lambda path, key: float(np.median([key(s) for run in rec["runs"][path] for s in run]))
    names = {"parent": ("input", "layer1", "layer2", "layer3", "network"), "fused": ("input", "layer1", "layer2", "layer3", "layer4", "head")}
    rec["median_per_lock_step_ms"] = {p: dict({k: med(p, lambda s, k=k: s[k]) for k in names[p]},
                                              behind_layer3=med(p, lambda s, p=p: sum(s[k] for k in names[p][4:])),
                                              stage=med(p, lambda s: s["stage_ms"])) for p in paths}
    # the spread between the alternations: the median stage of every single run
    rec["stage_median_of_each_run_ms"] = {p: [float(np.median([s["stage_ms"] for s in run])) for run in rec["runs"][p]] for p in paths}
    m = rec["median_per_lock_step_ms"]
    rec["fused_layer4_over_parent"] = m["fused"]["stage"] / m["parent"]["stage"]
    scale = lambda r, rows: r["ms_median"] * (rows_step / rows)
    tl, te, bk, hk = rec["torch_layer4_alone"], rec["torch_pool_and_head_alone"], rec["block4_kernels"], rec["head_kernel"]
    rec["torch_layer4_per_lock_step_ms"], rec["torch_pool_and_head_per_lock_step_ms"] = scale(tl, tl["samples"]), scale(te, te["samples"])
    rec["block4_kernels_per_lock_step_ms"], rec["head_kernel_per_lock_step_ms"] = scale(bk, bk["rows"]), scale(hk, hk["rows"])
    rec["block4_kernels_over_torch_layer4"] = rec["block4_kernels_per_lock_step_ms"] / rec["torch_layer4_per_lock_step_ms"]
    rec["head_kernel_over_torch_pool_and_head"] = rec["head_kernel_per_lock_step_ms"] / rec["torch_pool_and_head_per_lock_step_ms"]
    rec["block4_kernels_over_model"] = rec["block4_kernels_per_lock_step_ms"] * (20480 / rows_step) / MODEL4["mfma_pipe_never_waits"]
    rec["head_kernel_over_model"] = rec["head_kernel_per_lock_step_ms"] * (20480 / rows_step) / MODEL4["head_vector_memory_instructions"]
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: rec[k] for k in ("median_per_lock_step_ms", "stage_median_of_each_run_ms", "chunk_pedestrians", "fused_layer4_over_parent",
                                          "torch_layer4_per_lock_step_ms", "torch_pool_and_head_per_lock_step_ms", "block4_kernels_per_lock_step_ms",
                                          "head_kernel_per_lock_step_ms", "block4_kernels_over_torch_layer4", "head_kernel_over_torch_pool_and_head",
                                          "block4_kernels_over_model", "head_kernel_over_model")}))
    print(json.dumps({"block4": [(b["Cin"], b["stride"], b["ms_median"], b["TFMAps_median"]) for b in bk["blocks"]], "all": (bk["ms_median"], bk["TFMAps_median"])}))


def half_layer3_main(out_path, B, steps, dt, n_ped, K, reps):
    """``--half-layer3``: the whole network on the device (the new path of ``--fused-layer4``) with layer3 on float32 operands and with
    ``mmp_half=("layer3",)`` (nmpc_mmp_block3_f16), alternated in one process: the six launches alone on one chunk, then the closed
    loop with events around every part."""
    from types import SimpleNamespace

    from dyobav_mpcnwta_warehouse_amd.mmp_stem import split_network_whole
    Hm, Wm, ref, tf, sc = _world(B, n_ped)
    torch.manual_seed(0)
    net = make_network(K).cuda().eval()
    as_block = lambda b: SimpleNamespace(conv1=b.a, conv2=b.b, downsample=b.skip, leaky=b.act)
    L = list(net)
    shaped = SimpleNamespace(resnet34=SimpleNamespace(stem=SimpleNamespace(conv1=L[0], pooling=L[1]), layer1=[as_block(b) for b in L[2:5]],
                                                      layer2=[as_block(b) for b in L[5:9]], layer3=[as_block(b) for b in L[9:15]],
                                                      layer4=[as_block(b) for b in L[15:18]], apool=L[18]), fc1=L[20], leaky=L[21], swarm=L[22])
    spec, blocks, blocks2, blocks3, blocks4, head = split_network_whole(shaped)
    head = head._replace(c2=head.c2 + np.float32(150.0))   # (the "+ 150" that puts the random network's hypotheses on the map)
    whole = dict(network=None, mmp_stem=spec, mmp_blocks=blocks, mmp_blocks2=blocks2, mmp_blocks3=blocks3, mmp_blocks4=blocks4, mmp_head=head)
    paths = {"fp32": dict(whole), "f16": dict(whole, mmp_half=("layer3",))}

    def evaluator(path):
        return BatchEvaluator(nm.default_config_struct(), dtype=np.float32 if dt == "f32" else np.float64, predictor="mmp", mmp_hyp=K,
                              ref_image=ref, transform=tf, **paths[path], **sc)
    rows_step = B * n_ped * nm.default_config_struct().N_hor
    rec = {"what": "closed loop (row f3) on the reference scenarios, multi-hypothesis predictor stage, the whole network on the device: layer3 "
                   "on float32 MFMA operands (nmpc_mmp_block3_f32) and on binary16 operands with float32 accumulation (nmpc_mmp_block3_f16, "
                   "mmp_half = ('layer3',)), alternated in one process; random network of the reference's layer shapes",
           "B": B, "n_ped": n_ped, "n_hyp": K, "dtype": dt, "max_steps": steps, "map": [Hm, Wm], "repetitions": reps,
           "compared_with": {"float4_copy_TBps": COPY_TBS, "fp32_peak_TFMAps": PEAK_TFMAS},
           "model_of_the_f16_header_per_lock_step_ms": {"mfma_pipe_never_waits": 4.3, "memory_at_copy_rate": 4.3},
           "fp32_mfma_never_waits_floor_over_fp32_measured": 0.57, "chunk_pedestrians": {}, "block3_kernels": {p: [] for p in paths},
           "runs": {p: [] for p in paths}}
    for _ in range(reps):                                   # the six launches alone, three runs per arm, alternated (the first also warms up)
        for path in paths:
            ev = evaluator(path)
            rec["chunk_pedestrians"][path] = ev.mmp_chunk
            try:
                rec["block3_kernels"][path].append(block3_kernel_rate(ev, min(ev.mmp_chunk, B * n_ped)))
                ev.run(max_steps=1)
            finally:
                ev.close()
            r = rec["block3_kernels"][path][-1]
            print(path, json.dumps({"rows": r["rows"], "six_launches_ms": r["ms_median"], "each": [b["ms_median"] for b in r["blocks"]]}), flush=True)
            with open(out_path, "w") as f:
                json.dump(rec, f, indent=1)
    for _ in range(reps):
        for path in paths:
            ev = evaluator(path)
            ev.time_predictor = ev.time_predictor_parts = True
            try:
                res = ev.run(max_steps=steps)
            finally:
                ev.close()
            parts = ev.predictor_part_ms
            rec["runs"][path].append([dict(step=t, stage_ms=ev.predictor_ms[t], solve_ms=res.solve_ms[t], **{k: v[t] for k, v in parts.items()})
                                      for t in range(len(ev.predictor_ms))])
            print(path, json.dumps(rec["runs"][path][-1]), flush=True)
            with open(out_path, "w") as f:                  # (kept even if a later run does not finish)
                json.dump(rec, f, indent=1)
    med = lambda path, key: float(np.median([key(s) for run in rec["runs"][path] for s in run]))
    names = ("input", "layer1", "layer2", "layer3", "layer4", "head")
    rec["median_per_lock_step_ms"] = {p: dict({k: med(p, lambda s, k=k: s[k]) for k in names}, stage=med(p, lambda s: s["stage_ms"])) for p in paths}
    rec["stage_median_of_each_run_ms"] = {p: [float(np.median([s["stage_ms"] for s in run])) for run in rec["runs"][p]] for p in paths}
    rec["layer3_median_of_each_run_ms"] = {p: [float(np.median([s["layer3"] for s in run])) for run in rec["runs"][p]] for p in paths}
    rec["six_launches_of_each_run_ms"] = {p: [r["ms_median"] for r in rec["block3_kernels"][p]] for p in paths}
    rec["six_launches_per_lock_step_ms"] = {p: float(np.median([r["ms_median"] * rows_step / r["rows"] for r in rec["block3_kernels"][p]])) for p in paths}
    six, m = rec["six_launches_of_each_run_ms"], rec["median_per_lock_step_ms"]
    rec["f16_over_fp32_six_launches"] = float(np.median(six["f16"]) / np.median(six["fp32"]))
    rec["f16_over_fp32_stage"] = m["f16"]["stage"] / m["fp32"]["stage"]
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: rec[k] for k in ("median_per_lock_step_ms", "stage_median_of_each_run_ms", "layer3_median_of_each_run_ms", "six_launches_of_each_run_ms",
                                          "six_launches_per_lock_step_ms", "f16_over_fp32_six_launches", "f16_over_fp32_stage", "chunk_pedestrians")}))
    for p in paths:
        r = rec["block3_kernels"][p][-1]
        print(p, json.dumps([(b["Cin"], b["stride"], b["ms_median"], b["TFMAps_median"], b["GBps_median"]) for b in r["blocks"]]))


def block4_kernel_rate(ev, n_item, reps=10):
    """The three layer4 launches of the evaluator's front end (float32 or binary16 operands) alone on the layer3 output of ``n_item``
    pedestrians (``_strided_kernel_rate``)."""
    fe = ev.mmp_front
    rows, x = _layer3_output(ev, n_item)
    first = len(fe.blocks) + len(fe.blocks2) + len(fe.blocks3)
    return {"items": n_item, **_strided_kernel_rate(fe, rows, reps, fe.blocks4, 128, first, tuple(x.shape[2:]), fe.run_blocks4,
                                                    cins=fe.stage("layer4").cins)}


def half_layer4_main(out_path, B, steps, dt, n_ped, K, reps):
    """``--half-layer4``: the whole network on the device with ``mmp_half=("layer3",)`` (layer4 on float32 operands) and with
    ``mmp_half=("layer3", "layer4")`` (nmpc_mmp_block4_f16), alternated in one process: the three launches alone on one chunk, then
    the closed loop with events around every part."""
    from types import SimpleNamespace

    from dyobav_mpcnwta_warehouse_amd.mmp_stem import split_network_whole
    Hm, Wm, ref, tf, sc = _world(B, n_ped)
    torch.manual_seed(0)
    net = make_network(K).cuda().eval()
    as_block = lambda b: SimpleNamespace(conv1=b.a, conv2=b.b, downsample=b.skip, leaky=b.act)
    L = list(net)
    shaped = SimpleNamespace(resnet34=SimpleNamespace(stem=SimpleNamespace(conv1=L[0], pooling=L[1]), layer1=[as_block(b) for b in L[2:5]],
                                                      layer2=[as_block(b) for b in L[5:9]], layer3=[as_block(b) for b in L[9:15]],
                                                      layer4=[as_block(b) for b in L[15:18]], apool=L[18]), fc1=L[20], leaky=L[21], swarm=L[22])
    spec, blocks, blocks2, blocks3, blocks4, head = split_network_whole(shaped)
    head = head._replace(c2=head.c2 + np.float32(150.0))   # (the "+ 150" that puts the random network's hypotheses on the map)
    whole = dict(network=None, mmp_stem=spec, mmp_blocks=blocks, mmp_blocks2=blocks2, mmp_blocks3=blocks3, mmp_blocks4=blocks4, mmp_head=head)
    paths = {"fp32": dict(whole, mmp_half=("layer3",)), "f16": dict(whole, mmp_half=("layer3", "layer4"))}

    def evaluator(path):
        return BatchEvaluator(nm.default_config_struct(), dtype=np.float32 if dt == "f32" else np.float64, predictor="mmp", mmp_hyp=K,
                              ref_image=ref, transform=tf, **paths[path], **sc)
    rows_step = B * n_ped * nm.default_config_struct().N_hor
    rec = {"what": "closed loop (row f3) on the reference scenarios, multi-hypothesis predictor stage, the whole network on the device, layer3 "
                   "on binary16 operands in both arms: layer4 on float32 MFMA operands (nmpc_mmp_block4_f32, mmp_half = ('layer3',)) and on "
                   "binary16 operands with float32 accumulation (nmpc_mmp_block4_f16, mmp_half = ('layer3', 'layer4')), alternated in one "
                   "process; random network of the reference's layer shapes",
           "B": B, "n_ped": n_ped, "n_hyp": K, "dtype": dt, "max_steps": steps, "map": [Hm, Wm], "repetitions": reps,
           "compared_with": {"float4_copy_TBps": COPY_TBS, "fp32_peak_TFMAps": PEAK_TFMAS},
           "model_of_the_f16_header_per_lock_step_ms": {"mfma_pipe_never_waits": 1.71, "activations_at_copy_rate": 1.3,
                                                        "weights_out_of_L2_33.6_to_67_GB_at_17_to_19_TBps": [1.8, 3.9]},
           "fp32_mfma_never_waits_floor_over_fp32_measured": 0.47, "chunk_pedestrians": {}, "block4_kernels": {p: [] for p in paths},
           "runs": {p: [] for p in paths}}
    for _ in range(reps):                                   # the three launches alone, three runs per arm, alternated (the first also warms up)
        for path in paths:
            ev = evaluator(path)
            rec["chunk_pedestrians"][path] = ev.mmp_chunk
            try:
                rec["block4_kernels"][path].append(block4_kernel_rate(ev, min(ev.mmp_chunk, B * n_ped)))
                ev.run(max_steps=1)
            finally:
                ev.close()
            r = rec["block4_kernels"][path][-1]
            print(path, json.dumps({"rows": r["rows"], "three_launches_ms": r["ms_median"], "each": [b["ms_median"] for b in r["blocks"]]}), flush=True)
            with open(out_path, "w") as f:
                json.dump(rec, f, indent=1)
    for _ in range(reps):
        for path in paths:
            ev = evaluator(path)
            ev.time_predictor = ev.time_predictor_parts = True
            try:
                res = ev.run(max_steps=steps)
            finally:
                ev.close()
            parts = ev.predictor_part_ms
            rec["runs"][path].append([dict(step=t, stage_ms=ev.predictor_ms[t], solve_ms=res.solve_ms[t], **{k: v[t] for k, v in parts.items()})
                                      for t in range(len(ev.predictor_ms))])
            print(path, json.dumps(rec["runs"][path][-1]), flush=True)
            with open(out_path, "w") as f:                  # (kept even if a later run does not finish)
                json.dump(rec, f, indent=1)
    med = lambda path, key: float(np.median([key(s) for run in rec["runs"][path] for s in run]))
    names = ("input", "layer1", "layer2", "layer3", "layer4", "head")
    rec["median_per_lock_step_ms"] = {p: dict({k: med(p, lambda s, k=k: s[k]) for k in names}, stage=med(p, lambda s: s["stage_ms"])) for p in paths}
    rec["stage_median_of_each_run_ms"] = {p: [float(np.median([s["stage_ms"] for s in run])) for run in rec["runs"][p]] for p in paths}
    rec["layer4_median_of_each_run_ms"] = {p: [float(np.median([s["layer4"] for s in run])) for run in rec["runs"][p]] for p in paths}
    rec["three_launches_of_each_run_ms"] = {p: [r["ms_median"] for r in rec["block4_kernels"][p]] for p in paths}
    rec["three_launches_per_lock_step_ms"] = {p: float(np.median([r["ms_median"] * rows_step / r["rows"] for r in rec["block4_kernels"][p]])) for p in paths}
    three, m = rec["three_launches_of_each_run_ms"], rec["median_per_lock_step_ms"]
    rec["f16_over_fp32_three_launches"] = float(np.median(three["f16"]) / np.median(three["fp32"]))
    rec["f16_over_fp32_stage"] = m["f16"]["stage"] / m["fp32"]["stage"]
    rec["f16_three_launches_over_mfma_model"] = rec["three_launches_per_lock_step_ms"]["f16"] * (20480 / rows_step) / 1.71
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: rec[k] for k in ("median_per_lock_step_ms", "stage_median_of_each_run_ms", "layer4_median_of_each_run_ms", "three_launches_of_each_run_ms",
                                          "three_launches_per_lock_step_ms", "f16_over_fp32_three_launches", "f16_over_fp32_stage",
                                          "f16_three_launches_over_mfma_model", "chunk_pedestrians")}))
    for p in paths:
        r = rec["block4_kernels"][p][-1]
        print(p, json.dumps([(b["Cin"], b["stride"], b["ms_median"], b["TFMAps_median"], b["GBps_median"]) for b in r["blocks"]]))
        print(p, json.dumps({"all": (r["ms_median"], r["TFMAps_median"], r["GBps_median"])}))


def half_layer2_main(out_path, B, steps, dt, n_ped, K, reps):
    """``--half-layer2``: the whole network on the device with ``mmp_half=("layer3", "layer4")`` (layer2 on float32 operands: the parent
    arrangement) and with ``mmp_operands={"layer2": "f16"}`` on top (nmpc_mmp_block2_f16), alternated in one process: the four
    launches alone on one chunk, then the closed loop with events around every part."""
    from types import SimpleNamespace

    from dyobav_mpcnwta_warehouse_amd.mmp_stem import split_network_whole
    Hm, Wm, ref, tf, sc = _world(B, n_ped)
    torch.manual_seed(0)
    net = make_network(K).cuda().eval()
    as_block = lambda b: SimpleNamespace(conv1=b.a, conv2=b.b, downsample=b.skip, leaky=b.act)
    L = list(net)
    shaped = SimpleNamespace(resnet34=SimpleNamespace(stem=SimpleNamespace(conv1=L[0], pooling=L[1]), layer1=[as_block(b) for b in L[2:5]],
                                                      layer2=[as_block(b) for b in L[5:9]], layer3=[as_block(b) for b in L[9:15]],
                                                      layer4=[as_block(b) for b in L[15:18]], apool=L[18]), fc1=L[20], leaky=L[21], swarm=L[22])
    spec, blocks, blocks2, blocks3, blocks4, head = split_network_whole(shaped)
    head = head._replace(c2=head.c2 + np.float32(150.0))   # (the "+ 150" that puts the random network's hypotheses on the map)
    whole = dict(network=None, mmp_stem=spec, mmp_blocks=blocks, mmp_blocks2=blocks2, mmp_blocks3=blocks3, mmp_blocks4=blocks4, mmp_head=head,
                 mmp_half=("layer3", "layer4"))
    paths = {"fp32": dict(whole), "f16": dict(whole, mmp_operands={"layer2": "f16"})}

    def evaluator(path):
        return BatchEvaluator(nm.default_config_struct(), dtype=np.float32 if dt == "f32" else np.float64, predictor="mmp", mmp_hyp=K,
                              ref_image=ref, transform=tf, **paths[path], **sc)
    rows_step = B * n_ped * nm.default_config_struct().N_hor
    rec = {"what": "closed loop (row f3) on the reference scenarios, multi-hypothesis predictor stage, the whole network on the device, layer3 "
                   "and layer4 on binary16 operands in both arms: layer2 on float32 MFMA operands (nmpc_mmp_block2_f32, mmp_half = ('layer3', "
                   "'layer4')) and on binary16 operands with float32 accumulation (nmpc_mmp_block2_f16, mmp_operands = {'layer2': 'f16'} on "
                   "top), alternated in one process; random network of the reference's layer shapes",
           "B": B, "n_ped": n_ped, "n_hyp": K, "dtype": dt, "max_steps": steps, "map": [Hm, Wm], "repetitions": reps,
           "compared_with": {"float4_copy_TBps": COPY_TBS, "fp32_peak_TFMAps": PEAK_TFMAS},
           "model_of_the_f16_header_per_lock_step_ms": {"mfma_pipe_never_waits": 2.7, "activations_at_copy_rate": 5.8},
           "fp32_mfma_never_waits_floor_over_fp32_measured": 0.56, "chunk_pedestrians": {}, "block2_kernels": {p: [] for p in paths},
           "runs": {p: [] for p in paths}}
    for _ in range(reps):                                   # the four launches alone, three runs per arm, alternated (the first also warms up)
        for path in paths:
            ev = evaluator(path)
            rec["chunk_pedestrians"][path] = ev.mmp_chunk
            try:
                rec["block2_kernels"][path].append(block2_kernel_rate(ev, min(ev.mmp_chunk, B * n_ped)))
                ev.run(max_steps=1)
            finally:
                ev.close()
            r = rec["block2_kernels"][path][-1]
            print(path, json.dumps({"rows": r["rows"], "four_launches_ms": r["ms_median"], "each": [b["ms_median"] for b in r["blocks"]]}), flush=True)
            with open(out_path, "w") as f:
                json.dump(rec, f, indent=1)
    for _ in range(reps):
        for path in paths:
            ev = evaluator(path)
            ev.time_predictor = ev.time_predictor_parts = True
            try:
                res = ev.run(max_steps=steps)
            finally:
                ev.close()
            parts = ev.predictor_part_ms
            rec["runs"][path].append([dict(step=t, stage_ms=ev.predictor_ms[t], solve_ms=res.solve_ms[t], **{k: v[t] for k, v in parts.items()})
                                      for t in range(len(ev.predictor_ms))])
            print(path, json.dumps(rec["runs"][path][-1]), flush=True)
            with open(out_path, "w") as f:                  # (kept even if a later run does not finish)
                json.dump(rec, f, indent=1)
    med = lambda path, key: float(np.median([key(s) for run in rec["runs"][path] for s in run]))
    names = ("input", "layer1", "layer2", "layer3", "layer4", "head")
    rec["median_per_lock_step_ms"] = {p: dict({k: med(p, lambda s, k=k: s[k]) for k in names}, stage=med(p, lambda s: s["stage_ms"])) for p in paths}
    rec["stage_median_of_each_run_ms"] = {p: [float(np.median([s["stage_ms"] for s in run])) for run in rec["runs"][p]] for p in paths}
    rec["layer2_median_of_each_run_ms"] = {p: [float(np.median([s["layer2"] for s in run])) for run in rec["runs"][p]] for p in paths}
    rec["four_launches_of_each_run_ms"] = {p: [r["ms_median"] for r in rec["block2_kernels"][p]] for p in paths}
    rec["four_launches_per_lock_step_ms"] = {p: float(np.median([r["ms_median"] * rows_step / r["rows"] for r in rec["block2_kernels"][p]])) for p in paths}
    four, m = rec["four_launches_of_each_run_ms"], rec["median_per_lock_step_ms"]
    rec["f16_over_fp32_four_launches"] = float(np.median(four["f16"]) / np.median(four["fp32"]))
    rec["f16_over_fp32_stage"] = m["f16"]["stage"] / m["fp32"]["stage"]
    rec["f16_four_launches_over_mfma_model"] = rec["four_launches_per_lock_step_ms"]["f16"] * (20480 / rows_step) / 2.7
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: rec[k] for k in ("median_per_lock_step_ms", "stage_median_of_each_run_ms", "layer2_median_of_each_run_ms", "four_launches_of_each_run_ms",
                                          "four_launches_per_lock_step_ms", "f16_over_fp32_four_launches", "f16_over_fp32_stage",
                                          "f16_four_launches_over_mfma_model", "chunk_pedestrians")}))
    for p in paths:
        r = rec["block2_kernels"][p][-1]
        print(p, json.dumps([(b["Cin"], b["stride"], b["ms_median"], b["TFMAps_median"], b["GBps_median"]) for b in r["blocks"]]))
        print(p, json.dumps({"all": (r["ms_median"], r["TFMAps_median"], r["GBps_median"])}))


def activations_kernel_rate(ev, n_item, reps=10, names=("layer2", "layer3", "layer4")):
    """The 13 launches of layer2, layer3 and layer4 of the evaluator's front end alone on the layer1 output of ``n_item`` pedestrians:
    ms each and together (``run_block``: the launches only, nothing is decoded), and the bytes of x and out as they lie in memory.
    ``names`` beginning with ``"layer1"``: all 16 launches on the fill's output (the later stages' buffers lie inside it, so behind
    the first pass the first block reads what they left there: the time of a launch does not depend on the values)."""
    fe = ev.mmp_front
    rows = _fill(ev, n_item)().shape[0]
    fe.run_blocks(rows)
    first, stages = (0 if names[0] == "layer1" else len(fe.blocks)), [fe.stage(n) for n in names]
    count = sum(len(st.args) for st in stages)
    run_all = lambda: [fe.run_block(first + i, rows) for i in range(count)]
    run_all()
    rec, i = {"items": n_item, "rows": rows, "blocks": []}, first
    for st in stages:
        for j in range(len(st.args)):
            xh, oh = st.io[j] if st.io else (0, 0)
            (H, W), (H2, W2), Cin = st.planes[j], st.planes[j + 1], st.cins[j]
            nbytes = rows * ((2 if xh else 4) * Cin * H * W + (2 if oh else 4) * st.channels * H2 * W2)
            t = _timed(lambda i=i: fe.run_block(i, rows), reps, warm=3)
            rec["blocks"].append(dict(stage=st.name, Cin=Cin, plane_in=[H, W], plane_out=[H2, W2], x_f16=xh, out_f16=oh, bytes=nbytes,
                                      GBps_median=nbytes / t["ms_median"] * 1e-6, share_of_copy_rate=nbytes / t["ms_median"] * 1e-9 / COPY_TBS, **t))
            i += 1
    rec.update(bytes=sum(b["bytes"] for b in rec["blocks"]), **_timed(run_all, reps, warm=3))
    return rec


def activations_f16_main(out_path, B, steps, dt, n_ped, K, reps):
    """``--activations-f16``: the protocol of ``--half-layer2`` for binary16 activations in memory. Both arms run the whole network on
    the device with layer2, layer3 and layer4 on binary16 operands; ``f32`` keeps the activations float32 (``mmp_activations="f32"``: the
    parent's path), ``f16`` keeps them binary16 between those blocks (``mmp_activations="f16"``, nmpc_mmp_block{2,3,4}_f16_io),
    alternated in one process: the 13 launches alone on one chunk, then the closed loop with events around every part."""
    from types import SimpleNamespace

    from dyobav_mpcnwta_warehouse_amd.mmp_stem import split_network_whole
    Hm, Wm, ref, tf, sc = _world(B, n_ped)
    torch.manual_seed(0)
    net = make_network(K).cuda().eval()
    as_block = lambda b: SimpleNamespace(conv1=b.a, conv2=b.b, downsample=b.skip, leaky=b.act)
    L = list(net)
    shaped = SimpleNamespace(resnet34=SimpleNamespace(stem=SimpleNamespace(conv1=L[0], pooling=L[1]), layer1=[as_block(b) for b in L[2:5]],
                                                      layer2=[as_block(b) for b in L[5:9]], layer3=[as_block(b) for b in L[9:15]],
                                                      layer4=[as_block(b) for b in L[15:18]], apool=L[18]), fc1=L[20], leaky=L[21], swarm=L[22])
    spec, blocks, blocks2, blocks3, blocks4, head = split_network_whole(shaped)
    head = head._replace(c2=head.c2 + np.float32(150.0))   # (the "+ 150" that puts the random network's hypotheses on the map)
    whole = dict(network=None, mmp_stem=spec, mmp_blocks=blocks, mmp_blocks2=blocks2, mmp_blocks3=blocks3, mmp_blocks4=blocks4, mmp_head=head,
                 mmp_operands={"layer2": "f16", "layer3": "f16", "layer4": "f16"})
    paths = {"f32": dict(whole, mmp_activations="f32"), "f16": dict(whole, mmp_activations="f16")}

    def evaluator(path):
        return BatchEvaluator(nm.default_config_struct(), dtype=np.float32 if dt == "f32" else np.float64, predictor="mmp", mmp_hyp=K,
                              ref_image=ref, transform=tf, **paths[path], **sc)
    rows_step = B * n_ped * nm.default_config_struct().N_hor
    rec = {"what": "closed loop (row f3) on the reference scenarios, multi-hypothesis predictor stage, the whole network on the device, layer2, "
                   "layer3 and layer4 on binary16 operands in both arms: activations float32 in memory (mmp_activations = 'f32', the parent's "
                   "path) and binary16 in the octet form between those blocks (mmp_activations = 'f16', nmpc_mmp_block{2,3,4}_f16_io), "
                   "alternated in one process; random network of the reference's layer shapes",
           "B": B, "n_ped": n_ped, "n_hyp": K, "dtype": dt, "max_steps": steps, "map": [Hm, Wm], "repetitions": reps,
           "compared_with": {"float4_copy_TBps": COPY_TBS}, "chunk_pedestrians": {}, "kernels": {p: [] for p in paths}, "runs": {p: [] for p in paths}}
    for _ in range(reps):                                   # the 13 launches alone, per arm, alternated (the first also warms up)
        for path in paths:
            ev = evaluator(path)
            rec["chunk_pedestrians"][path] = ev.mmp_chunk
            try:
                rec["kernels"][path].append(activations_kernel_rate(ev, min(ev.mmp_chunk, B * n_ped)))
                ev.run(max_steps=1)
            finally:
                ev.close()
            r = rec["kernels"][path][-1]
            print(path, json.dumps({"rows": r["rows"], "thirteen_launches_ms": r["ms_median"], "each": [b["ms_median"] for b in r["blocks"]]}), flush=True)
            with open(out_path, "w") as f:
                json.dump(rec, f, indent=1)
    for _ in range(reps):
        for path in paths:
            ev = evaluator(path)
            ev.time_predictor = ev.time_predictor_parts = True
            try:
                res = ev.run(max_steps=steps)
            finally:
                ev.close()
            parts = ev.predictor_part_ms
            rec["runs"][path].append([dict(step=t, stage_ms=ev.predictor_ms[t], solve_ms=res.solve_ms[t], **{k: v[t] for k, v in parts.items()})
                                      for t in range(len(ev.predictor_ms))])
            print(path, json.dumps(rec["runs"][path][-1]), flush=True)
            with open(out_path, "w") as f:                  # (kept even if a later run does not finish)
                json.dump(rec, f, indent=1)
    med = lambda path, key: float(np.median([key(s) for run in rec["runs"][path] for s in run]))
    names = ("input", "layer1", "layer2", "layer3", "layer4", "head")
    spread = lambda v: (max(v) - min(v)) / float(np.median(v))
    rec["median_per_lock_step_ms"] = {p: dict({k: med(p, lambda s, k=k: s[k]) for k in names}, stage=med(p, lambda s: s["stage_ms"])) for p in paths}
    rec["stage_median_of_each_run_ms"] = {p: [float(np.median([s["stage_ms"] for s in run])) for run in rec["runs"][p]] for p in paths}
    rec["thirteen_launches_of_each_run_ms"] = {p: [r["ms_median"] for r in rec["kernels"][p]] for p in paths}
    rec["thirteen_launches_per_lock_step_ms"] = {p: float(np.median([r["ms_median"] * rows_step / r["rows"] for r in rec["kernels"][p]])) for p in paths}
    rec["each_block_median_ms"] = {p: [float(np.median([r["blocks"][i]["ms_median"] for r in rec["kernels"][p]])) for i in range(13)] for p in paths}
    thirteen, stage = rec["thirteen_launches_of_each_run_ms"], rec["stage_median_of_each_run_ms"]
    rec["run_to_run_spread"] = {"thirteen_launches": {p: spread(thirteen[p]) for p in paths}, "stage": {p: spread(stage[p]) for p in paths}}
    rec["f16_over_f32_thirteen_launches_of_each_run"] = [a / b for a, b in zip(thirteen["f16"], thirteen["f32"])]
    rec["f16_over_f32_stage_of_each_run"] = [a / b for a, b in zip(stage["f16"], stage["f32"])]
    # the criterion: in every run the f16 arm is below the f32 arm by more than the larger of the two arms' run-to-run spreads
    rec["margin"] = {"thirteen_launches": max(rec["run_to_run_spread"]["thirteen_launches"].values()), "stage": max(rec["run_to_run_spread"]["stage"].values())}
    rec["faster_in_every_run"] = {"thirteen_launches": all(r < 1.0 - rec["margin"]["thirteen_launches"] for r in rec["f16_over_f32_thirteen_launches_of_each_run"]),
                                  "stage": all(r < 1.0 - rec["margin"]["stage"] for r in rec["f16_over_f32_stage_of_each_run"])}
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: rec[k] for k in ("median_per_lock_step_ms", "stage_median_of_each_run_ms", "thirteen_launches_of_each_run_ms",
                                          "thirteen_launches_per_lock_step_ms", "each_block_median_ms", "run_to_run_spread",
                                          "f16_over_f32_thirteen_launches_of_each_run", "f16_over_f32_stage_of_each_run", "margin", "faster_in_every_run",
                                          "chunk_pedestrians")}))


def half_layer1_main(out_path, B, steps, dt, n_ped, K, reps):
    """``--half-layer1``: the protocol of ``--half-layer2`` for layer1 on binary16 operands (``nmpc_mmp_block_f16``), reached by the
    switch for the whole network. Both arms run the whole network on the device, alternated in one process: ``parent`` is layer2 ..
    layer4 on binary16 operands with binary16 activations between them and layer1 on float32 (``mmp_operands`` + ``mmp_activations =
    "f16"``: the fastest path without this kernel), ``f16`` is ``mmp_precision="f16"``. The 16 launches alone on one chunk per run and
    per block, then the closed loop with events around every part. The criterion is the sibling records': layer1's three launches
    faster in every run by more than the larger of the two arms' run-to-run spreads, the stage not slower by more than its own."""
    from types import SimpleNamespace

    from dyobav_mpcnwta_warehouse_amd.mmp_stem import split_network_whole
    Hm, Wm, ref, tf, sc = _world(B, n_ped)
    torch.manual_seed(0)
    net = make_network(K).cuda().eval()
    as_block = lambda b: SimpleNamespace(conv1=b.a, conv2=b.b, downsample=b.skip, leaky=b.act)
    L = list(net)
    shaped = SimpleNamespace(resnet34=SimpleNamespace(stem=SimpleNamespace(conv1=L[0], pooling=L[1]), layer1=[as_block(b) for b in L[2:5]],
                                                      layer2=[as_block(b) for b in L[5:9]], layer3=[as_block(b) for b in L[9:15]],
                                                      layer4=[as_block(b) for b in L[15:18]], apool=L[18]), fc1=L[20], leaky=L[21], swarm=L[22])
    spec, blocks, blocks2, blocks3, blocks4, head = split_network_whole(shaped)
    head = head._replace(c2=head.c2 + np.float32(150.0))   # (the "+ 150" that puts the random network's hypotheses on the map)
    whole = dict(network=None, mmp_stem=spec, mmp_blocks=blocks, mmp_blocks2=blocks2, mmp_blocks3=blocks3, mmp_blocks4=blocks4, mmp_head=head)
    paths = {"parent": dict(whole, mmp_operands={"layer2": "f16", "layer3": "f16", "layer4": "f16"}, mmp_activations="f16"),
             "f16": dict(whole, mmp_precision="f16")}
    layers = ("layer1", "layer2", "layer3", "layer4")

    def evaluator(path):
        return BatchEvaluator(nm.default_config_struct(), dtype=np.float32 if dt == "f32" else np.float64, predictor="mmp", mmp_hyp=K,
                              ref_image=ref, transform=tf, **paths[path], **sc)
    rows_step = B * n_ped * nm.default_config_struct().N_hor
    rec = {"what": "closed loop (row f3) on the reference scenarios, multi-hypothesis predictor stage, the whole network on the device: layer2, "
                   "layer3 and layer4 on binary16 operands with binary16 activations between them and layer1 on float32 (arm 'parent': "
                   "nmpc_mmp_block_f32) against the whole network on binary16 operands from layer1 on (arm 'f16': mmp_precision = 'f16', "
                   "nmpc_mmp_block_f16_io), alternated in one process; random network of the reference's layer shapes",
           "B": B, "n_ped": n_ped, "n_hyp": K, "dtype": dt, "max_steps": steps, "map": [Hm, Wm], "repetitions": reps,
           "compared_with": {"float4_copy_TBps": COPY_TBS, "fp32_peak_TFMAps": PEAK_TFMAS},
           "model_of_the_f16_header_per_lock_step_ms": {"mfma_pipe_never_waits": 4.4, "activations_at_copy_rate": 10.0},
           "chunk_pedestrians": {}, "kernels": {p: [] for p in paths}, "runs": {p: [] for p in paths}}
    for _ in range(reps):                                   # the 16 launches alone, per arm, alternated (the first also warms up)
        for path in paths:
            ev = evaluator(path)
            rec["chunk_pedestrians"][path] = ev.mmp_chunk
            try:
                rec["kernels"][path].append(activations_kernel_rate(ev, min(ev.mmp_chunk, B * n_ped), names=layers))
                ev.run(max_steps=1)
            finally:
                ev.close()
            r = rec["kernels"][path][-1]
            print(path, json.dumps({"rows": r["rows"], "sixteen_launches_ms": r["ms_median"], "each": [b["ms_median"] for b in r["blocks"]]}), flush=True)
            with open(out_path, "w") as f:
                json.dump(rec, f, indent=1)
    for _ in range(reps):
        for path in paths:
            ev = evaluator(path)
            ev.time_predictor = ev.time_predictor_parts = True
            try:
                res = ev.run(max_steps=steps)
            finally:
                ev.close()
            parts = ev.predictor_part_ms
            rec["runs"][path].append([dict(step=t, stage_ms=ev.predictor_ms[t], solve_ms=res.solve_ms[t], **{k: v[t] for k, v in parts.items()})
                                      for t in range(len(ev.predictor_ms))])
            print(path, json.dumps(rec["runs"][path][-1]), flush=True)
            with open(out_path, "w") as f:                  # (kept even if a later run does not finish)
                json.dump(rec, f, indent=1)
    med = lambda path, key: float(np.median([key(s) for run in rec["runs"][path] for s in run]))
    names = ("input",) + layers + ("head",)
    spread = lambda v: (max(v) - min(v)) / float(np.median(v))
    rec["median_per_lock_step_ms"] = {p: dict({k: med(p, lambda s, k=k: s[k]) for k in names}, stage=med(p, lambda s: s["stage_ms"])) for p in paths}
    rec["stage_median_of_each_run_ms"] = {p: [float(np.median([s["stage_ms"] for s in run])) for run in rec["runs"][p]] for p in paths}
    rec["layer1_median_of_each_run_ms"] = {p: [float(np.median([s["layer1"] for s in run])) for run in rec["runs"][p]] for p in paths}
    rec["each_block_median_ms"] = {p: [float(np.median([r["blocks"][i]["ms_median"] for r in rec["kernels"][p]])) for i in range(16)] for p in paths}
    rec["each_block_GBps_median"] = {p: [float(np.median([r["blocks"][i]["GBps_median"] for r in rec["kernels"][p]])) for i in range(16)] for p in paths}
    rec["layer1_three_launches_of_each_run_ms"] = {p: [sum(b["ms_median"] for b in r["blocks"][:3]) for r in rec["kernels"][p]] for p in paths}
    rec["layer1_three_launches_per_lock_step_ms"] = {p: float(np.median([sum(b["ms_median"] for b in r["blocks"][:3]) * rows_step / r["rows"]
                                                                          for r in rec["kernels"][p]])) for p in paths}
    three, stage = rec["layer1_three_launches_of_each_run_ms"], rec["stage_median_of_each_run_ms"]
    rec["run_to_run_spread"] = {"layer1_three_launches": {p: spread(three[p]) for p in paths}, "stage": {p: spread(stage[p]) for p in paths}}
    rec["f16_over_parent_layer1_three_launches_of_each_run"] = [a / b for a, b in zip(three["f16"], three["parent"])]
    rec["f16_over_parent_stage_of_each_run"] = [a / b for a, b in zip(stage["f16"], stage["parent"])]
    rec["margin"] = {"layer1_three_launches": max(rec["run_to_run_spread"]["layer1_three_launches"].values()), "stage": max(rec["run_to_run_spread"]["stage"].values())}
    # the two conditions: layer1 faster in every run by more than the margin; the stage not slower by more than its margin
    rec["conditions"] = {"layer1_faster_in_every_run": all(r < 1.0 - rec["margin"]["layer1_three_launches"] for r in rec["f16_over_parent_layer1_three_launches_of_each_run"]),
                         "stage_not_slower": all(r <= 1.0 + rec["margin"]["stage"] for r in rec["f16_over_parent_stage_of_each_run"])}
    rec["f16_layer1_over_mfma_model"] = rec["layer1_three_launches_per_lock_step_ms"]["f16"] * (20480 / rows_step) / 4.4
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: rec[k] for k in ("median_per_lock_step_ms", "stage_median_of_each_run_ms", "layer1_median_of_each_run_ms", "each_block_median_ms",
                                          "each_block_GBps_median", "layer1_three_launches_of_each_run_ms", "layer1_three_launches_per_lock_step_ms",
                                          "run_to_run_spread", "f16_over_parent_layer1_three_launches_of_each_run", "f16_over_parent_stage_of_each_run",
                                          "margin", "conditions", "f16_layer1_over_mfma_model", "chunk_pedestrians")}))


def fill_launch_rate(ev, n_item, reps=10):
    """ms and GB/s stored of the fill's launch alone (``nmpc_mmp_stem_*`` or ``nmpc_mmp_stem_io_*``: nothing is decoded) on ``n_item``
    pedestrians of the evaluator's start state, with the bytes of its output as they lie in memory."""
    fe = ev.mmp_front
    fe.allocate(n_item)
    hist, hcount = ev.hist.contiguous(), ev.hcount.contiguous()
    t = _timed(lambda: fe._launch_fill(hist.data_ptr(), hcount.data_ptr(), ev.B, ev.H, None, n_item), reps, warm=3)
    nbytes = n_item * ev.N * int(np.prod(fe.fill_row)) * (2 if fe.fill_f16 else 4)
    return {"items": n_item, "out_f16": int(fe.fill_f16), "bytes_stored": nbytes, **t, "store_GBps_median": nbytes / t["ms_median"] * 1e-6}


def fill_f16_main(out_path, B, steps, dt, n_ped, K, reps):
    """``--fill-f16``: the protocol of ``--half-layer1`` for the fused first layer writing binary16 (``nmpc_mmp_stem_io_*``). Both arms
    run the whole network on the device on binary16 operands, alternated in one process: ``parent`` is ``mmp_precision="f16"``,
    ``fill16`` the same with ``mmp_fill="f16"``. The fill's launch and the 16 block launches alone on one chunk per run and per block,
    then the closed loop with events around every part. The two merge conditions, each in each run against the parent arm of the same
    process: (a) the stage per lock-step faster by more than the larger of the two arms' run-to-run spreads; (b) neither ``input``
    nor layer1's first block slower."""
    from types import SimpleNamespace

    from dyobav_mpcnwta_warehouse_amd.mmp_stem import split_network_whole
    Hm, Wm, ref, tf, sc = _world(B, n_ped)
    torch.manual_seed(0)
    net = make_network(K).cuda().eval()
    as_block = lambda b: SimpleNamespace(conv1=b.a, conv2=b.b, downsample=b.skip, leaky=b.act)
    L = list(net)
    shaped = SimpleNamespace(resnet34=SimpleNamespace(stem=SimpleNamespace(conv1=L[0], pooling=L[1]), layer1=[as_block(b) for b in L[2:5]],
                                                      layer2=[as_block(b) for b in L[5:9]], layer3=[as_block(b) for b in L[9:15]],
                                                      layer4=[as_block(b) for b in L[15:18]], apool=L[18]), fc1=L[20], leaky=L[21], swarm=L[22])
    spec, blocks, blocks2, blocks3, blocks4, head = split_network_whole(shaped)
    head = head._replace(c2=head.c2 + np.float32(150.0))   # (the "+ 150" that puts the random network's hypotheses on the map)
    whole = dict(network=None, mmp_stem=spec, mmp_blocks=blocks, mmp_blocks2=blocks2, mmp_blocks3=blocks3, mmp_blocks4=blocks4, mmp_head=head,
                 mmp_precision="f16")
    paths = {"parent": dict(whole), "fill16": dict(whole, mmp_fill="f16")}
    layers = ("layer1", "layer2", "layer3", "layer4")

    def evaluator(path):
        return BatchEvaluator(nm.default_config_struct(), dtype=np.float32 if dt == "f32" else np.float64, predictor="mmp", mmp_hyp=K,
                              ref_image=ref, transform=tf, **paths[path], **sc)
    rows_step = B * n_ped * nm.default_config_struct().N_hor
    rec = {"what": "closed loop (row f3) on the reference scenarios, multi-hypothesis predictor stage, the whole network on the device on "
                   "binary16 operands with binary16 activations between all blocks in both arms: the fused first layer writing float32 (arm "
                   "'parent': mmp_precision = 'f16', nmpc_mmp_stem_*) against the same layer writing binary16 in the octet form, which "
                   "layer1's first block reads as such (arm 'fill16': mmp_fill = 'f16', nmpc_mmp_stem_io_*), alternated in one process; "
                   "random network of the reference's layer shapes",
           "B": B, "n_ped": n_ped, "n_hyp": K, "dtype": dt, "max_steps": steps, "map": [Hm, Wm], "repetitions": reps,
           "compared_with": {"float4_copy_TBps": COPY_TBS}, "chunk_pedestrians": {}, "bytes_per_item": {},
           "fill": {p: [] for p in paths}, "kernels": {p: [] for p in paths}, "runs": {p: [] for p in paths}}
    for _ in range(reps):                                   # the launches alone, per arm, alternated (the first also warms up)
        for path in paths:
            ev = evaluator(path)
            rec["chunk_pedestrians"][path], rec["bytes_per_item"][path] = ev.mmp_chunk, ev.mmp_front.bytes_per_item
            try:
                n_item = min(ev.mmp_chunk, B * n_ped)
                rec["fill"][path].append(fill_launch_rate(ev, n_item))
                rec["kernels"][path].append(activations_kernel_rate(ev, n_item, names=layers))
                ev.run(max_steps=1)
            finally:
                ev.close()
            r, f = rec["kernels"][path][-1], rec["fill"][path][-1]
            print(path, json.dumps({"items": f["items"], "fill_ms": f["ms_median"], "fill_GBps": f["store_GBps_median"], "rows": r["rows"],
                                    "sixteen_launches_ms": r["ms_median"], "each": [b["ms_median"] for b in r["blocks"]]}), flush=True)
            with open(out_path, "w") as f:
                json.dump(rec, f, indent=1)
    for _ in range(reps):
        for path in paths:
            ev = evaluator(path)
            ev.time_predictor = ev.time_predictor_parts = True
            try:
                res = ev.run(max_steps=steps)
            finally:
                ev.close()
            parts = ev.predictor_part_ms
            rec["runs"][path].append([dict(step=t, stage_ms=ev.predictor_ms[t], solve_ms=res.solve_ms[t], **{k: v[t] for k, v in parts.items()})
                                      for t in range(len(ev.predictor_ms))])
            print(path, json.dumps(rec["runs"][path][-1]), flush=True)
            with open(out_path, "w") as f:                  # (kept even if a later run does not finish)
                json.dump(rec, f, indent=1)
    med = lambda path, key: float(np.median([key(s) for run in rec["runs"][path] for s in run]))
    names = ("input",) + layers + ("head",)
    spread = lambda v: (max(v) - min(v)) / float(np.median(v))
    per_run = lambda key: {p: [float(np.median([s[key] for s in run])) for run in rec["runs"][p]] for p in paths}
    rec["median_per_lock_step_ms"] = {p: dict({k: med(p, lambda s, k=k: s[k]) for k in names}, stage=med(p, lambda s: s["stage_ms"])) for p in paths}
    rec["stage_median_of_each_run_ms"], rec["input_median_of_each_run_ms"] = per_run("stage_ms"), per_run("input")
    rec["layer1_median_of_each_run_ms"] = per_run("layer1")
    rec["each_block_median_ms"] = {p: [float(np.median([r["blocks"][i]["ms_median"] for r in rec["kernels"][p]])) for i in range(16)] for p in paths}
    rec["each_block_GBps_median"] = {p: [float(np.median([r["blocks"][i]["GBps_median"] for r in rec["kernels"][p]])) for i in range(16)] for p in paths}
    # per lock-step: the launch alone on one chunk, scaled to the rows of a lock-step (the arms' chunks differ: bytes_per_item does)
    rec["rows_of_a_chunk"] = {p: rec["kernels"][p][0]["rows"] for p in paths}
    rec["each_block_per_lock_step_ms"] = {p: [float(np.median([r["blocks"][i]["ms_median"] * rows_step / r["rows"] for r in rec["kernels"][p]]))
                                              for i in range(16)] for p in paths}
    rec["fill_launch_of_each_run_ms"] = {p: [f["ms_median"] * B * n_ped / f["items"] for f in rec["fill"][p]] for p in paths}
    rec["fill_store_GBps_of_each_run"] = {p: [f["store_GBps_median"] for f in rec["fill"][p]] for p in paths}
    rec["first_block_of_each_run_ms"] = {p: [r["blocks"][0]["ms_median"] * rows_step / r["rows"] for r in rec["kernels"][p]] for p in paths}
    stage, inp, first, fill = (rec[k] for k in ("stage_median_of_each_run_ms", "input_median_of_each_run_ms", "first_block_of_each_run_ms",
                                                "fill_launch_of_each_run_ms"))
    rec["run_to_run_spread"] = {"stage": {p: spread(stage[p]) for p in paths}}
    ratio = lambda v: [a / b for a, b in zip(v["fill16"], v["parent"])]
    rec["fill16_over_parent_of_each_run"] = {"stage": ratio(stage), "input": ratio(inp), "first_block": ratio(first), "fill_launch": ratio(fill)}
    rec["margin"] = {"stage": max(rec["run_to_run_spread"]["stage"].values())}
    # (a) the stage faster in every run by more than the margin; (b) neither input nor layer1's first block slower in any run
    rec["conditions"] = {"a_stage_faster_in_every_run": all(r < 1.0 - rec["margin"]["stage"] for r in rec["fill16_over_parent_of_each_run"]["stage"]),
                         "b_input_not_slower": all(r <= 1.0 for r in rec["fill16_over_parent_of_each_run"]["input"]),
                         "b_first_block_not_slower": all(r <= 1.0 for r in rec["fill16_over_parent_of_each_run"]["first_block"])}
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: rec[k] for k in ("median_per_lock_step_ms", "stage_median_of_each_run_ms", "input_median_of_each_run_ms",
                                          "layer1_median_of_each_run_ms", "rows_of_a_chunk", "each_block_median_ms", "each_block_per_lock_step_ms",
                                          "each_block_GBps_median", "fill_launch_of_each_run_ms",
                                          "fill_store_GBps_of_each_run", "first_block_of_each_run_ms", "run_to_run_spread",
                                          "fill16_over_parent_of_each_run", "margin", "conditions", "chunk_pedestrians", "bytes_per_item")}))


def main():
    for flag, run in (("--fill-f16", fill_f16_main), ("--half-layer1", half_layer1_main), ("--activations-f16", activations_f16_main), ("--half-layer2", half_layer2_main), ("--half-layer4", half_layer4_main), ("--half-layer3", half_layer3_main), ("--fused-layer4", fused_layer4_main), ("--fused-layer3", fused_layer3_main), ("--fused-layer2", fused_layer2_main), ("--fused-layer1", fused_layer1_main), ("--fused-stem", fused_stem_main)):
        if flag in sys.argv:
            i = sys.argv.index(flag)
            reps = int(sys.argv[i + 1]) if len(sys.argv) > i + 1 else 3
            argv = sys.argv[1:i]
            B, steps, dt, n_ped, K = (argv[1:] + ["256", "3", "f32", "4", "20"][len(argv) - 1:])[:5]
            return run(argv[0], int(B), int(steps), dt, int(n_ped), int(K), reps)
    out_path = sys.argv[1]
    B, steps, dt, n_ped, K = (sys.argv[2:] + ["256", "3", "f32", "4", "20"][len(sys.argv) - 2:])[:5]
    B, steps, n_ped, K = int(B), int(steps), int(n_ped), int(K)
    Hm, Wm, ref, tf, sc = _world(B, n_ped)
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
