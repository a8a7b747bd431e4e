#!/usr/bin/env python3
"""Record the architecture of the multi-hypothesis predictor's network from THE REFERENCE'S OWN CLASS,
``pkg_motion_prediction.net_module.net.ConvMultiHypoNet(7, 2, fc_input, K, lite=True)``: built, put in ``eval()``, filled by the
rule of tests/mmp_net_reference.py (``fill_by_rule``: no trained weights exist) and run in float64 on the CPU. Runs only in the
authoring container (needs /root/reference); what it writes is data:

  mmp_net.json   per shape of ``mmp_net_reference.SHAPES`` (the 37 x 41 map with fc_input 128 and K = 3; the 293 x 329 map with
                 fc_input 3 200 and K = 10): the ``(name, shape)`` list of the class's ``state_dict()``, 226 entries in its order; for
                 the input ``rule_input(Hm, Wm)`` ``[4, 7, Hm, Wm]`` (made by rule, not stored) the float64 output of the class's own
                 ``forward`` in full; 64 hashed positions of each of the five tensors in front of the head (``sample_index``).

Before anything is written, the stand-in ``mmp_net_reference.Net`` is compared with the class: the same entries, the same values at
every stage to 1e-10 relative. One thread, so that the sums come out in one order.

Usage:  python tests/golden/make_mmp_net_golden.py [out_dir]
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REF, "src"))

import mmp_net_reference as nr  # noqa: E402

RTOL = 1e-10


def entries(module):
    return [[name, [int(v) for v in t.shape]] for name, t in module.state_dict().items()]


def record(shape):
    from pkg_motion_prediction.net_module.net import ConvMultiHypoNet
    ref = nr.fill_by_rule(ConvMultiHypoNet(7, 2, shape["fc_input"], shape["K"], lite=True).eval()).double()
    x = nr.rule_input(shape["Hm"], shape["Wm"])
    got = nr.stages(ref, x)
    with torch.no_grad():
        out = ref(torch.from_numpy(x).double())             # the class's own forward, not the helper's walk through its members
    assert out.shape == (4, 2 * shape["K"]) and torch.equal(out, got[5])
    net = nr.made_net(shape)
    assert entries(net) == entries(ref) and len(entries(ref)) == 226
    for name, a, b in zip(nr.STAGE_NAMES, nr.stages(nr.in_double(net), x), got):
        assert a.shape == b.shape and float((a - b).abs().max()) <= RTOL * float(b.abs().max()), name
    samples = {}
    for name, t in zip(nr.STAGE_NAMES[:5], got):
        idx = nr.sample_index(name, t.numel())
        samples[name] = {"shape": [int(v) for v in t.shape], "values": [float(v) for v in t.reshape(-1)[torch.from_numpy(idx)]]}
    return {**shape, "state_dict": entries(ref), "output": [[float(v) for v in row] for row in out], "samples": samples}


def main(out_dir=HERE):
    torch.set_num_threads(1)
    doc = {"shapes": [record(shape) for shape in nr.SHAPES]}
    path = os.path.join(out_dir, "mmp_net.json")
    with open(path, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(doc['shapes'])} shapes, {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main(*sys.argv[1:2])
