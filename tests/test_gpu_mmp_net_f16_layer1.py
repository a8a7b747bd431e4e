"""GPU test of the WHOLE network on the device on binary16 MFMA operands from layer1 on -- ``MmpFrontEnd(..., precision="f16")``,
csrc/nmpc_mmp_block1_f16.h -- against the float64 module, by the protocol of tests/test_gpu_mmp_net_f16_layer2.py and
tests/test_gpu_mmp_front_activations.py, with the real-valued network, worlds and float64 module of tests/test_gpu_mmp_net.py: the
37 x 41 map on M = 4 rows in the suite; the 293 x 329 one (M = 2) once by hand through ``accuracy(handle, 1)``.

Yardstick: the rule's own cost. ``model_chain`` (tests/mmp_act_f16_reference.py on tests/mmp_block{1,2,3,4}_f16_reference.py) -- the
rounding rule in float64, m rounded, every tensor between two blocks rounded to binary16, the 16 blocks one after the other -- runs
on the float64 module's stem output; the float64 module's head finishes it. Its distance from the float64 module at layer1, layer2,
layer3, layer4 and the output is what the rule costs on this input, with no float32 effect in it. Bar: the device lies within
``mmp_net_reference.BAR`` = 4 times that yardstick from the float64 module at all five. The distance from the model itself is printed
and NOT a criterion.

Measured on an MI355X, |device - float64| / yardstick (the bar is 4) and |device - model| / yardstick:

    map          M    layer1        layer2        layer3        layer4        output
    37 x 41      4    1.00  0.52    0.91  0.94    1.16  0.83    1.13  1.09    0.58  0.64
    293 x 329    2    1.00  0.88    1.00  0.86    1.31  0.94    1.09  1.00    0.92  0.67      (by hand; not in the suite)

The yardsticks themselves: 7.4e-3 / 8.3e-3 / 9.4e-3 / 3.9e-3 / 3.8e-4 on the small map (with layer2 .. layer4 only: - / 5.6e-3 / 6.3e-3 /
3.7e-3 / 3.7e-4), 6.6e-3 / 9.0e-3 / 1.7e-2 / 1.5e-2 / 1.1e-3 on the large one (- / 7.6e-3 / 1.5e-2 / 1.8e-2 / 8.2e-4)."""
import numpy as np
import pytest
import torch

import mmp_act_f16_reference as ha
import mmp_block1_f16_reference as h1
import mmp_block2_f16_reference as h2
import mmp_block3_f16_reference as h3
import mmp_block4_f16_reference as h4
import mmp_net_reference as nr
import test_gpu_mmp_front_activations as fa
import test_gpu_mmp_net as tn

pytestmark = pytest.mark.gpu

handle = tn.handle
LAYERS = fa.LAYERS
ARGS = ("blocks", "blocks2", "blocks3", "blocks4")


def accuracy(handle, k):
    """|device - float64 module| over the yardstick |model_chain - float64 module| at layer1 .. layer4 and the output on shape ``k``;
    prints the yardsticks, those of layer2 .. layer4 alone on f16 (today's fastest path) beside them."""
    w = fa._net(k)
    net64, want, specs, rows = w["net64"], w["want"], w["specs"], w["rows"]
    stages = [(name, len(specs[arg])) for name, arg in zip(LAYERS, ARGS)]

    def model(operands):
        flags = ha.binary16_outputs(stages, operands, "f16")
        x, out = want[0].astype(np.float32), []
        for (name, _), arg, h in zip(stages, ARGS, (h1, h2, h3, h4)):
            if operands.get(name) == "f16":
                x = ha.model_chain(h, x, specs[arg], flags[name])[-1]
            else:                                                        # (the parent arm: layer1 is the float64 module's)
                x = want[1 + LAYERS.index(name)].astype(np.float32)
            out.append(np.asarray(x, dtype=np.float64))
        with torch.no_grad():
            out.append(nr.finish(net64, torch.as_tensor(out[-1]).double(), 4).numpy())
        return out
    mine, parent = model({name: "f16" for name in LAYERS}), model(fa.ALL3)
    yard = [float(np.abs(m - t).max()) for m, t in zip(mine, want[1:])]
    yard0 = [float(np.abs(m - t).max()) for m, t in zip(parent, want[1:])]
    assert all(y > 0 for y in yard) and yard0[0] < yard[0]
    got = [g.cpu().numpy() for g in fa._by_stage(fa._front(handle, w, precision="f16"), w)]
    ratios = []
    for name, g, t, m, y, y0 in zip(nr.STAGE_NAMES[1:], got, want[1:], mine, yard, yard0):
        assert g.shape == t.shape == m.shape and g.shape[0] == rows and np.isfinite(g).all()
        r64, rm = float(np.abs(g - t).max()) / y, float(np.abs(g - m).max()) / y
        print(f"{w['Hm']} x {w['Wm']} M {rows} {name}: yardstick |model - float64| = {y:.3e} (layer2 .. layer4 only: {y0:.3e}; "
              f"|float64| up to {np.abs(t).max():.2f}); |device - float64| / yardstick = {r64:.2f}, |device - model| / yardstick = {rm:.2f}")
        ratios.append(r64)
    return ratios


def test_whole_network_in_f16_from_layer1_against_the_float64_module(handle):
    ratios = accuracy(handle, 0)
    assert len(ratios) == 5 and max(ratios) <= nr.BAR, ratios
