"""GPU test of the WHOLE network on the device with layer2 on binary16 MFMA operands -- ``MmpFrontEnd(..., operands={"layer2":
"f16"})`` and all three of layer2, layer3 and layer4 on them, csrc/nmpc_mmp_block2_f16.h --, with the real-valued network, worlds and
float64 module of tests/test_gpu_mmp_net.py and the two shapes of tests/test_gpu_mmp_net_f16.py: the 37 x 41 map on M = 4 rows, the
293 x 329 one (the warehouse's planes) on M = 2.

Yardstick: the rule's own cost. ``mmp_block2_f16_reference.model_chain`` -- the rounding rule in float64, m rounded, the four blocks
of layer2 one after the other -- runs on the float64 module's layer1 output; behind it the float64 module's layer3 and layer4 or,
with all three stages on, their own ``model_chain`` (tests/mmp_block3_f16_reference.py, tests/mmp_block4_f16_reference.py); the
float64 module's head finishes it. Its distance from the float64 module at layer2, layer3, layer4 and the output is what rounding
the operands to binary16 costs on this input, with no float32 effect in it. Bar: the device lies within ``BAR`` = 4 times that
yardstick from the float64 module at all four, the project's standing margin over a rounding yardstick (tests/mmp_net_reference.py).
The distance from the model itself is printed and NOT a criterion: one float32 bit of difference in x or m flips a binary16 rounding
now and then, and the maximum over a plane finds those.

Measured on an MI355X, |device - float64| / yardstick (the bar is 4) and |device - model| / yardstick:

    map          M    on f16       layer2        layer3        layer4        output
    37 x 41      4    layer2       0.99  0.43    0.87  0.33    0.95  0.64    1.04  0.52
    37 x 41      4    all three    0.99  0.43    0.98  0.68    1.54  0.88    1.34  0.62
    293 x 329    2    layer2       0.95  0.56    1.05  0.37    1.00  0.42    0.98  0.19
    293 x 329    2    all three    0.95  0.56    0.89  0.88    1.03  0.81    0.99  0.80

The yardsticks themselves, layer2 / layer3 / layer4 / output: 4.0e-3 / 3.7e-3 / 1.4e-3 / 1.1e-4 and 4.0e-3 / 5.3e-3 / 2.2e-3 / 2.3e-4 on
the small map (values up to 6.46 / 7.99 / 4.27 / 0.91), 4.8e-3 / 9.7e-3 / 6.3e-3 / 5.4e-4 and 4.8e-3 / 1.4e-2 / 1.1e-2 / 7.0e-4 on the
large one (up to 7.90 / 10.38 / 12.05 / 1.72). The same chain on the CPU, ``emulate`` in the kernel's place
(tests/test_mmp_block2_f16_cpu.py): 1.11 / 1.02 / 1.11 / 0.91 on 37 x 41 and 1.06 / 1.03 / 1.01 / 0.96 on 293 x 329 with layer2 alone."""
import numpy as np
import pytest
import torch

import mmp_block2_f16_reference as h2
import mmp_block3_f16_reference as h3
import mmp_block4_f16_reference as h4
import mmp_cases as mc
import mmp_net_reference as nr
import mmp_reference as mr
import test_gpu_mmp_net as tn
from dyobav_mpcnwta_warehouse_amd import mmp_stem as ms
from dyobav_mpcnwta_warehouse_amd.mmp_front import MmpFrontEnd

pytestmark = pytest.mark.gpu

handle = tn.handle
PEDESTRIANS = {tn.SHAPE_IDS[0]: (2, 1), tn.SHAPE_IDS[1]: (2,)}      # M = 4 and M = 2 rows; pedestrian 2 has 7 past positions, 1 has 3
ARMS = {"layer2": {"layer2": "f16"}, "all-three": {"layer2": "f16", "layer3": "f16", "layer4": "f16"}}


def _stage_out(fe, name, rows):
    st = fe.stage(name)
    row = (st.channels,) + st.planes[-1]
    return st.pp[(len(st.args) - 1) % 2][:rows * int(np.prod(row))].view(rows, *row).cpu().numpy()


@pytest.mark.parametrize("arm", list(ARMS))
@pytest.mark.parametrize("sid", tn.SHAPE_IDS)
def test_whole_network_with_layer2_on_f16_against_the_float64_module(handle, sid, arm):
    shape = nr.SHAPES[tn.SHAPE_IDS.index(sid)]
    Hm, Wm, peds, operands = shape["Hm"], shape["Wm"], PEDESTRIANS[sid], ARMS[arm]
    rows = len(peds) * tn.N_OFF
    ref = nr.label_image(Hm, Wm)
    trajs = tn._trajectories(tn.SPREAD[Hm])
    hist, hcount = mc.hist_arrays(trajs)
    stack = np.concatenate([mr.input_stack(mr.input_planes(mr.to_pixels(trajs[p], tn.TF, tn.RESCALE), ref), tn.N_OFF) for p in peds])
    net64 = nr.in_double(nr.made_net(shape))
    want = [t.numpy() for t in nr.stages(net64, stack)]
    specs = dict(zip(("stem", "blocks", "blocks2", "blocks3", "blocks4", "head"), ms.split_network_whole(net64)))
    # the yardstick: the rule in float64 on the float64 module's layer1, each later stage by its own model where it is on
    model2 = h2.model_chain(want[1].astype(np.float32), specs["blocks2"])[-1]
    with torch.no_grad():
        body = net64.resnet34
        if "layer3" in operands:
            model3 = h3.model_chain(model2, specs["blocks3"])[-1]
            model4 = h4.model_chain(model3, specs["blocks4"])[-1]
        else:
            model3 = body.layer3(torch.as_tensor(model2).double())
            model4 = body.layer4(model3).numpy()
            model3 = model3.numpy()
        model = [np.asarray(m, dtype=np.float64) for m in (model2, model3, model4)]
        model.append(nr.finish(net64, torch.as_tensor(model[-1]).double(), 4).numpy())
    yard = [float(np.abs(m - w).max()) for m, w in zip(model, want[2:])]
    assert all(y > 0 for y in yard)
    # the device
    d_ref = torch.from_numpy(ref).cuda()
    fe = MmpFrontEnd(handle, dtype=np.float64, device=d_ref.device, Hm=Hm, Wm=Wm, n_off=tn.N_OFF, transform=tn.TF, rescale=tn.RESCALE,
                     sigma=tn.SIGMA, ref_image=d_ref, operands=operands, **specs)
    fe.allocate(len(peds))
    d_hist = torch.from_numpy(np.ascontiguousarray(hist.reshape(tn.B, tn.H, 5, 2))).cuda()
    d_hcount = torch.from_numpy(np.ascontiguousarray(hcount.reshape(tn.B, tn.H))).cuda()
    items = torch.tensor(peds, dtype=torch.long, device="cuda")
    out = fe.run(d_hist.data_ptr(), d_hcount.data_ptr(), tn.B, tn.H, items.data_ptr(), len(peds))
    torch.cuda.synchronize()
    got = [_stage_out(fe, name, rows) for name in ("layer2", "layer3", "layer4")] + [out.cpu().numpy()]
    ratios = []
    for name, g, w, m, y in zip(nr.STAGE_NAMES[2:], got, want[2:], model, yard):
        assert g.shape == w.shape == m.shape and g.shape[0] == rows and np.isfinite(g).all()
        r64, rm = float(np.abs(g - w).max()) / y, float(np.abs(g - m).max()) / y
        print(f"{sid} M {rows} {arm} {name}: yardstick |model - float64| = {y:.3e} (|float64| up to {np.abs(w).max():.2f}); "
              f"|device - float64| / yardstick = {r64:.2f}, |device - model| / yardstick = {rm:.2f}")
        ratios.append(r64)
    assert max(ratios) <= nr.BAR, ratios
