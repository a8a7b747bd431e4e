"""GPU test of the WHOLE network on the device with layer3 on binary16 MFMA operands (``MmpFrontEnd(..., half=("layer3",))``,
csrc/nmpc_mmp_block3_f16.h), with the real-valued network, worlds and float64 module of tests/test_gpu_mmp_net.py: the first shape
(37 x 41 map) on M = 4 rows -- two pedestrians, with 7 and 3 past positions, two time offsets each --, the second (293 x 329: the
warehouse's planes) on M = 2.

Yardstick: the rule's own cost. ``mmp_block3_f16_reference.model_chain`` -- the rounding rule in float64, m rounded, the six blocks
of layer3 one after the other on the float64 module's layer2 -- is finished by the float64 module's layer4 and head; its distance
from the float64 module at layer3, at layer4 and at the output is what rounding the operands to binary16 costs on this input, with no
float32 effect in it. Bar: the device lies within ``BAR`` = 4 times that yardstick from the float64 module at each of the three, the
project's standing margin over a rounding yardstick (tests/mmp_net_reference.py). The distance from the model itself is printed and
NOT a criterion: one float32 bit of difference in x or m flips a binary16 rounding now and then, and the maximum over a plane
finds those.

Measured on an MI355X, |device - float64| / yardstick (the bar is 4) and |device - model| / yardstick:

    map          M    layer3        layer4        output
    37 x 41      4    0.96  0.57    1.32  0.65    0.96  0.41
    293 x 329    2    1.02  0.67    1.05  0.74    1.40  0.40

The yardsticks themselves: 3.2e-3, 1.8e-3, 1.4e-4 on the small map (values up to 8.0, 4.3, 0.91) and 8.3e-3, 7.6e-3, 3.5e-4 on
the large one (up to 10.4, 12.1, 1.72). On the CPU ``emulate`` chained through the six blocks lies 0.91 yardsticks from the float64
module at layer3 and 0.30 / 0.59 from the model."""
import numpy as np
import pytest
import torch

import mmp_block3_f16_reference as h3
import mmp_cases as mc
import mmp_net_reference as nr
import mmp_reference as mr
import test_gpu_mmp_net as tn
from dyobav_mpcnwta_warehouse_amd import mmp_stem as ms
from dyobav_mpcnwta_warehouse_amd.mmp_front import MmpFrontEnd

pytestmark = pytest.mark.gpu

handle = tn.handle
PEDESTRIANS = {tn.SHAPE_IDS[0]: (2, 1), tn.SHAPE_IDS[1]: (2,)}      # M = 4 and M = 2 rows; pedestrian 2 has 7 past positions, 1 has 3


def _stage_out(fe, name, rows):
    st = fe.stage(name)
    row = (st.channels,) + st.planes[-1]
    return st.pp[(len(st.args) - 1) % 2][:rows * int(np.prod(row))].view(rows, *row).cpu().numpy()


@pytest.mark.parametrize("sid", tn.SHAPE_IDS)
def test_whole_network_with_half_layer3_against_the_float64_module(handle, sid):
    shape = nr.SHAPES[tn.SHAPE_IDS.index(sid)]
    Hm, Wm, peds = shape["Hm"], shape["Wm"], PEDESTRIANS[sid]
    rows = len(peds) * tn.N_OFF
    ref = nr.label_image(Hm, Wm)
    trajs = tn._trajectories(tn.SPREAD[Hm])
    hist, hcount = mc.hist_arrays(trajs)
    stack = np.concatenate([mr.input_stack(mr.input_planes(mr.to_pixels(trajs[p], tn.TF, tn.RESCALE), ref), tn.N_OFF) for p in peds])
    net64 = nr.in_double(nr.made_net(shape))
    want = [t.numpy() for t in nr.stages(net64, stack)]
    specs = dict(zip(("stem", "blocks", "blocks2", "blocks3", "blocks4", "head"), ms.split_network_whole(net64)))
    # the yardstick: the rule in float64 on the float64 module's layer2, finished by the float64 module
    model3 = h3.model_chain(want[2].astype(np.float32), specs["blocks3"])[-1]
    with torch.no_grad():
        model4 = net64.resnet34.layer4(torch.as_tensor(model3).double())
        model = [model3.astype(np.float64), model4.numpy(), nr.finish(net64, model4, 4).numpy()]
    yard = [float(np.abs(m - w).max()) for m, w in zip(model, want[3:])]
    assert all(y > 0 for y in yard)
    # the device
    d_ref = torch.from_numpy(ref).cuda()
    fe = MmpFrontEnd(handle, dtype=np.float64, device=d_ref.device, Hm=Hm, Wm=Wm, n_off=tn.N_OFF, transform=tn.TF, rescale=tn.RESCALE,
                     sigma=tn.SIGMA, ref_image=d_ref, half=("layer3",), **specs)
    fe.allocate(len(peds))
    d_hist = torch.from_numpy(np.ascontiguousarray(hist.reshape(tn.B, tn.H, 5, 2))).cuda()
    d_hcount = torch.from_numpy(np.ascontiguousarray(hcount.reshape(tn.B, tn.H))).cuda()
    items = torch.tensor(peds, dtype=torch.long, device="cuda")
    out = fe.run(d_hist.data_ptr(), d_hcount.data_ptr(), tn.B, tn.H, items.data_ptr(), len(peds))
    torch.cuda.synchronize()
    got = [_stage_out(fe, "layer3", rows), _stage_out(fe, "layer4", rows), out.cpu().numpy()]
    ratios = []
    for name, g, w, m, y in zip(nr.STAGE_NAMES[3:], got, want[3:], model, yard):
        assert g.shape == w.shape == m.shape and g.shape[0] == rows and np.isfinite(g).all()
        r64, rm = float(np.abs(g - w).max()) / y, float(np.abs(g - m).max()) / y
        print(f"{sid} M {rows} {name}: yardstick |model - float64| = {y:.3e} (|float64| up to {np.abs(w).max():.2f}); "
              f"|device - float64| / yardstick = {r64:.2f}, |device - model| / yardstick = {rm:.2f}")
        ratios.append(r64)
    assert max(ratios) <= nr.BAR, ratios
