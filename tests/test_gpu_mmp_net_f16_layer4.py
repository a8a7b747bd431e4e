"""GPU test of the WHOLE network on the device with layer4 on binary16 MFMA operands -- ``MmpFrontEnd(..., half=("layer4",))`` and
``half=("layer3", "layer4")``, csrc/nmpc_mmp_block4_f16.h --, with the real-valued network, worlds and float64 module of
tests/test_gpu_mmp_net.py and the two shapes of tests/test_gpu_mmp_net_f16.py: the 37 x 41 map on M = 4 rows, the 293 x 329 one (the
warehouse's planes) on M = 2.

Yardstick: the rule's own cost. ``mmp_block4_f16_reference.model_chain`` -- the rounding rule in float64, m rounded, the three blocks
of layer4 one after the other -- runs on the float64 module's layer3 output or, with both names, on the output of layer3's own
``model_chain`` (tests/mmp_block3_f16_reference.py) on the float64 module's layer2; the float64 module's head finishes it. Its
distance from the float64 module at layer4 and at the output is what rounding the operands to binary16 costs on this input, with no
float32 effect in it. Bar: the device lies within ``BAR`` = 4 times that yardstick from the float64 module at both, the project's
standing margin over a rounding yardstick (tests/mmp_net_reference.py). The distance from the model itself is printed and NOT a
criterion: one float32 bit of difference in x or m flips a binary16 rounding now and then, and the maximum over a plane finds those.

Measured on an MI355X, |device - float64| / yardstick (the bar is 4) and |device - model| / yardstick:

    map          M    half             layer4        output
    37 x 41      4    layer4           1.02  0.34    1.22  0.22
    37 x 41      4    layer3+layer4    1.09  0.72    0.85  0.43
    293 x 329    2    layer4           1.08  0.45    1.06  0.25
    293 x 329    2    layer3+layer4    1.00  0.92    0.90  0.58

The yardsticks themselves, layer4 / output: 1.5e-3 / 1.5e-4 and 2.3e-3 / 2.4e-4 on the small map (values up to 4.27 / 0.91), 6.0e-3 /
4.2e-4 and 9.0e-3 / 5.9e-4 on the large one (up to 12.05 / 1.72)."""
import numpy as np
import pytest
import torch

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


def _stage_out(fe, name, rows):
    st = fe.stage(name)
    row = (st.channels,) + st.planes[-1]
    return st.pp[(len(st.args) - 1) % 2][:rows * int(np.prod(row))].view(rows, *row).cpu().numpy()


@pytest.mark.parametrize("half", [("layer4",), ("layer3", "layer4")], ids=["layer4", "both"])
@pytest.mark.parametrize("sid", tn.SHAPE_IDS)
def test_whole_network_with_half_layer4_against_the_float64_module(handle, sid, half):
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
    # the yardstick: the rule in float64 on the float64 module's layer3 (both names: on layer3's model), finished by the float64 module
    x3 = want[3].astype(np.float32) if "layer3" not in half else h3.model_chain(want[2].astype(np.float32), specs["blocks3"])[-1]
    model4 = h4.model_chain(x3, specs["blocks4"])[-1]
    with torch.no_grad():
        model = [model4.astype(np.float64), nr.finish(net64, torch.as_tensor(model4).double(), 4).numpy()]
    yard = [float(np.abs(m - w).max()) for m, w in zip(model, want[4:])]
    assert all(y > 0 for y in yard)
    # the device
    d_ref = torch.from_numpy(ref).cuda()
    fe = MmpFrontEnd(handle, dtype=np.float64, device=d_ref.device, Hm=Hm, Wm=Wm, n_off=tn.N_OFF, transform=tn.TF, rescale=tn.RESCALE,
                     sigma=tn.SIGMA, ref_image=d_ref, half=half, **specs)
    fe.allocate(len(peds))
    d_hist = torch.from_numpy(np.ascontiguousarray(hist.reshape(tn.B, tn.H, 5, 2))).cuda()
    d_hcount = torch.from_numpy(np.ascontiguousarray(hcount.reshape(tn.B, tn.H))).cuda()
    items = torch.tensor(peds, dtype=torch.long, device="cuda")
    out = fe.run(d_hist.data_ptr(), d_hcount.data_ptr(), tn.B, tn.H, items.data_ptr(), len(peds))
    torch.cuda.synchronize()
    got = [_stage_out(fe, "layer4", rows), out.cpu().numpy()]
    ratios = []
    for name, g, w, m, y in zip(nr.STAGE_NAMES[4:], got, want[4:], model, yard):
        assert g.shape == w.shape == m.shape and g.shape[0] == rows and np.isfinite(g).all()
        r64, rm = float(np.abs(g - w).max()) / y, float(np.abs(g - m).max()) / y
        print(f"{sid} M {rows} {'+'.join(half)} {name}: yardstick |model - float64| = {y:.3e} (|float64| up to {np.abs(w).max():.2f}); "
              f"|device - float64| / yardstick = {r64:.2f}, |device - model| / yardstick = {rm:.2f}")
        ratios.append(r64)
    assert max(ratios) <= nr.BAR, ratios
