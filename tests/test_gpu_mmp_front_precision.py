"""GPU tests of ``MmpFrontEnd(..., precision="f16")`` -- the whole network on binary16 MFMA operands, layer1 included
(``nmpc_mmp_block_f16``, csrc/nmpc_mmp_block1_f16.h), with binary16 activations between all blocks -- with the real-valued network,
world and float64 module of tests/test_gpu_mmp_net.py on its 37 x 41 map (M = 4 rows), by the protocol of
tests/test_gpu_mmp_front_activations.py, whose helpers this file uses:

1. the front end against a CHAIN of the block kernels on float32 memory through the C ABI (``nmpc_mmp_block_f16``,
   ``nmpc_mmp_block{2,3,4}_f16``), one launch per block on buffers of the test's own, rounded between blocks on the host with
   ``round_f16``: every stage's ``run_stage`` result and the head's output, bit for bit;
2. ``precision`` of ``None`` or ``"f32"`` against the front end built without the keyword, at every stage, bit for bit;
3. the closed loop: ``BatchEvaluator(mmp_precision="f16")`` reports the operands and activations of the switch, and its predictor
   output on its own histories is that of a stand-alone front end with the same arguments."""
import numpy as np
import pytest
import torch

import test_gpu_mmp_block2_f16_loop as l2
import test_gpu_mmp_block3_loop as lp
import test_gpu_mmp_front_activations as fa
import test_gpu_mmp_net as tn
from dyobav_mpcnwta_warehouse_amd import _capi
from dyobav_mpcnwta_warehouse_amd.evaluate import MMP_SIGMA
from dyobav_mpcnwta_warehouse_amd.mmp_front import MmpFrontEnd
from dyobav_mpcnwta_warehouse_amd.mmp_stem import round_f16

pytestmark = pytest.mark.gpu

handle, world = tn.handle, lp.world
LAYERS = fa.LAYERS
ALL4 = {name: "f16" for name in LAYERS}
FLOAT32_ENTRY = {"layer1": "mmp_block_f16", "layer2": "mmp_block2_f16", "layer3": "mmp_block3_f16", "layer4": "mmp_block4_f16"}
FLAGS16 = [(0, 1)] + [(1, 1)] * 14 + [(1, 0)]                          # the 16 blocks: (x_f16, out_f16)


def _chain(handle, w):
    """[layer1, layer2, layer3, layer4, output] from one launch per block of the kernels on FLOAT32 memory, each on buffers of its
    own, every tensor between two blocks rounded on the host."""
    fe0, rows = fa._front(handle, w, precision="f16"), w["rows"]
    x = fe0.fill(*fa._fill_args(w)).reshape(rows, *fe0.fill_row).clone()
    blocks = sum(len(st.args) for st in fe0.stages)
    outs, keep, k = [], [], 0
    for st in fe0.stages:
        launch = getattr(handle, FLOAT32_ENTRY[st.name])
        for j, a in enumerate(st.args):
            out = torch.full((rows, st.channels) + tuple(st.planes[j + 1]), float("nan"), dtype=torch.float32, device="cuda")
            a.x, a.out, a.M = x.data_ptr(), out.data_ptr(), rows
            launch(a)
            torch.cuda.synchronize()
            k += 1
            if k < blocks:
                out = torch.from_numpy(round_f16(out.cpu().numpy()).astype(np.float32)).cuda()
            keep.append(x)
            x = out
        outs.append(x)
    fe1 = fa._front(handle, w, precision="f16")                          # (fe0's structs point at the test's buffers now)
    last = fe1.stages[-1]
    last.pp[(len(last.args) - 1) % 2][:x.numel()].copy_(x.reshape(-1))  # where the head reads layer4
    outs.append(fe1.run_head(rows).clone())
    torch.cuda.synchronize()
    return outs


def test_front_end_equals_the_chain_of_kernels_on_float32_memory(handle):
    w = fa._net(0)
    want = _chain(handle, w)
    fe = fa._front(handle, w, precision="f16")
    assert fe.operands == ALL4 and fe.activations == "f16" and fe.half == ()
    assert [io for st in fe.stages for io in st.io] == FLAGS16
    assert fe.stage("layer1").Args is _capi.NmpcMmpBlockF16Args and [st.out_f16 for st in fe.stages] == [True, True, True, False]
    got = fa._by_stage(fe, w)
    for name, g, t in zip(LAYERS + ("output",), got, want):
        assert g.shape == t.shape and g.dtype == torch.float32 and bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0, name
        assert torch.equal(g, t), (name, float((g - t).abs().max()))
    # run() launches the same and returns the head's output; its parts keep their names
    names = []
    out = fe.run(*fa._fill_args(w), lambda what, call: (names.append(what), call())[1])
    torch.cuda.synchronize()
    assert names == ["input"] + list(LAYERS) + ["head"] and torch.equal(out, want[-1])
    # the switch is what its parts say: beside agreeing keywords it is the same front end ...
    same = fa._by_stage(fa._front(handle, w, precision="f16", operands=fa.ALL3, activations="f16", half=("layer3",)), w)
    assert all(torch.equal(a, b) for a, b in zip(same, got))
    # ... and layer1 on f16 is something: today's fastest path gives other bits from layer1 on
    parent = fa._by_stage(fa._front(handle, w, operands=fa.ALL3, activations="f16"), w)
    assert not torch.equal(parent[0], got[0]) and not torch.equal(parent[-1], got[-1])


@pytest.mark.parametrize("precision", [None, "f32"])
def test_no_precision_is_the_parent_bit_for_bit(handle, precision):
    w = fa._net(0)
    for kw in ({}, dict(operands=fa.ALL3), dict(operands=fa.ALL3, activations="f16")):
        base = fa._front(handle, w, **kw)
        fe = fa._front(handle, w, precision=precision, **kw)
        assert fe.operands == base.operands and fe.activations == base.activations
        assert [(st.Args, st.io) for st in fe.stages] == [(st.Args, st.io) for st in base.stages]
        for name, g, t in zip(LAYERS + ("output",), fa._by_stage(fe, w), fa._by_stage(base, w)):
            assert torch.equal(g, t), (kw, name)


def test_closed_loop_on_the_whole_network_in_f16(world):
    H, K = 2, 5
    ev = l2._evaluator(world, H, K, mmp_precision="f16")
    rec = []
    try:
        fe = ev.mmp_front
        assert fe.activations == "f16" and fe.operands == ALL4
        assert [io for n in LAYERS for io in fe.stage(n).io] == FLAGS16
        res = ev.run(max_steps=1, record=rec)
        assert len(rec) == 1 and np.isfinite(res.trajectory).all() and all(np.isfinite(r["P"]).all() and np.isfinite(r["dyn"]).all() for r in rec)
        n = lp.B * H
        assert ev.mmp_chunk >= n
        specs = {k[4:]: v for k, v in l2.l4.FRONT.items()}
        alone = MmpFrontEnd(ev.h, ev.dt, ev.dev, ev.mmp_Hm, ev.mmp_Wm, ev.N, lp.TF, ev.mmp_rescale, MMP_SIGMA, ev.mmp_ref, blocks4=l2.l4.BLOCKS4,
                            head=l2.l4.exact_head(K, H)[0], precision="f16", **specs)
        alone.allocate(n)
        args = (ev.hist.data_ptr(), ev.hcount.data_ptr(), ev.B, H, None, n)
        a, b = fe.run(*args).clone(), alone.run(*args).clone()
        torch.cuda.synchronize()
        assert a.shape == (n * ev.N, 2 * K) and bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0 and torch.equal(a, b)
    finally:
        ev.close()
    with pytest.raises(ValueError, match="mmp_precision: 'f16', but mmp_activations is 'f32'"):
        l2._evaluator(world, H, K, mmp_precision="f16", mmp_activations="f32")
    with pytest.raises(ValueError, match="mmp_precision: 'half' is none of None, 'f32' and 'f16'"):
        l2._evaluator(world, H, K, mmp_precision="half")
