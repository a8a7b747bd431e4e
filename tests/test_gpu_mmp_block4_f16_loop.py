"""GPU tests of ``half=("layer4",)`` and ``half=("layer3", "layer4")`` -- layer4 on binary16 MFMA operands (``nmpc_mmp_block4_f16``,
csrc/nmpc_mmp_block4_f16.h) -- in the three host classes, with the shapes, networks and worlds of tests/test_gpu_mmp_block4_loop.py:
``MmpFrontEnd`` against three direct launches of the entry point on the same layer3 output, bit for bit, with layer4's buffers
allocated and with them inside the stem's output; ``half=()`` and ``half=("layer3",)`` against the float32 launches of layer4 (the
parent's bits); ``BatchEvaluator(mmp_half=("layer3", "layer4"))`` through the closed loop with the whole network on the device, H x K
= 2 x 5, its first step's layer4 output against the direct launches, then to the end; ``MmpInterface(None, ..., head=, half=)``
likewise."""
import numpy as np
import pytest
import torch

import dyobav_mpcnwta_warehouse_amd as nm
import mmp_block4_reference as b4
import mmp_cases as mc
import test_gpu_mmp_block3_loop as lp
import test_gpu_mmp_block4_loop as l4
from dyobav_mpcnwta_warehouse_amd import _capi
from dyobav_mpcnwta_warehouse_amd.evaluate import BatchEvaluator
from dyobav_mpcnwta_warehouse_amd.mmp_front import MmpFrontEnd
from dyobav_mpcnwta_warehouse_amd.mmp_stem import pack_block4_f16

pytestmark = pytest.mark.gpu

handle, fworld, world = lp.handle, lp.fworld, lp.world      # the fixtures of the float32 tests
PACKED = ("w1", "w2", "wd")
BOTH = ("layer3", "layer4")
SENTENCE = "only layer3 has an f16 kernel, and layer4 where {0}blocks4 is given"


def _direct_f16(handle, x, blocks):
    """``blocks`` (Block4Specs) through ``nmpc_mmp_block4_f16`` on x [M, 64, H3, W3], a buffer of its own per block: no ping-pong here."""
    keep = []
    for b in blocks:
        p = pack_block4_f16(b)
        g = _capi.NmpcMmpBlock4F16Args()
        g.M, g.Cin, g.H, g.W = (int(v) for v in x.shape)
        g.stride = b.stride
        out = torch.empty(g.M, 128, *b4.out_plane(g.H, g.W, b.stride), dtype=torch.float32, device="cuda")
        for name in lp.POINTERS:
            v = getattr(p, name)
            if v is not None:
                keep.append(torch.from_numpy(np.ascontiguousarray(v).view(np.int16) if name in PACKED else np.ascontiguousarray(v)).cuda())
                setattr(g, name, keep[-1].data_ptr())
        g.slope_mid, g.slope_out, g.x, g.out = b.slope_mid, b.slope_out, x.data_ptr(), out.data_ptr()
        handle.mmp_block4_f16(g)
        keep.append(x)
        x = out
    torch.cuda.synchronize()
    return x


def _stage_out(fe, name, rows):
    """What stage ``name`` of a front end left in its last buffer for the first ``rows`` rows."""
    st = fe.stage(name)
    row = (st.channels,) + st.planes[-1]
    return st.pp[(len(st.args) - 1) % 2][:rows * int(np.prod(row))].view(rows, *row)


def _front(handle, fworld, C, half):
    return MmpFrontEnd(handle, dtype=np.float64, device=fworld["d_ref"].device, Hm=lp.HM, Wm=lp.WM, n_off=lp.N_OFF, transform=lp.FTF,
                       rescale=lp.FRESCALE, sigma=lp.SIGMA, ref_image=fworld["d_ref"], stem=lp._integer_stem(C), blocks=lp._front_blocks(C),
                       blocks2=lp.FBLOCKS2, blocks3=lp.FBLOCKS3, blocks4=l4.FBLOCKS4, head=l4.FHEAD, half=half)


# ---- 1. the front end -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [("layer4",), BOTH], ids=["layer4", "both"])
@pytest.mark.parametrize("C", [8, 64], ids=["allocated", "inside-the-stem-output"])
def test_front_end_with_half_layer4(handle, fworld, C, half):
    items = torch.tensor(lp.ITEMS, dtype=torch.long, device="cuda")
    rest = tuple(n for n in half if n != "layer4")           # () or ("layer3",): the parent's options
    fe, plain, parent = _front(handle, fworld, C, half), _front(handle, fworld, C, rest), l4._front(handle, fworld, C)
    inside = C == 64
    st, sp = fe.stage("layer4"), plain.stage("layer4")
    assert fe.half == half and plain.half == rest and parent.half == ()
    assert st.Args is _capi.NmpcMmpBlock4F16Args and sp.Args is _capi.NmpcMmpBlock4Args and st.launch == handle.mmp_block4_f16
    assert fe.stage("layer3").Args is (_capi.NmpcMmpBlock3F16Args if rest else _capi.NmpcMmpBlock3Args) is plain.stage("layer3").Args
    assert st.cins == sp.cins == (64, 128, 128) and st.in_fill == sp.in_fill == inside
    # nothing but the stage's record moves: the rows, the bytes and the other stages are the parent's
    assert fe.row == plain.row == parent.row == (l4.O,) and fe.bytes_per_item == plain.bytes_per_item == parent.bytes_per_item
    assert all(b.w1.dtype == torch.int16 and b.w1.is_cuda for b in fe.blocks4) and all(b.w1.dtype == torch.float32 for b in plain.blocks4)
    assert fe.blocks4[0].w1.shape == (9, 2, 8, 64, 8) and fe.blocks4[0].wd.shape == (2, 8, 64, 8) and fe.blocks4[1].w1.shape == (9, 4, 8, 64, 8)
    assert fe.blocks4[1].wd is None and fe.blocks4[0].stride == 2
    for f in (fe, plain, parent):
        f.allocate(lp.CHUNK)
    args = (fworld["d_hist"].data_ptr(), fworld["d_hcount"].data_ptr(), lp.FB, lp.FH)
    for c0 in range(0, len(lp.ITEMS), lp.CHUNK):
        n, names = min(lp.CHUNK, len(lp.ITEMS) - c0), []
        rows = n * lp.N_OFF
        got = fe.run(*args, items[c0:].data_ptr(), n, lambda what, call: (names.append(what), call())[1]).clone()
        assert names == ["input", "layer1", "layer2", "layer3", "layer4", "head"]
        mid, out4 = _stage_out(fe, "layer3", rows).clone(), _stage_out(fe, "layer4", rows).clone()
        want4 = _direct_f16(handle, mid, l4.FBLOCKS4)
        assert out4.shape == want4.shape == (rows, 128, l4.H4, l4.W4) and out4.dtype == torch.float32
        assert bool(torch.isfinite(want4).all()) and float(want4.abs().max()) > 0 and torch.equal(out4, want4), c0
        assert got.shape == (rows, l4.O) and bool(torch.isfinite(got).all())
        # without "layer4" the stage is the parent's: the float32 launches' bits on the same layer3 output
        base = plain.run(*args, items[c0:].data_ptr(), n).clone()
        assert torch.equal(_stage_out(plain, "layer3", rows), mid)
        planes, head = l4._direct(handle, mid)
        assert torch.equal(_stage_out(plain, "layer4", rows), planes) and torch.equal(base, head)
        if not rest:                                        # half = () is the parent altogether
            assert torch.equal(base, parent.run(*args, items[c0:].data_ptr(), n))
    # run_block's one index space and run_stage launch the same kernels
    fe.fill(*args, items.data_ptr(), lp.CHUNK)
    for i in range(16):
        fe.run_block(i, lp.CHUNK * lp.N_OFF)
    first4 = _stage_out(fe, "layer4", lp.CHUNK * lp.N_OFF).clone()
    fe.run(*args, items.data_ptr(), lp.CHUNK)
    assert torch.equal(_stage_out(fe, "layer4", lp.CHUNK * lp.N_OFF), first4)
    with pytest.raises(ValueError, match=SENTENCE.format("")):
        _front(handle, fworld, C, ("layer4", "layer2"))


# ---- 2. the closed loop -------------------------------------------------------------------------------------------------------------------------
def _evaluator(world, H, K, half):
    head, *_ = l4.exact_head(K, H)
    return BatchEvaluator(nm.default_config_struct(), dtype=np.float32, predictor="mmp", mmp_hyp=K, ref_image=world["ref"], transform=lp.TF,
                          rescale=lp.RESCALE, network=None, mmp_blocks4=l4.BLOCKS4, mmp_head=head, mmp_half=half, compact=False, **l4.FRONT,
                          **lp._scenarios(H))


def test_closed_loop_with_half_layer3_and_layer4(world):
    H, K = 2, 5
    ev = _evaluator(world, H, K, BOTH)
    try:
        fe = ev.mmp_front
        assert fe.half == BOTH and fe.stage("layer4").Args is _capi.NmpcMmpBlock4F16Args and fe.stage("layer3").Args is _capi.NmpcMmpBlock3F16Args
        assert ev.mmp_row == (2 * K,) and ev.network is None
        ev.run(max_steps=1)
        rows = lp.B * H * ev.N                              # every scenario is alive in the first step: one chunk
        assert ev.mmp_chunk >= lp.B * H
        torch.cuda.synchronize()
        mid, got = _stage_out(fe, "layer3", rows).clone(), _stage_out(fe, "layer4", rows).clone()
        want = _direct_f16(ev.h, mid, l4.BLOCKS4)
        assert got.shape == (rows, 128) + l4.PLANE4 and bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0 and torch.equal(got, want)
    finally:
        ev.close()
    # to the end, with finite metrics
    ev = _evaluator(world, H, K, BOTH)
    rec = []
    try:
        res = ev.run(max_steps=lp.STEPS, record=rec)
    finally:
        ev.close()
    assert len(rec) == lp.STEPS and res.steps.max() == lp.STEPS and np.isfinite(res.trajectory).all()
    assert all(np.isfinite(r["P"]).all() and np.isfinite(r["dyn"]).all() for r in rec) and (res.n_obs[0] >= 1).all()
    with pytest.raises(ValueError, match="mmp_half: 'layer1': " + SENTENCE.format("mmp_")):
        _evaluator(world, H, K, ("layer4", "layer1"))


# ---- 3. the drop-in interface ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [("layer4",), BOTH], ids=["layer4", "both"])
def test_interface_without_a_network_with_half_layer4(golden_dir, half):
    from dyobav_mpcnwta_warehouse_amd.mmp_interface import MmpInterface
    ref = torch.from_numpy(mc.load_maps(golden_dir)["warehouse"].astype(np.float64))
    head, *_ = l4.exact_head(20, 7)
    itf = MmpInterface(None, stem=lp.SPEC, blocks=lp.BLOCKS, blocks2=lp.BLOCKS2, blocks3=lp.BLOCKS3, blocks4=l4.BLOCKS4, head=head, half=half)
    try:
        traj = [(150.25 + 0.75 * i, 120.125 + 0.25 * i) for i in range(7)]
        got = itf.get_motion_prediction(traj, ref, 5, lp.RESCALE, batch_size=3)
        assert len(got) == 5 and all(g.shape == (20, 2) and g.dtype == np.float64 and np.isfinite(g).all() for g in got)
        (fe,) = itf._fronts.values()
        assert fe.half == half and fe.stage("layer4").Args is _capi.NmpcMmpBlock4F16Args
        torch.cuda.synchronize()
        mid, out = _stage_out(fe, "layer3", 5).clone(), _stage_out(fe, "layer4", 5).clone()
        assert out.shape == (5, 128) + l4.PLANE4 and torch.equal(out, _direct_f16(fe.h, mid, l4.BLOCKS4)) and float(out.abs().max()) > 0
    finally:
        itf.close()
