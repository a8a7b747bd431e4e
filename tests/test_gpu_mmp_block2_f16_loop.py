"""GPU tests of ``operands={"layer2": "f16"}`` -- layer2 on binary16 MFMA operands (``nmpc_mmp_block2_f16``,
csrc/nmpc_mmp_block2_f16.h) -- alone and with layer3 and layer4 on them too, in the three host classes, with the shapes, networks and
worlds of tests/test_gpu_mmp_block4_loop.py: ``MmpFrontEnd`` through ``run``, ``run_stage`` and ``run_block`` against four direct
launches of the entry point on the same layer1 output, bit for bit, with layer2's buffers allocated and with them inside the stem's
output; ``operands=None``, ``{}`` and all ``"f32"`` against the parent's front end at every stage (the parent's bits);
``BatchEvaluator(mmp_operands=...)`` through the closed loop with the whole network on the device, H x K = 2 x 5, its first step's
layer2 output against the direct launches, then to the end; ``MmpInterface(None, ..., head=, operands=)`` likewise."""
import numpy as np
import pytest
import torch

import dyobav_mpcnwta_warehouse_amd as nm
import mmp_block2_reference as b2
import mmp_cases as mc
import test_gpu_mmp_block3_loop as lp
import test_gpu_mmp_block4_loop as l4
from dyobav_mpcnwta_warehouse_amd import _capi
from dyobav_mpcnwta_warehouse_amd.evaluate import BatchEvaluator
from dyobav_mpcnwta_warehouse_amd.mmp_front import MmpFrontEnd
from dyobav_mpcnwta_warehouse_amd.mmp_stem import pack_block2_f16

pytestmark = pytest.mark.gpu

handle, fworld, world = lp.handle, lp.fworld, lp.world      # the fixtures of the float32 tests
PACKED = ("w1", "w2", "wd")
LAYERS = ("layer1", "layer2", "layer3", "layer4")
ONLY2 = {"layer2": "f16"}
ALL3 = {"layer2": "f16", "layer3": "f16", "layer4": "f16"}
HALF_SENTENCE = "only layer3 has an f16 kernel, and layer4 where {0}blocks4 is given"


def _direct_f16(handle, x, blocks):
    """``blocks`` (Block2Specs) through ``nmpc_mmp_block2_f16`` on x [M, 16, Hp, Wp], a buffer of its own per block: no ping-pong here."""
    keep = []
    for b in blocks:
        p = pack_block2_f16(b)
        g = _capi.NmpcMmpBlock2F16Args()
        g.M, g.Cin, g.H, g.W = (int(v) for v in x.shape)
        g.stride = b.stride
        out = torch.empty(g.M, 32, *b2.out_plane(g.H, g.W, b.stride), dtype=torch.float32, device="cuda")
        for name in lp.POINTERS:
            v = getattr(p, name)
            if v is not None:
                keep.append(torch.from_numpy(np.ascontiguousarray(v).view(np.int16) if name in PACKED else np.ascontiguousarray(v)).cuda())
                setattr(g, name, keep[-1].data_ptr())
        g.slope_mid, g.slope_out, g.x, g.out = b.slope_mid, b.slope_out, x.data_ptr(), out.data_ptr()
        handle.mmp_block2_f16(g)
        keep.append(x)
        x = out
    torch.cuda.synchronize()
    return x


def _stage_out(fe, name, rows):
    """What stage ``name`` of a front end left in its last buffer for the first ``rows`` rows."""
    st = fe.stage(name)
    row = (st.channels,) + st.planes[-1]
    return st.pp[(len(st.args) - 1) % 2][:rows * int(np.prod(row))].view(rows, *row)


def _front(handle, fworld, C, **kw):
    return MmpFrontEnd(handle, dtype=np.float64, device=fworld["d_ref"].device, Hm=lp.HM, Wm=lp.WM, n_off=lp.N_OFF, transform=lp.FTF,
                       rescale=lp.FRESCALE, sigma=lp.SIGMA, ref_image=fworld["d_ref"], stem=lp._integer_stem(C), blocks=lp._front_blocks(C),
                       blocks2=lp.FBLOCKS2, blocks3=lp.FBLOCKS3, blocks4=l4.FBLOCKS4, head=l4.FHEAD, **kw)


# ---- 1. the front end -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("operands", [ONLY2, ALL3], ids=["layer2", "all-three"])
@pytest.mark.parametrize("C", [8, 64], ids=["allocated", "inside-the-stem-output"])
def test_front_end_with_layer2_on_f16(handle, fworld, C, operands):
    items = torch.tensor(lp.ITEMS, dtype=torch.long, device="cuda")
    fe, parent = _front(handle, fworld, C, operands=operands), l4._front(handle, fworld, C)
    st, sp = fe.stage("layer2"), parent.stage("layer2")
    assert fe.half == () and fe.operands == dict({n: "f32" for n in LAYERS}, **operands)
    assert st.Args is _capi.NmpcMmpBlock2F16Args and sp.Args is _capi.NmpcMmpBlock2Args and st.launch == handle.mmp_block2_f16
    assert fe.stage("layer3").Args is (_capi.NmpcMmpBlock3F16Args if "layer3" in operands else _capi.NmpcMmpBlock3Args)
    assert fe.stage("layer4").Args is (_capi.NmpcMmpBlock4F16Args if "layer4" in operands else _capi.NmpcMmpBlock4Args)
    # nothing but the stage's record moves: the rows, the bytes, the placement and the other stages are the parent's
    assert st.cins == sp.cins == (16, 32, 32, 32) and st.in_fill == sp.in_fill == (C == 64) and st.offset == sp.offset and st.planes == sp.planes
    assert fe.row == parent.row == (l4.O,) and fe.bytes_per_item == parent.bytes_per_item
    assert all(b.w1.dtype == torch.int16 and b.w1.is_cuda for b in fe.blocks2) and all(b.w1.dtype == torch.float32 for b in parent.blocks2)
    assert fe.blocks2[0].w1.shape == (9, 1, 2, 64, 8) == fe.blocks2[1].w1.shape and fe.blocks2[0].wd.shape == (1, 2, 64, 8)
    assert fe.blocks2[1].wd is None and fe.blocks2[0].stride == 2
    for f in (fe, parent):
        f.allocate(lp.CHUNK)
    args = (fworld["d_hist"].data_ptr(), fworld["d_hcount"].data_ptr(), lp.FB, lp.FH)
    for c0 in range(0, len(lp.ITEMS), lp.CHUNK):
        n, names = min(lp.CHUNK, len(lp.ITEMS) - c0), []
        rows = n * lp.N_OFF
        got = fe.run(*args, items[c0:].data_ptr(), n, lambda what, call: (names.append(what), call())[1]).clone()
        assert names == ["input", "layer1", "layer2", "layer3", "layer4", "head"]
        mid, out2 = _stage_out(fe, "layer1", rows).clone(), _stage_out(fe, "layer2", rows).clone()
        want2 = _direct_f16(handle, mid, lp.FBLOCKS2)
        assert out2.shape == want2.shape == (rows, 32, lp.H2, lp.W2) and out2.dtype == torch.float32
        assert bool(torch.isfinite(want2).all()) and float(want2.abs().max()) > 0 and torch.equal(out2, want2), c0
        assert got.shape == (rows, l4.O) and bool(torch.isfinite(got).all())
        parent.run(*args, items[c0:].data_ptr(), n)
        assert torch.equal(_stage_out(parent, "layer1", rows), mid)                # layer1 is untouched
    # run_block's one index space and run_stage launch the same kernels
    rows = lp.CHUNK * lp.N_OFF
    fe.run(*args, items.data_ptr(), lp.CHUNK)
    mid, by_run = _stage_out(fe, "layer1", rows).clone(), _stage_out(fe, "layer2", rows).clone()
    want2 = _direct_f16(handle, mid, lp.FBLOCKS2)
    assert torch.equal(by_run, want2)
    fe.fill(*args, items.data_ptr(), lp.CHUNK)
    for i in range(16):
        fe.run_block(i, rows)
    assert torch.equal(_stage_out(fe, "layer2", rows), want2)
    fe.fill(*args, items.data_ptr(), lp.CHUNK)
    fe.run_stage("layer1", rows)
    by_stage = fe.run_stage("layer2", rows)
    assert by_stage.shape == want2.shape and torch.equal(by_stage, want2) and torch.equal(fe.run_blocks2(rows), want2)
    with pytest.raises(ValueError, match=HALF_SENTENCE.format("")):
        _front(handle, fworld, C, operands=operands, half=("layer2",))


@pytest.mark.parametrize("C", [8, 64], ids=["allocated", "inside-the-stem-output"])
def test_no_operands_is_the_parent_bit_for_bit(handle, fworld, C):
    items = torch.tensor(lp.ITEMS, dtype=torch.long, device="cuda")
    parent = l4._front(handle, fworld, C)
    parent.allocate(lp.CHUNK)
    args = (fworld["d_hist"].data_ptr(), fworld["d_hcount"].data_ptr(), lp.FB, lp.FH)
    rows = lp.CHUNK * lp.N_OFF
    base = parent.run(*args, items.data_ptr(), lp.CHUNK).clone()
    want = [_stage_out(parent, name, rows).clone() for name in LAYERS]
    for operands in (None, {}, {n: "f32" for n in LAYERS}, {"layer2": "f32"}):
        fe = _front(handle, fworld, C, operands=operands)
        assert fe.half == () and fe.operands == {n: "f32" for n in LAYERS} and fe.bytes_per_item == parent.bytes_per_item
        assert [fe.stage(n).Args for n in LAYERS] == [parent.stage(n).Args for n in LAYERS]
        fe.allocate(lp.CHUNK)
        got = fe.run(*args, items.data_ptr(), lp.CHUNK)
        assert torch.equal(got, base)
        for name, w in zip(LAYERS, want):
            assert torch.equal(_stage_out(fe, name, rows), w), (operands, name)
    # and operands= says what half= says: the same bits
    a, b = _front(handle, fworld, C, half=("layer3", "layer4")), _front(handle, fworld, C, operands={"layer3": "f16", "layer4": "f16"})
    for f in (a, b):
        f.allocate(lp.CHUNK)
    assert torch.equal(a.run(*args, items.data_ptr(), lp.CHUNK), b.run(*args, items.data_ptr(), lp.CHUNK))
    assert torch.equal(_stage_out(a, "layer4", rows), _stage_out(b, "layer4", rows))


# ---- 2. the closed loop -------------------------------------------------------------------------------------------------------------------------
def _evaluator(world, H, K, **kw):
    head, *_ = l4.exact_head(K, H)
    return BatchEvaluator(nm.default_config_struct(), dtype=np.float32, predictor="mmp", mmp_hyp=K, ref_image=world["ref"], transform=lp.TF,
                          rescale=lp.RESCALE, network=None, mmp_blocks4=l4.BLOCKS4, mmp_head=head, compact=False, **l4.FRONT,
                          **lp._scenarios(H), **kw)


def test_closed_loop_with_all_three_stages_on_f16(world):
    H, K = 2, 5
    ev = _evaluator(world, H, K, mmp_operands=ALL3)
    try:
        fe = ev.mmp_front
        assert fe.half == () and fe.operands == dict(ALL3, layer1="f32") and fe.stage("layer2").Args is _capi.NmpcMmpBlock2F16Args
        assert fe.stage("layer3").Args is _capi.NmpcMmpBlock3F16Args and fe.stage("layer4").Args is _capi.NmpcMmpBlock4F16Args
        assert ev.mmp_row == (2 * K,) and ev.network is None
        ev.run(max_steps=1)
        rows = lp.B * H * ev.N                              # every scenario is alive in the first step: one chunk
        assert ev.mmp_chunk >= lp.B * H
        torch.cuda.synchronize()
        mid, got = _stage_out(fe, "layer1", rows).clone(), _stage_out(fe, "layer2", rows).clone()
        want = _direct_f16(ev.h, mid, lp.BLOCKS2)
        assert got.shape == (rows, 32, 37, 42) and bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0 and torch.equal(got, want)
    finally:
        ev.close()
    # to the end, with finite metrics
    ev = _evaluator(world, H, K, mmp_operands=ONLY2, mmp_half=("layer3",))
    rec = []
    try:
        assert ev.mmp_front.half == ("layer3",) and ev.mmp_front.operands == {"layer1": "f32", "layer2": "f16", "layer3": "f16", "layer4": "f32"}
        res = ev.run(max_steps=lp.STEPS, record=rec)
    finally:
        ev.close()
    assert len(rec) == lp.STEPS and res.steps.max() == lp.STEPS and np.isfinite(res.trajectory).all()
    assert all(np.isfinite(r["P"]).all() and np.isfinite(r["dyn"]).all() for r in rec) and (res.n_obs[0] >= 1).all()
    with pytest.raises(ValueError, match="mmp_half: 'layer2': " + HALF_SENTENCE.format("mmp_")):
        _evaluator(world, H, K, mmp_operands=ONLY2, mmp_half=("layer2",))
    with pytest.raises(ValueError, match="mmp_operands: 'layer1': only layer2, layer3 and layer4 have an f16 kernel"):
        _evaluator(world, H, K, mmp_operands={"layer1": "f16"})


# ---- 3. the drop-in interface ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("operands", [ONLY2, ALL3], ids=["layer2", "all-three"])
def test_interface_without_a_network_with_layer2_on_f16(golden_dir, operands):
    from dyobav_mpcnwta_warehouse_amd.mmp_interface import MmpInterface
    ref = torch.from_numpy(mc.load_maps(golden_dir)["warehouse"].astype(np.float64))
    head, *_ = l4.exact_head(20, 7)
    itf = MmpInterface(None, stem=lp.SPEC, blocks=lp.BLOCKS, blocks2=lp.BLOCKS2, blocks3=lp.BLOCKS3, blocks4=l4.BLOCKS4, head=head,
                       operands=operands)
    try:
        traj = [(150.25 + 0.75 * i, 120.125 + 0.25 * i) for i in range(7)]
        got = itf.get_motion_prediction(traj, ref, 5, lp.RESCALE, batch_size=3)
        assert len(got) == 5 and all(g.shape == (20, 2) and g.dtype == np.float64 and np.isfinite(g).all() for g in got)
        (fe,) = itf._fronts.values()
        assert fe.half == () and fe.operands == dict({n: "f32" for n in LAYERS}, **operands) and fe.stage("layer2").Args is _capi.NmpcMmpBlock2F16Args
        torch.cuda.synchronize()
        mid, out = _stage_out(fe, "layer1", 5).clone(), _stage_out(fe, "layer2", 5).clone()
        assert out.shape == (5, 32, 37, 42) and torch.equal(out, _direct_f16(fe.h, mid, lp.BLOCKS2)) and float(out.abs().max()) > 0
    finally:
        itf.close()
