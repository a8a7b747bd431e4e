"""GPU tests of ``half=("layer3",)`` -- layer3 on binary16 MFMA operands (``nmpc_mmp_block3_f16``, csrc/nmpc_mmp_block3_f16.h) -- in
the three host classes, with the shapes, networks and worlds of tests/test_gpu_mmp_block3_loop.py (B = 6): ``MmpFrontEnd`` against
six direct launches of the entry point, bit for bit, with layer3's buffers allocated and with them inside the stem's output;
``half=()`` against the float32 launches (the parent's bits); ``BatchEvaluator(mmp_half=("layer3",))`` through the closed loop, its
first step's layer3 output against the direct launches; ``MmpInterface(half=("layer3",))`` likewise."""
import numpy as np
import pytest
import torch

import dyobav_mpcnwta_warehouse_amd as nm
import mmp_block3_reference as b3
import mmp_cases as mc
import mmp_reference as mr
import test_gpu_mmp_block3_loop as lp
from dyobav_mpcnwta_warehouse_amd import _capi
from dyobav_mpcnwta_warehouse_amd.evaluate import BatchEvaluator
from dyobav_mpcnwta_warehouse_amd.mmp_front import MmpFrontEnd
from dyobav_mpcnwta_warehouse_amd.mmp_stem import pack_block3_f16

pytestmark = pytest.mark.gpu

handle, fworld, world = lp.handle, lp.fworld, lp.world      # the fixtures of the float32 test
PACKED = ("w1", "w2", "wd")


def _direct_f16(handle, x, blocks):
    """``blocks`` (Block3Specs) through ``nmpc_mmp_block3_f16`` on x [M, 32, H2, W2], a buffer of its own per block: no ping-pong here."""
    keep = []
    for b in blocks:
        p = pack_block3_f16(b)
        g = _capi.NmpcMmpBlock3F16Args()
        g.M, g.Cin, g.H, g.W = (int(v) for v in x.shape)
        g.stride = b.stride
        out = torch.empty(g.M, 64, *b3.out_plane(g.H, g.W, b.stride), dtype=torch.float32, device="cuda")
        for name in lp.POINTERS:
            v = getattr(p, name)
            if v is not None:
                keep.append(torch.from_numpy(np.ascontiguousarray(v).view(np.int16) if name in PACKED else np.ascontiguousarray(v)).cuda())
                setattr(g, name, keep[-1].data_ptr())
        g.slope_mid, g.slope_out, g.x, g.out = b.slope_mid, b.slope_out, x.data_ptr(), out.data_ptr()
        handle.mmp_block3_f16(g)
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
                       blocks2=lp.FBLOCKS2, blocks3=lp.FBLOCKS3, half=half)


# ---- 1. the front end -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [8, 64], ids=["allocated", "inside-the-stem-output"])
def test_front_end_with_half_layer3(handle, fworld, C):
    items = torch.tensor(lp.ITEMS, dtype=torch.long, device="cuda")
    fe, plain, parent = _front(handle, fworld, C, ("layer3",)), _front(handle, fworld, C, ()), lp._front(handle, fworld, C)
    inside = C == 64
    st, sp = fe.stage("layer3"), plain.stage("layer3")
    assert fe.half == ("layer3",) and plain.half == () and st.Args is _capi.NmpcMmpBlock3F16Args and sp.Args is _capi.NmpcMmpBlock3Args
    assert st.cins == sp.cins == (32, 64, 64, 64, 64, 64) and st.in_fill == sp.in_fill == inside
    # nothing but the stage's record moves: the rows, the bytes and the other stages are the parent's
    assert fe.row == plain.row == parent.row == (64, lp.H3, lp.W3) and fe.bytes_per_item == plain.bytes_per_item == parent.bytes_per_item
    assert fe.stage("layer2").Args is _capi.NmpcMmpBlock2Args and all(b.w1.dtype == torch.int16 and b.w1.is_cuda for b in fe.blocks3)
    assert fe.blocks3[0].w1.shape == (9, 1, 4, 64, 8) and fe.blocks3[1].w1.shape == (9, 2, 4, 64, 8) and fe.blocks3[1].wd is None
    for f in (fe, plain, parent):
        f.allocate(lp.CHUNK)
    args = (fworld["d_hist"].data_ptr(), fworld["d_hcount"].data_ptr(), lp.FB, lp.FH)
    for c0 in range(0, len(lp.ITEMS), lp.CHUNK):
        n, names = min(lp.CHUNK, len(lp.ITEMS) - c0), []
        got = fe.run(*args, items[c0:].data_ptr(), n, lambda what, call: (names.append(what), call())[1]).clone()
        assert names == ["input", "layer1", "layer2", "layer3"]
        mid = _stage_out(fe, "layer2", n * lp.N_OFF).clone()
        want = _direct_f16(handle, mid, lp.FBLOCKS3)
        assert got.shape == want.shape == (n * lp.N_OFF, 64, lp.H3, lp.W3) and got.dtype == torch.float32
        assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0 and torch.equal(got, want), c0
        # half = () is the parent: the float32 launches' bits
        base = plain.run(*args, items[c0:].data_ptr(), n)
        assert torch.equal(_stage_out(plain, "layer2", n * lp.N_OFF), mid)
        assert torch.equal(base, parent.run(*args, items[c0:].data_ptr(), n)) and torch.equal(base, lp._direct_layer3(handle, mid))
    # run_block's one index space and run_stage launch the same kernels
    fe.fill(*args, items.data_ptr(), lp.CHUNK)
    for i in range(13):
        fe.run_block(i, lp.CHUNK * lp.N_OFF)
    torch.cuda.synchronize()
    first = fe.run(*args, items.data_ptr(), lp.CHUNK)
    assert torch.equal(fe._out.view(-1)[:first.numel()].view(first.shape), first)
    with pytest.raises(ValueError, match="only layer3 has an f16 kernel"):
        _front(handle, fworld, C, ("layer2",))


# ---- 2. the closed loop -------------------------------------------------------------------------------------------------------------------------
def test_closed_loop_with_half_layer3(world):
    H, K = 2, 5
    trunk = lp.trunk_of(mr.fan(K, H))
    ev = BatchEvaluator(nm.default_config_struct(), dtype=np.float32, predictor="mmp", mmp_hyp=K, ref_image=world["ref"], transform=lp.TF,
                        rescale=lp.RESCALE, network=trunk, mmp_stem=lp.SPEC, mmp_blocks=lp.BLOCKS, mmp_blocks2=lp.BLOCKS2, mmp_blocks3=lp.BLOCKS3,
                        mmp_half=("layer3",), compact=False, **lp._scenarios(H))
    try:
        fe = ev.mmp_front
        assert fe.half == ("layer3",) and fe.stage("layer3").Args is _capi.NmpcMmpBlock3F16Args and ev.mmp_row == (64, 19, 21)
        ev.run(max_steps=1)
        rows = lp.B * H * ev.N                              # every scenario is alive in the first step: one chunk
        assert ev.mmp_chunk >= lp.B * H
        torch.cuda.synchronize()
        mid, got = _stage_out(fe, "layer2", rows).clone(), _stage_out(fe, "layer3", rows).clone()
        want = _direct_f16(ev.h, mid, lp.BLOCKS3)
        assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0 and torch.equal(got, want)
    finally:
        ev.close()
    # to the end, with finite metrics
    ev = BatchEvaluator(nm.default_config_struct(), dtype=np.float32, predictor="mmp", mmp_hyp=K, ref_image=world["ref"], transform=lp.TF,
                        rescale=lp.RESCALE, network=trunk, mmp_stem=lp.SPEC, mmp_blocks=lp.BLOCKS, mmp_blocks2=lp.BLOCKS2, mmp_blocks3=lp.BLOCKS3,
                        mmp_half=("layer3",), compact=False, **lp._scenarios(H))
    rec = []
    try:
        res = ev.run(max_steps=lp.STEPS, record=rec)
    finally:
        ev.close()
    assert len(rec) == lp.STEPS and res.steps.max() == lp.STEPS and np.isfinite(res.trajectory).all()
    assert all(np.isfinite(r["P"]).all() and np.isfinite(r["dyn"]).all() for r in rec) and (res.n_obs[0] >= 1).all()
    with pytest.raises(ValueError, match="only layer3 has an f16 kernel"):
        BatchEvaluator(nm.default_config_struct(), dtype=np.float32, predictor="mmp", mmp_hyp=K, ref_image=world["ref"], transform=lp.TF,
                       rescale=lp.RESCALE, network=trunk, mmp_stem=lp.SPEC, mmp_blocks=lp.BLOCKS, mmp_blocks2=lp.BLOCKS2, mmp_blocks3=lp.BLOCKS3,
                       mmp_half=("layer1",), **lp._scenarios(H))


# ---- 3. the drop-in interface ---------------------------------------------------------------------------------------------------------------------
def test_interface_with_half_layer3_runs_the_front_end(golden_dir):
    from dyobav_mpcnwta_warehouse_amd.mmp_interface import MmpInterface
    maps = mc.load_maps(golden_dir)
    case = mc.INTERFACE_CASES[0]
    trunk = lp.trunk_of(mr.fan(case["K"], case["seed"]))
    itf = MmpInterface(trunk, stem=lp.SPEC, blocks=lp.BLOCKS, blocks2=lp.BLOCKS2, blocks3=lp.BLOCKS3, half=("layer3",))
    try:
        ref = torch.from_numpy(maps[case["map"]].astype(np.float64))
        got = itf.get_motion_prediction([tuple(p) for p in case["traj"]], ref, case["pred_offset"], case["rescale"], batch_size=case["batch_size"])
        assert len(got) == case["pred_offset"] and all(g.shape == (case["K"], 2) and np.isfinite(g).all() for g in got)
        (fe,) = itf._fronts.values()
        assert fe.half == ("layer3",) and fe.stage("layer3").Args is _capi.NmpcMmpBlock3F16Args
        torch.cuda.synchronize()
        rows = case["pred_offset"]
        mid, out = _stage_out(fe, "layer2", rows).clone(), _stage_out(fe, "layer3", rows).clone()
        assert torch.equal(out, _direct_f16(fe.h, mid, lp.BLOCKS3)) and float(out.abs().max()) > 0
    finally:
        itf.close()
