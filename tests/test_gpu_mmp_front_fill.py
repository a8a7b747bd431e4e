"""GPU tests of ``MmpFrontEnd(..., precision="f16", fill="f16")`` -- the fused first layer writing binary16 in the octet form
(``nmpc_mmp_stem_io_*``, csrc/nmpc_mmp_stem.h), layer1's first block reading it as such -- with the real-valued network and world of
tests/test_gpu_mmp_front_activations.py (37 x 41 map, M = 4 rows), whose helpers this file uses. There is no tolerance here: the
rule of csrc/nmpc_mmp_block_f16.h rounds x when it is staged and the projection rounds it again in the same way, so behind a first
block WITH a projection every bit is that of ``precision="f16"`` alone; without one the identity becomes the binary16 value, and
the result is that of the float32-memory kernel on a host-rounded x.

1. identity to ``precision="f16"`` at every stage and at the head; ``fill()`` is ``round_f16`` of the parent's;
2. the flags, ``bytes_per_item``, the part names of ``run()``;
3. ``fill`` of ``None`` or ``"f32"`` against the front end built without the keyword;
4. a 16-channel stem (no projection in the first block);
5. the closed loop."""
import numpy as np
import pytest
import torch

import mmp_stem_reference as sr
import test_gpu_mmp_block2_f16_loop as l2
import test_gpu_mmp_block3_loop as lp
import test_gpu_mmp_front_activations as fa
import test_gpu_mmp_net as tn
from dyobav_mpcnwta_warehouse_amd.evaluate import MMP_SIGMA
from dyobav_mpcnwta_warehouse_amd.mmp_front import MmpFrontEnd
from dyobav_mpcnwta_warehouse_amd.mmp_stem import round_f16

pytestmark = pytest.mark.gpu

handle, world = tn.handle, lp.world
LAYERS = fa.LAYERS
FLAGS16 = [(1, 1)] * 15 + [(1, 0)]                                     # the 16 blocks: (x_f16, out_f16)


def _rounded(t):
    return torch.from_numpy(round_f16(t.cpu().numpy()).astype(np.float32)).cuda()


# ---- 1., 2. the same bits as precision="f16"; flags, sizes, part names ---------------------------------------------------------------------------
def test_same_bits_as_the_parent_at_every_stage(handle):
    w = fa._net(0)
    parent = fa._front(handle, w, precision="f16")
    fe = fa._front(handle, w, precision="f16", fill="f16")
    assert fe.fill_f16 and not parent.fill_f16 and fe.operands == parent.operands and fe.activations == "f16"
    assert w["specs"]["blocks"][0].wd is not None, "the first block of this network has a projection"
    want_fill = parent.fill(*fa._fill_args(w)).clone()
    got_fill = fe.fill(*fa._fill_args(w))
    torch.cuda.synchronize()
    assert got_fill.shape == want_fill.shape == (w["rows"],) + fe.fill_row and got_fill.dtype == torch.float32
    assert torch.equal(got_fill, _rounded(want_fill)) and not torch.equal(got_fill, want_fill)
    # a decoded copy, not a view of the buffer
    assert not (fe._fill_buf.data_ptr() <= got_fill.data_ptr() < fe._fill_buf.data_ptr() + fe._fill_buf.numel() * 4)
    want, got = fa._by_stage(parent, w), fa._by_stage(fe, w)
    for name, g, t in zip(LAYERS + ("output",), got, want):
        assert g.shape == t.shape and g.dtype == torch.float32 and bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0, name
        assert torch.equal(g, t), (name, float((g - t).abs().max()))
    # flags and sizes
    assert [io for st in fe.stages for io in st.io] == FLAGS16 and [io for st in parent.stages for io in st.io] == [(0, 1)] + FLAGS16[1:]
    C, Hp, Wp = fe.fill_row
    # bytes_per_item is smaller by exactly the half fill, n_off * C * Hp * Wp * 2 -- less what the placement rule, in bytes, no
    # longer fits inside the halved fill and therefore allocates and counts: on this 10 x 11 plane layer4's 4 096 B (layer2's 7 680
    # and layer3's 4 608 still lie inside 14 080); on the warehouse plane nothing moves (tests/test_mmp_fill_cpu.py)
    moved = [st for st, st0 in zip(fe.stages, parent.stages) if st0.in_fill and not st.in_fill]
    assert [st.name for st in moved] == ["layer4"] and [st.in_fill for st in fe.stages] == [False, True, True, False]
    assert [st.offset for st in fe.stages[1:3]] == [st.offset for st in parent.stages[1:3]]
    assert parent.bytes_per_item - fe.bytes_per_item == tn.N_OFF * (C * Hp * Wp * 2 - sum(2 * int(np.prod(st.buf_row)) * 4 for st in moved))
    assert fe._fill_buf.numel() * 4 == len(w["peds"]) * tn.N_OFF * C * Hp * Wp * 2
    # run() launches the same, returns the head's output and keeps the part names
    names = []
    out = fe.run(*fa._fill_args(w), lambda what, call: (names.append(what), call())[1])
    torch.cuda.synchronize()
    assert names == ["input"] + list(LAYERS) + ["head"] and torch.equal(out, want[-1])


# ---- 3. None and "f32" are the front end without the keyword -------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [None, "f32"])
def test_no_fill_is_the_parent_bit_for_bit(handle, fill):
    w = fa._net(0)
    for kw in ({}, dict(precision="f16"), dict(operands=fa.ALL3)):
        base = fa._front(handle, w, **kw)
        fe = fa._front(handle, w, fill=fill, **kw)
        assert not fe.fill_f16 and fe.operands == base.operands and fe.activations == base.activations
        assert [(st.Args, st.io, st.in_fill, st.offset) for st in fe.stages] == [(st.Args, st.io, st.in_fill, st.offset) for st in base.stages]
        assert fe.bytes_per_item == base.bytes_per_item and fe._fill_buf.shape == base._fill_buf.shape and fe._fill == base._fill
        assert [tuple(st.pp.shape) for st in fe.stages] == [tuple(st.pp.shape) for st in base.stages]
        assert torch.equal(fe.fill(*fa._fill_args(w)), base.fill(*fa._fill_args(w)))
        for name, g, t in zip(LAYERS + ("output",), fa._by_stage(fe, w), fa._by_stage(base, w)):
            assert torch.equal(g, t), (kw, name)


# ---- 4. a 16-channel stem: the first block has no projection, its identity is the binary16 value -------------------------------------------------
def test_sixteen_channel_stem_without_projection(handle):
    w = fa._net(0)
    blocks = w["specs"]["blocks"][1:]                                  # two blocks 16 -> 16
    assert len(blocks) == 2 and all(b.wd is None and b.w1.shape[1] == 16 for b in blocks)
    w16 = dict(w, specs=dict(stem=sr.random_spec(16, seed=16), blocks=blocks))
    rows = w["rows"]
    parent = fa._front(handle, w16, precision="f16")
    x = _rounded(parent.fill(*fa._fill_args(w16)).reshape(rows, *parent.fill_row))
    parent_out = parent.run_stage("layer1", rows).clone()
    # the chain: the float32-memory kernel on the host-rounded x, rounded between the two blocks
    st, keep = parent.stages[0], []
    for j, a in enumerate(st.args):
        out = torch.full((rows, 16) + tuple(st.planes[j + 1]), float("nan"), dtype=torch.float32, device="cuda")
        a.x, a.out, a.M = x.data_ptr(), out.data_ptr(), rows
        handle.mmp_block_f16(a)
        torch.cuda.synchronize()
        keep.append(x)
        x = out if j == len(st.args) - 1 else _rounded(out)
    fe = fa._front(handle, w16, precision="f16", fill="f16")
    assert [io for s in fe.stages for io in s.io] == [(1, 1), (1, 0)]
    fe.fill(*fa._fill_args(w16))
    got = fe.run_stage("layer1", rows).clone()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
    assert torch.equal(got, x), float((got - x).abs().max())
    assert not torch.equal(got, parent_out), "the unrounded identity of the parent gave the same bits: the case shows nothing"


# ---- 5. the closed loop --------------------------------------------------------------------------------------------------------------------------
def test_closed_loop_with_a_binary16_fill(world):
    H, K = 2, 5
    recs = {}
    for key, kw in (("parent", {}), ("fill16", dict(mmp_fill="f16"))):
        ev = l2._evaluator(world, H, K, mmp_precision="f16", **kw)
        rec = recs[key] = []
        try:
            fe = ev.mmp_front
            assert fe.fill_f16 == (key == "fill16")
            res = ev.run(max_steps=1, record=rec)
            assert len(rec) == 1 and np.isfinite(res.trajectory).all() and all(np.isfinite(r["P"]).all() and np.isfinite(r["dyn"]).all() for r in rec)
            if key == "fill16":
                assert [io for n in LAYERS for io in fe.stage(n).io] == FLAGS16
                n = lp.B * H
                assert ev.mmp_chunk >= n
                specs = {k[4:]: v for k, v in l2.l4.FRONT.items()}
                alone = MmpFrontEnd(ev.h, ev.dt, ev.dev, ev.mmp_Hm, ev.mmp_Wm, ev.N, lp.TF, ev.mmp_rescale, MMP_SIGMA, ev.mmp_ref, blocks4=l2.l4.BLOCKS4,
                                    head=l2.l4.exact_head(K, H)[0], precision="f16", fill="f16", **specs)
                alone.allocate(n)
                args = (ev.hist.data_ptr(), ev.hcount.data_ptr(), ev.B, H, None, n)
                a, b = fe.run(*args).clone(), alone.run(*args).clone()
                torch.cuda.synchronize()
                assert a.shape == (n * ev.N, 2 * K) and bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0 and torch.equal(a, b)
        finally:
            ev.close()
    for a, b in zip(recs["parent"], recs["fill16"]):
        assert np.array_equal(a["P"], b["P"]) and np.array_equal(a["dyn"], b["dyn"])
    with pytest.raises(ValueError, match="mmp_fill: 'f16' needs mmp_precision = 'f16'"):
        l2._evaluator(world, H, K, mmp_fill="f16")
    with pytest.raises(ValueError, match="mmp_fill: 'half' is none of None, 'f32' and 'f16'"):
        l2._evaluator(world, H, K, mmp_precision="f16", mmp_fill="half")
