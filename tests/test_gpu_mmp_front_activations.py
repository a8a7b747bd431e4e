"""GPU tests of ``MmpFrontEnd(..., activations="f16")`` -- binary16 activations in memory between the blocks on f16 operands
(csrc/nmpc_mmp_block_f16.h, ``nmpc_mmp_block{2,3,4}_f16_io``) -- with the real-valued network, world and float64 module of
tests/test_gpu_mmp_net.py on its 37 x 41 map (M = 4 rows):

1. the front end against a CHAIN of the kernels on float32 memory (``nmpc_mmp_block{2,3,4}_f16``, and the float32 kernels for a
   float32 stage), one launch per block on buffers of the test's own, rounded between blocks on the host with ``round_f16`` wherever
   the rule says the tensor is binary16 (tests/mmp_act_f16_reference.binary16_outputs): every stage's ``run_stage`` result and the
   head's output, bit for bit; with layer2 .. layer4 on f16, with layer3 and layer4 only, and with layer3 on float32 between them;
2. ``activations`` of ``None`` or ``"f32"`` against the front end built without the argument, at every stage;
3. accuracy against the float64 module by the protocol of tests/test_gpu_mmp_net_f16_layer2.py: the yardstick is |model_chain -
   float64 module| with ``model_chain`` rounding between blocks as the rule says (tests/mmp_act_f16_reference.py); the device lies
   within ``BAR`` = 4 yardsticks at layer2, layer3, layer4 and the output;
4. the closed loop: ``BatchEvaluator(mmp_activations="f16")`` against a stand-alone front end with the same arguments.

Measured on an MI355X, all three stages on f16 operands, |device - float64| / yardstick (the bar is 4) and |device - model| /
yardstick at layer2, layer3, layer4 and the output:

    map          M    layer2        layer3        layer4        output
    37 x 41      4    1.19  1.04    1.46  1.24    1.09  1.11    0.70  0.58
    293 x 329    2    0.85  1.03    1.12  1.05    0.67  1.01    1.17  0.68      (once by hand through ``accuracy(handle, 1)``; not in the suite)

The yardsticks themselves, next to the parent's (operands only): 5.6e-3 / 6.3e-3 / 3.7e-3 / 3.7e-4 against 4.0e-3 / 5.3e-3 / 2.2e-3 /
2.3e-4 on the small map, 7.6e-3 / 1.5e-2 / 1.8e-2 / 8.2e-4 against 4.8e-3 / 1.4e-2 / 1.1e-2 / 7.0e-4 on the large one: the roundings
between the blocks cost 1.07-1.65 times what the operands alone do."""
import functools

import numpy as np
import pytest
import torch

import mmp_act_f16_reference as ha
import mmp_block2_f16_reference as h2
import mmp_block3_f16_reference as h3
import mmp_block4_f16_reference as h4
import mmp_cases as mc
import mmp_net_reference as nr
import mmp_reference as mr
import test_gpu_mmp_block2_f16_loop as l2
import test_gpu_mmp_block3_loop as lp
import test_gpu_mmp_net as tn
from dyobav_mpcnwta_warehouse_amd import mmp_stem as ms
from dyobav_mpcnwta_warehouse_amd.evaluate import MMP_SIGMA
from dyobav_mpcnwta_warehouse_amd.mmp_front import MmpFrontEnd
from dyobav_mpcnwta_warehouse_amd.mmp_stem import round_f16

pytestmark = pytest.mark.gpu

handle, world = tn.handle, lp.world
LAYERS = ("layer1", "layer2", "layer3", "layer4")
ALL3 = {"layer2": "f16", "layer3": "f16", "layer4": "f16"}
SETTINGS = {"all-three": ALL3, "layer3-layer4": {"layer3": "f16", "layer4": "f16"}, "layer2-layer4": {"layer2": "f16", "layer4": "f16"}}
PEDESTRIANS = ((2, 1), (2,))                                        # M = 4 rows on the small map, M = 2 on the large one


@functools.lru_cache(maxsize=None)
def _net(k):
    """The world of shape ``k`` of ``nr.SHAPES``: the float64 module, its stages on the pedestrians' stack, the specs, the device arrays."""
    shape, peds = nr.SHAPES[k], PEDESTRIANS[k]
    Hm, Wm = shape["Hm"], shape["Wm"]
    ref = nr.label_image(Hm, Wm)
    trajs = tn._trajectories(tn.SPREAD[Hm])
    hist, hcount = mc.hist_arrays(trajs)
    stack = np.concatenate([mr.input_stack(mr.input_planes(mr.to_pixels(trajs[p], tn.TF, tn.RESCALE), ref), tn.N_OFF) for p in peds])
    net64 = nr.in_double(nr.made_net(shape))
    want = [t.numpy() for t in nr.stages(net64, stack)]
    specs = dict(zip(("stem", "blocks", "blocks2", "blocks3", "blocks4", "head"), ms.split_network_whole(net64)))
    dev = dict(ref=torch.from_numpy(ref).cuda(), hist=torch.from_numpy(np.ascontiguousarray(hist.reshape(tn.B, tn.H, 5, 2))).cuda(),
               hcount=torch.from_numpy(np.ascontiguousarray(hcount.reshape(tn.B, tn.H))).cuda(), items=torch.tensor(peds, dtype=torch.long, device="cuda"))
    return dict(Hm=Hm, Wm=Wm, peds=peds, rows=len(peds) * tn.N_OFF, net64=net64, want=want, specs=specs, dev=dev)


def _front(handle, w, **kw):
    fe = MmpFrontEnd(handle, dtype=np.float64, device=w["dev"]["ref"].device, Hm=w["Hm"], Wm=w["Wm"], n_off=tn.N_OFF, transform=tn.TF,
                     rescale=tn.RESCALE, sigma=tn.SIGMA, ref_image=w["dev"]["ref"], **w["specs"], **kw)
    fe.allocate(len(w["peds"]))
    return fe


def _fill_args(w):
    d = w["dev"]
    return d["hist"].data_ptr(), d["hcount"].data_ptr(), tn.B, tn.H, d["items"].data_ptr(), len(w["peds"])


def _by_stage(fe, w):
    """[layer1, layer2, layer3, layer4, output] through the public steps: ``fill``, ``run_stage`` per stage, ``run_head``."""
    fe.fill(*_fill_args(w))
    got = [fe.run_stage(name, w["rows"]).clone() for name in LAYERS] + [fe.run_head(w["rows"]).clone()]
    torch.cuda.synchronize()
    return got


def _chain(handle, w, operands):
    """The same five tensors from one launch per block of the kernels on FLOAT32 memory, each on buffers of its own, rounded in
    between on the host where the rule makes the tensor binary16."""
    fe0, rows = _front(handle, w, operands=operands), w["rows"]
    fe0.fill(*_fill_args(w))
    x = fe0.run_stage("layer1", rows).clone()
    flags = ha.binary16_outputs([(st.name, len(st.specs)) for st in fe0.stages], fe0.operands, "f16")
    outs, keep = [x], []
    for st in fe0.stages[1:]:
        for j, a in enumerate(st.args):
            out = torch.full((rows, st.channels) + tuple(st.planes[j + 1]), float("nan"), dtype=torch.float32, device="cuda")
            a.x, a.out, a.M = x.data_ptr(), out.data_ptr(), rows
            st.launch(a)
            torch.cuda.synchronize()
            if flags[st.name][j]:
                out = torch.from_numpy(round_f16(out.cpu().numpy()).astype(np.float32)).cuda()
            keep.append(x)
            x = out
        outs.append(x)
    last = fe0.stages[-1]
    last.pp[(len(last.args) - 1) % 2][:x.numel()].copy_(x.reshape(-1))          # where the head reads layer4
    outs.append(fe0.run_head(rows).clone())
    torch.cuda.synchronize()
    return outs, flags


# ---- 1. against the chain of the parent's kernels ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_front_end_equals_the_chain_of_kernels_on_float32_memory(handle, setting):
    w, operands = _net(0), SETTINGS[setting]
    want, flags = _chain(handle, w, operands)
    assert sum(sum(v) for v in flags.values()) == {"all-three": 12, "layer3-layer4": 8, "layer2-layer4": 5}[setting]
    fe = _front(handle, w, operands=operands, activations="f16")
    got = _by_stage(fe, w)
    for name, g, t in zip(LAYERS + ("output",), got, want):
        assert g.shape == t.shape and g.dtype == torch.float32 and bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0, name
        assert torch.equal(g, t), (setting, name, float((g - t).abs().max()))
    # a stage whose last tensor is binary16 returns a decoded copy, every other one a view of its buffer
    for st in fe.stages:
        res = fe.run_stage(st.name, w["rows"])
        inside = st.pp.data_ptr() <= res.data_ptr() < st.pp.data_ptr() + st.pp.numel() * 4
        assert inside == (not st.out_f16) and st.out_f16 == flags[st.name][-1], st.name
    # run() launches the same and returns the head's output; its parts keep their names
    names = []
    out = fe.run(*_fill_args(w), lambda what, call: (names.append(what), call())[1])
    torch.cuda.synchronize()
    assert names == ["input"] + list(LAYERS) + ["head"] and torch.equal(out, want[-1])
    # ... and the rounding between the blocks is something: the front end on float32 activations gives other bits
    plain = _by_stage(_front(handle, w, operands=operands), w)
    assert torch.equal(plain[0], got[0]) and not torch.equal(plain[-1], got[-1])


# ---- 2. None and "f32" are the front end without the argument ---------------------------------------------------------------------------------
@pytest.mark.parametrize("activations", [None, "f32"])
def test_no_activations_is_the_parent_bit_for_bit(handle, activations):
    w = _net(0)
    for operands in (ALL3, None):
        want = _by_stage(_front(handle, w, operands=operands), w)
        fe = _front(handle, w, operands=operands, activations=activations)
        assert fe.activations == "f32" and all(st.io is None and not st.out_f16 for st in fe.stages)
        for name, g, t in zip(LAYERS + ("output",), _by_stage(fe, w), want):
            assert torch.equal(g, t), (operands, name)


# ---- 3. accuracy against the float64 module ---------------------------------------------------------------------------------------------------
def accuracy(handle, k):
    """|device - float64 module| over the yardstick |model_chain - float64 module| at layer2, layer3, layer4 and the output on shape
    ``k``, all three stages on f16 operands with binary16 activations; prints the yardsticks, the parent's (operands only) beside them."""
    w = _net(k)
    net64, want, specs, rows = w["net64"], w["want"], w["specs"], w["rows"]
    stages = [(name, len(specs[arg])) for name, arg in zip(LAYERS, ("blocks", "blocks2", "blocks3", "blocks4"))]

    def model(activations):
        flags = ha.binary16_outputs(stages, ALL3, activations)
        m2 = ha.model_chain(h2, want[1].astype(np.float32), specs["blocks2"], flags["layer2"])[-1]
        m3 = ha.model_chain(h3, m2, specs["blocks3"], flags["layer3"])[-1]
        m4 = ha.model_chain(h4, m3, specs["blocks4"], flags["layer4"])[-1]
        out = [np.asarray(m, dtype=np.float64) for m in (m2, m3, m4)]
        with torch.no_grad():
            out.append(nr.finish(net64, torch.as_tensor(out[-1]).double(), 4).numpy())
        return out
    mine, parent = model("f16"), model("f32")
    yard = [float(np.abs(m - t).max()) for m, t in zip(mine, want[2:])]
    yard0 = [float(np.abs(m - t).max()) for m, t in zip(parent, want[2:])]
    assert all(y > 0 for y in yard + yard0)
    got = [g.cpu().numpy() for g in _by_stage(_front(handle, w, operands=ALL3, activations="f16"), w)[1:]]
    ratios = []
    for name, g, t, m, y, y0 in zip(nr.STAGE_NAMES[2:], got, want[2:], mine, yard, yard0):
        assert g.shape == t.shape == m.shape and g.shape[0] == rows and np.isfinite(g).all()
        r64, rm = float(np.abs(g - t).max()) / y, float(np.abs(g - m).max()) / y
        print(f"{w['Hm']} x {w['Wm']} M {rows} {name}: yardstick |model - float64| = {y:.3e} (operands only: {y0:.3e}, x {y / y0:.2f}; "
              f"|float64| up to {np.abs(t).max():.2f}); |device - float64| / yardstick = {r64:.2f}, |device - model| / yardstick = {rm:.2f}")
        ratios.append(r64)
    return ratios


def test_whole_network_with_binary16_activations_against_the_float64_module(handle):
    ratios = accuracy(handle, 0)
    assert max(ratios) <= nr.BAR, ratios


# ---- 4. the closed loop -----------------------------------------------------------------------------------------------------------------------
def test_closed_loop_with_binary16_activations(world):
    H, K = 2, 5
    ev = l2._evaluator(world, H, K, mmp_operands=ALL3, mmp_activations="f16")
    rec = []
    try:
        fe = ev.mmp_front
        assert fe.activations == "f16" and fe.operands == dict(ALL3, layer1="f32")
        assert [io for n in LAYERS[1:] for io in fe.stage(n).io] == [(0, 1)] + [(1, 1)] * 11 + [(1, 0)]
        res = ev.run(max_steps=2, record=rec)
        assert len(rec) == 2 and np.isfinite(res.trajectory).all() and all(np.isfinite(r["P"]).all() and np.isfinite(r["dyn"]).all() for r in rec)
        # the hypotheses of the evaluator's front end on its own histories are those of a stand-alone front end with the same arguments
        n = lp.B * H
        assert ev.mmp_chunk >= n
        specs = {k[4:]: v for k, v in l2.l4.FRONT.items()}
        alone = MmpFrontEnd(ev.h, ev.dt, ev.dev, ev.mmp_Hm, ev.mmp_Wm, ev.N, lp.TF, ev.mmp_rescale, MMP_SIGMA, ev.mmp_ref, blocks4=l2.l4.BLOCKS4,
                            head=l2.l4.exact_head(K, H)[0], operands=ALL3, activations="f16", **specs)
        alone.allocate(n)
        args = (ev.hist.data_ptr(), ev.hcount.data_ptr(), ev.B, H, None, n)
        a, b = fe.run(*args).clone(), alone.run(*args).clone()
        torch.cuda.synchronize()
        assert a.shape == (n * ev.N, 2 * K) and bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0 and torch.equal(a, b)
    finally:
        ev.close()
    with pytest.raises(ValueError, match="mmp_activations: 'f16' needs a stage on f16 operands \\(mmp_operands\\)"):
        l2._evaluator(world, H, K, mmp_activations="f16")
    with pytest.raises(ValueError, match="mmp_activations: 'half' is none of None, 'f32' and 'f16'"):
        l2._evaluator(world, H, K, mmp_operands=ALL3, mmp_activations="half")
