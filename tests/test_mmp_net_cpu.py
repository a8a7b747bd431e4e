"""CPU tests of the multi-hypothesis predictor's WHOLE network: the stand-in ``mmp_net_reference.Net`` against what was recorded
from the reference's own class (tests/golden/mmp_net.json), and the chain the device runs -- ``split_network_whole`` of that module,
through the float64 restatements of every stage (tests/mmp_stem_reference.py, mmp_block*_reference.py, mmp_head_reference.py) --
against the module itself in float64, at the full size of the network and at both recorded shapes: the 37 x 41 map (planes
10 x 11, 5 x 6, 3 x 3, 2 x 2; F = 128) and the 293 x 329 map (the warehouse's planes 74 x 83, 37 x 42, 19 x 21, 10 x 11; F = 3 200).

The bar of every comparison is 4 x ``twin_error``: per stage, four times what torch's own float32 module differs from the float64
module by on the same input (the project's standing margin over the reference's own float32 rounding). The restated chain differs
from the module only by the one rounding of each folded weight, scale and shift to float32; measured here, in units of the twin
error (the bar is 4):

    stage            stem    layer1  layer2  layer3  layer4  output
    37 x 41          0.05    0.07    0.10    0.09    0.14    0.12
    293 x 329        0.07    0.06    0.10    0.08    0.09    0.20

Controls: each wrong whole-network variant below runs through the same chain and must MISS the bar at the output. Measured
|variant - module| at the output in units of the twin error there (a variant passes below 4):

    variant                                                         37 x 41     293 x 329
    "eps"      the norms' eps left out of every fold                113         136
    "slopes"   slope_mid and slope_out swapped in every block       1.25e5      2.93e5
    "shift"    the projection's shift dropped, layer3's block 0     7.3e4       3.74e4
    "phase"    layer2's block 0 samples the odd phase               1.37e5      5.65e4
    "order"    fc1 reads the flatten as [H, W, C]                   (0.12)      2.15e6

Every variant bites where it is a defect. "order" on the 37 x 41 map is none: layer4's plane is 2 x 2 there, the pooled plane one
pixel, and [c][h][w] and [h][w][c] are the same list, so the variant IS the definition (0.12 is rounding alone) -- the bar cannot see
it at that shape and the test says so; the 293 x 329 map holds it.

The twin error itself (``test_twin_table``): 2.4e-6 to 6.1e-6 behind the convolution stages and 2.3e-7 at the output on the small
map, 2.1e-6 to 7.5e-6 and 6.9e-7 on the large one. The large shape runs on the first two rows of the rule's input, the small one
on all four."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mmp_block2_reference as b2
import mmp_block3_reference as b3
import mmp_block4_reference as b4
import mmp_block_reference as br
import mmp_head_reference as hr
import mmp_net_reference as nr
import mmp_stem_reference as sr
from dyobav_mpcnwta_warehouse_amd.mmp_stem import split_network_whole

SHAPE_IDS = [f"{s['Hm']}x{s['Wm']}" for s in nr.SHAPES]
ROWS = {37: 4, 293: 2}
CONTROLS = ("eps", "slopes", "shift", "phase", "order")
_BLOCK_MODULES = (br, b2, b3, b4)


@pytest.fixture(scope="module")
def recorded(golden_dir):
    doc = json.load(open(os.path.join(golden_dir, "mmp_net.json")))
    assert [{k: s[k] for k in ("Hm", "Wm", "fc_input", "K")} for s in doc["shapes"]] == list(nr.SHAPES)
    return dict(zip(SHAPE_IDS, doc["shapes"]))


@pytest.fixture(scope="module")
def made():
    """shape id -> (net, x, the float64 module's six stages, the twin error's six floats), computed once and shared (read-only)."""
    out = {}
    for sid, shape in zip(SHAPE_IDS, nr.SHAPES):
        net = nr.made_net(shape)
        x = nr.rule_input(shape["Hm"], shape["Wm"])[:ROWS[shape["Hm"]]]
        out[sid] = (net, x, [t.numpy() for t in nr.stages(nr.in_double(net), x)], nr.twin_error(net, x))
    return out


def _chain(specs, x=None, wrong=None, start=None):
    """The folded network through the float64 restatements: the six tensors of ``nr.STAGE_NAMES`` -- or, with ``start = (k, y)``,
    those behind stage ``k`` whose tensor is ``y``. ``wrong``: "phase" / "order" are the restatements' own wrong variants, in the
    first block of layer2 and in the head."""
    stem, head = specs[0], specs[5]
    out = [sr.stem(x, stem.weight, stem.scale, stem.shift, stem.slope)[0]] if start is None else [start[1]]
    first = 0 if start is None else start[0]
    for k, (mod, blocks) in enumerate(zip(_BLOCK_MODULES, specs[1:5])):
        if k < first:
            continue
        y = out[-1]
        for i, b in enumerate(blocks):
            y = mod.block(y, b, wrong="phase" if wrong == "phase" and (k, i) == (1, 0) else None)[0]
        out.append(y)
    out.append(hr.head(out[-1], head, wrong="order" if wrong == "order" else None)[0])
    return out if start is None else out[1:]


# ---- 1. the architecture pin: the stand-in is the reference's class -------------------------------------------------------------------
@pytest.mark.parametrize("sid", SHAPE_IDS)
def test_the_stand_in_is_the_recorded_class(recorded, sid):
    """Names and shapes of ``state_dict()`` in order, then the float64 values at every stage to 1e-10 relative: both sides ran the
    same float64 torch operations, only the library's order of summation may differ."""
    rec = recorded[sid]
    net = nr.made_net(rec)
    mine = [[name, list(t.shape)] for name, t in net.state_dict().items()]
    assert len(rec["state_dict"]) == 226 and mine == rec["state_dict"]
    x = nr.rule_input(rec["Hm"], rec["Wm"])
    got = nr.stages(nr.in_double(net), x)
    for name, t in zip(nr.STAGE_NAMES[:5], got):
        s = rec["samples"][name]
        want = np.array(s["values"])
        assert list(t.shape) == s["shape"] and want.shape == (64,) and np.abs(want).max() > 0.1
        have = t.reshape(-1).numpy()[nr.sample_index(name, t.numel())]
        assert np.abs(have - want).max() <= 1e-10 * np.abs(want).max(), name
    want = np.array(rec["output"])
    assert want.shape == got[5].shape == (4, 2 * rec["K"])
    assert np.abs(got[5].numpy() - want).max() <= 1e-10 * np.abs(want).max()
    # the rule itself: float32 values, gains of both signs, the rows differ
    assert all(torch.equal(t, t.float().double()) for t in nr.in_double(net).state_dict().values())
    gains = torch.cat([t for name, t in net.state_dict().items() if t.dim() == 1 and name.endswith(".weight")])
    assert 0.08 < float((gains < 0).float().mean()) < 0.25
    assert np.abs(want[0] - want[1]).max() > 1e-3


def test_the_small_stand_in_of_the_fold_tests_shares_the_recorded_entries(recorded):
    """``_Net4`` of tests/test_mmp_block4_cpu.py (on which ``_Net3`` and the layer tests build): the recorded names in the recorded
    order, and the recorded shapes but for its stem of 8 channels in place of 64."""
    from test_mmp_block4_cpu import _Net4
    rec = recorded[SHAPE_IDS[0]]["state_dict"]
    mine = [[name, list(t.shape)] for name, t in _Net4().state_dict().items()]
    assert [n for n, _ in mine] == [n for n, _ in rec]
    differ = [n for (n, a), (_, b) in zip(mine, rec) if a != b]
    assert differ == [f"resnet34.stem.conv1.{k}" for k in ("0.weight", "1.weight", "1.bias", "1.running_mean", "1.running_var")] + \
        ["resnet34.layer1.0.conv1.0.weight", "resnet34.layer1.0.downsample.0.weight"]
    assert all([8 if v == 64 else v for v in b] == a for (n, a), (_, b) in zip(mine, rec) if n in differ)


def test_hash_uniform_is_the_stated_generator():
    """splitmix64, written out with Python's integers."""
    M = (1 << 64) - 1

    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)
    for salt in (0, 1, 0xFFFFFFFF, (1 << 32) + 12345):
        seed = mix((salt * 0x9E3779B97F4A7C15 + 0x9E3779B97F4A7C15) & M)
        want = [(mix((seed + 0x9E3779B97F4A7C15 * i) & M) >> 11) * 2.0 ** -53 for i in range(1, 6)]
        assert nr.hash_uniform(5, salt).tolist() == want
    u = nr.hash_uniform(100000, 7)
    assert u.dtype == np.float64 and 0.0 <= u.min() and u.max() < 1.0 and abs(u.mean() - 0.5) < 0.005 and abs(u.var() - 1 / 12) < 0.002


def test_fixture_regenerates(golden_dir, tmp_path):
    """tests/golden/make_mmp_net_golden.py run on the reference's class reproduces mmp_net.json byte for byte (where the reference
    tree exists; the recording itself is what every other test reads)."""
    recipe = os.path.join(golden_dir, "make_mmp_net_golden.py")
    ref = next(l.split('"')[1] for l in open(recipe) if l.startswith("REF = "))
    if not os.path.exists(os.path.join(ref, "src", "pkg_motion_prediction", "net_module", "net.py")):
        pytest.skip("the reference tree is not on this machine")
    subprocess.run([sys.executable, recipe, str(tmp_path)], check=True, capture_output=True, timeout=600)
    assert open(os.path.join(str(tmp_path), "mmp_net.json"), "rb").read() == open(os.path.join(golden_dir, "mmp_net.json"), "rb").read()


# ---- 2. the restated chain on the folded weights against the module, stage by stage -----------------------------------------------------
@pytest.fixture(scope="module")
def chains(made):
    """shape id -> (the specs of ``split_network_whole``, the restated chain's six tensors)."""
    out = {}
    for sid, (net, x, want, twin) in made.items():
        specs = split_network_whole(net)
        out[sid] = (specs, _chain(specs, x))
    return out


@pytest.mark.parametrize("sid", SHAPE_IDS)
def test_restated_chain_equals_the_module_in_float64(made, chains, sid):
    net, x, want, twin = made[sid]
    specs, got = chains[sid]
    assert [len(s) for s in specs[1:5]] == [3, 4, 6, 3] and specs[5].w1.shape == (128, net.fc1.in_features)
    if sid == SHAPE_IDS[1]:
        assert [g.shape[2:] for g in got[:5]] == [(74, 83), (74, 83), (37, 42), (19, 21), (10, 11)] and net.fc1.in_features == 3200
    ratios = []
    for name, g, w, t in zip(nr.STAGE_NAMES, got, want, twin):
        assert g.shape == w.shape and t > 0
        ratios.append(float(np.abs(g - w).max()) / t)
    print(f"{sid}: |restated chain - module| / twin error per stage: " + "  ".join(f"{n} {r:.2f}" for n, r in zip(nr.STAGE_NAMES, ratios)))
    assert max(ratios) <= nr.BAR, ratios


def _variant(name, net, specs, x, got):
    """The output of the wrong whole-network variant ``name``; ``got``: the right chain's tensors, whose front it shares."""
    if name == "eps":
        bare = copy.deepcopy(net)
        for m in bare.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.eps = 0.0
        return _chain(split_network_whole(bare), x)[-1]
    if name == "slopes":
        swap = lambda bs: tuple(b._replace(slope_mid=b.slope_out, slope_out=b.slope_mid) for b in bs)
        return _chain((specs[0], *(swap(bs) for bs in specs[1:5]), specs[5]), start=(0, got[0]))[-1]
    if name == "shift":
        blocks3 = (specs[3][0]._replace(bd=np.zeros_like(specs[3][0].bd)),) + specs[3][1:]
        return _chain((*specs[:3], blocks3, *specs[4:]), start=(2, got[2]))[-1]
    if name == "phase":
        return _chain(specs, wrong="phase", start=(1, got[1]))[-1]
    return _chain(specs, wrong="order", start=(4, got[4]))[-1]


@pytest.mark.parametrize("name", CONTROLS)
@pytest.mark.parametrize("sid", SHAPE_IDS)
def test_wrong_variants_miss_the_bar(made, chains, sid, name):
    net, x, want, twin = made[sid]
    specs, got = chains[sid]
    assert specs[2][0].stride == 2 and specs[3][0].bd is not None and np.abs(specs[3][0].bd).min() > 0
    out = _variant(name, net, specs, x, got)
    factor = float(np.abs(out - want[5]).max()) / twin[5]
    print(f"{sid}: variant {name!r}: |variant - module| at the output = {factor:.3g} x the twin error (the bar is {nr.BAR:g})")
    if name == "order" and not hr.applies("order", *got[4].shape[1:]):
        # (a pooled plane of one pixel: [c][h][w] and [h][w][c] are the same list, the variant IS the definition at this shape)
        assert got[4].shape[2:] == (2, 2) and factor <= nr.BAR
        return
    assert factor > nr.BAR, f"the bar admits the variant {name!r}"


# ---- 3. the twin table ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sid", SHAPE_IDS)
def test_twin_table(made, sid):
    """The yardstick itself, printed: it is a float32 rounding error -- far above the float64 module's own, far below the signal."""
    net, x, want, twin = made[sid]
    print(f"{sid}: twin error per stage: " + "  ".join(f"{n} {t:.2e}" for n, t in zip(nr.STAGE_NAMES, twin)))
    for t, w in zip(twin, want):
        assert 2.0 ** -30 * np.abs(w).max() < t < 2.0 ** -12 * np.abs(w).max()
