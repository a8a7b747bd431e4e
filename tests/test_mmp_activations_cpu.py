"""CPU tests of binary16 activations between the mmp network's f16 blocks (csrc/nmpc_mmp_block_f16.h, ``MmpFrontEnd(activations=...)``):
the octet form on the host (``mmp_stem.pack_activations_f16`` / ``unpack_activations_f16``), ``check_activations`` in the three host
classes, which tensors a front end makes binary16 and what it launches for them, the model's extension
(tests/mmp_act_f16_reference.py), the entry points, and the resources of the 27 kernels from the cross-compiled code object. The device
side: tests/test_gpu_mmp_block_f16_io.py and tests/test_gpu_mmp_front_activations.py."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import dyobav_mpcnwta_warehouse_amd as nm
import mmp_act_f16_reference as ha
import mmp_block2_f16_reference as h2
import mmp_block2_reference as b2
import mmp_net_reference as nr
from dyobav_mpcnwta_warehouse_amd import _capi, snap
from dyobav_mpcnwta_warehouse_amd import mmp_stem as ms
from dyobav_mpcnwta_warehouse_amd.mmp_front import MmpFrontEnd
from dyobav_mpcnwta_warehouse_amd.mmp_interface import MmpInterface
from dyobav_mpcnwta_warehouse_amd.mmp_stem import pack_activations_f16, round_f16, unpack_activations_f16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE_OF = "{0}activations: {1!r} is none of None, 'f32' and 'f16'"
NO_STAGE = "{0}activations: 'f16' needs a stage on f16 operands ({0}operands)"
ALL_F16 = {"layer2": "f16", "layer3": "f16", "layer4": "f16"}


# ---- 1. the octet form on the host --------------------------------------------------------------------------------------------------------------
def test_pack_is_the_octet_form_and_unpack_inverts_it():
    x = np.random.default_rng(1).standard_normal((3, 24, 5, 7)).astype(np.float32)
    a = pack_activations_f16(x)
    assert a.shape == (3, 3, 5, 7, 8) and a.dtype == np.uint16 and a.flags.c_contiguous
    h = round_f16(x)
    for n, c, y, xx in ((0, 0, 0, 0), (2, 23, 4, 6), (1, 7, 2, 3), (1, 8, 2, 3), (0, 17, 4, 0), (2, 9, 0, 6)):
        assert a[n, c // 8, y, xx, c % 8] == h[n, c, y, xx].view(np.uint16), (n, c, y, xx)
        # ... which is element ((((n C / 8 + c / 8) H + y) W + x) 8 + c % 8 of the flat array: row n starts n C H W halves in
        assert a.reshape(-1)[(((n * 3 + c // 8) * 5 + y) * 7 + xx) * 8 + c % 8] == h[n, c, y, xx].view(np.uint16)
    back = unpack_activations_f16(a)
    assert back.shape == x.shape and back.dtype == np.float32 and back.flags.c_contiguous
    assert np.array_equal(back, h.astype(np.float32)) and not np.array_equal(back, x)
    assert np.array_equal(pack_activations_f16(back), a)                     # binary16 values round to themselves
    assert np.array_equal(pack_activations_f16(x.astype(np.float64)), a)


def test_pack_saturates_keeps_nan_and_subnormals():
    x = np.zeros((1, 8, 1, 2), dtype=np.float32)
    x[0, :, 0, 0] = [1e6, -7e4, np.inf, -np.inf, np.nan, 65504.0, 65520.0, -65519.0]
    x[0, :, 0, 1] = [2.0 ** -24, -2.0 ** -24, 3 * 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24, 2.0 ** -14, 1023 * 2.0 ** -24, 0.0]
    f = unpack_activations_f16(pack_activations_f16(x))
    big = f[0, :, 0, 0]
    assert np.array_equal(big[[0, 1, 2, 3, 5, 6, 7]], np.float32([65504, -65504, 65504, -65504, 65504, 65504, -65504])) and np.isnan(big[4])
    assert np.isnan(f).sum() == 1
    # subnormals are kept and ties go to even: 2^-25 -> 0, 1.5 x 2^-24 -> 2 x 2^-24
    assert np.array_equal(f[0, :, 0, 1], np.float32([1, -1, 3, 0, 2, 1024, 1023, 0]) * np.float32(2.0 ** -24))
    assert pack_activations_f16(x)[0, 0, 0, 1, 0] == 1 and pack_activations_f16(x)[0, 0, 0, 0, 4] & 0x7C00 == 0x7C00


def test_pack_and_unpack_refuse_other_shapes():
    for bad in (np.zeros((2, 12, 3, 3)), np.zeros((2, 0, 3, 3)), np.zeros((8, 3, 3)), np.zeros((1, 2, 8, 3, 3))):
        with pytest.raises(ValueError, match="pack_activations_f16"):
            pack_activations_f16(bad)
    for bad in (np.zeros((2, 1, 3, 3, 4), dtype=np.uint16), np.zeros((2, 1, 3, 3, 8), dtype=np.float16), np.zeros((2, 8, 3, 3), dtype=np.uint16)):
        with pytest.raises(ValueError, match="unpack_activations_f16"):
            unpack_activations_f16(bad)


# ---- 2. check_activations in the three classes ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def specs():
    return dict(zip(("stem", "blocks", "blocks2", "blocks3", "blocks4", "head"), ms.split_network_whole(nr.in_double(nr.made_net(nr.SHAPES[0])))))


def test_check_activations_accepts_and_refuses_with_one_sentence_each():
    ca = MmpFrontEnd.check_activations
    f32 = {"layer1": "f32", "layer2": "f32", "layer3": "f32", "layer4": "f32"}
    for operands in ({}, f32, dict(f32, layer3="f16")):
        assert ca(None, operands) == ca("f32", operands) == ca(None, operands, prefix="mmp_") == "f32"
    for operands in (dict(f32, layer2="f16"), dict(f32, layer4="f16"), dict(f32, **ALL_F16), {"layer3": "f16"}):
        assert ca("f16", operands) == ca("f16", operands, prefix="mmp_") == "f16"
    for prefix in ("", "mmp_"):
        for value in ("bf16", "F16", "half", 16, True, ("f16",), ""):
            with pytest.raises(ValueError, match=re.escape(NONE_OF.format(prefix, value))):
                ca(value, dict(f32, layer2="f16"), prefix=prefix)
        for operands in ({}, f32, {"layer1": "f32"}):
            with pytest.raises(ValueError, match=re.escape(NO_STAGE.format(prefix))):
                ca("f16", operands, prefix=prefix)


def test_the_three_classes_take_and_refuse_the_same_before_any_device_is_touched(specs):
    from dyobav_mpcnwta_warehouse_amd.evaluate import BatchEvaluator
    it = MmpInterface(None, operands=ALL_F16, activations="f16", **specs)
    assert it._activations == "f16" and MmpInterface(None, operands=ALL_F16, **specs)._activations == "f32"
    assert MmpInterface(None, activations="f32", **specs)._activations == "f32"
    with pytest.raises(ValueError, match=re.escape(NO_STAGE.format(""))):
        MmpInterface(None, activations="f16", **specs)
    with pytest.raises(ValueError, match=re.escape(NONE_OF.format("", "f64"))):
        MmpInterface(None, operands=ALL_F16, activations="f64", **specs)
    with pytest.raises(ValueError, match=re.escape("operands: 'layer1': only layer2, layer3 and layer4 have an f16 kernel")):
        MmpInterface(None, operands={"layer1": "f16"}, activations="f64", **specs)      # check_operands speaks first
    ok = dict(predictor="mmp", network=None, ref_image=np.zeros((37, 41)), transform=snap.WorldTransform(), **{"mmp_" + k: v for k, v in specs.items()})
    ev = lambda **kw: BatchEvaluator(None, None, None, None, None, None, **dict(ok, **kw))
    with pytest.raises(ValueError, match=re.escape(NO_STAGE.format("mmp_"))):
        ev(mmp_activations="f16")
    with pytest.raises(ValueError, match=re.escape(NO_STAGE.format("mmp_"))):
        ev(mmp_activations="f16", mmp_operands={"layer2": "f32"})
    with pytest.raises(ValueError, match=re.escape(NONE_OF.format("mmp_", "f64"))):
        ev(mmp_activations="f64", mmp_operands=ALL_F16)
    with pytest.raises(ValueError, match=re.escape("mmp_activations needs predictor = 'mmp'")):
        BatchEvaluator(None, None, None, None, None, None, predictor="cvmp", mmp_activations="f16")
    for activations in ("f16", "f32", None):                                       # accepted: the NEXT refusal is the one that speaks
        with pytest.raises(ValueError, match="needs n_hyp = 1 and fused = True"):
            ev(mmp_activations=activations, mmp_operands=ALL_F16, fused=False)


# ---- 3. which tensors a front end makes binary16, and what it launches for them ---------------------------------------------------------------
class _NoDevice:
    """Stands where the handle does in a front end that launches nothing: every launch method is its own name."""

    def __getattr__(self, name):
        return name


def _front(specs, **kw):
    return MmpFrontEnd(_NoDevice(), np.float32, "cpu", 37, 41, 2, snap.WorldTransform(), 1.0, 1.0, torch.zeros(37, 41), **specs, **kw)


def test_all_three_stages_make_twelve_of_thirteen_inputs_binary16(specs):
    fe, plain = _front(specs, operands=ALL_F16, activations="f16"), _front(specs, operands=ALL_F16)
    assert fe.activations == "f16" and plain.activations == "f32"
    assert [len(st.specs) for st in fe.stages] == [3, 4, 6, 3]
    assert fe.stage("layer1").io is None and fe.stage("layer1").launch == "mmp_block"
    flags = [io for name in ("layer2", "layer3", "layer4") for io in fe.stage(name).io]
    assert flags == [(0, 1)] + [(1, 1)] * 11 + [(1, 0)] and sum(x for x, _ in flags) == 12
    assert [fe.stage(n).launch for n in ("layer2", "layer3", "layer4")] == ["mmp_block2_f16_io", "mmp_block3_f16_io", "mmp_block4_f16_io"]
    assert [fe.stage(n).out_f16 for n in ("layer1", "layer2", "layer3", "layer4")] == [False, True, True, False]
    # the flags are those of the model's statement of the rule
    want = ha.binary16_outputs([(st.name, len(st.specs)) for st in fe.stages], fe.operands, "f16")
    for st in fe.stages[1:]:
        assert tuple(bool(o) for _, o in st.io) == want[st.name]
        assert tuple(bool(x) for x, _ in st.io)[1:] == want[st.name][:-1]
    # nothing else of a stage's record moves, nor the buffers: the halved footprint is not exploited
    for a, b in zip(fe.stages, plain.stages):
        assert (a.name, a.cins, a.Args, a.planes, a.buf_row, a.in_fill, a.offset) == (b.name, b.cins, b.Args, b.planes, b.buf_row, b.in_fill, b.offset)
    assert fe.bytes_per_item == plain.bytes_per_item and fe.row == plain.row and fe.fill_row == plain.fill_row


def test_mixed_operands_keep_float32_at_every_float32_reader_and_writer(specs):
    fe = _front(specs, operands={"layer3": "f16", "layer4": "f16"}, activations="f16")
    assert fe.stage("layer2").io is None and fe.stage("layer2").launch == "mmp_block2"
    assert fe.stage("layer3").io == ((0, 1),) + ((1, 1),) * 5 and fe.stage("layer4").io == ((1, 1), (1, 1), (1, 0))
    fe = _front(specs, operands={"layer2": "f16", "layer4": "f16"}, activations="f16")
    assert fe.stage("layer3").io is None and fe.stage("layer3").launch == "mmp_block3"
    assert fe.stage("layer2").io == ((0, 1), (1, 1), (1, 1), (1, 0)) and fe.stage("layer4").io == ((0, 1), (1, 1), (1, 0))
    assert not fe.stage("layer2").out_f16 and not fe.stage("layer4").out_f16
    fe = _front(dict(specs, head=None, blocks4=None), operands={"layer3": "f16"}, activations="f16")     # the caller's network reads float32
    assert fe.stage("layer3").io == ((0, 1),) + ((1, 1),) * 4 + ((1, 0),)


def test_none_and_f32_change_no_launch(specs):
    plain = _front(specs, operands=ALL_F16)
    for activations in (None, "f32"):
        fe = _front(specs, operands=ALL_F16, activations=activations)
        assert fe.activations == "f32"
        for a, b in zip(fe.stages, plain.stages):
            assert a.io is None and b.io is None and a.launch == b.launch and not a.out_f16
    assert [st.launch for st in plain.stages] == ["mmp_block", "mmp_block2_f16", "mmp_block3_f16", "mmp_block4_f16"]
    with pytest.raises(ValueError, match=re.escape(NO_STAGE.format(""))):
        _front(specs, activations="f16")


# ---- 4. the model's extension -------------------------------------------------------------------------------------------------------------------
def test_the_extended_model_chain_is_the_old_one_when_nothing_is_binary16():
    x = b2.random_x(2, 16, 9, 13, seed=3)
    blocks = [b2.random_block2(16, 4, 2, True), b2.random_block2(32, 5, 1, False), b2.random_block2(32, 6, 1, False)]
    old = h2.model_chain(x, blocks)
    for flags in (None, (False, False, False)):
        new = ha.model_chain(h2, x, blocks, flags)
        assert len(new) == 3 and all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(old, new))
    half = ha.model_chain(h2, x, blocks, (True, True, False))
    assert np.array_equal(half[0], round_f16(old[0]).astype(np.float32)) and not np.array_equal(half[0], old[0])
    assert np.array_equal(half[1], round_f16(half[1]).astype(np.float32)) and not np.array_equal(half[2], round_f16(half[2]).astype(np.float32))
    # the second block's identity is the binary16 value: the float32 chain from the rounded tensor on gives the same
    assert np.array_equal(half[2], h2.model_chain(half[1], blocks[2:])[0])
    stages = [("layer1", 3), ("layer2", 4), ("layer3", 6), ("layer4", 3)]
    none = {name: (False,) * count for name, count in stages}
    assert ha.binary16_outputs(stages, ALL_F16, "f32") == ha.binary16_outputs(stages, ALL_F16, None) == ha.binary16_outputs(stages, {}, "f16") == none
    assert ha.binary16_outputs(stages, ALL_F16, "f16") == dict(none, layer2=(True,) * 4, layer3=(True,) * 6, layer4=(True, True, False))
    assert ha.binary16_outputs(stages, {"layer2": "f16", "layer4": "f16"}, "f16") == dict(none, layer2=(True, True, True, False), layer4=(True, True, False))


# ---- 5. the entry points and the kernels -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 4])
def test_entry_points_refuse_null_arguments_and_bad_flags_without_a_device(n):
    lib = nm.load_library()
    name = f"nmpc_mmp_block{n}_f16_io"
    assert name in nm.EXPORTED_SYMBOLS and hasattr(lib, name) and hasattr(nm.Handle, f"mmp_block{n}_f16_io")
    a = getattr(_capi, f"NmpcMmpBlock{n}F16Args")()
    assert ctypes.sizeof(a) == 120
    fn = getattr(lib, name)
    assert fn(None, ctypes.byref(a), 0, 0) == -1 and fn(None, None, 1, 1) == -1
    header = open(os.path.join(ROOT, "include", "nmpc_hip.h")).read()
    assert f"int {name}(nmpc_handle h, const nmpc_mmp_block{n}_f16_args *a, int32_t x_f16, int32_t out_f16);" in header
    assert "#define NMPC_ABI_VERSION 5" in header


GEOMETRIES = {2: dict(lds={1: 4 * 592 * 16, 2: 8 * 592 * 16}, wg={1: 4, 2: 2}),
              3: dict(lds={1: 36864, 2: 73728}, wg={1: 4, 2: 2}),
              4: dict(lds={1: 40960, 2: 40960}, wg={1: 3, 2: 3})}


def test_the_27_kernels_use_no_scratch_and_keep_their_siblings_occupancy():
    """From the shipped code object: per geometry and form of x and out in memory (three of each) the three kernels <stride 2,
    projection>, <stride 1, projection>, <stride 1, identity>; no scratch, no spills, the static LDS of the sibling on float32
    memory, and registers that allow the workgroups per CU the kernel's __launch_bounds__ claims (four waves of a workgroup on
    four SIMDs: workgroups per CU = waves per SIMD)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    nm.build_library()
    res = {kernel_resources.short_name(k): v for k, v in kernel_resources.kernel_resources(nm.library_path()).items()}
    pattern = r"mmp_blkh_kernel<nmpc::MmpBlkhIo<nmpc::MmpBlock(\d)HGeom, (true|false), (true|false)>, (\d), (true|false)>"
    mine = {re.search(pattern, k).groups(): v for k, v in res.items() if re.search(pattern, k)}
    forms = [("false", "true"), ("true", "false"), ("true", "true")]
    assert sorted(mine) == sorted((str(n), x, o, s, p) for n in (2, 3, 4) for x, o in forms for s, p in (("2", "true"), ("1", "true"), ("1", "false")))
    for (n, x, o, s, p), r in sorted(mine.items()):
        sibling = res[next(k for k in res if re.search(rf"mmp_blkh_kernel<nmpc::MmpBlock{n}HGeom, {s}, {p}>", k))]
        g = GEOMETRIES[int(n)]
        print(n, x, o, s, p, r)
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, ((n, x, o, s, p), r)
        assert r["lds_static"] == sibling["lds_static"] == g["lds"][int(s)], ((n, x, o, s, p), r)
        claimed = g["wg"][int(s)]
        assert (160 * 1024) // r["lds_static"] >= claimed
        regs = r["vgpr"] + max(r["agpr"], 0)
        assert 512 // (-(-regs // 8) * 8) >= claimed, ((n, x, o, s, p), r)
