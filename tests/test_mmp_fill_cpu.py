"""CPU tests of the fused first layer's binary16 output (``nmpc_mmp_stem_io_*``, csrc/nmpc_mmp_stem.h) and of the switch that reaches
it, ``fill=`` / ``mmp_fill=``: ``check_fill`` in the three host classes, the two entry points without a device, the placement rule
in bytes as a pure function, the stage records a front end builds under the switch, and the resources of the shipped kernels. The
device side: tests/test_gpu_mmp_stem_io.py and tests/test_gpu_mmp_front_fill.py."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import dyobav_mpcnwta_warehouse_amd as nm
import mmp_net_reference as nr
from dyobav_mpcnwta_warehouse_amd import _capi, snap
from dyobav_mpcnwta_warehouse_amd import mmp_stem as ms
from dyobav_mpcnwta_warehouse_amd.mmp_front import MmpFrontEnd
from dyobav_mpcnwta_warehouse_amd.mmp_interface import MmpInterface

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS = ("layer1", "layer2", "layer3", "layer4")
NONE_OF = "{0}fill: {1!r} is none of None, 'f32' and 'f16'"
NEEDS_STEM = "{0}fill: 'f16' needs {0}stem (the input stack stays float32: only the fused first layer writes binary16)"
NEEDS_PRECISION = "{0}fill: 'f16' needs {0}precision = 'f16' (layer1's first block reads binary16 only on f16 operands)"


@pytest.fixture(scope="module")
def specs():
    return dict(zip(("stem", "blocks", "blocks2", "blocks3", "blocks4", "head"), ms.split_network_whole(nr.in_double(nr.made_net(nr.SHAPES[0])))))


# ---- 1. check_fill ---------------------------------------------------------------------------------------------------------------------------------
def test_check_fill_accepts_and_refuses_with_one_sentence_each(specs):
    six = MmpFrontEnd.check_specs(**specs)
    none = MmpFrontEnd.check_specs(None, None, head=None)
    cf = MmpFrontEnd.check_fill
    for precision in (None, "f32", "f16"):
        assert cf(None, precision, six) == cf("f32", precision, six) == cf(None, precision, none) == cf("f32", precision, none) == "f32"
    assert cf("f16", "f16", six) == cf("f16", "f16", six, prefix="mmp_") == "f16"
    for prefix in ("", "mmp_"):
        for value in ("f64", "bf16", "F16", "half", 16, True, ("f16",)):
            with pytest.raises(ValueError, match=re.escape(NONE_OF.format(prefix, value))):
                cf(value, "f16", six, prefix=prefix)
        with pytest.raises(ValueError, match=re.escape(NEEDS_STEM.format(prefix))):
            cf("f16", "f16", none, prefix=prefix)
        for precision in (None, "f32", "half"):
            with pytest.raises(ValueError, match=re.escape(NEEDS_PRECISION.format(prefix))):
                cf("f16", precision, six, prefix=prefix)


class _NoDevice:
    """Stands where the handle does in a front end that launches nothing: every launch method is its own name."""

    def __getattr__(self, name):
        return name


def _front(specs, Hm=37, Wm=41, **kw):
    return MmpFrontEnd(_NoDevice(), np.float32, "cpu", Hm, Wm, 2, snap.WorldTransform(), 1.0, 1.0, torch.zeros(Hm, Wm), **specs, **kw)


def test_the_three_classes_take_and_refuse_the_same_before_any_device_is_touched(specs):
    from dyobav_mpcnwta_warehouse_amd.evaluate import BatchEvaluator
    it = MmpInterface(None, precision="f16", fill="f16", **specs)
    assert it._fill == "f16" and it._switches["fill"] == "f16"
    for fill in (None, "f32"):
        assert MmpInterface(None, precision="f16", fill=fill, **specs)._fill == "f32" and MmpInterface(None, fill=fill, **specs)._fill == "f32"
    ok = dict(predictor="mmp", network=None, ref_image=np.zeros((37, 41)), transform=snap.WorldTransform(), **{"mmp_" + k: v for k, v in specs.items()})
    ev = lambda **kw: BatchEvaluator(None, None, None, None, None, None, **dict(ok, **kw))
    classes = ((lambda **kw: MmpInterface(None, **dict(specs, **kw)), ""), (lambda **kw: ev(**{"mmp_" + k: v for k, v in kw.items()}), "mmp_"),
               (lambda **kw: _front(specs, **kw), ""))
    for make, prefix in classes:
        with pytest.raises(ValueError, match=re.escape(NONE_OF.format(prefix, "f64"))):
            make(precision="f16", fill="f64")
        for precision in (None, "f32"):
            with pytest.raises(ValueError, match=re.escape(NEEDS_PRECISION.format(prefix))):
                make(precision=precision, fill="f16")
        # check_fill runs behind check_precision: the earlier refusals speak first and unchanged
        with pytest.raises(ValueError, match=re.escape(f"{prefix}precision: 'f64' is none of None, 'f32' and 'f16'")):
            make(precision="f64", fill="f16")
        with pytest.raises(ValueError, match=re.escape(f"{prefix}precision: 'f16', but {prefix}activations is 'f32'")):
            make(precision="f16", activations="f32", fill="f64")
    # without a stem nothing else can be given either, so the front end and the interface refuse on the stem
    with pytest.raises(ValueError, match=re.escape(NEEDS_STEM.format(""))):
        MmpInterface(lambda x: x, fill="f16")
    with pytest.raises(ValueError, match=re.escape(NEEDS_STEM.format(""))):
        _front({}, fill="f16")
    with pytest.raises(ValueError, match=re.escape(NEEDS_STEM.format("mmp_"))):
        BatchEvaluator(None, None, None, None, None, None, predictor="mmp", network=lambda x: x, ref_image=np.zeros((37, 41)),
                       transform=snap.WorldTransform(), mmp_fill="f16")
    with pytest.raises(ValueError, match=re.escape("mmp_fill needs predictor = 'mmp'")):
        BatchEvaluator(None, None, None, None, None, None, predictor="cvmp", mmp_fill="f16")
    for kw in (dict(mmp_precision="f16", mmp_fill="f16"), dict(mmp_fill="f32"), dict(mmp_fill=None)):     # accepted: the NEXT refusal speaks
        with pytest.raises(ValueError, match="needs n_hyp = 1 and fused = True"):
            ev(fused=False, **kw)


# ---- 2. the symbols, without a device ----------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_null_arguments_and_bad_flags_without_a_device():
    lib = nm.load_library()
    a = _capi.NmpcMmpStemArgs()
    for name in ("nmpc_mmp_stem_io_f32", "nmpc_mmp_stem_io_f64"):
        assert name in nm.EXPORTED_SYMBOLS and hasattr(lib, name)
        fn = getattr(lib, name)
        assert fn(None, ctypes.byref(a), 0) == -1 and fn(None, None, 1) == -1 and "null argument" in lib.nmpc_last_error().decode()
        for flag in (-1, 2, 7):
            assert fn(None, ctypes.byref(a), flag) == -1
    assert hasattr(nm.Handle, "mmp_stem_io")
    header = open(os.path.join(ROOT, "include", "nmpc_hip.h")).read()
    assert "int nmpc_mmp_stem_io_f32(nmpc_handle h, const nmpc_mmp_stem_args *a, int32_t out_f16);" in header
    assert "int nmpc_mmp_stem_io_f64(nmpc_handle h, const nmpc_mmp_stem_args *a, int32_t out_f16);" in header
    assert "#define NMPC_ABI_VERSION 5" in header and nm.default_config_struct().abi_version == 5


# ---- 3. the placement rule, in bytes -------------------------------------------------------------------------------------------------------------------
def _slots(Hp, Wp):
    """Bytes of a row of the two float-sized buffers of layer1 .. layer4 behind an ``Hp x Wp`` plane (one strided block per later stage)."""
    out, plane = [], (Hp, Wp)
    for k, C in enumerate((16, 32, 64, 128)):
        if k:
            plane = ms.block2_plane(*plane, 2)
        out.append(2 * C * plane[0] * plane[1] * 4)
    return out


def test_placement_in_bytes():
    place = MmpFrontEnd.place_stages
    # the warehouse plane: 64 x 74 x 83; the three stages behind layer1 take 4 * 178 688 B
    slots = _slots(74, 83)
    assert slots[1:] == [4 * 99456, 4 * 51072, 4 * 28160] and sum(slots[1:]) == 4 * 178688
    fill32, fill16 = 64 * 74 * 83 * 4, 64 * 74 * 83 * 2
    assert fill16 == 2 * 393088 and sum(slots[1:]) <= fill16
    assert place(fill32, slots) == place(fill16, slots) == (None, 0, slots[1], slots[1] + slots[2])
    # the 37 x 41 map: 64 x 10 x 11; as float32 all three fit, as binary16 layer2 and layer3 still do and layer4 does not
    slots = _slots(10, 11)
    fill32, fill16 = 64 * 10 * 11 * 4, 64 * 10 * 11 * 2
    assert place(fill32, slots) == (None, 0, slots[1], slots[1] + slots[2])
    assert slots[1] + slots[2] <= fill16 < sum(slots[1:]) and place(fill16, slots) == (None, 0, slots[1], None)
    # a plane where layer2 no longer fits: a 16-channel first layer in binary16
    assert slots[1] > 16 * 10 * 11 * 2 and place(16 * 10 * 11 * 2, slots) == (None, None, None, None)
    # once a stage is outside, a smaller one behind it stays outside too; layer1 is never inside; nothing given, nothing placed
    assert place(100, [8, 200, 50]) == (None, None, None) and place(100, [8, 50, 60, 10]) == (None, 0, None, None)
    assert place(100, [1000]) == (None,) and place(100, []) == ()
    assert place(100, [8, 60, 40]) == (None, 0, 60)


def test_the_front_end_places_and_counts_in_bytes(specs):
    parent, fe = _front(specs, precision="f16"), _front(specs, precision="f16", fill="f16")
    assert fe.fill_f16 and not parent.fill_f16 and fe.fill_row == parent.fill_row == (64, 10, 11) and fe.row == parent.row
    assert [io for st in fe.stages for io in st.io] == [(1, 1)] * 15 + [(1, 0)]
    assert [io for st in parent.stages for io in st.io] == [(0, 1)] + [(1, 1)] * 14 + [(1, 0)]
    slots = [2 * int(np.prod(st.buf_row)) * 4 for st in fe.stages]
    assert [(st.in_fill, st.offset) for st in parent.stages] == [(False, None), (True, 0), (True, slots[1] // 4), (True, (slots[1] + slots[2]) // 4)]
    assert [(st.in_fill, st.offset) for st in fe.stages] == [(False, None), (True, 0), (True, slots[1] // 4), (False, None)]
    n_off, fill = 2, 64 * 10 * 11
    assert parent.bytes_per_item == n_off * (fill * 4 + slots[0] + fe.row[0] * 4)
    assert fe.bytes_per_item == n_off * (fill * 2 + slots[0] + slots[3] + fe.row[0] * 4)
    # on the warehouse plane all three stay inside, and bytes_per_item drops by exactly the half fill
    head = specs["head"]._replace(w1=np.zeros((128, ms.head_features(128, 10, 11)), dtype=np.float32))
    big = dict(specs, head=head)
    parent, fe = _front(big, 293, 330, precision="f16"), _front(big, 293, 330, precision="f16", fill="f16")
    assert fe.fill_row == (64, 74, 83) and [st.in_fill for st in fe.stages] == [st.in_fill for st in parent.stages] == [False, True, True, True]
    assert [st.offset for st in fe.stages] == [st.offset for st in parent.stages]
    assert parent.bytes_per_item - fe.bytes_per_item == n_off * 64 * 74 * 83 * 2


@pytest.mark.parametrize("fill", [None, "f32"])
def test_none_and_f32_give_the_parents_records(specs, fill):
    for kw in ({}, dict(precision="f16"), dict(operands={"layer2": "f16", "layer3": "f16", "layer4": "f16"}, activations="f16")):
        base, fe = _front(specs, **kw), _front(specs, fill=fill, **kw)
        assert not fe.fill_f16 and fe._fill == base._fill == "mmp_stem"
        assert (fe.operands, fe.activations, fe.half, fe.row, fe.fill_row, fe.bytes_per_item) == \
            (base.operands, base.activations, base.half, base.row, base.fill_row, base.bytes_per_item)
        for a, b in zip(fe.stages, base.stages):
            assert (a.name, a.Args, a.launch, a.planes, a.buf_row, a.reads_fill, a.in_fill, a.offset, a.io) == \
                (b.name, b.Args, b.launch, b.planes, b.buf_row, b.reads_fill, b.in_fill, b.offset, b.io)


# ---- 4. the shipped kernels ------------------------------------------------------------------------------------------------------------------------------
def test_kernels_use_no_scratch_and_keep_the_stems_occupancy():
    """From the shipped code object: ``mmp_stem_kernel<float>`` and ``<double>`` are still there under their names, and beside them
    exactly the two kernels with binary16 out, ``mmp_stem_kernel<MmpStemH<float>>`` and ``<MmpStemH<double>>``: no scratch, no spills, the
    siblings' static LDS (53 240 B: three workgroups per CU) and registers that allow the same three waves per SIMD."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    nm.build_library()
    res = {kernel_resources.short_name(k): v for k, v in kernel_resources.kernel_resources(nm.library_path()).items()}
    mine = {k: v for k, v in res.items() if "mmp_stem_kernel" in k}
    names = sorted(re.sub(r"\s+", "", k.split("mmp_stem_kernel", 1)[1]) for k in mine)
    assert names == sorted(["<float>", "<double>", "<nmpc::MmpStemH<float>>", "<nmpc::MmpStemH<double>>"]), sorted(mine)
    for name, r in mine.items():
        print(name, r)
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
        assert r["lds_static"] == 53240 and (160 * 1024) // r["lds_static"] == 3, (name, r)
        regs = r["vgpr"] + max(r["agpr"], 0)
        assert 512 // (-(-regs // 8) * 8) >= 3, (name, r)
