"""CPU tests of the layer1 block with binary16 MFMA operands (``nmpc_mmp_block_f16`` / ``nmpc_mmp_block_f16_io``,
csrc/nmpc_mmp_block1_f16.h) and of the switch that reaches it, ``precision=`` / ``mmp_precision=``: the packing of the weights
(``mmp_stem.pack_block1_f16``), the struct and the ABI version against the C compiler, the entry points, the resources of the eight
shipped kernels, ``check_precision`` in the three host classes, the stage records a front end builds under the switch, and the
controls of the float64 model's bound (tests/mmp_block1_f16_reference.py) before any device run. The sibling of
tests/test_mmp_block2_f16_cpu.py. The device side: tests/test_gpu_mmp_block1_f16.py, tests/test_gpu_mmp_block1_f16_io.py,
tests/test_gpu_mmp_front_precision.py and tests/test_gpu_mmp_net_f16_layer1.py.

Recorded over ``CASES + REAL`` (14 cases): ``emulate`` -- torch's float32 convolutions on the rounded operands, m rounded -- lies at
most 0.311 of the bound (19 x 37, Cin 8); the wrong variants miss it by at least 103."""
import ctypes
import functools
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import dyobav_mpcnwta_warehouse_amd as nm
import mmp_block1_f16_reference as h1
import mmp_block_reference as br
import mmp_net_reference as nr
from dyobav_mpcnwta_warehouse_amd import _capi, snap
from dyobav_mpcnwta_warehouse_amd import mmp_stem as ms
from dyobav_mpcnwta_warehouse_amd.mmp_front import MmpFrontEnd
from dyobav_mpcnwta_warehouse_amd.mmp_interface import MmpInterface
from dyobav_mpcnwta_warehouse_amd.mmp_stem import Block1F16Spec, BlockSpec, pack_block1_f16, round_f16, unpack_block1_f16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = h1.CASES + h1.REAL
_rows = lambda c: 2 if c in h1.REAL else br.M_MAX
LAYERS = ("layer1", "layer2", "layer3", "layer4")
ALL3 = {"layer2": "f16", "layer3": "f16", "layer4": "f16"}
ALL4 = {name: "f16" for name in LAYERS}
NONE_OF = "{0}precision: {1!r} is none of None, 'f32' and 'f16'"
NEEDS_BLOCKS = "{0}precision: 'f16' needs {0}blocks"
BESIDE_OPERANDS = "{0}precision: 'f16', but {0}operands says {1!r} is 'f32'"
BESIDE_ACTIVATIONS = "{0}precision: 'f16', but {0}activations is 'f32'"
NO_KERNEL = "{0}operands: {1!r}: only layer2, layer3 and layer4 have an f16 kernel"
HALF_SENTENCE = "{0}half: {1!r}: only layer3 has an f16 kernel, and layer4 where {0}blocks4 is given"


# ---- 1. the packing ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cin,projection", [(8, True), (16, False), (16, True), (64, True), (72, True)])
def test_pack_is_the_fragment_order_and_unpack_inverts_it(Cin, projection):
    spec = br.random_block(Cin, 7 + Cin, projection)
    p = pack_block1_f16(spec)
    KB = (Cin + 31) // 32
    assert isinstance(p, Block1F16Spec) and p._fields == BlockSpec._fields and type(ms.pack_block_f16(spec)) is Block1F16Spec
    assert p.w1.shape == (9, KB, 1, 64, 8) and p.w2.shape == (9, 1, 1, 64, 8) and all(a.dtype == np.uint16 and a.flags.c_contiguous for a in (p.w1, p.w2))
    assert (p.wd is None) == (not projection) and (p.wd is None or (p.wd.shape == (KB, 1, 64, 8) and p.wd.dtype == np.uint16))
    for a in (p.w1, p.w2, p.wd):                                     # what the entry point asks of the device copies holds for the host arrays
        assert a is None or a.ctypes.data % 16 == 0
    for name in ("s1", "b1", "s2", "b2", "sd", "bd", "slope_mid", "slope_out"):                     # passed through, float32
        a, b = getattr(p, name), getattr(spec, name)
        assert (a is None and b is None) or (np.array_equal(a, b) and np.asarray(a).dtype == np.asarray(b).dtype), name
    # the documented order, element by element, against np.float16 of the weights; zeros behind Cin, and behind 16 in w2
    hw1, hw2 = spec.w1.astype(np.float16), spec.w2.astype(np.float16)
    rng = np.random.default_rng(Cin)
    for t, kb, l, j in zip(rng.integers(0, 9, 300), rng.integers(0, KB, 300), rng.integers(0, 64, 300), rng.integers(0, 8, 300)):
        co, ci = l & 15, 32 * kb + 8 * (l >> 4) + j
        assert p.w1[t, kb, 0, l, j] == (hw1[co, ci, t // 3, t % 3].view(np.uint16) if ci < Cin else 0), (t, kb, l, j)
        if kb < 1:
            assert p.w2[t, 0, 0, l, j] == (hw2[co, ci, t // 3, t % 3].view(np.uint16) if ci < 16 else 0)
        if projection:
            assert p.wd[kb, 0, l, j] == (spec.wd.astype(np.float16)[co, ci].view(np.uint16) if ci < Cin else 0)
    assert not p.w2.reshape(9, 4, 16, 8)[:, 2:].any() and p.w2.reshape(9, 4, 16, 8)[:, :2].any()   # m is half a K block: lane groups 2, 3 hold zeros
    if Cin % 32:
        pad = p.w1.reshape(9, KB, 4, 16, 8)[:, -1, (Cin % 32) // 8:]
        assert pad.size and not pad.any()
        if projection:
            pad = p.wd.reshape(KB, 4, 16, 8)[-1, (Cin % 32) // 8:]
            assert pad.size and not pad.any()
    u = unpack_block1_f16(p, Cin)
    assert isinstance(u, BlockSpec) and u.w1.dtype == np.float16 and np.array_equal(u.w1, hw1) and np.array_equal(u.w2, hw2)
    assert (u.wd is None) == (not projection) and (u.wd is None or np.array_equal(u.wd, spec.wd.astype(np.float16)))
    again = pack_block1_f16(u)                                       # a round trip: rounded weights round to themselves
    assert np.array_equal(again.w1, p.w1) and np.array_equal(again.w2, p.w2) and (p.wd is None or np.array_equal(again.wd, p.wd))


def test_pack_saturates_and_refuses_what_check_block_refuses():
    import mmp_block2_reference as b2
    ok = br.random_block(16, 1, False)
    big = ok.w1.copy()
    big[0, 0, 0, 0], big[1, 0, 0, 0] = 1e6, -7e4
    u = unpack_block1_f16(pack_block1_f16(ok._replace(w1=big)), 16)
    assert u.w1[0, 0, 0, 0] == 65504.0 and u.w1[1, 0, 0, 0] == -65504.0 and np.isfinite(u.w1).all()
    for bad in (ok._replace(s1=np.zeros(4)), ok._replace(w1=np.zeros((16, 12, 3, 3))), ok._replace(wd=np.zeros((16, 16))),
                ok._replace(slope_mid=float("nan")), ok._replace(slope_out=2.0), br.random_block(64, 1, True)._replace(sd=None),
                b2.random_block2(32, 1, 1, False)):
        with pytest.raises(ValueError, match="BlockSpec"):
            pack_block1_f16(bad)


# ---- 2. the struct, the version and the symbols: no device needed ---------------------------------------------------------------------------------
def test_entry_points_refuse_null_arguments_and_bad_flags_without_a_device():
    lib = nm.load_library()
    for name in ("nmpc_mmp_block_f16", "nmpc_mmp_block_f16_io"):
        assert name in nm.EXPORTED_SYMBOLS and hasattr(lib, name) and hasattr(nm.Handle, name[5:])
    a = _capi.NmpcMmpBlockF16Args()
    assert lib.nmpc_mmp_block_f16(None, ctypes.byref(a)) == -1 and lib.nmpc_mmp_block_f16(None, None) == -1
    assert lib.nmpc_mmp_block_f16_io(None, ctypes.byref(a), 0, 0) == -1 and lib.nmpc_mmp_block_f16_io(None, None, 1, 1) == -1
    header = open(os.path.join(ROOT, "include", "nmpc_hip.h")).read()
    assert "int nmpc_mmp_block_f16(nmpc_handle h, const nmpc_mmp_block_f16_args *a);" in header
    assert "int nmpc_mmp_block_f16_io(nmpc_handle h, const nmpc_mmp_block_f16_args *a, int32_t x_f16, int32_t out_f16);" in header
    assert "#define NMPC_ABI_VERSION 5" in header and "covers C = 16" in header


def test_args_layout_matches_the_c_compiler():
    fields = [f[0] for f in _capi.NmpcMmpBlockF16Args._fields_]
    assert fields == ["M", "Cin", "H", "W", "x", "w1", "s1", "b1", "w2", "s2", "b2", "wd", "sd", "bd", "slope_mid", "slope_out", "out"]
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "sz.c")
        body = "".join(f'printf(" %zu %zu", offsetof(nmpc_mmp_block_f16_args, {f}), offsetof(nmpc_mmp_block_args, {f}));' for f in fields)
        open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "nmpc_hip.h"\nint main(void){printf("%zu %zu", sizeof(nmpc_mmp_block_f16_args), '
                             'sizeof(nmpc_mmp_block_args));' + body + 'printf(" %zu %d", sizeof(nmpc_mmp_block2_f16_args), NMPC_ABI_VERSION);return 0;}\n')
        exe = os.path.join(td, "sz")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert ctypes.sizeof(_capi.NmpcMmpBlockF16Args) == out[0] == out[1] == ctypes.sizeof(_capi.NmpcMmpBlockArgs) == 112
    mine = [getattr(_capi.NmpcMmpBlockF16Args, f).offset for f in fields]
    assert mine == out[2:-2:2] == out[3:-2:2] == [getattr(_capi.NmpcMmpBlockArgs, f).offset for f in fields]
    assert out[-2] == 120 and out[-1] == 5                                                          # nothing that existed changed; no version change
    cfg = nm.default_config_struct()                                                                # ... and the library agrees
    assert cfg.abi_version == 5


def test_kernels_use_no_scratch_and_fit_the_occupancy_the_header_states():
    """From the shipped code object: exactly eight kernels of layer1's geometry -- <projection> on the geometry with chunks of 32 and
    <identity> on the one with chunks of 16, each in the four forms of x and out in memory --, no scratch and no spills. The LDS is
    the header's count of planes (4 with a projection, 2 without) times 9 984 B, and LDS and registers both allow the four
    workgroups per CU that the header's __launch_bounds__ claims."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    nm.build_library()
    res = {kernel_resources.short_name(k): v for k, v in kernel_resources.kernel_resources(nm.library_path()).items()}
    mine = {k: v for k, v in res.items() if "MmpBlock1HGeom" in k}
    plain = r"mmp_blkh_kernel<nmpc::MmpBlock1HGeom<(true|false)>, 1, (true|false)>"
    io = r"mmp_blkh_kernel<nmpc::MmpBlkhIo<nmpc::MmpBlock1HGeom<(true|false)>, (true|false), (true|false)>, 1, (true|false)>"
    found = sorted((m.group(1), m.group(2) if len(m.groups()) == 4 else "false", m.group(3) if len(m.groups()) == 4 else "false", m.groups()[-1])
                   for k in mine for m in [re.search(io, k) or re.search(plain, k)])
    forms = [("false", "false"), ("false", "true"), ("true", "false"), ("true", "true")]
    assert len(mine) == 8 and found == sorted((p, x, o, p) for p in ("true", "false") for x, o in forms), sorted(mine)
    header = open(os.path.join(ROOT, "dyobav-mpcnwta-warehouse_amd", "csrc", "nmpc_mmp_block1_f16.h")).read()
    assert "Threads = kBlkThreads" in header and "min_wg(int) { return 4; }" in header and "ck(int) { return PROJ ? 32 : 16; }" in header
    assert "PL = kBlkP" in header and "39 936 B (projection) or 19 968 B (identity)" in header
    shared = open(os.path.join(ROOT, "dyobav-mpcnwta-warehouse_amd", "csrc", "nmpc_mmp_block_f16.h")).read()
    assert "__launch_bounds__(G::Threads, G::min_wg(STRIDE))" in shared
    for name, r in mine.items():
        print(name, r)
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
        assert r["lds_static"] == (4 if "Geom<true>" in name else 2) * 624 * 16, (name, r)
        assert (160 * 1024) // r["lds_static"] >= 4, (name, r)
        regs = r["vgpr"] + max(r["agpr"], 0)
        assert 512 // (-(-regs // 8) * 8) >= 4, (name, r)                     # the registers hold as many waves per SIMD


# ---- 3. precision= in the three host classes -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def specs():
    return dict(zip(("stem", "blocks", "blocks2", "blocks3", "blocks4", "head"), ms.split_network_whole(nr.in_double(nr.made_net(nr.SHAPES[0])))))


def test_check_precision_accepts_and_refuses_with_one_sentence_each(specs):
    six = MmpFrontEnd.check_specs(**specs)
    three = MmpFrontEnd.check_specs(specs["stem"], specs["blocks"], blocks2=specs["blocks2"], head=None)
    f32 = {name: "f32" for name in LAYERS}
    cp = MmpFrontEnd.check_precision
    for precision in (None, "f32"):                                   # the parts' own answers, unchanged
        assert cp(precision, None, (), None, six) == (f32, "f32")
        assert cp(precision, ALL3, (), "f16", six) == (dict(f32, **ALL3), "f16")
        assert cp(precision, {"layer2": "f16"}, ("layer4",), None, six) == (dict(f32, layer2="f16", layer4="f16"), "f32")
    assert cp("f16", None, (), None, six) == (ALL4, "f16")
    assert cp("f16", None, (), None, three, prefix="mmp_") == ({"layer1": "f16", "layer2": "f16"}, "f16")
    # accepted beside values that agree; "f32" for a stage that is not given names nothing
    assert cp("f16", ALL3, ("layer3", "layer4"), "f16", six) == cp("f16", {}, "layer3", None, six) == (ALL4, "f16")
    assert cp("f16", {"layer4": "f32", "layer2": "f16"}, (), "f16", three) == ({"layer1": "f16", "layer2": "f16"}, "f16")
    for prefix in ("", "mmp_"):
        for value in ("f64", "bf16", "F16", "half", 16, True, ("f16",)):
            with pytest.raises(ValueError, match=re.escape(NONE_OF.format(prefix, value))):
                cp(value, None, (), None, six, prefix=prefix)
        for none in (MmpFrontEnd.check_specs(None, None, head=None), MmpFrontEnd.check_specs(specs["stem"], None, head=None)):
            with pytest.raises(ValueError, match=re.escape(NEEDS_BLOCKS.format(prefix))):
                cp("f16", None, (), None, none, prefix=prefix)
        for name in LAYERS:
            with pytest.raises(ValueError, match=re.escape(BESIDE_OPERANDS.format(prefix, name))):
                cp("f16", {name: "f32"}, (), None, six, prefix=prefix)
        with pytest.raises(ValueError, match=re.escape(BESIDE_ACTIVATIONS.format(prefix))):
            cp("f16", None, (), "f32", six, prefix=prefix)
        # the refusals of operands, half and activations speak first and unchanged
        with pytest.raises(ValueError, match=re.escape(NO_KERNEL.format(prefix, "layer1"))):
            cp("f16", {"layer1": "f16"}, (), None, six, prefix=prefix)
        with pytest.raises(ValueError, match=re.escape(HALF_SENTENCE.format(prefix, "layer1"))):
            cp("f16", None, ("layer1",), None, six, prefix=prefix)
        with pytest.raises(ValueError, match=re.escape(f"{prefix}activations: 'f64' is none of None, 'f32' and 'f16'")):
            cp("f16", None, (), "f64", six, prefix=prefix)
        with pytest.raises(ValueError, match=re.escape(f"{prefix}activations: 'f16' needs a stage on f16 operands ({prefix}operands)")):
            cp("f32", None, (), "f16", six, prefix=prefix)


def test_the_three_classes_take_and_refuse_the_same_before_any_device_is_touched(specs):
    from dyobav_mpcnwta_warehouse_amd.evaluate import BatchEvaluator
    it = MmpInterface(None, precision="f16", **specs)
    assert it._operands == ALL4 and it._activations == "f16" and it._half == ()
    for precision in (None, "f32"):
        it = MmpInterface(None, precision=precision, operands=ALL3, **specs)
        assert it._operands == dict(ALL3, layer1="f32") and it._activations == "f32"
    assert MmpInterface(None, precision="f16", operands=ALL3, half=("layer4",), activations="f16", **specs)._operands == ALL4
    ok = dict(predictor="mmp", network=None, ref_image=np.zeros((37, 41)), transform=snap.WorldTransform(), **{"mmp_" + k: v for k, v in specs.items()})
    ev = lambda **kw: BatchEvaluator(None, None, None, None, None, None, **dict(ok, **kw))
    classes = ((lambda **kw: MmpInterface(None, **dict(specs, **kw)), ""), (lambda **kw: ev(**{"mmp_" + k: v for k, v in kw.items()}), "mmp_"))
    for make, prefix in classes:
        with pytest.raises(ValueError, match=re.escape(NONE_OF.format(prefix, "f64"))):
            make(precision="f64")
        with pytest.raises(ValueError, match=re.escape(BESIDE_OPERANDS.format(prefix, "layer3"))):
            make(precision="f16", operands={"layer2": "f16", "layer3": "f32"})
        with pytest.raises(ValueError, match=re.escape(BESIDE_ACTIVATIONS.format(prefix))):
            make(precision="f16", activations="f32")
        with pytest.raises(ValueError, match=re.escape(NO_KERNEL.format(prefix, "layer1"))):          # operands keeps refusing layer1, and speaks first
            make(precision="f16", operands={"layer1": "f16"})
        with pytest.raises(ValueError, match=re.escape(HALF_SENTENCE.format(prefix, "layer1"))):
            make(precision="f64", half=("layer1",))
    with pytest.raises(ValueError, match=re.escape(NEEDS_BLOCKS.format(""))):
        MmpInterface(lambda x: x, stem=specs["stem"], precision="f16")
    with pytest.raises(ValueError, match=re.escape(NEEDS_BLOCKS.format("mmp_"))):
        BatchEvaluator(None, None, None, None, None, None, predictor="mmp", network=lambda x: x, ref_image=np.zeros((37, 41)),
                       transform=snap.WorldTransform(), mmp_stem=specs["stem"], mmp_precision="f16")
    with pytest.raises(ValueError, match=re.escape("mmp_precision needs predictor = 'mmp'")):
        BatchEvaluator(None, None, None, None, None, None, predictor="cvmp", mmp_precision="f16")
    for precision in ("f16", "f32", None):                                         # accepted: the NEXT refusal is the one that speaks
        with pytest.raises(ValueError, match="needs n_hyp = 1 and fused = True"):
            ev(mmp_precision=precision, fused=False)
    # the front end itself
    for kw, sentence in ((dict(precision="f64"), NONE_OF.format("", "f64")), (dict(precision="f16", activations="f32"), BESIDE_ACTIVATIONS.format("")),
                         (dict(precision="f16", operands={"layer1": "f32"}), BESIDE_OPERANDS.format("", "layer1"))):
        with pytest.raises(ValueError, match=re.escape(sentence)):
            _front(specs, **kw)


class _NoDevice:
    """Stands where the handle does in a front end that launches nothing: every launch method is its own name."""

    def __getattr__(self, name):
        return name


def _front(specs, **kw):
    return MmpFrontEnd(_NoDevice(), np.float32, "cpu", 37, 41, 2, snap.WorldTransform(), 1.0, 1.0, torch.zeros(37, 41), **specs, **kw)


def _same_stage(a, b):
    assert (a.name, a.channels, a.cins, a.Args, a.launch, a.planes, a.buf_row, a.reads_fill, a.in_fill, a.offset, a.io) == \
        (b.name, b.channels, b.cins, b.Args, b.launch, b.planes, b.buf_row, b.reads_fill, b.in_fill, b.offset, b.io)
    assert len(a.specs) == len(b.specs)
    for sa, sb in zip(a.specs, b.specs):
        assert type(sa) is type(sb)
        for va, vb in zip(sa, sb):
            assert (va is None and vb is None) or (torch.is_tensor(va) and va.dtype == vb.dtype and torch.equal(va, vb)) or va == vb


@pytest.mark.parametrize("precision", [None, "f32"])
def test_none_and_f32_give_the_parents_stage_records(specs, precision):
    for kw in ({}, dict(operands=ALL3), dict(operands=ALL3, activations="f16"), dict(half=("layer3",))):
        base, fe = _front(specs, **kw), _front(specs, precision=precision, **kw)
        assert (fe.operands, fe.activations, fe.half, fe.row, fe.fill_row, fe.bytes_per_item) == \
            (base.operands, base.activations, base.half, base.row, base.fill_row, base.bytes_per_item)
        for name in LAYERS:
            _same_stage(fe.stage(name), base.stage(name))
        assert fe.stage("layer1").Args is _capi.NmpcMmpBlockArgs and fe.stage("layer1").launch == "mmp_block" and fe.stage("layer1").io is None


def test_f16_makes_every_tensor_between_two_blocks_binary16(specs):
    fe, plain, parent = _front(specs, precision="f16"), _front(specs), _front(specs, operands=ALL3, activations="f16")
    assert fe.operands == ALL4 and fe.activations == "f16" and fe.half == ()
    assert [len(st.specs) for st in fe.stages] == [3, 4, 6, 3]
    assert [io for st in fe.stages for io in st.io] == [(0, 1)] + [(1, 1)] * 14 + [(1, 0)]
    assert [st.launch for st in fe.stages] == ["mmp_block_f16_io", "mmp_block2_f16_io", "mmp_block3_f16_io", "mmp_block4_f16_io"]
    assert [st.out_f16 for st in fe.stages] == [True, True, True, False]
    st = fe.stage("layer1")
    assert st.Args is _capi.NmpcMmpBlockF16Args and fe.blocks is st.specs and st.cins == (64, 16, 16)
    assert all(isinstance(b, Block1F16Spec) and b.w1.dtype == torch.int16 and b.w2.shape == (9, 1, 1, 64, 8) for b in st.specs)
    assert st.specs[0].w1.shape == (9, 2, 1, 64, 8) and st.specs[0].wd.shape == (2, 1, 64, 8) and st.specs[1].wd is None
    # buffers, placement and bytes_per_item stay as they are
    for a, b in zip(fe.stages, plain.stages):
        assert (a.cins, a.planes, a.buf_row, a.reads_fill, a.in_fill, a.offset) == (b.cins, b.planes, b.buf_row, b.reads_fill, b.in_fill, b.offset)
    assert fe.bytes_per_item == plain.bytes_per_item and fe.row == plain.row and fe.fill_row == plain.fill_row
    # behind the border to layer2 only that border's flag differs from today's fastest path
    assert parent.stage("layer2").io[0] == (0, 1) and fe.stage("layer2").io[0] == (1, 1)
    assert fe.stage("layer2").io[1:] == parent.stage("layer2").io[1:] and fe.stage("layer3").io == parent.stage("layer3").io
    # without a head and without layer3, layer4: the last block given writes float32
    some = {k: v for k, v in specs.items() if k in ("stem", "blocks", "blocks2")}
    fe2 = _front(some, precision="f16")
    assert fe2.operands == {"layer1": "f16", "layer2": "f16"} and [io for st in fe2.stages for io in st.io] == [(0, 1)] + [(1, 1)] * 5 + [(1, 0)]


# ---- 4. the controls of the bound, before any device run -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _figures(c):
    """(|emulate - model| / bound at its worst, {wrong variant: the factor by which it misses the bound}) of a case, computed once."""
    x, spec, want, bound = h1.case("random", *c, _rows(c))
    r = (np.abs(h1.emulate(x, spec) - want) / bound).max()
    factors = {}
    for wrong in ("slope", "halo"):
        bad, _ = h1.block(x, spec, wrong=wrong)
        assert bad.shape == want.shape
        factors[wrong] = (np.abs(bad - want) / bound).max()
    return r, factors


@pytest.mark.parametrize("c", ALL, ids=h1.case_id)
def test_the_bound_admits_the_emulation_and_refuses_the_wrong_variants(c):
    H, W, Cin, projection = c
    x, spec, want, bound = h1.case("random", *c, _rows(c))
    assert want.shape == (x.shape[0], 16, H, W) and (bound > 0).all()
    r, factors = _figures(c)
    print(f"{h1.case_id(c)}: emulate {r:.4f}" + "".join(f", {k} x {v:.0f}" for k, v in factors.items()))
    assert r <= 1.0, "the bound refuses a correct implementation of the rule"
    assert all(v > 1.0 for v in factors.values()), "the bound admits a wrong variant"
    assert not np.array_equal(want, br.case("random", *c, _rows(c))[2])      # the rule costs something


def test_the_recorded_margins_hold_over_all_cases():
    figs = {c: _figures(c) for c in ALL}
    worst = max(figs, key=lambda c: figs[c][0])
    least = min(((v, k, c) for c in ALL for k, v in figs[c][1].items()), key=lambda t: t[0])
    print(f"emulate at most {figs[worst][0]:.4f} of the bound ({h1.case_id(worst)}); wrong variants at least x {least[0]:.1f} ({least[1]}, {h1.case_id(least[2])})")
    assert figs[worst][0] <= 0.32 and least[0] >= 100.0


@pytest.mark.parametrize("c", ALL, ids=h1.case_id)
def test_integer_cases_are_bit_equal_to_the_float32_reference(c):
    """Every operand and every m of the integer cases is a binary16 value: the rule rounds nothing on them, so the model equals the
    float32 reference, and ``emulate`` gives that reference's bits."""
    x, spec, want, _ = br.case("integer", *c, _rows(c))
    is_h = lambda a: np.array_equal(np.asarray(a, dtype=np.float64), round_f16(a).astype(np.float64))
    assert is_h(x) and is_h(spec.w1) and is_h(spec.w2) and (spec.wd is None or is_h(spec.wd)) and br.integer_units(x, spec) < 2 ** 24
    model, _ = h1.block(x, spec)
    assert np.array_equal(model, want) and np.array_equal(h1.block(x, spec, round_m=True)[0], want)
    assert np.array_equal(h1.emulate(x, spec), want.astype(np.float32))


def test_the_exact_block_under_the_rule():
    x = round_f16(np.abs(br.random_x(2, 16, 16, 29, seed=5))).astype(np.float32)
    assert np.array_equal(h1.emulate(x, br.doubling_block()), x + x) and np.array_equal(h1.block(x, br.doubling_block())[0], x + x)
