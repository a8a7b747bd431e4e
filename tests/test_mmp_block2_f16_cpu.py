"""CPU tests of the layer2 block with binary16 MFMA operands (``nmpc_mmp_block2_f16``, csrc/nmpc_mmp_block2_f16.h): the packing of
the weights (``mmp_stem.pack_block2_f16``), the struct against the C compiler, the entry point, the resources of the three shipped
kernels, ``operands=`` / ``check_operands`` in the three host classes, the controls of the float64 model's bound
(tests/mmp_block2_f16_reference.py) before any device run, and the rule's cost through the whole network on the CPU. The sibling of
tests/test_mmp_block3_f16_cpu.py and tests/test_mmp_block4_f16_cpu.py.

Recorded over ``mmp_block2_reference.CASES + REAL`` (22 cases): ``emulate`` -- torch's float32 convolutions on the rounded operands,
m rounded -- lies at most 0.230 of the bound (4 x 6, Cin 8, stride 2); the wrong variants miss it by at least 78 ("slope", 8 x 44,
Cin 64). Every operand and every m of the integer cases is a binary16 value (|m| <= 127), and ``emulate`` gives the float32
reference's bits on them. Network level (``emulate`` chained through layer2, torch's float32 module behind it), |. - float64| over
the yardstick at layer2 / layer3 / layer4 / output: 1.11 / 1.02 / 1.11 / 0.91 on 37 x 41 (M = 4), 1.06 / 1.03 / 1.01 / 0.96 on
293 x 329 (M = 2); the bar is 4."""
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
import mmp_block2_f16_reference as h2
import mmp_block2_reference as b2
import mmp_block3_reference as b3
import mmp_block4_reference as b4
import mmp_block_reference as br
import mmp_net_reference as nr
import mmp_stem_reference as sr
from dyobav_mpcnwta_warehouse_amd import _capi, snap
from dyobav_mpcnwta_warehouse_amd import mmp_stem as ms
from dyobav_mpcnwta_warehouse_amd.mmp_front import MmpFrontEnd
from dyobav_mpcnwta_warehouse_amd.mmp_interface import MmpInterface
from dyobav_mpcnwta_warehouse_amd.mmp_stem import (Block2F16Spec, Block2Spec, check_blocks, check_blocks2, pack_block2_f16, round_f16,
                                                   unpack_block2_f16)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = b2.CASES + b2.REAL
_rows = lambda c: 2 if c in b2.REAL else b2.M_MAX
HALF_SENTENCE = "{0}half: {1!r}: only layer3 has an f16 kernel, and layer4 where {0}blocks4 is given"
NO_KERNEL = "{0}operands: {1!r}: only layer2, layer3 and layer4 have an f16 kernel"
NEITHER = "{0}operands: {1!r}: {2!r} is neither 'f32' nor 'f16'"
NEEDS = "{0}operands: {1!r} needs {0}{2}"
CONTRADICTS = "{0}operands: {1!r} is 'f32', but {0}half names it"


# ---- 1. the packing ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cin,stride,projection", [(8, 2, True), (16, 2, True), (24, 1, True), (32, 1, False), (32, 2, True), (64, 1, True), (72, 1, True)])
def test_pack_is_the_fragment_order_and_unpack_inverts_it(Cin, stride, projection):
    spec = b2.random_block2(Cin, 7 + Cin, stride, projection)
    p = pack_block2_f16(spec)
    KB = (Cin + 31) // 32
    assert isinstance(p, Block2F16Spec) and p._fields == Block2Spec._fields
    assert p.w1.shape == (9, KB, 2, 64, 8) and p.w2.shape == (9, 1, 2, 64, 8) and all(a.dtype == np.uint16 and a.flags.c_contiguous for a in (p.w1, p.w2))
    assert (p.wd is None) == (not projection) and (p.wd is None or (p.wd.shape == (KB, 2, 64, 8) and p.wd.dtype == np.uint16))
    for a in (p.w1, p.w2, p.wd):                                     # what the entry point asks of the device copies holds for the host arrays
        assert a is None or a.ctypes.data % 16 == 0
    for name in ("s1", "b1", "s2", "b2", "sd", "bd", "slope_mid", "slope_out", "stride"):           # passed through, float32
        a, b = getattr(p, name), getattr(spec, name)
        assert (a is None and b is None) or (np.array_equal(a, b) and np.asarray(a).dtype == np.asarray(b).dtype), name
    # the documented order, element by element, against np.float16 of the weights; zeros behind Cin
    h1, hh2 = spec.w1.astype(np.float16), spec.w2.astype(np.float16)
    rng = np.random.default_rng(Cin)
    for t, kb, g, l, j in zip(rng.integers(0, 9, 300), rng.integers(0, KB, 300), rng.integers(0, 2, 300), rng.integers(0, 64, 300), rng.integers(0, 8, 300)):
        co, ci = 16 * g + (l & 15), 32 * kb + 8 * (l >> 4) + j
        want = h1[co, ci, t // 3, t % 3].view(np.uint16) if ci < Cin else 0
        assert p.w1[t, kb, g, l, j] == want, (t, kb, g, l, j)
        if kb < 1:
            assert p.w2[t, kb, g, l, j] == hh2[co, ci, t // 3, t % 3].view(np.uint16)
        if projection:
            assert p.wd[kb, g, l, j] == (spec.wd.astype(np.float16)[co, ci].view(np.uint16) if ci < Cin else 0)
    if Cin % 32:
        pad = p.w1.reshape(9, KB, 2, 4, 16, 8)[:, -1, :, (Cin % 32) // 8:]
        assert pad.size and not pad.any()
        if projection:
            pad = p.wd.reshape(KB, 2, 4, 16, 8)[-1, :, (Cin % 32) // 8:]
            assert pad.size and not pad.any()
    u = unpack_block2_f16(p, Cin)
    assert isinstance(u, Block2Spec) and u.w1.dtype == np.float16 and np.array_equal(u.w1, h1) and np.array_equal(u.w2, hh2)
    assert (u.wd is None) == (not projection) and (u.wd is None or np.array_equal(u.wd, spec.wd.astype(np.float16)))
    again = pack_block2_f16(u)                                       # a round trip: rounded weights round to themselves
    assert np.array_equal(again.w1, p.w1) and np.array_equal(again.w2, p.w2) and (p.wd is None or np.array_equal(again.wd, p.wd))


def test_pack_saturates_and_refuses_what_check_block2_refuses():
    ok = b2.random_block2(32, 1, 1, False)
    big = ok.w1.copy()
    big[0, 0, 0, 0], big[1, 0, 0, 0] = 1e6, -7e4
    u = unpack_block2_f16(pack_block2_f16(ok._replace(w1=big)), 32)
    assert u.w1[0, 0, 0, 0] == 65504.0 and u.w1[1, 0, 0, 0] == -65504.0 and np.isfinite(u.w1).all()
    for bad in (ok._replace(s1=np.zeros(4)), ok._replace(w1=np.zeros((32, 12, 3, 3))), ok._replace(wd=np.zeros((32, 32))),
                ok._replace(slope_mid=float("nan")), ok._replace(slope_out=2.0), ok._replace(stride=2), ok._replace(stride=0),
                b2.random_block2(64, 1, 1, True)._replace(sd=None), b3.random_block3(64, 1, 1, False)):
        with pytest.raises(ValueError, match="Block2Spec"):
            pack_block2_f16(bad)


# ---- 2. the struct and the symbol: no device needed ---------------------------------------------------------------------------------------------
def test_entry_point_refuses_null_arguments():
    lib = nm.load_library()
    assert "nmpc_mmp_block2_f16" in nm.EXPORTED_SYMBOLS and hasattr(lib, "nmpc_mmp_block2_f16")
    a = _capi.NmpcMmpBlock2F16Args()
    assert lib.nmpc_mmp_block2_f16(None, ctypes.byref(a)) == -1 and lib.nmpc_mmp_block2_f16(None, None) == -1


def test_args_layout_matches_the_c_compiler():
    fields = [f[0] for f in _capi.NmpcMmpBlock2F16Args._fields_]
    assert fields == ["M", "Cin", "H", "W", "x", "w1", "s1", "b1", "w2", "s2", "b2", "wd", "sd", "bd", "slope_mid", "slope_out", "out", "stride"]
    old = ("nmpc_mmp_block2_args", "nmpc_mmp_block3_f16_args", "nmpc_mmp_block4_f16_args")
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "sz.c")
        body = "".join(f'printf(" %zu", offsetof(nmpc_mmp_block2_f16_args, {f}));' for f in fields)
        body += "".join(f'printf(" %zu", sizeof({s}));' + "".join(f'printf(" %zu", offsetof({s}, {f}));' for f in fields) for s in old)
        open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "nmpc_hip.h"\nint main(void){printf("%zu", sizeof(nmpc_mmp_block2_f16_args));'
                             + body + 'printf(" %d", NMPC_ABI_VERSION);return 0;}\n')
        exe = os.path.join(td, "sz")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    n = len(fields)
    assert ctypes.sizeof(_capi.NmpcMmpBlock2F16Args) == out[0] == 120
    mine = [getattr(_capi.NmpcMmpBlock2F16Args, f).offset for f in fields]
    assert mine == out[1:1 + n]
    for k, mirror in enumerate((_capi.NmpcMmpBlock2Args, _capi.NmpcMmpBlock3F16Args, _capi.NmpcMmpBlock4F16Args)):   # nothing that existed changed
        part = out[1 + n + k * (n + 1):1 + n + (k + 1) * (n + 1)]
        assert part[0] == ctypes.sizeof(mirror) == 120 and part[1:] == [getattr(mirror, f).offset for f in fields] == mine
    assert out[-1] == 5                                                                             # no version change


def test_kernels_use_no_scratch_and_fit_the_occupancy_the_header_states():
    """From the shipped code object: exactly three kernels, no scratch and no spills. The numbers are the compiler's: the LDS it
    reports is the header's count of planes (4 at stride 1, 8 at stride 2) times 9 472 B, the workgroups per CU that LDS allows are
    the ones the header's __launch_bounds__ claims (4 and 2), and the registers allow as many waves per SIMD. Recorded: <2, true>
    126 VGPRs, <1, true> 126, <1, false> 122; 75 776 B and 37 888 B."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    nm.build_library()
    res = {kernel_resources.short_name(k): v for k, v in kernel_resources.kernel_resources(nm.library_path()).items()}
    mine = {k: v for k, v in res.items() if re.search(r"mmp_blkh_kernel<nmpc::MmpBlock2HGeom, ", k)}
    assert len(mine) == 3, sorted(mine)
    assert not any(re.search(r"mmp_blkf_kernel<nmpc::MmpBlock2Geom, ", k) for k in mine)                 # the f32 family's pattern does not take these in
    header = open(os.path.join(ROOT, "dyobav-mpcnwta-warehouse_amd", "csrc", "nmpc_mmp_block2_f16.h")).read()
    assert "Threads = kB2Threads" in header and "min_wg(int stride) { return stride == 2 ? 2 : 4; }" in header   # the geometry's figures ...
    shared = open(os.path.join(ROOT, "dyobav-mpcnwta-warehouse_amd", "csrc", "nmpc_mmp_block_f16.h")).read()
    assert "__launch_bounds__(G::Threads, G::min_wg(STRIDE))" in shared   # ... are the one kernel's launch bound
    for name, r in mine.items():
        print(name, r)
        claimed = 2 if "Geom, 2," in name else 4                                         # workgroups per CU = waves per SIMD (four waves, four SIMDs)
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
        assert r["lds_static"] == (8 if "Geom, 2," in name else 4) * 592 * 16, (name, r)
        assert (160 * 1024) // r["lds_static"] == claimed, (name, r)
        regs = r["vgpr"] + max(r["agpr"], 0)
        assert 512 // (-(-regs // 8) * 8) >= claimed, (name, r)                     # the registers hold as many waves per SIMD


# ---- 3. operands= in the three host classes -----------------------------------------------------------------------------------------------------
def _given():
    stem = sr.delta_spec(16)
    blocks = check_blocks(stem, [br.doubling_block()])
    blocks2 = check_blocks2(blocks, [b2.duplicate_and_double_block2(16), b2.doubling_block2()])
    blocks3 = [b3.duplicate_and_double_block3(32), b3.doubling_block3()]
    blocks4 = [b4.duplicate_and_double_block4(64), b4.doubling_block4()]
    return stem, blocks, blocks2, blocks3, blocks4


def test_check_operands_accepts_and_returns_every_given_stage():
    stem, blocks, blocks2, blocks3, blocks4 = _given()
    six = MmpFrontEnd.check_specs(stem, blocks, blocks2=blocks2, blocks3=blocks3, blocks4=blocks4, head=None)
    f32 = {"layer1": "f32", "layer2": "f32", "layer3": "f32", "layer4": "f32"}
    co = MmpFrontEnd.check_operands
    for none in (None, {}, dict(f32), {"layer1": "f32"}, {"layer4": "f32", "layer2": "f32"}):
        assert co(none, (), six) == f32
    assert co({"layer2": "f16"}, (), six) == dict(f32, layer2="f16")
    assert co({"layer3": "f16"}, (), six) == co(None, ("layer3",), six) == co({"layer3": "f16"}, ("layer3",), six) == dict(f32, layer3="f16")
    assert co({"layer4": "f16"}, (), six) == co(None, "layer4", six) == dict(f32, layer4="f16")
    assert co({"layer2": "f16", "layer3": "f16", "layer4": "f16"}, (), six) == co({"layer2": "f16"}, ("layer3", "layer4"), six) \
        == co({"layer2": "f16", "layer1": "f32"}, ("layer4", "layer3"), six, prefix="mmp_") == dict(f32, layer2="f16", layer3="f16", layer4="f16")
    # the stages given decide the keys; "f32" for a stage that is not given names nothing
    three = MmpFrontEnd.check_specs(stem, blocks, blocks2=blocks2, head=None)
    assert co(None, (), three) == {"layer1": "f32", "layer2": "f32"} and co({"layer2": "f16", "layer4": "f32"}, (), three) == {"layer1": "f32", "layer2": "f16"}
    assert co(None, (), MmpFrontEnd.check_specs(None, None, head=None)) == {}


def test_check_operands_refuses_with_one_sentence_each():
    stem, blocks, blocks2, blocks3, blocks4 = _given()
    six = MmpFrontEnd.check_specs(stem, blocks, blocks2=blocks2, blocks3=blocks3, blocks4=blocks4, head=None)
    co = MmpFrontEnd.check_operands
    for prefix in ("", "mmp_"):
        for name in ("layer1", "stem", "head", "layer5"):
            with pytest.raises(ValueError, match=re.escape(NO_KERNEL.format(prefix, name))):
                co({name: "f16"}, (), six, prefix=prefix)
        for name in ("stem", "head", "layer5"):                                      # an unknown stage, whatever it asks for
            with pytest.raises(ValueError, match=re.escape(NO_KERNEL.format(prefix, name))):
                co({name: "f32"}, (), six, prefix=prefix)
        for value in ("bf16", "F16", "half", None, 16, True):
            with pytest.raises(ValueError, match=re.escape(NEITHER.format(prefix, "layer2", value))):
                co({"layer2": value}, (), six, prefix=prefix)
        for name, arg, specs in (("layer2", "blocks2", MmpFrontEnd.check_specs(stem, blocks, head=None)),
                                 ("layer3", "blocks3", MmpFrontEnd.check_specs(stem, blocks, blocks2=blocks2, head=None)),
                                 ("layer4", "blocks4", MmpFrontEnd.check_specs(stem, blocks, blocks2=blocks2, blocks3=blocks3, head=None))):
            with pytest.raises(ValueError, match=re.escape(NEEDS.format(prefix, name, arg))):
                co({name: "f16"}, (), specs, prefix=prefix)
        for name in ("layer3", "layer4"):
            with pytest.raises(ValueError, match=re.escape(CONTRADICTS.format(prefix, name))):
                co({name: "f32"}, ("layer3", "layer4"), six, prefix=prefix)
        # half's refusals speak first and unchanged, with operands present
        for operands in (None, {"layer2": "f16"}, {"layer2": "bf16"}):
            with pytest.raises(ValueError, match=re.escape(HALF_SENTENCE.format(prefix, "layer2"))):
                co(operands, ("layer2",), six, prefix=prefix)
            with pytest.raises(ValueError, match=re.escape(HALF_SENTENCE.format(prefix, "layer1"))):
                co(operands, ("layer3", "layer1"), six, prefix=prefix)


def test_the_three_classes_take_and_refuse_the_same_before_any_device_is_touched():
    from dyobav_mpcnwta_warehouse_amd.evaluate import BatchEvaluator
    stem, blocks, blocks2, blocks3, blocks4 = _given()
    net = lambda x: x
    given = dict(stem=stem, blocks=blocks, blocks2=blocks2, blocks3=blocks3)
    f32 = {"layer1": "f32", "layer2": "f32", "layer3": "f32", "layer4": "f32"}
    for operands, half, want in ((None, (), f32), ({"layer2": "f16"}, (), dict(f32, layer2="f16")),
                                 ({"layer2": "f16"}, ("layer3", "layer4"), dict(f32, layer2="f16", layer3="f16", layer4="f16")),
                                 ({"layer2": "f16", "layer3": "f16", "layer4": "f16"}, (), dict(f32, layer2="f16", layer3="f16", layer4="f16"))):
        it = MmpInterface(net, blocks4=blocks4, half=half, operands=operands, **given)
        assert it._operands == want and it._half == tuple(half)
        it.close()
    for cls_kw, refuse in (({"layer1": "f16"}, NO_KERNEL.format("{0}", "layer1")), ({"layer2": "f64"}, NEITHER.format("{0}", "layer2", "f64")),
                           ({"layer4": "f16"}, NEEDS.format("{0}", "layer4", "blocks4"))):
        with pytest.raises(ValueError, match=re.escape(refuse.format(""))):
            MmpInterface(net, operands=cls_kw, **given)
    with pytest.raises(ValueError, match=re.escape(CONTRADICTS.format("", "layer3"))):
        MmpInterface(net, half=("layer3",), operands={"layer3": "f32"}, **given)
    with pytest.raises(ValueError, match=re.escape(HALF_SENTENCE.format("", "layer2"))):
        MmpInterface(net, blocks4=blocks4, half=("layer2",), operands={"layer2": "f16"}, **given)
    ok = dict(predictor="mmp", network=net, ref_image=np.zeros((4, 5)), transform=snap.WorldTransform(), mmp_stem=stem, mmp_blocks=blocks,
              mmp_blocks2=blocks2, mmp_blocks3=blocks3)
    ev = lambda **kw: BatchEvaluator(None, None, None, None, None, None, **dict(ok, **kw))
    with pytest.raises(ValueError, match=re.escape(NO_KERNEL.format("mmp_", "layer1"))):
        ev(mmp_operands={"layer1": "f16"})
    with pytest.raises(ValueError, match=re.escape(NEITHER.format("mmp_", "layer2", "f64"))):
        ev(mmp_operands={"layer2": "f64"})
    with pytest.raises(ValueError, match=re.escape(NEEDS.format("mmp_", "layer4", "blocks4"))):
        ev(mmp_operands={"layer4": "f16"})
    with pytest.raises(ValueError, match=re.escape(NEEDS.format("mmp_", "layer2", "blocks2"))):
        ev(mmp_operands={"layer2": "f16"}, mmp_blocks2=None, mmp_blocks3=None)
    with pytest.raises(ValueError, match=re.escape(CONTRADICTS.format("mmp_", "layer3"))):
        ev(mmp_operands={"layer3": "f32"}, mmp_half=("layer3",))
    with pytest.raises(ValueError, match=re.escape(HALF_SENTENCE.format("mmp_", "layer2"))):
        ev(mmp_blocks4=blocks4, mmp_half=("layer2",), mmp_operands={"layer2": "f16"})
    with pytest.raises(ValueError, match=re.escape("mmp_operands needs predictor = 'mmp'")):
        BatchEvaluator(None, None, None, None, None, None, predictor="cvmp", mmp_operands={"layer2": "f16"})
    # accepted: with fused=False the NEXT refusal is the one that speaks
    for operands in ({"layer2": "f16"}, {"layer2": "f16", "layer3": "f16"}, {"layer2": "f32"}):
        with pytest.raises(ValueError, match="needs n_hyp = 1 and fused = True"):
            ev(mmp_operands=operands, fused=False)


class _NoDevice:
    """Stands where the handle does in a front end that launches nothing: every launch method is its own name."""

    def __getattr__(self, name):
        return name


def _front(**kw):
    stem, blocks, blocks2, blocks3, blocks4 = _given()
    return MmpFrontEnd(_NoDevice(), np.float32, "cpu", 9, 11, 2, snap.WorldTransform(), 1.0, 1.0, torch.zeros(9, 11), stem=stem, blocks=blocks,
                       blocks2=blocks2, blocks3=blocks3, blocks4=blocks4, **kw)


def _same_stage(a, b):
    assert (a.name, a.channels, a.cins, a.Args, a.launch, a.planes, a.buf_row, a.reads_fill, a.in_fill, a.offset) == \
        (b.name, b.channels, b.cins, b.Args, b.launch, b.planes, b.buf_row, b.reads_fill, b.in_fill, b.offset)
    assert len(a.specs) == len(b.specs)
    for sa, sb in zip(a.specs, b.specs):
        assert type(sa) is type(sb)
        for va, vb in zip(sa, sb):
            assert (va is None and vb is None) or (torch.is_tensor(va) and va.dtype == vb.dtype and torch.equal(va, vb)) or va == vb


def test_operands_give_the_stage_records_half_gives_and_layer2_its_own():
    plain, by_half, by_operands = _front(), _front(half=("layer3",)), _front(operands={"layer3": "f16"})
    assert plain.half == () and by_half.half == ("layer3",) and by_operands.half == ()
    assert by_half.operands == by_operands.operands == {"layer1": "f32", "layer2": "f32", "layer3": "f16", "layer4": "f32"}
    for name in ("layer1", "layer2", "layer3", "layer4"):
        _same_stage(by_half.stage(name), by_operands.stage(name))
    assert by_operands.stage("layer3").Args is _capi.NmpcMmpBlock3F16Args and by_operands.stage("layer3").launch == "mmp_block3_f16"
    for none in ({}, {"layer2": "f32"}, {"layer1": "f32", "layer2": "f32", "layer3": "f32", "layer4": "f32"}):
        same = _front(operands=none)
        for name in ("layer1", "layer2", "layer3", "layer4"):
            _same_stage(plain.stage(name), same.stage(name))
        assert same.bytes_per_item == plain.bytes_per_item and same.row == plain.row
    fe = _front(operands={"layer2": "f16"}, half=("layer4",))
    assert fe.half == ("layer4",) and fe.operands == {"layer1": "f32", "layer2": "f16", "layer3": "f32", "layer4": "f16"}
    st, st0 = fe.stage("layer2"), plain.stage("layer2")
    assert st.Args is _capi.NmpcMmpBlock2F16Args and st.launch == "mmp_block2_f16" and st0.Args is _capi.NmpcMmpBlock2Args
    assert all(isinstance(b, Block2F16Spec) and b.w1.dtype == torch.int16 and b.w2.shape == (9, 1, 2, 64, 8) for b in st.specs) and fe.blocks2 is st.specs
    assert (st.cins, st.planes, st.buf_row, st.in_fill, st.offset) == (st0.cins, st0.planes, st0.buf_row, st0.in_fill, st0.offset)
    assert fe.bytes_per_item == plain.bytes_per_item and fe.row == plain.row and fe.fill_row == plain.fill_row
    _same_stage(fe.stage("layer3"), plain.stage("layer3"))
    _same_stage(fe.stage("layer4"), _front(half=("layer4",)).stage("layer4"))


# ---- 4. the controls of the bound, before any device run -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _figures(c):
    """(|emulate - model| / bound at its worst, {wrong variant: the factor by which it misses the bound}) of a case, computed once."""
    x, spec, want, bound = h2.case("random", *c, _rows(c))
    r = (np.abs(h2.emulate(x, spec) - want) / bound).max()
    factors = {}
    for wrong in ("slope", "halo") + (("phase", "idphase") if c[3] == 2 else ()):
        bad, _ = h2.block(x, spec, wrong=wrong)
        assert bad.shape == want.shape
        factors[wrong] = (np.abs(bad - want) / bound).max()
    return r, factors


@pytest.mark.parametrize("c", ALL, ids=b2.case_id)
def test_the_bound_admits_the_emulation_and_refuses_the_wrong_variants(c):
    """On every case of the GPU tests: ``emulate`` meets the bound, each wrong variant of the float32 reference, run on the rounded
    operands, misses it."""
    H, W, Cin, stride, projection = c
    x, spec, want, bound = h2.case("random", *c, _rows(c))
    assert want.shape == (x.shape[0], 32) + b2.out_plane(H, W, stride) and (bound > 0).all()
    r, factors = _figures(c)
    print(f"{b2.case_id(c)}: emulate {r:.4f}" + "".join(f", {k} x {v:.0f}" for k, v in factors.items()))
    assert r <= 1.0, "the bound refuses a correct implementation of the rule"
    assert all(v > 1.0 for v in factors.values()), "the bound admits a wrong variant"
    # the rule costs something: on random data the model's value is not the float32 reference's
    assert not np.array_equal(want, b2.case("random", *c, _rows(c))[2])


@pytest.mark.parametrize("c", [(17, 89, 32, 2, True), (16, 88, 64, 2, True)], ids=b2.case_id)
def test_the_bound_on_strided_blocks_of_more_than_one_chunk(c):
    """The two strided cases beyond ``mmp_block2_reference.CASES`` that tests/test_gpu_mmp_block2_f16.py adds (Cin = 32 and 64 at stride
    2: two and four staged chunks): the same controls."""
    x, spec, want, bound = h2.case("random", *c, 2)
    r = (np.abs(h2.emulate(x, spec) - want) / bound).max()
    factors = {wrong: (np.abs(h2.block(x, spec, wrong=wrong)[0] - want) / bound).max() for wrong in ("slope", "halo", "phase", "idphase")}
    print(f"{b2.case_id(c)}: emulate {r:.4f}" + "".join(f", {k} x {v:.0f}" for k, v in factors.items()))
    assert r <= 1.0 and all(v > 1.0 for v in factors.values())
    xi, si, wi, _ = b2.case("integer", *c, 2)
    assert b2.integer_units(xi, si) < 2 ** 24 and np.array_equal(h2.emulate(xi, si), wi.astype(np.float32))


def test_the_recorded_margins_hold_over_all_cases():
    """``emulate`` at most 0.230 of the bound; every wrong variant at least 78 times over it."""
    figs = {c: _figures(c) for c in ALL}
    worst = max(figs, key=lambda c: figs[c][0])
    least = min(((v, k, c) for c in ALL for k, v in figs[c][1].items()), key=lambda t: t[0])
    print(f"emulate at most {figs[worst][0]:.4f} of the bound ({b2.case_id(worst)}); wrong variants at least x {least[0]:.1f} ({least[1]}, {b2.case_id(least[2])})")
    assert figs[worst][0] <= 0.24 and least[0] >= 75.0


@pytest.mark.parametrize("c", ALL, ids=b2.case_id)
def test_integer_cases_are_binary16_values_throughout(c):
    """Every operand and every m of the integer cases is a binary16 value, |m| <= 127: the rule rounds nothing on them, so the model
    equals the float32 reference, and ``emulate`` gives that reference's bits."""
    import torch.nn.functional as F
    x, spec, want, _ = b2.case("integer", *c, _rows(c))
    is_h = lambda a: np.array_equal(np.asarray(a, dtype=np.float64), round_f16(a).astype(np.float64))
    assert is_h(x) and is_h(spec.w1) and is_h(spec.w2) and (spec.wd is None or is_h(spec.wd))
    xt, w1, s1, b1, _, _, _ = b2._parts(x, spec)
    m = F.leaky_relu(s1 * F.conv2d(xt, w1, stride=int(spec.stride), padding=1) + b1, float(spec.slope_mid)).numpy()
    assert is_h(m) and np.abs(m).max() <= 127
    assert b2.integer_units(x, spec) < 2 ** 24
    model, _ = h2.block(x, spec)
    assert np.array_equal(model, want) and np.array_equal(h2.block(x, spec, round_m=True)[0], want)
    assert np.array_equal(h2.emulate(x, spec), want.astype(np.float32))


def test_the_exact_blocks_under_the_rule():
    x = round_f16(np.abs(b2.random_x(2, 32, 9, 45, seed=5))).astype(np.float32)
    assert np.array_equal(h2.emulate(x, b2.doubling_block2()), x + x) and np.array_equal(h2.block(x, b2.doubling_block2())[0], x + x)
    x = round_f16(np.abs(b2.random_x(2, 16, 17, 21, seed=6))).astype(np.float32)
    half = x[:, :, ::2, ::2]
    want = np.concatenate([half + half, half + half], axis=1)
    assert np.array_equal(h2.emulate(x, b2.duplicate_and_double_block2()), want)
    assert np.array_equal(h2.block(x, b2.duplicate_and_double_block2())[0], want)


SATURATING = [(17, 89, 16, 2, True), (9, 45, 32, 1, False), (8, 44, 64, 1, True)]


def test_the_bound_covers_inputs_that_saturate():
    """|x| up to 1e5, a twentieth of the values beyond +-65504: x saturates, and here and there m does too. The model clips both
    (saturation is the rule, not an error of it), and ``emulate`` stays within the bound."""
    for c in SATURATING:
        x, spec, _, _ = b2.case("random", *c)
        rng = np.random.default_rng(17)
        x = x.copy()
        big = rng.random(x.shape) < 0.05
        x[big] = (rng.uniform(6e4, 1e5, x.shape) * rng.choice([-1.0, 1.0], x.shape)).astype(np.float32)[big]
        want, bound = h2.block(x, spec)
        got = h2.emulate(x, spec)
        r = (np.abs(got - want) / bound).max()
        print(f"{b2.case_id(c)}: emulate {r:.4f} of the bound, |x| up to {np.abs(x).max():.0f}")
        assert np.isfinite(got).all() and r <= 1.0


# ---- 5. the rule's cost through the whole network, on the CPU ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(nr.SHAPES)), ids=[f"{s['Hm']}x{s['Wm']}" for s in nr.SHAPES])
def test_emulation_through_the_network_stays_within_the_bar(k):
    """``emulate`` chained through the four real-valued blocks of layer2 on the float64 module's layer1, finished by torch's float32
    layer3, layer4 and head, against the float64 module. Yardstick per stage: ``model_chain`` on the same input, finished by the
    float64 module -- what the rule alone costs. Within ``nr.BAR`` = 4 yardsticks at layer2, layer3, layer4 and the output."""
    shape, M = nr.SHAPES[k], (4, 2)[k]
    x = nr.rule_input(shape["Hm"], shape["Wm"], M)
    net32 = nr.made_net(shape)
    net64 = nr.in_double(net32)
    want = [t.numpy() for t in nr.stages(net64, x)]
    blocks2 = ms.split_network_whole(net64)[2]
    x1 = want[1].astype(np.float32)

    def behind(net, x2):
        """layer2's output ``x2`` -> [layer2, layer3, layer4, output] through ``net``, in its own dtype."""
        with torch.no_grad():
            t = torch.as_tensor(x2).to(next(net.parameters()).dtype)
            out = [t, net.resnet34.layer3(t)]
            out.append(net.resnet34.layer4(out[-1]))
            out.append(nr.finish(net, out[-1], 4))
        return [o.double().numpy() for o in out]

    model = behind(net64, h2.model_chain(x1, blocks2)[-1])
    e = x1
    for spec in blocks2:
        e = h2.emulate(e, spec)
    emu = behind(net32, e)
    ratios = []
    for name, g, w, m in zip(nr.STAGE_NAMES[2:], emu, want[2:], model):
        assert g.shape == w.shape == m.shape and np.isfinite(g).all()
        y = float(np.abs(m - w).max())
        assert y > 0
        ratios.append(float(np.abs(g - w).max()) / y)
        print(f"{shape['Hm']} x {shape['Wm']} M {M} {name}: yardstick {y:.3e}, |emulate - float64| / yardstick = {ratios[-1]:.2f}")
    assert max(ratios) <= nr.BAR, ratios
