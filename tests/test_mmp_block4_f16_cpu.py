"""CPU tests of the layer4 block with binary16 MFMA operands (``nmpc_mmp_block4_f16``, csrc/nmpc_mmp_block4_f16.h): the packing of
the weights (``mmp_stem.pack_block4_f16``), the struct against the C compiler, the entry point, the resources of the three shipped
kernels, ``half=`` with ``layer4`` in the three host classes, and the controls of the float64 model's bound
(tests/mmp_block4_f16_reference.py) before any device run. The sibling of tests/test_mmp_block3_f16_cpu.py.

Recorded over ``mmp_block4_reference.CASES + REAL`` (27 cases): ``emulate`` -- torch's float32 convolutions on the rounded operands,
m rounded -- lies at most 0.103 of the bound (20 x 22, Cin 8, stride 2); the wrong variants miss it by at least 11.3 ("slope", 4 x 6,
Cin 256). Every operand and every m of the integer cases is a binary16 value (|m| <= 112), and ``emulate`` gives the float32
reference's bits on them."""
import ctypes
import functools
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import dyobav_mpcnwta_warehouse_amd as nm
import mmp_block2_reference as b2
import mmp_block3_reference as b3
import mmp_block4_f16_reference as h4
import mmp_block4_reference as b4
import mmp_block_reference as br
import mmp_stem_reference as sr
from dyobav_mpcnwta_warehouse_amd import _capi, snap
from dyobav_mpcnwta_warehouse_amd.mmp_front import MmpFrontEnd
from dyobav_mpcnwta_warehouse_amd.mmp_interface import MmpInterface
from dyobav_mpcnwta_warehouse_amd.mmp_stem import (Block4F16Spec, Block4Spec, check_blocks, check_blocks2, pack_block4_f16, round_f16,
                                                   unpack_block4_f16)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = b4.CASES + b4.REAL
_rows = lambda c: 2 if c in b4.REAL else b4.M_MAX
SENTENCE = "{0}half: {1!r}: only layer3 has an f16 kernel, and layer4 where {0}blocks4 is given"


# ---- 1. the packing ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cin,stride,projection", [(8, 2, True), (48, 1, True), (64, 2, True), (128, 1, False), (256, 1, True)])
def test_pack_is_the_fragment_order_and_unpack_inverts_it(Cin, stride, projection):
    spec = b4.random_block4(Cin, 7 + Cin, stride, projection)
    p = pack_block4_f16(spec)
    KB = (Cin + 31) // 32
    assert isinstance(p, Block4F16Spec) and p._fields == Block4Spec._fields
    assert p.w1.shape == (9, KB, 8, 64, 8) and p.w2.shape == (9, 4, 8, 64, 8) and all(a.dtype == np.uint16 and a.flags.c_contiguous for a in (p.w1, p.w2))
    assert (p.wd is None) == (not projection) and (p.wd is None or (p.wd.shape == (KB, 8, 64, 8) and p.wd.dtype == np.uint16))
    for name in ("s1", "b1", "s2", "b2", "sd", "bd", "slope_mid", "slope_out", "stride"):           # passed through, float32
        a, b = getattr(p, name), getattr(spec, name)
        assert (a is None and b is None) or (np.array_equal(a, b) and np.asarray(a).dtype == np.asarray(b).dtype), name
    # the documented order, element by element, against np.float16 of the weights; zeros behind Cin
    h1, h2 = spec.w1.astype(np.float16), spec.w2.astype(np.float16)
    rng = np.random.default_rng(Cin)
    for t, kb, g, l, j in zip(rng.integers(0, 9, 300), rng.integers(0, KB, 300), rng.integers(0, 8, 300), rng.integers(0, 64, 300), rng.integers(0, 8, 300)):
        co, ci = 16 * g + (l & 15), 32 * kb + 8 * (l >> 4) + j
        want = h1[co, ci, t // 3, t % 3].view(np.uint16) if ci < Cin else 0
        assert p.w1[t, kb, g, l, j] == want, (t, kb, g, l, j)
        if kb < 4:
            assert p.w2[t, kb, g, l, j] == h2[co, ci, t // 3, t % 3].view(np.uint16)
        if projection:
            assert p.wd[kb, g, l, j] == (spec.wd.astype(np.float16)[co, ci].view(np.uint16) if ci < Cin else 0)
    if Cin % 32:
        pad = p.w1.reshape(9, KB, 8, 4, 16, 8)[:, -1, :, (Cin % 32) // 8:]
        assert pad.size and not pad.any()
        if projection:
            pad = p.wd.reshape(KB, 8, 4, 16, 8)[-1, :, (Cin % 32) // 8:]
            assert pad.size and not pad.any()
    u = unpack_block4_f16(p, Cin)
    assert isinstance(u, Block4Spec) and u.w1.dtype == np.float16 and np.array_equal(u.w1, h1) and np.array_equal(u.w2, h2)
    assert (u.wd is None) == (not projection) and (u.wd is None or np.array_equal(u.wd, spec.wd.astype(np.float16)))
    again = pack_block4_f16(u)                                       # a round trip: rounded weights round to themselves
    assert np.array_equal(again.w1, p.w1) and np.array_equal(again.w2, p.w2) and (p.wd is None or np.array_equal(again.wd, p.wd))


def test_pack_saturates_and_refuses_what_check_block4_refuses():
    ok = b4.random_block4(128, 1, 1, False)
    big = ok.w1.copy()
    big[0, 0, 0, 0], big[1, 0, 0, 0] = 1e6, -7e4
    u = unpack_block4_f16(pack_block4_f16(ok._replace(w1=big)), 128)
    assert u.w1[0, 0, 0, 0] == 65504.0 and u.w1[1, 0, 0, 0] == -65504.0 and np.isfinite(u.w1).all()
    for bad in (ok._replace(s1=np.zeros(4)), ok._replace(w1=np.zeros((128, 12, 3, 3))), ok._replace(wd=np.zeros((128, 128))),
                ok._replace(slope_mid=float("nan")), ok._replace(slope_out=2.0), ok._replace(stride=2), ok._replace(stride=0),
                b4.random_block4(256, 1, 1, True)._replace(sd=None), b3.random_block3(64, 1, 1, False)):
        with pytest.raises(ValueError, match="Block4Spec"):
            pack_block4_f16(bad)


# ---- 2. the struct and the symbol: no device needed ---------------------------------------------------------------------------------------------
def test_entry_point_refuses_null_arguments():
    lib = nm.load_library()
    assert "nmpc_mmp_block4_f16" in nm.EXPORTED_SYMBOLS and hasattr(lib, "nmpc_mmp_block4_f16")
    a = _capi.NmpcMmpBlock4F16Args()
    assert lib.nmpc_mmp_block4_f16(None, ctypes.byref(a)) == -1 and lib.nmpc_mmp_block4_f16(None, None) == -1


def test_args_layout_matches_the_c_compiler():
    fields = [f[0] for f in _capi.NmpcMmpBlock4F16Args._fields_]
    assert fields == ["M", "Cin", "H", "W", "x", "w1", "s1", "b1", "w2", "s2", "b2", "wd", "sd", "bd", "slope_mid", "slope_out", "out", "stride"]
    old = ("nmpc_mmp_block3_args", "nmpc_mmp_block3_f16_args", "nmpc_mmp_block4_args")
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "sz.c")
        body = "".join(f'printf(" %zu", offsetof(nmpc_mmp_block4_f16_args, {f}));' for f in fields)
        body += "".join(f'printf(" %zu", sizeof({s}));' + "".join(f'printf(" %zu", offsetof({s}, {f}));' for f in fields) for s in old)
        open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "nmpc_hip.h"\nint main(void){printf("%zu", sizeof(nmpc_mmp_block4_f16_args));'
                             + body + 'printf(" %d", NMPC_ABI_VERSION);return 0;}\n')
        exe = os.path.join(td, "sz")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    n = len(fields)
    assert ctypes.sizeof(_capi.NmpcMmpBlock4F16Args) == out[0] == 120
    mine = [getattr(_capi.NmpcMmpBlock4F16Args, f).offset for f in fields]
    assert mine == out[1:1 + n]
    for k, mirror in enumerate((_capi.NmpcMmpBlock3Args, _capi.NmpcMmpBlock3F16Args, _capi.NmpcMmpBlock4Args)):   # nothing that existed changed
        part = out[1 + n + k * (n + 1):1 + n + (k + 1) * (n + 1)]
        assert part[0] == ctypes.sizeof(mirror) == 120 and part[1:] == [getattr(mirror, f).offset for f in fields] == mine
    assert out[-1] == 5                                                                             # no version change


def test_kernels_use_no_scratch_and_fit_the_occupancy_the_header_states():
    """From the shipped code object: exactly three kernels, no scratch and no spills, 40 960 B of LDS and at most 168 registers --
    three workgroups of four waves per CU, 3 waves per SIMD, the header's __launch_bounds__(256, 3). Recorded: <2, true> 162
    VGPRs, <1, true> 142, <1, false> 146."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    nm.build_library()
    res = {kernel_resources.short_name(k): v for k, v in kernel_resources.kernel_resources(nm.library_path()).items()}
    mine = {k: v for k, v in res.items() if re.search(r"mmp_blkh_kernel<nmpc::MmpBlock4HGeom, ", k)}
    assert len(mine) == 3, sorted(mine)
    assert not any(re.search(r"mmp_blkf_kernel<nmpc::MmpBlock4Geom, ", k) for k in mine)                 # the f32 family's pattern does not take these in
    header = open(os.path.join(ROOT, "dyobav-mpcnwta-warehouse_amd", "csrc", "nmpc_mmp_block4_f16.h")).read()
    assert "Threads = kB4HThreads" in header and "min_wg(int) { return 3; }" in header and "kB4HThreads = 256" in header   # the geometry's figures ...
    shared = open(os.path.join(ROOT, "dyobav-mpcnwta-warehouse_amd", "csrc", "nmpc_mmp_block_f16.h")).read()
    assert "__launch_bounds__(G::Threads, G::min_wg(STRIDE))" in shared   # ... are the one kernel's launch bound
    for name, r in mine.items():
        print(name, r)
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
        assert r["lds_static"] == 40960, (name, r)
        regs = r["vgpr"] + max(r["agpr"], 0)
        assert regs <= 168 and 512 // (-(-regs // 8) * 8) == 3, (name, r)           # 3 waves per SIMD by the registers
        assert (160 * 1024) // r["lds_static"] >= 3, (name, r)                      # and the LDS holds the three workgroups they make


# ---- 3. half= in the three host classes -----------------------------------------------------------------------------------------------------------
def test_half_takes_layer4_where_blocks4_is_given():
    from dyobav_mpcnwta_warehouse_amd.evaluate import BatchEvaluator
    stem = sr.delta_spec(16)
    blocks = check_blocks(stem, [br.doubling_block()])
    blocks2 = check_blocks2(blocks, [b2.duplicate_and_double_block2(16)])
    blocks3 = [b3.duplicate_and_double_block3(32), b3.doubling_block3()]
    blocks4 = [b4.duplicate_and_double_block4(64), b4.doubling_block4()]
    six = MmpFrontEnd.check_specs(stem, blocks, blocks2=blocks2, blocks3=blocks3, blocks4=blocks4, head=None)
    assert MmpFrontEnd.check_half((), six) == () and MmpFrontEnd.check_half(("layer3",), six) == ("layer3",)
    assert MmpFrontEnd.check_half(("layer4",), six) == ("layer4",) and MmpFrontEnd.check_half("layer4", six) == ("layer4",)
    assert MmpFrontEnd.check_half(("layer3", "layer4"), six) == ("layer3", "layer4")
    assert MmpFrontEnd.check_half(["layer4", "layer3", "layer4", "layer3"], six) == ("layer4", "layer3")     # deduplicated, order kept
    for name in ("layer1", "layer2", "stem", "head", "layer5"):                       # with everything given
        with pytest.raises(ValueError, match=re.escape(SENTENCE.format("", name))):
            MmpFrontEnd.check_half((name,), six)
        with pytest.raises(ValueError, match=re.escape(SENTENCE.format("mmp_", name))):
            MmpFrontEnd.check_half(("layer3", name), six, prefix="mmp_")
    none4 = MmpFrontEnd.check_specs(stem, blocks, blocks2=blocks2, blocks3=blocks3, head=None)
    for half in (("layer4",), ("layer3", "layer4")):
        with pytest.raises(ValueError, match=re.escape(SENTENCE.format("", "layer4"))):
            MmpFrontEnd.check_half(half, none4)
    with pytest.raises(ValueError, match="'layer3' needs blocks3"):
        MmpFrontEnd.check_half(("layer3", "layer4"), MmpFrontEnd.check_specs(stem, blocks, blocks2=blocks2, head=None))
    # MmpInterface and BatchEvaluator take and refuse the same in their constructors, before any device is touched
    net = lambda x: x
    given = dict(stem=stem, blocks=blocks, blocks2=blocks2, blocks3=blocks3)
    for half in (("layer4",), ("layer3", "layer4"), ["layer4", "layer4"]):
        it = MmpInterface(net, blocks4=blocks4, half=half, **given)
        assert it._half == tuple(dict.fromkeys(half))
        it.close()
    with pytest.raises(ValueError, match=re.escape(SENTENCE.format("", "layer2"))):
        MmpInterface(net, blocks4=blocks4, half=("layer2",), **given)
    with pytest.raises(ValueError, match=re.escape(SENTENCE.format("", "layer4"))):
        MmpInterface(net, half=("layer4",), **given)
    ok = dict(predictor="mmp", network=net, ref_image=np.zeros((4, 5)), transform=snap.WorldTransform(), mmp_stem=stem, mmp_blocks=blocks,
              mmp_blocks2=blocks2, mmp_blocks3=blocks3)
    with pytest.raises(ValueError, match=re.escape(SENTENCE.format("mmp_", "layer4"))):
        BatchEvaluator(None, None, None, None, None, None, **dict(ok, mmp_half=("layer3", "layer4")))
    with pytest.raises(ValueError, match=re.escape(SENTENCE.format("mmp_", "layer2"))):
        BatchEvaluator(None, None, None, None, None, None, **dict(ok, mmp_blocks4=blocks4, mmp_half=("layer2",)))


def test_batch_evaluator_takes_layer4_with_its_blocks():
    """The constructor's check of ``mmp_half`` passes both names with ``mmp_blocks4``: with ``fused=False`` the NEXT refusal is the one
    that speaks, and without ``mmp_blocks4`` the same call stops at ``mmp_half``."""
    from dyobav_mpcnwta_warehouse_amd.evaluate import BatchEvaluator
    stem = sr.delta_spec(16)
    blocks = check_blocks(stem, [br.doubling_block()])
    blocks2 = check_blocks2(blocks, [b2.duplicate_and_double_block2(16)])
    kw = dict(predictor="mmp", network=lambda x: x, ref_image=np.zeros((4, 5)), transform=snap.WorldTransform(), mmp_stem=stem, mmp_blocks=blocks,
              mmp_blocks2=blocks2, mmp_blocks3=[b3.duplicate_and_double_block3(32), b3.doubling_block3()], fused=False)
    blocks4 = [b4.duplicate_and_double_block4(64), b4.doubling_block4()]
    for half in (("layer4",), ("layer3", "layer4"), ("layer4", "layer3", "layer4")):
        with pytest.raises(ValueError, match="needs n_hyp = 1 and fused = True"):
            BatchEvaluator(None, None, None, None, None, None, **dict(kw, mmp_blocks4=blocks4, mmp_half=half))
        with pytest.raises(ValueError, match=re.escape(SENTENCE.format("mmp_", "layer4"))):
            BatchEvaluator(None, None, None, None, None, None, **dict(kw, mmp_half=half))


# ---- 4. the controls of the bound, before any device run -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _figures(c):
    """(|emulate - model| / bound at its worst, {wrong variant: the factor by which it misses the bound}) of a case, computed once."""
    x, spec, want, bound = h4.case("random", *c, _rows(c))
    r = (np.abs(h4.emulate(x, spec) - want) / bound).max()
    factors = {}
    for wrong in ("slope", "halo") + (("phase", "idphase") if c[3] == 2 else ()):
        bad, _ = h4.block(x, spec, wrong=wrong)
        assert bad.shape == want.shape
        factors[wrong] = (np.abs(bad - want) / bound).max()
    return r, factors


@pytest.mark.parametrize("c", ALL, ids=b4.case_id)
def test_the_bound_admits_the_emulation_and_refuses_the_wrong_variants(c):
    """On every case of the GPU tests: ``emulate`` meets the bound, each wrong variant of the float32 reference, run on the rounded
    operands, misses it."""
    H, W, Cin, stride, projection = c
    x, spec, want, bound = h4.case("random", *c, _rows(c))
    assert want.shape == (x.shape[0], 128) + b4.out_plane(H, W, stride) and (bound > 0).all()
    r, factors = _figures(c)
    print(f"{b4.case_id(c)}: emulate {r:.4f}" + "".join(f", {k} x {v:.0f}" for k, v in factors.items()))
    assert r <= 1.0, "the bound refuses a correct implementation of the rule"
    assert all(v > 1.0 for v in factors.values()), "the bound admits a wrong variant"
    # the rule costs something: on random data the model's value is not the float32 reference's
    assert not np.array_equal(want, b4.case("random", *c, _rows(c))[2])


def test_the_recorded_margins_hold_over_all_cases():
    """``emulate`` at most 0.103 of the bound; every wrong variant at least 11.3 times over it."""
    figs = {c: _figures(c) for c in ALL}
    worst = max(figs, key=lambda c: figs[c][0])
    least = min(((v, k, c) for c in ALL for k, v in figs[c][1].items()), key=lambda t: t[0])
    print(f"emulate at most {figs[worst][0]:.4f} of the bound ({b4.case_id(worst)}); wrong variants at least x {least[0]:.1f} ({least[1]}, {b4.case_id(least[2])})")
    assert figs[worst][0] <= 0.11 and least[0] >= 11.0


@pytest.mark.parametrize("c", ALL, ids=b4.case_id)
def test_integer_cases_are_binary16_values_throughout(c):
    """Every operand and every m of the integer cases is a binary16 value, |m| <= 112: the rule rounds nothing on them, so the model
    equals the float32 reference, and ``emulate`` gives that reference's bits."""
    import torch.nn.functional as F
    x, spec, want, _ = b4.case("integer", *c, _rows(c))
    is_h = lambda a: np.array_equal(np.asarray(a, dtype=np.float64), round_f16(a).astype(np.float64))
    assert is_h(x) and is_h(spec.w1) and is_h(spec.w2) and (spec.wd is None or is_h(spec.wd))
    xt, w1, s1, b1, _, _, _ = b4._parts(x, spec)
    m = F.leaky_relu(s1 * F.conv2d(xt, w1, stride=int(spec.stride), padding=1) + b1, float(spec.slope_mid)).numpy()
    assert is_h(m) and np.abs(m).max() <= 112
    model, _ = h4.block(x, spec)
    assert np.array_equal(model, want) and np.array_equal(h4.block(x, spec, round_m=True)[0], want)
    assert np.array_equal(h4.emulate(x, spec), want.astype(np.float32))


def test_the_exact_blocks_under_the_rule():
    x = round_f16(np.abs(b4.random_x(2, 128, 9, 12, seed=5))).astype(np.float32)
    assert np.array_equal(h4.emulate(x, b4.doubling_block4()), x + x) and np.array_equal(h4.block(x, b4.doubling_block4())[0], x + x)
    x = round_f16(np.abs(b4.random_x(2, 64, 19, 21, seed=6))).astype(np.float32)
    half = x[:, :, ::2, ::2]
    want = np.concatenate([half + half, half + half], axis=1)
    assert np.array_equal(h4.emulate(x, b4.duplicate_and_double_block4()), want)
    assert np.array_equal(h4.block(x, b4.duplicate_and_double_block4())[0], want)


SATURATING = [(21, 23, 64, 2, True), (11, 12, 128, 1, False), (10, 11, 48, 1, True)]


def test_the_bound_covers_inputs_that_saturate():
    """|x| up to 1e5, a twentieth of the values beyond +-65504: x saturates, and here and there m does too. The model clips both
    (saturation is the rule, not an error of it), and ``emulate`` stays within the bound."""
    for c in SATURATING:
        x, spec, _, _ = b4.case("random", *c)
        rng = np.random.default_rng(17)
        x = x.copy()
        big = rng.random(x.shape) < 0.05
        x[big] = (rng.uniform(6e4, 1e5, x.shape) * rng.choice([-1.0, 1.0], x.shape)).astype(np.float32)[big]
        want, bound = h4.block(x, spec)
        got = h4.emulate(x, spec)
        r = (np.abs(got - want) / bound).max()
        print(f"{b4.case_id(c)}: emulate {r:.4f} of the bound, |x| up to {np.abs(x).max():.0f}")
        assert np.isfinite(got).all() and r <= 1.0
