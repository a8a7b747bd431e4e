"""CPU tests of the layer3 block with binary16 MFMA operands (``nmpc_mmp_block3_f16``, csrc/nmpc_mmp_block3_f16.h): the packing of
the weights (``mmp_stem.pack_block3_f16``), the struct against the C compiler, the entry point, the resources of the three shipped
kernels, the ``half=`` refusals of the three host classes, and the controls of the float64 model's bound
(tests/mmp_block3_f16_reference.py) before any device run.

Recorded over ``mmp_block3_reference.CASES + REAL`` (27 cases): ``emulate`` -- torch's float32 convolutions on the rounded operands,
m rounded -- lies at most 0.21 of the bound (14 x 42, Cin 8, stride 2); the wrong variants miss it by at least 28 ("slope", 7 x 21,
Cin 128). Every operand and every m of the integer cases is a binary16 value (|m| <= 133), and ``emulate`` gives the float32
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
import mmp_block3_f16_reference as h3
import mmp_block3_reference as b3
import mmp_block_reference as br
import mmp_stem_reference as sr
from dyobav_mpcnwta_warehouse_amd import _capi, snap
from dyobav_mpcnwta_warehouse_amd.mmp_front import MmpFrontEnd
from dyobav_mpcnwta_warehouse_amd.mmp_interface import MmpInterface
from dyobav_mpcnwta_warehouse_amd.mmp_stem import (Block3F16Spec, Block3Spec, check_blocks, check_blocks2, pack_block3_f16, round_f16,
                                                   unpack_block3_f16)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = b3.CASES + b3.REAL
_rows = lambda c: 2 if c in b3.REAL else b3.M_MAX


# ---- 1. the rounding and the packing -------------------------------------------------------------------------------------------------------
def test_round_f16_is_the_rule():
    tiny = 2.0 ** -24
    a = np.array([0.0, 1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65504.0, 65519.0, 65520.0, 1e5, -1e5, np.inf, -np.inf, tiny, 3 * tiny, 0.5 * tiny,
                  1.5 * tiny, 2.0 ** -14 - tiny], dtype=np.float32)
    want = [0.0, 1.0, 1.0, 1.0 + 2.0 ** -9, 65504.0, 65504.0, 65504.0, 65504.0, -65504.0, 65504.0, -65504.0, tiny, 3 * tiny, 0.0, 2 * tiny,
            2.0 ** -14 - tiny]                                      # ties to even; saturation, not infinity; subnormals kept
    got = round_f16(a)
    assert got.dtype == np.float16 and np.array_equal(got.astype(np.float64), np.array(want))
    assert np.isnan(round_f16(np.array([np.nan], dtype=np.float32))[0])


@pytest.mark.parametrize("Cin,stride,projection", [(8, 2, True), (24, 1, True), (32, 2, True), (64, 1, False), (72, 1, True), (256, 1, True)])
def test_pack_is_the_fragment_order_and_unpack_inverts_it(Cin, stride, projection):
    spec = b3.random_block3(Cin, 7 + Cin, stride, projection)
    p = pack_block3_f16(spec)
    KB = (Cin + 31) // 32
    assert isinstance(p, Block3F16Spec) and p._fields == Block3Spec._fields
    assert p.w1.shape == (9, KB, 4, 64, 8) and p.w2.shape == (9, 2, 4, 64, 8) and all(a.dtype == np.uint16 and a.flags.c_contiguous for a in (p.w1, p.w2))
    assert (p.wd is None) == (not projection) and (p.wd is None or (p.wd.shape == (KB, 4, 64, 8) and p.wd.dtype == np.uint16))
    for name in ("s1", "b1", "s2", "b2", "sd", "bd", "slope_mid", "slope_out", "stride"):           # passed through, float32
        a, b = getattr(p, name), getattr(spec, name)
        assert (a is None and b is None) or (np.array_equal(a, b) and np.asarray(a).dtype == np.asarray(b).dtype), name
    # the documented order, element by element, against np.float16 of the weights; zeros behind Cin
    h1, h2 = spec.w1.astype(np.float16), spec.w2.astype(np.float16)
    rng = np.random.default_rng(Cin)
    for t, kb, g, l, j in zip(rng.integers(0, 9, 200), rng.integers(0, KB, 200), rng.integers(0, 4, 200), rng.integers(0, 64, 200), rng.integers(0, 8, 200)):
        co, ci = 16 * g + (l & 15), 32 * kb + 8 * (l >> 4) + j
        want = h1[co, ci, t // 3, t % 3].view(np.uint16) if ci < Cin else 0
        assert p.w1[t, kb, g, l, j] == want, (t, kb, g, l, j)
        if kb < 2:
            assert p.w2[t, kb, g, l, j] == h2[co, ci, t // 3, t % 3].view(np.uint16)
        if projection:
            assert p.wd[kb, g, l, j] == (spec.wd.astype(np.float16)[co, ci].view(np.uint16) if ci < Cin else 0)
    if Cin % 32:
        pad = p.w1.reshape(9, KB, 4, 4, 16, 8)[:, -1, :, (Cin % 32) // 8:]
        assert pad.size and not pad.any()
    u = unpack_block3_f16(p, Cin)
    assert isinstance(u, Block3Spec) and u.w1.dtype == np.float16 and np.array_equal(u.w1, h1) and np.array_equal(u.w2, h2)
    assert (u.wd is None) == (not projection) and (u.wd is None or np.array_equal(u.wd, spec.wd.astype(np.float16)))
    again = pack_block3_f16(u)                                       # a round trip: rounded weights round to themselves
    assert np.array_equal(again.w1, p.w1) and np.array_equal(again.w2, p.w2) and (p.wd is None or np.array_equal(again.wd, p.wd))


def test_pack_saturates_and_refuses_what_check_block3_refuses():
    ok = b3.random_block3(64, 1, 1, False)
    big = ok.w1.copy()
    big[0, 0, 0, 0], big[1, 0, 0, 0] = 1e6, -7e4
    u = unpack_block3_f16(pack_block3_f16(ok._replace(w1=big)), 64)
    assert u.w1[0, 0, 0, 0] == 65504.0 and u.w1[1, 0, 0, 0] == -65504.0 and np.isfinite(u.w1).all()
    for bad in (ok._replace(s1=np.zeros(4)), ok._replace(w1=np.zeros((64, 12, 3, 3))), ok._replace(wd=np.zeros((64, 64))),
                ok._replace(slope_mid=float("nan")), ok._replace(slope_out=2.0), ok._replace(stride=2), ok._replace(stride=0),
                b3.random_block3(128, 1, 1, True)._replace(sd=None), b2.random_block2(32, 1, 1, False)):
        with pytest.raises(ValueError, match="Block3Spec"):
            pack_block3_f16(bad)


# ---- 2. the struct and the symbol: no device needed ---------------------------------------------------------------------------------------------
def test_entry_point_refuses_null_arguments():
    lib = nm.load_library()
    assert "nmpc_mmp_block3_f16" in nm.EXPORTED_SYMBOLS and hasattr(lib, "nmpc_mmp_block3_f16")
    a = _capi.NmpcMmpBlock3F16Args()
    assert lib.nmpc_mmp_block3_f16(None, ctypes.byref(a)) == -1 and lib.nmpc_mmp_block3_f16(None, None) == -1


def test_args_layout_matches_the_c_compiler():
    fields = [f[0] for f in _capi.NmpcMmpBlock3F16Args._fields_]
    assert fields == ["M", "Cin", "H", "W", "x", "w1", "s1", "b1", "w2", "s2", "b2", "wd", "sd", "bd", "slope_mid", "slope_out", "out", "stride"]
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "sz.c")
        body = "".join(f'printf(" %zu", offsetof(nmpc_mmp_block3_f16_args, {f}));' for f in fields)
        open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "nmpc_hip.h"\nint main(void){printf("%zu", sizeof(nmpc_mmp_block3_f16_args));'
                             + body + 'printf(" %zu %d", sizeof(nmpc_mmp_block3_args), NMPC_ABI_VERSION);return 0;}\n')
        exe = os.path.join(td, "sz")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert ctypes.sizeof(_capi.NmpcMmpBlock3F16Args) == out[0] == 120
    assert [getattr(_capi.NmpcMmpBlock3F16Args, f).offset for f in fields] == out[1:1 + len(fields)]
    assert out[-2] == ctypes.sizeof(_capi.NmpcMmpBlock3Args) == 120 and out[-1] == 5        # nothing that existed changed; no version change


def test_kernels_use_no_scratch_and_fit_the_occupancy_the_header_states():
    """From the shipped code object: exactly three kernels, no scratch and no spills; at stride 1 36 864 B of LDS and at most 128
    registers -- four workgroups of four waves per CU, 4 waves per SIMD, the header's __launch_bounds__(256, 4) --, at stride 2
    73 728 B and at most 256: two. Recorded: <2, true> 165 VGPRs, <1, true> and <1, false> 124."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    nm.build_library()
    res = {kernel_resources.short_name(k): v for k, v in kernel_resources.kernel_resources(nm.library_path()).items()}
    mine = {k: v for k, v in res.items() if re.search(r"mmp_blkh_kernel<nmpc::MmpBlock3HGeom, ", k)}
    assert len(mine) == 3, sorted(mine)
    header = open(os.path.join(ROOT, "dyobav-mpcnwta-warehouse_amd", "csrc", "nmpc_mmp_block3_f16.h")).read()
    assert "Threads = kB3Threads" in header and "min_wg(int stride) { return stride == 2 ? 2 : 4; }" in header   # the geometry's figures ...
    shared = open(os.path.join(ROOT, "dyobav-mpcnwta-warehouse_amd", "csrc", "nmpc_mmp_block_f16.h")).read()
    assert "__launch_bounds__(G::Threads, G::min_wg(STRIDE))" in shared   # ... are the one kernel's launch bound
    for name, r in mine.items():
        print(name, r)
        strided = "Geom, 2," in name
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
        assert r["lds_static"] == (73728 if strided else 36864), (name, r)
        assert r["vgpr"] + max(r["agpr"], 0) <= (256 if strided else 128), (name, r)
        assert (160 * 1024) // r["lds_static"] == (2 if strided else 4), (name, r)          # LDS and registers agree


# ---- 3. half= in the three host classes -----------------------------------------------------------------------------------------------------------
def test_half_is_layer3_only_and_needs_its_blocks():
    from dyobav_mpcnwta_warehouse_amd.evaluate import BatchEvaluator
    stem = sr.delta_spec(16)
    blocks = check_blocks(stem, [br.doubling_block()])
    blocks2 = check_blocks2(blocks, [b2.duplicate_and_double_block2(16)])
    blocks3 = [b3.duplicate_and_double_block3(32), b3.doubling_block3()]
    six = MmpFrontEnd.check_specs(stem, blocks, blocks2=blocks2, blocks3=blocks3, head=None)
    assert MmpFrontEnd.check_half((), six) == () and MmpFrontEnd.check_half(("layer3",), six) == ("layer3",)
    assert MmpFrontEnd.check_half("layer3", six) == ("layer3",) and MmpFrontEnd.check_half(["layer3", "layer3"], six) == ("layer3",)
    for name in ("layer1", "layer2", "layer4", "stem", "head", "layer5"):
        with pytest.raises(ValueError, match="only layer3 has an f16 kernel"):
            MmpFrontEnd.check_half((name,), six)
    none3 = MmpFrontEnd.check_specs(stem, blocks, blocks2=blocks2, head=None)
    with pytest.raises(ValueError, match="'layer3' needs blocks3"):
        MmpFrontEnd.check_half(("layer3",), none3)
    # MmpInterface and BatchEvaluator refuse the same in their constructors, before any device is touched
    net = lambda x: x
    MmpInterface(net, stem=stem, blocks=blocks, blocks2=blocks2, blocks3=blocks3, half=("layer3",)).close()
    with pytest.raises(ValueError, match="only layer3 has an f16 kernel"):
        MmpInterface(net, stem=stem, blocks=blocks, blocks2=blocks2, blocks3=blocks3, half=("layer2",))
    with pytest.raises(ValueError, match="'layer3' needs blocks3"):
        MmpInterface(net, stem=stem, blocks=blocks, blocks2=blocks2, half=("layer3",))
    ok = dict(predictor="mmp", network=net, ref_image=np.zeros((4, 5)), transform=snap.WorldTransform(), mmp_stem=stem, mmp_blocks=blocks,
              mmp_blocks2=blocks2)
    with pytest.raises(ValueError, match="only layer3 has an f16 kernel"):
        BatchEvaluator(None, None, None, None, None, None, **dict(ok, mmp_blocks3=blocks3, mmp_half=("layer4",)))
    with pytest.raises(ValueError, match="mmp_half: 'layer3' needs mmp_blocks3"):
        BatchEvaluator(None, None, None, None, None, None, **dict(ok, mmp_half=("layer3",)))
    with pytest.raises(ValueError, match="mmp_half needs predictor = 'mmp'"):
        BatchEvaluator(None, None, None, None, None, None, predictor="cvmp", mmp_half=("layer3",), mmp_blocks3=None)


# ---- 4. the controls of the bound, before any device run -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _figures(c):
    """(|emulate - model| / bound at its worst, {wrong variant: the factor by which it misses the bound}) of a case, computed once."""
    x, spec, want, bound = h3.case("random", *c, _rows(c))
    r = (np.abs(h3.emulate(x, spec) - want) / bound).max()
    factors = {}
    for wrong in ("slope", "halo") + (("phase", "idphase") if c[3] == 2 else ()):
        bad, _ = h3.block(x, spec, wrong=wrong)
        assert bad.shape == want.shape
        factors[wrong] = (np.abs(bad - want) / bound).max()
    return r, factors


@pytest.mark.parametrize("c", ALL, ids=b3.case_id)
def test_the_bound_admits_the_emulation_and_refuses_the_wrong_variants(c):
    """On every case of the GPU tests: ``emulate`` meets the bound, each wrong variant of the float32 reference, run on the rounded
    operands, misses it."""
    H, W, Cin, stride, projection = c
    x, spec, want, bound = h3.case("random", *c, _rows(c))
    assert want.shape == (x.shape[0], 64) + b3.out_plane(H, W, stride) and (bound > 0).all()
    r, factors = _figures(c)
    print(f"{b3.case_id(c)}: emulate {r:.4f}" + "".join(f", {k} x {v:.0f}" for k, v in factors.items()))
    assert r <= 1.0, "the bound refuses a correct implementation of the rule"
    assert all(v > 1.0 for v in factors.values()), "the bound admits a wrong variant"
    # the rule costs something: on random data the model's value is not the float32 reference's
    assert not np.array_equal(want, b3.case("random", *c, _rows(c))[2])


def test_the_recorded_margins_hold_over_all_cases():
    """``emulate`` at most 0.21 of the bound; every wrong variant at least 28 times over it."""
    figs = {c: _figures(c) for c in ALL}
    worst = max(figs, key=lambda c: figs[c][0])
    least = min(((v, k, c) for c in ALL for k, v in figs[c][1].items()), key=lambda t: t[0])
    print(f"emulate at most {figs[worst][0]:.4f} of the bound ({b3.case_id(worst)}); wrong variants at least x {least[0]:.1f} ({least[1]}, {b3.case_id(least[2])})")
    assert figs[worst][0] <= 0.215 and least[0] >= 28.0


@pytest.mark.parametrize("c", ALL, ids=b3.case_id)
def test_integer_cases_are_binary16_values_throughout(c):
    """Every operand and every m of the integer cases is a binary16 value, |m| <= 133: the rule rounds nothing on them, so the model
    equals the float32 reference, and ``emulate`` gives that reference's bits."""
    import torch
    import torch.nn.functional as F
    x, spec, want, _ = b3.case("integer", *c, _rows(c))
    is_h = lambda a: np.array_equal(np.asarray(a, dtype=np.float64), round_f16(a).astype(np.float64))
    assert is_h(x) and is_h(spec.w1) and is_h(spec.w2) and (spec.wd is None or is_h(spec.wd))
    xt, w1, s1, b1, _, _, _ = b3._parts(x, spec)
    m = F.leaky_relu(s1 * F.conv2d(xt, w1, stride=int(spec.stride), padding=1) + b1, float(spec.slope_mid)).numpy()
    assert is_h(m) and np.abs(m).max() <= 133
    model, _ = h3.block(x, spec)
    assert np.array_equal(model, want) and np.array_equal(h3.block(x, spec, round_m=True)[0], want)
    assert np.array_equal(h3.emulate(x, spec), want.astype(np.float32))


def test_the_exact_blocks_under_the_rule():
    x = round_f16(np.abs(b3.random_x(2, 64, 8, 22, seed=5))).astype(np.float32)
    assert np.array_equal(h3.emulate(x, b3.doubling_block3()), x + x) and np.array_equal(h3.block(x, b3.doubling_block3())[0], x + x)
    x = round_f16(np.abs(b3.random_x(2, 32, 15, 43, seed=6))).astype(np.float32)
    half = x[:, :, ::2, ::2]
    assert np.array_equal(h3.emulate(x, b3.duplicate_and_double_block3()), np.concatenate([half + half, half + half], axis=1))


def test_the_bound_covers_inputs_that_saturate():
    """|x| up to 1e5, a twentieth of the values beyond +-65504: x saturates, and here and there m does too. The model clips both
    (saturation is the rule, not an error of it), and ``emulate`` stays within the bound: at most 0.15 of it."""
    for c in [(15, 43, 32, 2, True), (8, 22, 64, 1, False), (8, 22, 24, 1, True)]:
        x, spec, _, _ = b3.case("random", *c)
        rng = np.random.default_rng(17)
        x = x.copy()
        big = rng.random(x.shape) < 0.05
        x[big] = (rng.uniform(6e4, 1e5, x.shape) * rng.choice([-1.0, 1.0], x.shape)).astype(np.float32)[big]
        want, bound = h3.block(x, spec)
        got = h3.emulate(x, spec)
        assert np.isfinite(got).all() and (np.abs(got - want) / bound).max() <= 1.0
