"""CPU tests of the fused 128-channel residual block's host side: ``mmp_stem.fold_block4`` / ``split_network_layer4`` /
``split_network_whole`` against block-shaped torch modules run in float64 (the stand-ins of tests/test_mmp_block2_cpu.py at 128
channels), every refusal, the layout of the argument struct against the C compiler, the resources of the shipped kernels, and the
controls of the float64 restatement's bound (tests/mmp_block4_reference.py) before any device run."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import dyobav_mpcnwta_warehouse_amd as nm
import mmp_block2_reference as b2
import mmp_block3_reference as b3
import mmp_block4_reference as b4
import mmp_block_reference as br
import mmp_head_reference as hr
import mmp_stem_reference as sr
from dyobav_mpcnwta_warehouse_amd import _capi
from dyobav_mpcnwta_warehouse_amd.mmp_front import MmpFrontEnd
from dyobav_mpcnwta_warehouse_amd.mmp_stem import (BLOCK4_CHANNELS, Block4Spec, HeadSpec, check_block4, check_blocks, check_blocks2, check_blocks3,
                                                   check_blocks4, fold_block4, fold_doubles, split_network_layer3, split_network_layer4,
                                                   split_network_whole)
from test_mmp_block2_cpu import ROOT, _Block, _module_in_double, _randomise
from test_mmp_block3_cpu import _Net3


def _block(Cin, stride, projection, **kw):
    return _Block(Cin, stride, projection, Cout=128, **kw)


def _exact_spec(blk):
    """The fold in doubles, before the one rounding to float."""
    d1, d2 = fold_doubles(blk.conv1[0], blk.conv1[1]), fold_doubles(blk.conv2[0], blk.conv2[1])
    dd = fold_doubles(blk.downsample[0], blk.downsample[1]) if blk.downsample is not None else (None, None, None)
    return Block4Spec(*d1, 0.1, *d2, None if dd[0] is None else dd[0].reshape(128, -1), dd[1], dd[2], 0.01, int(blk.conv1[0].stride[0]))


# ---- 1. the fold: the restatement on the folded block equals the module in float64 ---------------------------------------------------
@pytest.mark.parametrize("Cin,stride,projection,bias", [(128, 1, False, False), (64, 2, True, False), (256, 1, True, False), (8, 2, True, True)],
                         ids=["identity", "strided", "projection", "strided-bias"])
def test_fold_equals_the_module_in_float64(Cin, stride, projection, bias):
    blk = _randomise(_block(Cin, stride, projection, bias=bias), seed=Cin + stride).eval()
    spec = fold_block4(blk)
    assert isinstance(spec, Block4Spec) and (spec.wd is not None) == projection
    assert spec.slope_mid == pytest.approx(0.1) and spec.slope_out == pytest.approx(0.01)
    assert spec.stride == stride and type(spec.stride) is int
    assert (spec.s1 < 0).any() and (spec.s1 > 0).any() and np.abs(spec.b1).min() > 0
    assert all(v.dtype == np.float32 and v.flags.c_contiguous for v in spec if isinstance(v, np.ndarray))
    assert spec.w1.shape == (128, Cin, 3, 3) and spec.w2.shape == (128, 128, 3, 3) and (not projection or spec.wd.shape == (128, Cin))
    for H, W in ((5, 7), (6, 8)):                           # both parities
        x = br.random_x(2, Cin, H, W, seed=3)
        want = _module_in_double(blk, x)
        exact = _exact_spec(blk)
        got, bound = b4.block(x, exact)
        print(f"Cin = {Cin}, stride {stride}, {H} x {W}: largest |restatement - module| = {np.abs(got - want).max():.2e}")
        assert got.shape == want.shape == (2, 128) + b4.out_plane(H, W, stride) and np.abs(got - want).max() <= 1e-12
    for a, b in zip(spec, exact):                           # fold_block4 is the same numbers, rounded once
        if isinstance(a, np.ndarray):
            assert np.array_equal(a, np.asarray(b).astype(np.float32))
    assert check_block4(spec).w1.flags.c_contiguous and check_block4(spec).stride == stride


# ---- 2. what fold_block4, check_block4, check_blocks4 and check_specs refuse -----------------------------------------------------------------
def test_fold_refuses_what_the_kernel_does_not_compute():
    nn = torch.nn
    good = lambda **kw: _block(kw.pop("Cin", 128), kw.pop("stride", 1), kw.pop("projection", False), **kw).eval()
    fold_block4(good())
    fold_block4(good(Cin=64, stride=2, projection=True))

    def with_(attr, value, **kw):
        b = good(**kw)
        setattr(b, attr, value)
        return b
    bn = lambda: nn.BatchNorm2d(128).eval()
    strided = dict(Cin=64, stride=2, projection=True)
    cases = [
        ("mismatched strides", with_("downsample", nn.Sequential(nn.Conv2d(64, 128, 1, 1), bn()), **strided)),
        ("stride 2 without 'downsample'", with_("downsample", None, Cin=128, stride=2, projection=True)),
        ("'conv2' must have stride 1", with_("conv2", nn.Sequential(nn.Conv2d(128, 128, 3, 2, 1), bn()))),
        ("stride 1 or 2", with_("conv1", nn.Sequential(nn.Conv2d(128, 128, 3, 3, 1), bn(), nn.LeakyReLU(0.1)))),
        ("padding 1", with_("conv1", nn.Sequential(nn.Conv2d(128, 128, 3, 1, 0), bn(), nn.LeakyReLU(0.1)))),
        ("padding 0", with_("downsample", nn.Sequential(nn.Conv2d(64, 128, 1, 2, 1), bn()), **strided)),
        ("dilation 1", with_("conv2", nn.Sequential(nn.Conv2d(128, 128, 3, 1, 1, dilation=2), bn()))),
        ("groups 1", with_("conv2", nn.Sequential(nn.Conv2d(128, 128, 3, 1, 1, groups=2), bn()))),
        ("zero padding", with_("conv1", nn.Sequential(nn.Conv2d(128, 128, 3, 1, 1, padding_mode="reflect"), bn(), nn.LeakyReLU(0.1)))),
        ("kernel 3", with_("conv2", nn.Sequential(nn.Conv2d(128, 128, 5, 1, 2), bn()))),
        ("kernel 1", with_("downsample", nn.Sequential(nn.Conv2d(64, 128, 3, 2, 1), bn()), **strided)),
        ("eval", with_("conv2", nn.Sequential(nn.Conv2d(128, 128, 3, 1, 1), nn.BatchNorm2d(128).train()))),
        ("128 output channels", with_("conv1", nn.Sequential(nn.Conv2d(128, 64, 3, 1, 1), nn.BatchNorm2d(64).eval(), nn.LeakyReLU(0.1)))),
        ("128 output channels", _Block(64, 1, False, Cout=64).eval()),                                                # a block of layer3
        ("multiple of 8", with_("conv1", nn.Sequential(nn.Conv2d(12, 128, 3, 1, 1), bn(), nn.LeakyReLU(0.1)))),
        ("no identity", with_("downsample", None, Cin=256, projection=True)),
        ("LeakyReLU", with_("leaky", nn.ReLU())),
        ("slope", with_("leaky", nn.LeakyReLU(1.5))),
        ("Sequential", with_("conv1", nn.Conv2d(128, 128, 3, 1, 1))),
    ]
    for match, blk in cases:
        with pytest.raises(ValueError, match="fold_block4: .*" + match):
            fold_block4(blk.eval() if match != "eval" else blk)
    with pytest.raises(ValueError, match="fold_block4: the module has no 'conv1'"):
        fold_block4(nn.Linear(3, 3))
    ok, strd = b4.random_block4(128, 1, 1, False), b4.random_block4(64, 1, 2, True)
    assert check_block4(strd).stride == 2 and isinstance(check_block4(strd), Block4Spec)
    for bad in (ok._replace(s1=np.zeros(4)), ok._replace(w1=np.zeros((128, 12, 3, 3))), ok._replace(w2=np.zeros((128, 8, 3, 3))),
                ok._replace(wd=np.zeros((128, 128))), ok._replace(w1=np.zeros((128, 64, 3, 3))), ok._replace(slope_mid=float("nan")),
                ok._replace(slope_out=2.0), b4.random_block4(256, 1, 1, True)._replace(sd=None), ok._replace(stride=2), ok._replace(stride=0),
                strd._replace(stride=3), ok._replace(w1=np.zeros((64, 128, 3, 3))), b3.random_block3(64, 1, 1, False)):
        with pytest.raises(ValueError, match="Block4Spec"):
            check_block4(bad)
    blocks = check_blocks(sr.delta_spec(16), [br.doubling_block()])
    blocks2 = check_blocks2(blocks, [b2.duplicate_and_double_block2(16)])
    blocks3 = check_blocks3(blocks2, [b3.duplicate_and_double_block3(32)])
    assert len(check_blocks4(blocks3, [strd, ok, ok])) == 3 and BLOCK4_CHANNELS == 128
    with pytest.raises(ValueError, match="mmp_blocks4: block 0 takes 128 channels, but 64 arrive \\(layer3 gives 64\\)"):
        check_blocks4(blocks3, [ok])
    with pytest.raises(ValueError, match="mmp_blocks4: block 1 takes 64 channels, but 128 arrive \\(every block of layer4 gives 128\\)"):
        check_blocks4(blocks3, [strd, strd])
    with pytest.raises(ValueError, match="mmp_blocks4: at least one"):
        check_blocks4(blocks3, [])
    with pytest.raises(ValueError, match="mmp_blocks4: the blocks of layer3 are needed"):
        check_blocks4((), [strd])
    # the front end's one place for these refusals, with its old two-, three- and four-value forms intact
    stem, head = sr.delta_spec(16), hr.random_head(128, 2, 2, 10, 1)
    assert len(MmpFrontEnd.check_specs(stem, blocks)) == 2 and len(MmpFrontEnd.check_specs(stem, blocks, blocks2=blocks2)) == 3
    assert len(MmpFrontEnd.check_specs(stem, blocks, blocks2=blocks2, blocks3=blocks3)) == 4
    assert MmpFrontEnd.check_specs(None, None, blocks4=None) == (None,) * 5 and MmpFrontEnd.check_specs(None, None, head=None) == (None,) * 6
    five = MmpFrontEnd.check_specs(stem, blocks, blocks2=blocks2, blocks3=blocks3, blocks4=[strd, ok])
    assert len(five) == 5 and len(five[3]) == 1 and len(five[4]) == 2
    six = MmpFrontEnd.check_specs(stem, blocks, blocks2=blocks2, blocks3=blocks3, blocks4=[strd], head=head)
    assert len(six) == 6 and isinstance(six[5], HeadSpec) and six[5].w2.shape == (10, 128)
    with pytest.raises(ValueError, match="mmp_blocks4 needs mmp_blocks3 "):
        MmpFrontEnd.check_specs(stem, blocks, prefix="mmp_", blocks2=blocks2, blocks4=[strd])
    with pytest.raises(ValueError, match="mmp_head needs mmp_blocks4 "):
        MmpFrontEnd.check_specs(stem, blocks, prefix="mmp_", blocks2=blocks2, blocks3=blocks3, head=head)
    with pytest.raises(ValueError, match="blocks3 needs blocks2 "):
        MmpFrontEnd.check_specs(stem, blocks, blocks3=blocks3, blocks4=[strd])
    with pytest.raises(ValueError, match="block 0 takes 128 channels"):
        MmpFrontEnd.check_specs(stem, blocks, blocks2=blocks2, blocks3=blocks3, blocks4=[ok])
    with pytest.raises(ValueError, match="HeadSpec"):
        MmpFrontEnd.check_specs(stem, blocks, blocks2=blocks2, blocks3=blocks3, blocks4=[strd], head=head._replace(c1=np.zeros(3)))


# ---- 3. the splits ----------------------------------------------------------------------------------------------------------------------------
class _Swarm(torch.nn.Module):
    """The attribute name of the reference's swarm head."""
    def __init__(self, K):
        super().__init__()
        self.layer_hypos = torch.nn.Linear(128, 2 * K)

    def forward(self, x):
        return self.layer_hypos(x)


class _Net4(_Net3):
    """The small stand-in net of the layer3 tests with a ``layer4`` of residual blocks at 128 channels, the 2 x 2 average pool and
    the two linear layers behind it; for a 40 x 56 map: 10 x 14 -> 5 x 7 -> 3 x 4 -> 2 x 2 -> 1 x 1, F = 128."""
    def __init__(self, n_blocks4=3, K=3):
        super().__init__()
        nn = torch.nn
        torch.manual_seed(17)
        self.resnet34.layer4 = nn.Sequential(*[_block(64 if i == 0 else 128, 2 if i == 0 else 1, i == 0) for i in range(n_blocks4)])
        self.resnet34.apool = nn.AvgPool2d(2, 2)
        self.fc1, self.leaky, self.swarm = nn.Linear(128, 128), nn.LeakyReLU(0.01), _Swarm(K)
        _randomise(self, seed=19)


def _stack():
    import mmp_reference as mr
    rng = np.random.default_rng(0)
    ref = np.where(rng.random((40, 56)) < 0.3, 0.0, 255.0).astype(np.float32)
    return mr.input_stack(mr.input_planes(np.array([[13.25, 14.5], [15.0, 16.75], [17.5, 18.0]]), ref), 2)


def _restated(stack, spec, blocks, blocks2, blocks3, blocks4):
    y, _ = sr.stem(stack, spec.weight, spec.scale, spec.shift, spec.slope)
    for mod, bs in ((br, blocks), (b2, blocks2), (b3, blocks3), (b4, blocks4)):
        for b in bs:
            y, _ = mod.block(y, b)
    return y


def test_split_network_layer4_gives_blocks_and_a_trunk_that_completes_them():
    net = _Net4().eval()
    spec, blocks, blocks2, blocks3, blocks4, trunk = split_network_layer4(net)
    assert len(blocks) == 3 and len(blocks2) == 4 and len(blocks3) == 6 and len(blocks4) == 3
    assert [b.stride for b in blocks4] == [2, 1, 1] and blocks4[0].wd.shape == (128, 64) and all(b.wd is None for b in blocks4[1:])
    assert all(isinstance(b, Block4Spec) for b in blocks4)
    three = split_network_layer3(net)[:4]
    assert all(np.array_equal(a.w1, b.w1) for a, b in zip(three[3], blocks3))
    stack = _stack()
    with torch.no_grad():
        want = net(torch.from_numpy(stack))
        y = _restated(stack, spec, blocks, blocks2, blocks3, blocks4)
        assert y.shape == (2, 128, 2, 2)
        got = trunk(torch.from_numpy(y.astype(np.float32)))
    assert got.shape == want.shape == (2, 6) and torch.allclose(got, want, rtol=1e-4, atol=1e-4)
    for fn in (split_network_layer4, split_network_whole):
        with pytest.raises(ValueError, match=fn.__name__ + ": .*three blocks"):
            fn(_Net4(n_blocks4=2).eval())
        with pytest.raises(ValueError, match="three blocks"):
            fn(_Net3().eval())                                  # (layer4 is a single convolution there)
        with pytest.raises(ValueError, match="eval"):
            fn(_Net4().train())
        with pytest.raises(ValueError, match="resnet34"):
            fn(torch.nn.Linear(3, 3))


def test_split_network_whole_equals_the_module_in_float64():
    """The restatements of every stage on the folded float32 weights against the module's own forward in float64: they differ by
    the one rounding of every folded weight to float32 (2^-24 relative each, through 17 layers), so 1e-4 as for the split of
    layer3 -- the bound of each stage against ITS restatement is the business of the GPU tests."""
    net = _Net4().eval()
    spec, blocks, blocks2, blocks3, blocks4, head = split_network_whole(net)
    assert isinstance(head, HeadSpec) and head.w1.shape == (128, 128) and head.w2.shape == (6, 128) and head.slope == pytest.approx(0.01)
    stack = _stack()
    want = _module_in_double(net, stack)
    got, _ = hr.head(_restated(stack, spec, blocks, blocks2, blocks3, blocks4), head)
    print(f"largest |whole restated network - module in float64| = {np.abs(got - want).max():.2e} at |out| up to {np.abs(want).max():.2e}")
    assert got.shape == want.shape == (2, 6) and np.allclose(got, want, rtol=1e-4, atol=1e-4)


# ---- 4. the struct and the symbol: no device needed -------------------------------------------------------------------------------------------
def test_block4_entry_point_refuses_null_arguments():
    lib = nm.load_library()
    assert "nmpc_mmp_block4_f32" in nm.EXPORTED_SYMBOLS and hasattr(lib, "nmpc_mmp_block4_f32")
    a = _capi.NmpcMmpBlock4Args()
    assert lib.nmpc_mmp_block4_f32(None, ctypes.byref(a)) == -1 and lib.nmpc_mmp_block4_f32(None, None) == -1


def test_block4_args_layout_matches_the_c_compiler():
    fields = [f[0] for f in _capi.NmpcMmpBlock4Args._fields_]
    assert fields == [f[0] for f in _capi.NmpcMmpBlock3Args._fields_]
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "sz.c")
        body = "".join(f'printf(" %zu", offsetof(nmpc_mmp_block4_args, {f}));' for f in fields)
        body += "".join(f'printf(" %zu", offsetof(nmpc_mmp_block3_args, {f}));' for f in fields)
        open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "nmpc_hip.h"\nint main(void){printf("%zu", sizeof(nmpc_mmp_block4_args));'
                             + body + 'printf(" %zu %d", sizeof(nmpc_mmp_block3_args), NMPC_ABI_VERSION);return 0;}\n')
        exe = os.path.join(td, "sz")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    n = len(fields)
    assert ctypes.sizeof(_capi.NmpcMmpBlock4Args) == out[0] == 120
    assert [getattr(_capi.NmpcMmpBlock4Args, f).offset for f in fields] == out[1:1 + n] == out[1 + n:1 + 2 * n]
    assert out[-2] == ctypes.sizeof(_capi.NmpcMmpBlock3Args) == 120 and out[-1] == 5      # nothing that existed changed


def test_block4_kernels_use_no_scratch_and_fit_one_workgroup_of_eight_waves_per_cu():
    """Read from the shipped code object: exactly three kernels (stride 2; stride 1 with and without the projection) without VGPR
    or SGPR spills or scratch, within the 256 registers of two wavefronts per SIMD, with the 90 112 B of LDS the header states
    (128 slots of 176 words: one workgroup in a CU's 160 KB, two do not fit): the occupancy of its __launch_bounds__(512, 1)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    nm.build_library()
    res = {kernel_resources.short_name(k): v for k, v in kernel_resources.kernel_resources(nm.library_path()).items()}
    mine = {k: v for k, v in res.items() if re.search(r"mmp_blkf_kernel<nmpc::MmpBlock4Geom, ", k)}
    assert len(mine) == 3, sorted(mine)
    header = open(os.path.join(ROOT, "dyobav-mpcnwta-warehouse_amd", "csrc", "nmpc_mmp_block4.h")).read()
    shared = open(os.path.join(ROOT, "dyobav-mpcnwta-warehouse_amd", "csrc", "nmpc_mmp_block_f32.h")).read()
    assert "__launch_bounds__(G::Threads, G::min_wg)" in shared and "Threads = kB4Threads, min_wg = 1," in header and "kB4Threads = 512" in header
    assert "constexpr int CC = G::cc(STRIDE);" in shared
    assert f"kB4MH = {b4.TILE[0]}, kB4MW = {b4.TILE[1]}" in header and "cc(int stride) { return stride == 2 ? 16 : 32; }" in header and b4.CHUNK == {1: 32, 2: 16}
    for name, r in mine.items():
        print(name, r)
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
        assert r["vgpr"] + max(r["agpr"], 0) <= 256 and r["lds_static"] == 128 * 176 * 4 == 90112, (name, r)
        assert 80 * 1024 < r["lds_static"] <= 160 * 1024, (name, r)


# ---- 5. the controls of the bound, before any device run ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", b4.CASES + b4.REAL, ids=b4.case_id)
def test_the_bound_admits_float32_and_refuses_the_wrong_variants(c):
    """On every case of the GPU tests: torch's own float32 block meets the bound, each wrong variant misses it ("phase" and
    "idphase" exist at stride 2 only; no plane had to be excluded). Recorded here: torch's float32 at most 0.0010 of the bound;
    the smallest factor by which a wrong variant misses it -- "slope" 13 (4 x 6, Cin 256), "halo" 54 (11 x 12, Cin 256), "phase" 306
    and "idphase" 931 (both 20 x 22, Cin 64). The factors fall with Cin because the bound grows with the number of terms,
    c(9 Cin) and c(1152), while a wrong slope or ring stays one error of the size of a value."""
    H, W, Cin, stride, projection = c
    x, spec, want, bound = b4.case("random", *c, 2 if c in b4.REAL else b4.M_MAX)
    assert want.shape == (x.shape[0], 128) + b4.out_plane(H, W, stride) and (bound > 0).all()
    r32 = (np.abs(b4.torch_float32(x, spec) - want) / bound).max()
    line = f"{b4.case_id(c)}: torch float32 {r32:.4f}"
    assert r32 <= 1.0, "the bound refuses torch's own float32 block"
    for wrong in ("slope", "halo") + (("phase", "idphase") if stride == 2 else ()):
        bad, _ = b4.block(x, spec, wrong=wrong)
        factor = (np.abs(bad - want) / bound).max()
        line += f", {wrong} x {factor:.0f}"
        assert bad.shape == want.shape and factor > 1.0, f"the bound admits the wrong variant {wrong!r}"
    print(line)
    if stride == 1:
        with pytest.raises(ValueError, match="stride 2 only"):
            b4.block(x[:1], spec, wrong="phase")
    # the integer block of the exact GPU test: nothing can round, and torch's float32 is exact on it as well
    xi, si, wi, _ = b4.case("integer", *c, 2 if c in b4.REAL else b4.M_MAX)
    assert b4.integer_units(xi, si) < 2.0 ** 24
    assert np.array_equal(wi.astype(np.float32).astype(np.float64), wi) and np.array_equal(b4.torch_float32(xi, si), wi.astype(np.float32))


def test_the_cases_are_named_from_the_tile():
    TH, TW = b4.TILE
    assert b4.PLANES[1][2:4] == ((TH, TW), (TH + 1, TW + 1)) and b4.PLANES[2][2:4] == ((2 * TH, 2 * TW), (2 * TH + 1, 2 * TW + 1))
    assert b4.out_plane(*b4.PLANES[2][2], 2) == (TH, TW) and b4.out_plane(*b4.PLANES[2][3], 2) == (TH + 1, TW + 1)
    assert b4.out_plane(*b4.PLANES[2][4], 2) == b4.PLANES[1][4] and b4.PLANES[1][4][0] > 3 * (TH - 2) and b4.PLANES[1][4][1] < TW
    assert {c[0] for c in b4.CHANNELS} == {8, 64, 128, 256, b4.CHUNK[1] * 3 // 2} and b4.REAL == ((19, 21, 64, 2, True), (10, 11, 128, 1, False))


def test_the_exact_blocks_of_the_loop_test():
    x = np.abs(br.random_x(2, 64, 7, 10, seed=5))
    half = x[:, :, ::2, ::2]
    got, _ = b4.block(x, b4.duplicate_and_double_block4(64))
    assert np.array_equal(got, np.concatenate([half + half, half + half], axis=1))
    got2, _ = b4.block(got, b4.doubling_block4())
    assert np.array_equal(got2, got + got)
    check_blocks4((b3.doubling_block3(),), (b4.duplicate_and_double_block4(64),) + (b4.doubling_block4(),) * 2)
