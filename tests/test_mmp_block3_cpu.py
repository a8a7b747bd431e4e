"""CPU tests of the fused 64-channel residual block's host side: ``mmp_stem.fold_block3`` / ``split_network_layer3`` against
block-shaped torch modules run in float64 (the stand-ins of tests/test_mmp_block2_cpu.py at 64 channels, and the reference's own
``BasicBlock`` / ``make_layer(..., stride=2)`` where its tree is present), every refusal, the layout of the argument struct against
the C compiler, the resources of the shipped kernels, and the controls of the float64 restatement's bound
(tests/mmp_block3_reference.py) before any device run."""
import ctypes
import importlib
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import dyobav_mpcnwta_warehouse_amd as nm
import mmp_block2_reference as b2
import mmp_block3_reference as b3
import mmp_block_reference as br
import mmp_stem_reference as sr
from dyobav_mpcnwta_warehouse_amd import _capi
from dyobav_mpcnwta_warehouse_amd.mmp_front import MmpFrontEnd
from dyobav_mpcnwta_warehouse_amd.mmp_stem import (BLOCK3_CHANNELS, Block3Spec, check_block3, check_blocks, check_blocks2, check_blocks3,
                                                   fold_block3, fold_doubles, split_network_layer3)
from test_mmp_block2_cpu import REFERENCE_SRC, ROOT, _Block, _module_in_double, _Net, _randomise


def _block(Cin, stride, projection, **kw):
    return _Block(Cin, stride, projection, Cout=64, **kw)


def _exact_spec(blk):
    """The fold in doubles, before the one rounding to float."""
    d1, d2 = fold_doubles(blk.conv1[0], blk.conv1[1]), fold_doubles(blk.conv2[0], blk.conv2[1])
    dd = fold_doubles(blk.downsample[0], blk.downsample[1]) if blk.downsample is not None else (None, None, None)
    return Block3Spec(*d1, 0.1, *d2, None if dd[0] is None else dd[0].reshape(64, -1), dd[1], dd[2], 0.01, int(blk.conv1[0].stride[0]))


# ---- 1. the fold: the restatement on the folded block equals the module in float64 ---------------------------------------------------
@pytest.mark.parametrize("Cin,stride,projection,bias", [(64, 1, False, False), (32, 2, True, False), (128, 1, True, False), (8, 2, True, True),
                                                        (64, 2, True, False)], ids=["identity", "strided", "projection", "strided-bias", "strided-64"])
def test_fold_equals_the_module_in_float64(Cin, stride, projection, bias):
    blk = _randomise(_block(Cin, stride, projection, bias=bias), seed=Cin + stride).eval()
    spec = fold_block3(blk)
    assert isinstance(spec, Block3Spec) and (spec.wd is not None) == projection
    assert spec.slope_mid == pytest.approx(0.1) and spec.slope_out == pytest.approx(0.01)
    assert spec.stride == stride and type(spec.stride) is int
    assert (spec.s1 < 0).any() and (spec.s1 > 0).any() and np.abs(spec.b1).min() > 0
    assert all(v.dtype == np.float32 and v.flags.c_contiguous for v in spec if isinstance(v, np.ndarray))
    assert spec.w1.shape == (64, Cin, 3, 3) and spec.w2.shape == (64, 64, 3, 3) and (not projection or spec.wd.shape == (64, Cin))
    for H, W in ((9, 11), (10, 12)):                        # both parities
        x = br.random_x(2, Cin, H, W, seed=3)
        want = _module_in_double(blk, x)
        exact = _exact_spec(blk)
        got, bound = b3.block(x, exact)
        print(f"Cin = {Cin}, stride {stride}, {H} x {W}: largest |restatement - module| = {np.abs(got - want).max():.2e}")
        assert got.shape == want.shape == (2, 64) + b3.out_plane(H, W, stride) and np.abs(got - want).max() <= 1e-12
    # and fold_block3 is the same numbers, rounded once
    for a, b in zip(spec, exact):
        if isinstance(a, np.ndarray):
            assert np.array_equal(a, np.asarray(b).astype(np.float32))
    assert check_block3(spec).w1.flags.c_contiguous and check_block3(spec).stride == stride


# ---- 2. the reference's own layer3, where its tree is present ---------------------------------------------------------------------------
def test_fold_equals_the_reference_layer3():
    if not os.path.isdir(os.path.join(REFERENCE_SRC, "pkg_motion_prediction", "net_module")):
        pytest.skip("the reference tree is not present")
    sys.path.insert(0, REFERENCE_SRC)
    try:
        net = importlib.import_module("pkg_motion_prediction.net_module.net")
    except ImportError as e:                                # (a dependency of the reference that is not installed)
        pytest.skip(f"the reference's net module does not import: {e}")
    finally:
        sys.path.remove(REFERENCE_SRC)
    layer3 = _randomise(net.make_layer(net.BasicBlock, 32, 64, 6, stride=2), seed=7).eval()
    x = br.random_x(2, 32, 10, 13, seed=4)
    want = _module_in_double(layer3, x)
    y = x.astype(np.float64)
    specs = [fold_block3(blk) for blk in layer3]
    for blk, spec in zip(layer3, specs):
        assert spec.slope_mid == pytest.approx(0.1) and spec.slope_out == pytest.approx(0.01)
        y, _ = b3.block(y, _exact_spec(blk))
    assert [s.stride for s in specs] == [2, 1, 1, 1, 1, 1] and specs[0].wd is not None and all(s.wd is None for s in specs[1:])
    assert len(check_blocks3((b2.doubling_block2(),), specs)) == 6
    print(f"largest |six folded blocks - the reference's layer3| = {np.abs(y - want).max():.2e}")
    assert y.shape == want.shape == (2, 64, 5, 7) and np.abs(y - want).max() <= 1e-12


# ---- 3. what fold_block3, check_block3, check_blocks3 and check_specs refuse ----------------------------------------------------------------
def test_fold_refuses_what_the_kernel_does_not_compute():
    nn = torch.nn
    good = lambda **kw: _block(kw.pop("Cin", 64), kw.pop("stride", 1), kw.pop("projection", False), **kw).eval()
    fold_block3(good())
    fold_block3(good(Cin=32, stride=2, projection=True))

    def with_(attr, value, **kw):
        b = good(**kw)
        setattr(b, attr, value)
        return b
    bn = lambda: nn.BatchNorm2d(64).eval()
    strided = dict(Cin=32, stride=2, projection=True)
    cases = [
        ("mismatched strides", with_("downsample", nn.Sequential(nn.Conv2d(32, 64, 1, 1), bn()), **strided)),
        ("mismatched strides", with_("downsample", nn.Sequential(nn.Conv2d(128, 64, 1, 2), bn()), Cin=128, projection=True)),
        ("stride 2 without 'downsample'", with_("downsample", None, Cin=64, stride=2, projection=True)),
        ("'conv2' must have stride 1", with_("conv2", nn.Sequential(nn.Conv2d(64, 64, 3, 2, 1), bn()))),
        ("stride 1 or 2", with_("conv1", nn.Sequential(nn.Conv2d(64, 64, 3, 3, 1), bn(), nn.LeakyReLU(0.1)))),
        ("stride 1 or 2", with_("conv1", nn.Sequential(nn.Conv2d(64, 64, 3, (1, 2), 1), bn(), nn.LeakyReLU(0.1)))),
        ("padding 1", with_("conv1", nn.Sequential(nn.Conv2d(64, 64, 3, 1, 0), bn(), nn.LeakyReLU(0.1)))),
        ("padding 0", with_("downsample", nn.Sequential(nn.Conv2d(32, 64, 1, 2, 1), bn()), **strided)),
        ("dilation 1", with_("conv2", nn.Sequential(nn.Conv2d(64, 64, 3, 1, 1, dilation=2), bn()))),
        ("groups 1", with_("conv2", nn.Sequential(nn.Conv2d(64, 64, 3, 1, 1, groups=2), bn()))),
        ("zero padding", with_("conv1", nn.Sequential(nn.Conv2d(64, 64, 3, 1, 1, padding_mode="reflect"), bn(), nn.LeakyReLU(0.1)))),
        ("kernel 3", with_("conv2", nn.Sequential(nn.Conv2d(64, 64, 5, 1, 2), bn()))),
        ("kernel 1", with_("downsample", nn.Sequential(nn.Conv2d(32, 64, 3, 2, 1), bn()), **strided)),
        ("eval", with_("conv2", nn.Sequential(nn.Conv2d(64, 64, 3, 1, 1), nn.BatchNorm2d(64).train()))),
        ("running statistics", with_("conv1", nn.Sequential(nn.Conv2d(64, 64, 3, 1, 1), nn.BatchNorm2d(64, track_running_stats=False).eval(), nn.LeakyReLU(0.1)))),
        ("64 output channels", with_("conv1", nn.Sequential(nn.Conv2d(64, 32, 3, 1, 1), nn.BatchNorm2d(32).eval(), nn.LeakyReLU(0.1)))),
        ("64 output channels", _Block(32, 1, False, Cout=32).eval()),                                                  # a block of layer2
        ("multiple of 8", with_("conv1", nn.Sequential(nn.Conv2d(12, 64, 3, 1, 1), bn(), nn.LeakyReLU(0.1)))),
        ("no identity", with_("downsample", None, Cin=128, projection=True)),
        ("LeakyReLU", with_("leaky", nn.ReLU())),
        ("LeakyReLU", with_("conv1", nn.Sequential(nn.Conv2d(64, 64, 3, 1, 1), bn(), nn.ReLU()))),
        ("slope", with_("leaky", nn.LeakyReLU(float("nan")))),
        ("slope", with_("leaky", nn.LeakyReLU(float("inf")))),
        ("slope", with_("leaky", nn.LeakyReLU(1.5))),
        ("slope", with_("conv1", nn.Sequential(nn.Conv2d(64, 64, 3, 1, 1), bn(), nn.LeakyReLU(-2.0)))),
        ("Sequential", with_("conv2", nn.Sequential(nn.Conv2d(64, 64, 3, 1, 1), bn(), nn.LeakyReLU(0.1)))),          # an activation where none is computed
        ("Sequential", with_("conv1", nn.Conv2d(64, 64, 3, 1, 1))),
    ]
    for match, blk in cases:
        with pytest.raises(ValueError, match="fold_block3: .*" + match):
            fold_block3(blk.eval() if match != "eval" else blk)
    with pytest.raises(ValueError, match="fold_block3: the module has no 'conv1'"):
        fold_block3(nn.Linear(3, 3))
    ok, strd = b3.random_block3(64, 1, 1, False), b3.random_block3(32, 1, 2, True)
    assert check_block3(strd).stride == 2 and isinstance(check_block3(strd), Block3Spec)
    for bad in (ok._replace(s1=np.zeros(4)), ok._replace(w1=np.zeros((64, 12, 3, 3))), ok._replace(w2=np.zeros((64, 8, 3, 3))),
                ok._replace(wd=np.zeros((64, 64))), ok._replace(w1=np.zeros((64, 128, 3, 3))), ok._replace(slope_mid=float("nan")),
                ok._replace(slope_out=2.0), b3.random_block3(128, 1, 1, True)._replace(sd=None), ok._replace(stride=2), ok._replace(stride=0),
                strd._replace(stride=3), strd._replace(stride=1.5), ok._replace(w1=np.zeros((32, 64, 3, 3))), b2.random_block2(32, 1, 1, False)):
        with pytest.raises(ValueError, match="Block3Spec"):
            check_block3(bad)
    blocks = check_blocks(sr.delta_spec(16), [br.doubling_block()])
    blocks2 = check_blocks2(blocks, [b2.duplicate_and_double_block2(16)])
    assert len(check_blocks3(blocks2, [strd, ok, ok, ok, ok, ok])) == 6 and BLOCK3_CHANNELS == 64
    with pytest.raises(ValueError, match="mmp_blocks3: block 0 takes 64 channels, but 32 arrive \\(layer2 gives 32\\)"):
        check_blocks3(blocks2, [ok])
    with pytest.raises(ValueError, match="mmp_blocks3: block 1 takes 32 channels, but 64 arrive \\(every block of layer3 gives 64\\)"):
        check_blocks3(blocks2, [strd, strd])
    with pytest.raises(ValueError, match="mmp_blocks3: at least one"):
        check_blocks3(blocks2, [])
    with pytest.raises(ValueError, match="mmp_blocks3: the blocks of layer2 are needed"):
        check_blocks3((), [strd])
    # the front end's one place for these refusals, with its old two- and three-value forms intact
    stem = sr.delta_spec(16)
    assert len(MmpFrontEnd.check_specs(stem, blocks)) == 2 and MmpFrontEnd.check_specs(None, None) == (None, None)
    assert len(MmpFrontEnd.check_specs(stem, blocks, blocks2=blocks2)) == 3
    assert MmpFrontEnd.check_specs(None, None, blocks3=None) == (None, None, None, None)
    four = MmpFrontEnd.check_specs(stem, blocks, blocks2=blocks2, blocks3=[strd, ok])
    assert len(four) == 4 and len(four[2]) == 1 and len(four[3]) == 2 and MmpFrontEnd.check_specs(stem, blocks, blocks2=blocks2, blocks3=None)[3] is None
    with pytest.raises(ValueError, match="mmp_blocks3 needs mmp_blocks2 "):
        MmpFrontEnd.check_specs(stem, blocks, prefix="mmp_", blocks2=None, blocks3=[strd])
    with pytest.raises(ValueError, match="mmp_blocks3 needs mmp_blocks2 "):
        MmpFrontEnd.check_specs(stem, blocks, prefix="mmp_", blocks3=[strd])
    with pytest.raises(ValueError, match="blocks2 needs blocks "):
        MmpFrontEnd.check_specs(stem, None, blocks2=blocks2, blocks3=[strd])
    with pytest.raises(ValueError, match="block 0 takes 64 channels"):
        MmpFrontEnd.check_specs(stem, blocks, blocks2=blocks2, blocks3=[ok])


# ---- 4. the split ---------------------------------------------------------------------------------------------------------------------------
class _Net3(_Net):
    """The small stand-in net of the layer2 tests with a ``layer3`` of residual blocks at 64 channels behind it."""
    def __init__(self, n_blocks3=6):
        super().__init__()
        nn = torch.nn
        self.resnet34.layer3 = nn.Sequential(*[_block(32 if i == 0 else 64, 2 if i == 0 else 1, i == 0) for i in range(n_blocks3)])
        self.resnet34.layer4 = nn.Conv2d(64, 4, 3, 2, 1)
        _randomise(self, seed=13)


def test_split_network_layer3_gives_stem_blocks_and_a_trunk_that_completes_them():
    import mmp_reference as mr
    net = _Net3().eval()
    spec, blocks, blocks2, blocks3, trunk = split_network_layer3(net)
    assert len(blocks) == 3 and len(blocks2) == 4 and [b.stride for b in blocks2] == [2, 1, 1, 1]
    assert len(blocks3) == 6 and [b.stride for b in blocks3] == [2, 1, 1, 1, 1, 1] and blocks3[0].wd.shape == (64, 32)
    assert all(b.wd is None for b in blocks3[1:]) and all(isinstance(b, Block3Spec) for b in blocks3)
    rng = np.random.default_rng(0)
    ref = np.where(rng.random((24, 31)) < 0.3, 0.0, 255.0).astype(np.float32)
    stack = mr.input_stack(mr.input_planes(np.array([[3.25, 4.5], [5.0, 6.75], [7.5, 8.0]]), ref), 2)
    with torch.no_grad():
        want = net(torch.from_numpy(stack))
        y, _ = sr.stem(stack, spec.weight, spec.scale, spec.shift, spec.slope)
        for b in blocks:
            y, _ = br.block(y, b)
        for b in blocks2:
            y, _ = b2.block(y, b)
        for b in blocks3:
            y, _ = b3.block(y, b)
        assert y.shape == (2, 64, 2, 2)                     # 24 x 31 -> 12 x 16 -> 6 x 8 -> 3 x 4 -> 2 x 2
        got = trunk(torch.from_numpy(y.astype(np.float32)))
    assert got.shape == want.shape == (2, 6) and torch.allclose(got, want, rtol=1e-4, atol=1e-4)
    with pytest.raises(ValueError, match="split_network_layer3: .*six blocks"):
        split_network_layer3(_Net3(n_blocks3=5).eval())
    with pytest.raises(ValueError, match="six blocks"):
        split_network_layer3(_Net().eval())                 # (layer3 is a single convolution there)
    with pytest.raises(ValueError, match="eval"):
        split_network_layer3(_Net3().train())
    with pytest.raises(ValueError, match="resnet34"):
        split_network_layer3(torch.nn.Linear(3, 3))


# ---- 5. the struct and the symbol: no device needed -------------------------------------------------------------------------------------------
def test_block3_entry_point_refuses_null_arguments():
    lib = nm.load_library()
    assert "nmpc_mmp_block3_f32" in nm.EXPORTED_SYMBOLS and hasattr(lib, "nmpc_mmp_block3_f32")
    a = _capi.NmpcMmpBlock3Args()
    assert lib.nmpc_mmp_block3_f32(None, ctypes.byref(a)) == -1 and lib.nmpc_mmp_block3_f32(None, None) == -1


def test_block3_args_layout_matches_the_c_compiler():
    fields = [f[0] for f in _capi.NmpcMmpBlock3Args._fields_]
    assert fields == ["M", "Cin", "H", "W", "x", "w1", "s1", "b1", "w2", "s2", "b2", "wd", "sd", "bd", "slope_mid", "slope_out", "out", "stride"]
    assert [f[0] for f in _capi.NmpcMmpBlock2Args._fields_] == fields and [f[0] for f in _capi.NmpcMmpBlockArgs._fields_] == fields[:-1]
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "sz.c")
        body = "".join(f'printf(" %zu", offsetof(nmpc_mmp_block3_args, {f}));' for f in fields)
        body += "".join(f'printf(" %zu", offsetof(nmpc_mmp_block2_args, {f}));' for f in fields)
        body += "".join(f'printf(" %zu", offsetof(nmpc_mmp_block_args, {f}));' for f in fields[:-1])
        open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "nmpc_hip.h"\nint main(void){printf("%zu", sizeof(nmpc_mmp_block3_args));'
                             + body + 'printf(" %zu %zu %d", sizeof(nmpc_mmp_block2_args), sizeof(nmpc_mmp_block_args), NMPC_ABI_VERSION);return 0;}\n')
        exe = os.path.join(td, "sz")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    n = len(fields)
    assert ctypes.sizeof(_capi.NmpcMmpBlock3Args) == out[0] == 120
    assert [getattr(_capi.NmpcMmpBlock3Args, f).offset for f in fields] == out[1:1 + n]
    assert [getattr(_capi.NmpcMmpBlock2Args, f).offset for f in fields] == out[1 + n:1 + 2 * n]      # nothing that existed changed
    assert [getattr(_capi.NmpcMmpBlockArgs, f).offset for f in fields[:-1]] == out[1 + 2 * n:3 * n]
    assert out[-3] == ctypes.sizeof(_capi.NmpcMmpBlock2Args) == 120 and out[-2] == ctypes.sizeof(_capi.NmpcMmpBlockArgs) == 112 and out[-1] == 5


def test_block3_kernels_use_no_scratch_and_fit_two_workgroups_per_cu():
    """Read from the shipped code object: exactly three kernels (stride 2; stride 1 with and without the projection) without VGPR
    spills or scratch, within the 256 registers of two wavefronts per SIMD, and under 80 KB of LDS (two workgroups in a CU's
    160 KB): the occupancy csrc/nmpc_mmp_block3.h states in its geometry, the kernel's __launch_bounds__(256, 2)."""
    import re
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    nm.build_library()
    res = {kernel_resources.short_name(k): v for k, v in kernel_resources.kernel_resources(nm.library_path()).items()}
    mine = {k: v for k, v in res.items() if re.search(r"mmp_blkf_kernel<nmpc::MmpBlock3Geom, ", k)}
    assert len(mine) == 3, sorted(mine)
    header = open(os.path.join(ROOT, "dyobav-mpcnwta-warehouse_amd", "csrc", "nmpc_mmp_block3.h")).read()
    shared = open(os.path.join(ROOT, "dyobav-mpcnwta-warehouse_amd", "csrc", "nmpc_mmp_block_f32.h")).read()
    assert "__launch_bounds__(G::Threads, G::min_wg)" in shared and "Threads = kB3Threads, min_wg = 2," in header and "kB3Threads = 256" in header
    for name, r in mine.items():
        print(name, r)
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
        assert r["vgpr"] + max(r["agpr"], 0) <= 256 and r["lds_static"] <= 80 * 1024, (name, r)


# ---- 6. the controls of the bound, before any device run ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", b3.CASES + b3.REAL, ids=b3.case_id)
def test_the_bound_admits_float32_and_refuses_the_wrong_variants(c):
    """On every case of the GPU tests: torch's own float32 block meets the bound, each wrong variant misses it ("phase" and
    "idphase" exist at stride 2 only; no plane had to be excluded). Recorded here: torch's float32 at most 0.0018 of the bound;
    the smallest factor by which a wrong variant misses it -- "slope" 38 (7 x 21, Cin 128), "halo" 176 (30 x 7, Cin 128), "phase"
    1 041 and "idphase" 3 463 (both 30 x 7, Cin 32). The factors fall with Cin because the bound grows with the number of terms,
    c(9 Cin) and c(576), while a wrong slope or ring stays one error of the size of a value."""
    H, W, Cin, stride, projection = c
    x, spec, want, bound = b3.case("random", *c, 2 if c in b3.REAL else b3.M_MAX)
    assert want.shape == (x.shape[0], 64) + b3.out_plane(H, W, stride) and (bound > 0).all()
    r32 = (np.abs(b3.torch_float32(x, spec) - want) / bound).max()
    line = f"{b3.case_id(c)}: torch float32 {r32:.4f}"
    assert r32 <= 1.0, "the bound refuses torch's own float32 block"
    for wrong in ("slope", "halo") + (("phase", "idphase") if stride == 2 else ()):
        bad, _ = b3.block(x, spec, wrong=wrong)
        factor = (np.abs(bad - want) / bound).max()
        line += f", {wrong} x {factor:.0f}"
        assert bad.shape == want.shape and factor > 1.0, f"the bound admits the wrong variant {wrong!r}"
    print(line)
    if stride == 1:
        with pytest.raises(ValueError, match="stride 2 only"):
            b3.block(x[:1], spec, wrong="phase")
    # the integer block of the exact GPU test: nothing can round, and torch's float32 is exact on it as well
    xi, si, wi, _ = b3.case("integer", *c, 2 if c in b3.REAL else b3.M_MAX)
    assert b3.integer_units(xi, si) < 2.0 ** 24
    assert np.array_equal(wi.astype(np.float32).astype(np.float64), wi) and np.array_equal(b3.torch_float32(xi, si), wi.astype(np.float32))


def test_the_exact_blocks_of_the_loop_test():
    x = np.abs(br.random_x(2, 32, 7, 10, seed=5))
    half = x[:, :, ::2, ::2]
    got, _ = b3.block(x, b3.duplicate_and_double_block3(32))
    assert np.array_equal(got, np.concatenate([half + half, half + half], axis=1))
    got2, _ = b3.block(got, b3.doubling_block3())
    assert np.array_equal(got2, got + got)
    check_blocks3((b2.doubling_block2(),), (b3.duplicate_and_double_block3(32),) + (b3.doubling_block3(),) * 5)
