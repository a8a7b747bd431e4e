"""CPU tests of the fused residual block's host side: ``mmp_stem.fold_block`` / ``split_network_layer1`` against block-shaped
torch modules run in float64 (written anew here, and the reference's own ``BasicBlock`` where its tree is present), every refusal,
and the layout of the argument struct against the C compiler."""
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
import mmp_block_reference as br
import mmp_stem_reference as sr
from dyobav_mpcnwta_warehouse_amd import _capi
from dyobav_mpcnwta_warehouse_amd.mmp_stem import BlockSpec, check_block, check_blocks, fold_block, split_network_layer1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the reference's ``src`` directory: NMPC_REFERENCE_SRC, or a checkout named ``reference`` next to this repository
REFERENCE_SRC = os.environ.get("NMPC_REFERENCE_SRC") or os.path.join(os.path.dirname(ROOT), "reference", "src")


def _randomise(module, seed):
    """Non-trivial weights, affine parameters of both signs and running statistics for every norm of ``module``."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.Conv2d):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) / (m.weight[0].numel() ** 0.5))
            elif isinstance(m, torch.nn.BatchNorm2d):
                C = m.num_features
                m.weight.copy_(torch.randn(C, generator=g))
                m.bias.copy_(torch.randn(C, generator=g))
                m.running_mean.copy_(torch.randn(C, generator=g) * 3)
                m.running_var.copy_(torch.rand(C, generator=g) * 4 + 0.25)
    return module


class _Block(torch.nn.Module):
    """A module with the attribute names of the reference's BasicBlock at stride 1, written anew."""
    def __init__(self, Cin, projection, slope_mid=0.1, slope_out=0.01, bias=False):
        super().__init__()
        nn = torch.nn
        self.conv1 = nn.Sequential(nn.Conv2d(Cin, 16, 3, 1, 1, bias=bias), nn.BatchNorm2d(16), nn.LeakyReLU(slope_mid))
        self.conv2 = nn.Sequential(nn.Conv2d(16, 16, 3, 1, 1, bias=bias), nn.BatchNorm2d(16))
        self.downsample = nn.Sequential(nn.Conv2d(Cin, 16, 1, 1, bias=bias), nn.BatchNorm2d(16)) if projection else None
        self.leaky = nn.LeakyReLU(slope_out)

    def forward(self, x):
        out = self.conv2(self.conv1(x))
        return self.leaky(out + (x if self.downsample is None else self.downsample(x)))


def _module_in_double(module, x):
    module.double()
    try:
        with torch.no_grad():
            return module(torch.from_numpy(x).double()).numpy()
    finally:
        module.float()


# ---- 1. the fold: the restatement on the folded block equals the module in float64 ---------------------------------------------------
@pytest.mark.parametrize("Cin,projection,bias", [(16, False, False), (64, True, False), (8, True, True)], ids=["identity", "projection", "bias"])
def test_fold_equals_the_module_in_float64(Cin, projection, bias):
    blk = _randomise(_Block(Cin, projection, bias=bias), seed=Cin).eval()
    spec = fold_block(blk)
    assert (spec.wd is not None) == projection and spec.slope_mid == pytest.approx(0.1) and spec.slope_out == pytest.approx(0.01)
    assert (spec.s1 < 0).any() and (spec.s1 > 0).any() and np.abs(spec.b1).min() > 0
    assert all(v.dtype == np.float32 and v.flags.c_contiguous for v in spec if isinstance(v, np.ndarray))
    assert spec.w1.shape == (16, Cin, 3, 3) and spec.w2.shape == (16, 16, 3, 3) and (not projection or spec.wd.shape == (16, Cin))
    x = br.random_x(2, Cin, 9, 11, seed=3)
    want = _module_in_double(blk, x)
    # the fold in doubles, before the one rounding to float: equal to the module to float64 rounding
    from dyobav_mpcnwta_warehouse_amd.mmp_stem import fold_doubles
    d = [fold_doubles(blk.conv1[0], blk.conv1[1]), fold_doubles(blk.conv2[0], blk.conv2[1])]
    dd = fold_doubles(blk.downsample[0], blk.downsample[1]) if projection else (None, None, None)
    exact = BlockSpec(*d[0], 0.1, *d[1], None if dd[0] is None else dd[0].reshape(16, Cin), dd[1], dd[2], 0.01)
    got, bound = br.block(x, exact)
    print(f"Cin = {Cin}: largest |restatement - module| = {np.abs(got - want).max():.2e}")
    assert got.shape == want.shape == (2, 16, 9, 11) and np.abs(got - want).max() <= 1e-12
    # and fold_block is the same numbers, rounded once
    for a, b in zip(spec, exact):
        if isinstance(a, np.ndarray):
            assert np.array_equal(a, np.asarray(b).astype(np.float32))
    assert check_block(spec).w1.flags.c_contiguous


# ---- 2. the reference's own block, where its tree is present -----------------------------------------------------------------------------
def test_fold_equals_the_reference_basic_block():
    if not os.path.isdir(os.path.join(REFERENCE_SRC, "pkg_motion_prediction", "net_module")):
        pytest.skip("the reference tree is not present")
    sys.path.insert(0, REFERENCE_SRC)
    try:
        net = importlib.import_module("pkg_motion_prediction.net_module.net")
    except ImportError as e:                                # (a dependency of the reference that is not installed)
        pytest.skip(f"the reference's net module does not import: {e}")
    finally:
        sys.path.remove(REFERENCE_SRC)
    layer1 = _randomise(net.make_layer(net.BasicBlock, 64, 16, 3), seed=7).eval()
    x = br.random_x(2, 64, 9, 11, seed=4)
    want = _module_in_double(layer1, x)
    y = x.astype(np.float64)
    for blk in layer1:
        spec = fold_block(blk)
        assert spec.slope_mid == pytest.approx(0.1) and spec.slope_out == pytest.approx(0.01)
        from dyobav_mpcnwta_warehouse_amd.mmp_stem import fold_doubles
        d1, d2 = fold_doubles(blk.conv1[0], blk.conv1[1]), fold_doubles(blk.conv2[0], blk.conv2[1])
        dd = fold_doubles(blk.downsample[0], blk.downsample[1]) if blk.downsample is not None else (None, None, None)
        y, _ = br.block(y, BlockSpec(*d1, 0.1, *d2, None if dd[0] is None else dd[0].reshape(16, -1), dd[1], dd[2], 0.01))
    assert fold_block(layer1[0]).wd is not None and fold_block(layer1[1]).wd is None
    print(f"largest |three folded blocks - the reference's layer1| = {np.abs(y - want).max():.2e}")
    assert np.abs(y - want).max() <= 1e-12


# ---- 3. what fold_block and check_block refuse -----------------------------------------------------------------------------------------------
def test_fold_refuses_what_the_kernel_does_not_compute():
    nn = torch.nn
    good = lambda **kw: _Block(kw.pop("Cin", 16), kw.pop("projection", False), **kw).eval()
    fold_block(good())

    def with_(attr, value, **kw):
        b = good(**kw)
        setattr(b, attr, value)
        return b
    bn = lambda: nn.BatchNorm2d(16).eval()
    cases = [
        ("stride 1", with_("conv1", nn.Sequential(nn.Conv2d(16, 16, 3, 2, 1), bn(), nn.LeakyReLU(0.1)))),             # a strided block of layer2-4
        ("padding 1", with_("conv1", nn.Sequential(nn.Conv2d(16, 16, 3, 1, 0), bn(), nn.LeakyReLU(0.1)))),
        ("dilation 1", with_("conv2", nn.Sequential(nn.Conv2d(16, 16, 3, 1, 1, dilation=2), bn()))),
        ("groups 1", with_("conv2", nn.Sequential(nn.Conv2d(16, 16, 3, 1, 1, groups=2), bn()))),
        ("zero padding", with_("conv1", nn.Sequential(nn.Conv2d(16, 16, 3, 1, 1, padding_mode="reflect"), bn(), nn.LeakyReLU(0.1)))),
        ("kernel 3", with_("conv2", nn.Sequential(nn.Conv2d(16, 16, 5, 1, 2), bn()))),
        ("kernel 1", with_("downsample", nn.Sequential(nn.Conv2d(16, 16, 3, 1, 1), bn()))),
        ("stride 1", with_("downsample", nn.Sequential(nn.Conv2d(16, 16, 1, 2), bn()))),
        ("eval", with_("conv2", nn.Sequential(nn.Conv2d(16, 16, 3, 1, 1), nn.BatchNorm2d(16).train()))),
        ("running statistics", with_("conv1", nn.Sequential(nn.Conv2d(16, 16, 3, 1, 1), nn.BatchNorm2d(16, track_running_stats=False).eval(), nn.LeakyReLU(0.1)))),
        ("16 output channels", with_("conv1", nn.Sequential(nn.Conv2d(16, 32, 3, 1, 1), nn.BatchNorm2d(32).eval(), nn.LeakyReLU(0.1)))),
        ("multiple of 8", with_("conv1", nn.Sequential(nn.Conv2d(12, 16, 3, 1, 1), bn(), nn.LeakyReLU(0.1)))),
        ("no identity", with_("downsample", None, Cin=64, projection=True)),
        ("LeakyReLU", with_("leaky", nn.ReLU())),
        ("LeakyReLU", with_("conv1", nn.Sequential(nn.Conv2d(16, 16, 3, 1, 1), bn(), nn.ReLU()))),
        ("slope", with_("leaky", nn.LeakyReLU(float("nan")))),
        ("slope", with_("leaky", nn.LeakyReLU(float("inf")))),
        ("slope", with_("leaky", nn.LeakyReLU(1.5))),
        ("slope", with_("conv1", nn.Sequential(nn.Conv2d(16, 16, 3, 1, 1), bn(), nn.LeakyReLU(-2.0)))),
        ("Sequential", with_("conv2", nn.Sequential(nn.Conv2d(16, 16, 3, 1, 1), bn(), nn.LeakyReLU(0.1)))),          # an activation where none is computed
        ("Sequential", with_("conv1", nn.Conv2d(16, 16, 3, 1, 1))),
    ]
    for match, blk in cases:
        with pytest.raises(ValueError, match=match):
            fold_block(blk.eval() if match != "eval" else blk)
    with pytest.raises(ValueError, match="has no 'conv1'"):
        fold_block(nn.Linear(3, 3))
    ok = br.random_block(16, 1, False)
    for bad in (ok._replace(s1=np.zeros(4)), ok._replace(w1=np.zeros((16, 12, 3, 3))), ok._replace(w2=np.zeros((16, 8, 3, 3))),
                ok._replace(wd=np.zeros((16, 16))), ok._replace(w1=np.zeros((16, 64, 3, 3))), ok._replace(slope_mid=float("nan")),
                ok._replace(slope_out=2.0), br.random_block(64, 1, True)._replace(sd=None)):
        with pytest.raises(ValueError, match="BlockSpec"):
            check_block(bad)
    stem = sr.delta_spec(8)
    assert len(check_blocks(stem, [br.random_block(8, 1, True), ok])) == 2
    with pytest.raises(ValueError, match="block 0 takes 16 channels"):
        check_blocks(stem, [ok])


# ---- 4. the split ---------------------------------------------------------------------------------------------------------------------------
class _Net(torch.nn.Module):
    """A module with the attribute names of the reference's ConvMultiHypoNet(lite=True), written anew and much smaller."""
    def __init__(self, C=8, K=3, n_blocks=3):
        super().__init__()
        nn = torch.nn
        body = nn.Module()
        body.stem = nn.Module()
        body.stem.conv1 = nn.Sequential(nn.Conv2d(7, C, 7, 2, 3, bias=False), nn.BatchNorm2d(C), nn.LeakyReLU(0.1))
        body.stem.pooling = nn.MaxPool2d(3, 2, 1)
        body.layer1 = nn.Sequential(*[_Block(C if i == 0 else 16, i == 0) for i in range(n_blocks)])
        body.layer2, body.layer3 = nn.Conv2d(16, 4, 3, 2, 1), nn.ReLU()
        body.layer4, body.apool = nn.Conv2d(4, 4, 3, 1, 1), nn.AdaptiveAvgPool2d(2)
        self.resnet34 = body
        self.fc1, self.leaky, self.swarm = nn.Linear(16, 8), nn.LeakyReLU(), nn.Linear(8, 2 * K)
        _randomise(self, seed=11)

    def forward(self, x):
        b = self.resnet34
        x = b.layer1(b.stem.pooling(b.stem.conv1(x)))
        x = b.apool(b.layer4(b.layer3(b.layer2(x))))
        return self.swarm(self.leaky(self.fc1(x.view(x.size(0), -1))))


def test_split_network_layer1_gives_stem_blocks_and_a_trunk_that_completes_them():
    import mmp_reference as mr
    net = _Net().eval()
    spec, blocks, trunk = split_network_layer1(net)
    assert len(blocks) == 3 and blocks[0].wd is not None and blocks[0].w1.shape[1] == 8 and all(b.wd is None for b in blocks[1:])
    rng = np.random.default_rng(0)
    ref = np.where(rng.random((24, 31)) < 0.3, 0.0, 255.0).astype(np.float32)
    stack = mr.input_stack(mr.input_planes(np.array([[3.25, 4.5], [5.0, 6.75], [7.5, 8.0]]), ref), 2)
    with torch.no_grad():
        want = net(torch.from_numpy(stack))
        y, _ = sr.stem(stack, spec.weight, spec.scale, spec.shift, spec.slope)
        for b in blocks:
            y, _ = br.block(y, b)
        got = trunk(torch.from_numpy(y.astype(np.float32)))
    assert got.shape == want.shape == (2, 6) and torch.allclose(got, want, rtol=1e-4, atol=1e-4)
    with pytest.raises(ValueError, match="three blocks"):
        split_network_layer1(_Net(n_blocks=2).eval())
    with pytest.raises(ValueError, match="eval"):
        split_network_layer1(_Net().train())
    with pytest.raises(ValueError, match="resnet34"):
        split_network_layer1(torch.nn.Linear(3, 3))


# ---- 5. the struct and the symbol: no device needed -------------------------------------------------------------------------------------------
def test_block_entry_point_refuses_null_arguments():
    lib = nm.load_library()
    assert "nmpc_mmp_block_f32" in nm.EXPORTED_SYMBOLS and hasattr(lib, "nmpc_mmp_block_f32")
    a = _capi.NmpcMmpBlockArgs()
    assert lib.nmpc_mmp_block_f32(None, ctypes.byref(a)) == -1 and lib.nmpc_mmp_block_f32(None, None) == -1


def test_block_args_layout_matches_the_c_compiler():
    fields = [f[0] for f in _capi.NmpcMmpBlockArgs._fields_]
    assert fields == ["M", "Cin", "H", "W", "x", "w1", "s1", "b1", "w2", "s2", "b2", "wd", "sd", "bd", "slope_mid", "slope_out", "out"]
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "sz.c")
        body = "".join(f'printf(" %zu", offsetof(nmpc_mmp_block_args, {f}));' for f in fields)
        open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "nmpc_hip.h"\nint main(void){printf("%zu", sizeof(nmpc_mmp_block_args));'
                             + body + 'printf(" %zu %d", sizeof(nmpc_mmp_stem_args), NMPC_ABI_VERSION);return 0;}\n')
        exe = os.path.join(td, "sz")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert ctypes.sizeof(_capi.NmpcMmpBlockArgs) == out[0]
    assert [getattr(_capi.NmpcMmpBlockArgs, f).offset for f in fields] == out[1:-2]
    assert out[-2] == ctypes.sizeof(_capi.NmpcMmpStemArgs) and out[-1] == 5      # nothing that existed changed


def test_block_kernels_use_no_scratch_and_fit_two_workgroups_per_cu():
    """Read from the shipped code object: both kernels (with and without the projection) without VGPR spills or scratch, within the
    256 registers of two wavefronts per SIMD, and under 80 KB of LDS (two workgroups in a CU's 160 KB)."""
    import re
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    nm.build_library()
    res = {kernel_resources.short_name(k): v for k, v in kernel_resources.kernel_resources(nm.library_path()).items()}
    mine = {k: v for k, v in res.items() if re.search(r"mmp_block_kernel", k)}
    assert len(mine) == 2, sorted(mine)
    for name, r in mine.items():
        print(name, r)
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, (name, r)      # (SGPRs parked in VGPR lanes touch no memory)
        assert r["vgpr"] + max(r["agpr"], 0) <= 256 and r["lds_static"] <= 80 * 1024, (name, r)
