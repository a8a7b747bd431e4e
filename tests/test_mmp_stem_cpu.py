"""CPU tests of the fused first layer's host side: ``mmp_stem.fold_stem`` / ``split_network`` against the torch modules run in
float64, the identity the kernel rests on (``conv(stack) = conv(channels 0 .. 5) + (off + 1) E`` with E from the taps inside
the map) on an even and an odd map height, every refusal, and ``mmp_stem_shape`` against torch's own output shapes."""
import ctypes
import subprocess
import tempfile
import os

import numpy as np
import pytest
import torch

import dyobav_mpcnwta_warehouse_amd as nm
import mmp_reference as mr
import mmp_stem_reference as sr
from dyobav_mpcnwta_warehouse_amd import _capi
from dyobav_mpcnwta_warehouse_amd.mmp_stem import StemSpec, check_spec, fold_doubles, fold_stem, split_network

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _modules(C, bias, seed):
    """Conv2d, BatchNorm2d (eval, non-trivial running statistics and affine), LeakyReLU(0.1), MaxPool2d(3, 2, 1)."""
    g = torch.Generator().manual_seed(seed)
    conv = torch.nn.Conv2d(7, C, 7, 2, 3, bias=bias)
    bn = torch.nn.BatchNorm2d(C)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(C, 7, 7, 7, generator=g) / 16)
        if bias:
            conv.bias.copy_(torch.randn(C, generator=g))
        bn.weight.copy_(torch.randn(C, generator=g))                    # both signs
        bn.bias.copy_(torch.randn(C, generator=g))
        bn.running_mean.copy_(torch.randn(C, generator=g) * 3)
        bn.running_var.copy_(torch.rand(C, generator=g) * 4 + 0.25)
    return conv, bn.eval(), torch.nn.LeakyReLU(0.1), torch.nn.MaxPool2d(3, 2, 1)


def _stack(Hm, Wm, n_off, seed=0):
    rng = np.random.default_rng(seed)
    ref = np.where(rng.random((Hm, Wm)) < 0.3, 0.0, 255.0).astype(np.float32)
    centres = np.array([[3.25, 4.5], [5.0, 6.75], [7.5, 8.0], [Wm - 2.5, Hm - 1.25]])
    planes = mr.input_planes(centres, ref)
    return planes, mr.input_stack(planes, n_off)


# ---- 1. the fold: the restatement with the folded doubles equals the modules in float64 ------------------------------------------
@pytest.mark.parametrize("C", [8, 64])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
def test_fold_equals_the_modules_in_float64(C, bias):
    conv, bn, act, pool = _modules(C, bias, seed=C + bias)
    _, stack = _stack(23, 31, 3)
    w, scale, shift = fold_doubles(conv, bn)
    assert (scale < 0).any() and (scale > 0).any() and np.abs(shift).min() > 0
    got, bound = sr.stem(stack, w, scale, shift, act.negative_slope)
    seq = torch.nn.Sequential(conv, bn, act, pool).double()
    try:
        with torch.no_grad():
            want = seq(torch.from_numpy(stack).double()).numpy()
    finally:
        seq.float()
    # float64 rounding of a 343-term sum, relative to |scale| S + |shift|: 343 * 2^-53 = 4e-14
    ratio = np.abs(got - want) / bound
    print(f"C = {C}, bias = {bias}: largest |restatement - modules| / (|scale| S + |shift|) = {ratio.max():.2e}")
    assert got.shape == want.shape == (3, C) + _capi.mmp_stem_shape(23, 31) and ratio.max() <= 1e-12
    # and fold_stem is the same numbers, rounded once
    spec = fold_stem(conv, bn, act, pool)
    assert spec.weight.dtype == spec.scale.dtype == spec.shift.dtype == np.float32 and spec.slope == pytest.approx(0.1)
    assert np.array_equal(spec.weight, w.astype(np.float32)) and np.array_equal(spec.scale, scale.astype(np.float32))
    assert np.array_equal(spec.shift, shift.astype(np.float32)) and spec.weight.shape == (C, 7, 7, 7)
    assert check_spec(spec).weight.flags.c_contiguous


# ---- 2. the split: conv of six channels + (off + 1) E, E from the taps inside the map ----------------------------------------------
@pytest.mark.parametrize("shape", [(23, 31), (24, 31)], ids=["odd_height", "even_height"])
def test_split_into_base_and_offset_term(shape):
    spec = sr.random_spec(8, seed=5)
    planes, stack = _stack(*shape, n_off=4)
    w = spec.weight.astype(np.float64)
    whole = torch.nn.functional.conv2d(torch.from_numpy(stack).double(), torch.from_numpy(w), stride=2, padding=3).numpy()
    S = torch.nn.functional.conv2d(torch.from_numpy(stack).double().abs(), torch.from_numpy(w).abs(), stride=2, padding=3).numpy()
    base, E = sr.split(planes, w)
    t = np.arange(1, 5, dtype=np.float64)[:, None, None, None]
    parts = base[None] + t * E[None]
    assert parts.shape == whole.shape == (4, 8, (shape[0] - 1) // 2 + 1, (shape[1] - 1) // 2 + 1)
    assert (np.abs(parts - whole) <= 1e-12 * S).all()
    # a border rule that counted every tap (E = the plain sum of the channel-6 weights) agrees inside and is caught at the border
    wrong = base[None] + t * w[:, 6].sum(axis=(1, 2))[None, :, None, None]
    assert (np.abs(wrong - whole) <= 1e-12 * S)[:, :, 2:-2, 2:-2].all() and not (np.abs(wrong - whole) <= 1e-12 * S).all()


# ---- 3. what fold_stem and split_network refuse --------------------------------------------------------------------------------------
def test_fold_refuses_what_the_kernel_does_not_compute():
    conv, bn, act, pool = _modules(8, False, seed=1)
    fold_stem(conv, bn, act, pool)
    with pytest.raises(ValueError, match="eval"):
        fold_stem(conv, torch.nn.BatchNorm2d(8).train(), act, pool)
    with pytest.raises(ValueError, match="running statistics"):
        fold_stem(conv, torch.nn.BatchNorm2d(8, track_running_stats=False).eval(), act, pool)
    with pytest.raises(ValueError, match="kernel 7"):
        fold_stem(torch.nn.Conv2d(7, 8, 3, 2, 1), bn, act, pool)                     # 3 x 3 stem
    with pytest.raises(ValueError, match="stride 2"):
        fold_stem(torch.nn.Conv2d(7, 8, 7, 1, 3), bn, act, pool)                     # stride 1
    with pytest.raises(ValueError, match="kernel 7"):
        fold_stem(torch.nn.Conv2d(6, 8, 7, 2, 3), bn, act, pool)                     # six input channels
    with pytest.raises(ValueError, match="groups 1"):
        fold_stem(torch.nn.Conv2d(7, 7, 7, 2, 3, groups=7), bn, act, pool)
    with pytest.raises(ValueError, match="multiple of 8"):
        fold_stem(torch.nn.Conv2d(7, 12, 7, 2, 3), torch.nn.BatchNorm2d(12).eval(), act, pool)
    with pytest.raises(ValueError, match="MaxPool2d"):
        fold_stem(conv, bn, act, torch.nn.MaxPool2d(2, 2))                           # pool 2 / 2
    with pytest.raises(ValueError, match="ceil_mode"):
        fold_stem(conv, bn, act, torch.nn.MaxPool2d(3, 2, 1, ceil_mode=True))
    with pytest.raises(ValueError, match="LeakyReLU"):
        fold_stem(conv, bn, torch.nn.ReLU(), pool)
    with pytest.raises(ValueError, match="StemSpec"):
        check_spec(StemSpec(np.zeros((8, 7, 7, 7)), np.zeros(8), np.zeros(4), 0.1))
    with pytest.raises(ValueError, match="slope"):
        check_spec(StemSpec(np.zeros((8, 7, 7, 7)), np.zeros(8), np.zeros(8), float("nan")))


class _Net(torch.nn.Module):
    """A module with the attribute names of the reference's ConvMultiHypoNet(lite=True), written anew and much smaller."""
    def __init__(self, C=8, K=3, stem=True):
        super().__init__()
        conv, bn, act, pool = _modules(C, False, seed=2)
        body = torch.nn.Module()
        if stem:
            body.stem = torch.nn.Module()
            body.stem.conv1 = torch.nn.Sequential(conv, bn, act)
            body.stem.pooling = pool
        body.layer1, body.layer2 = torch.nn.Conv2d(C, 4, 3, 1, 1), torch.nn.ReLU()
        body.layer3, body.layer4 = torch.nn.Conv2d(4, 4, 3, 2, 1), torch.nn.ReLU()
        body.apool = torch.nn.AdaptiveAvgPool2d(2)
        self.resnet34 = body
        self.fc1, self.leaky, self.swarm = torch.nn.Linear(16, 8), torch.nn.LeakyReLU(), torch.nn.Linear(8, 2 * K)

    def forward(self, x):
        b = self.resnet34
        x = b.stem.pooling(b.stem.conv1(x))
        x = b.apool(b.layer4(b.layer3(b.layer2(b.layer1(x)))))
        return self.swarm(self.leaky(self.fc1(x.view(x.size(0), -1))))


def test_split_network_gives_the_stem_and_a_trunk_that_completes_it():
    net = _Net().eval()
    spec, trunk = split_network(net)
    _, stack = _stack(24, 31, 2)
    with torch.no_grad():
        want = net(torch.from_numpy(stack))
        pooled, _ = sr.stem(stack, spec.weight, spec.scale, spec.shift, spec.slope)
        got = trunk(torch.from_numpy(pooled.astype(np.float32)))
    assert got.shape == want.shape == (2, 6) and torch.allclose(got, want, rtol=1e-4, atol=1e-4)
    with pytest.raises(ValueError, match="resnet34.stem"):
        split_network(_Net(stem=False))
    with pytest.raises(ValueError, match="resnet34"):
        split_network(torch.nn.Linear(3, 3))
    with pytest.raises(ValueError, match="eval"):
        split_network(_Net().train())
    headless = _Net().eval()
    del headless.swarm
    with pytest.raises(ValueError, match="swarm"):
        split_network(headless)


# ---- 4. the output shape, the struct and the symbols: no device needed ---------------------------------------------------------------
@pytest.mark.parametrize("shape", [(23, 31), (24, 31), (293, 330), (7, 7), (1, 1)])
def test_stem_shape_equals_torchs(shape):
    seq = torch.nn.Sequential(torch.nn.Conv2d(7, 8, 7, 2, 3), torch.nn.MaxPool2d(3, 2, 1))
    with torch.no_grad():
        want = tuple(seq(torch.zeros(1, 7, *shape)).shape[2:])
    assert _capi.mmp_stem_shape(*shape) == want
    if shape == (293, 330):
        assert want == (74, 83)


def test_stem_shape_and_entry_points_refuse_bad_arguments():
    lib = nm.load_library()
    for name in ("nmpc_mmp_stem_f32", "nmpc_mmp_stem_f64", "nmpc_mmp_stem_shape"):
        assert name in nm.EXPORTED_SYMBOLS and hasattr(lib, name), name
    for bad in ((0, 5), (5, 0), (-1, -1)):
        with pytest.raises(nm.NmpcError):
            _capi.mmp_stem_shape(*bad)
    hp = ctypes.c_int32()
    assert lib.nmpc_mmp_stem_shape(5, 5, ctypes.byref(hp), None) == -1
    a = _capi.NmpcMmpStemArgs()
    assert lib.nmpc_mmp_stem_f64(None, ctypes.byref(a)) == -1 and lib.nmpc_mmp_stem_f32(None, None) == -1


def test_stem_args_layout_matches_the_c_compiler():
    fields = [f[0] for f in _capi.NmpcMmpStemArgs._fields_]
    assert fields == [f[0] for f in _capi.NmpcMmpArgs._fields_[:-1]] + ["C", "slope", "weight", "bn_scale", "bn_shift", "out"]
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "sz.c")
        body = "".join(f'printf(" %zu", offsetof(nmpc_mmp_stem_args, {f}));' for f in fields)
        open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "nmpc_hip.h"\nint main(void){printf("%zu", sizeof(nmpc_mmp_stem_args));'
                             + body + 'printf(" %zu %d", sizeof(nmpc_mmp_args), NMPC_ABI_VERSION);return 0;}\n')
        exe = os.path.join(td, "sz")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert ctypes.sizeof(_capi.NmpcMmpStemArgs) == out[0]
    assert [getattr(_capi.NmpcMmpStemArgs, f).offset for f in fields] == out[1:-2]
    assert out[-2] == ctypes.sizeof(_capi.NmpcMmpArgs) and out[-1] == 5      # nothing that existed changed
