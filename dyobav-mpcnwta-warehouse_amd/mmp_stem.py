"""The first layer of the multi-hypothesis predictor's network as the fused kernel takes it (``nmpc_mmp_stem_*``,
csrc/nmpc_mmp_stem.h): ``StemSpec`` = the convolution's weight and the norm folded into one scale and shift per channel.

A network that starts as the reference's ``ConvMultiHypoNet(lite=True)`` does -- ``Conv2d(7, C, 7, stride 2, padding 3)`` ->
``BatchNorm2d`` -> ``LeakyReLU`` -> ``MaxPool2d(3, 2, 1)`` (net_module/net.py:24-43, submodules.py:21-27) -- can hand these
four modules to the device stage and keep the rest, the trunk: ``split_network(net)`` does both for a module of that class's
shape, ``fold_stem`` for the four modules alone. ``BatchEvaluator(predictor="mmp", network=trunk, mmp_stem=spec)`` and
``MmpInterface(trunk, stem=spec)`` then never build the input stack.

The fold is done in float64 and rounded once to float: ``scale = gamma / sqrt(var + eps)``, ``shift = beta - mean * scale``
(+ ``scale * bias`` for a convolution with a bias). It is only valid for a norm in inference mode: batch statistics couple the
rows of a batch, which a per-pedestrian kernel cannot reproduce."""
from __future__ import annotations

from typing import Callable, NamedTuple, Tuple

import numpy as np


class StemSpec(NamedTuple):
    weight: np.ndarray      # [C, 7, 7, 7] float32
    scale: np.ndarray       # [C] float32
    shift: np.ndarray       # [C] float32
    slope: float


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def fold_stem(conv, bn, act, pool) -> StemSpec:
    """The four torch modules of the first layer -> :class:`StemSpec`; ``ValueError`` for anything the kernel does not compute."""
    import torch
    if not isinstance(conv, torch.nn.Conv2d):
        raise ValueError(f"the stem's convolution must be a Conv2d, got {type(conv).__name__}")
    C = int(conv.out_channels)
    if (conv.in_channels != 7 or _pair(conv.kernel_size) != (7, 7) or _pair(conv.stride) != (2, 2) or _pair(conv.padding) != (3, 3)
            or conv.groups != 1 or _pair(conv.dilation) != (1, 1) or conv.padding_mode != "zeros"):
        raise ValueError(f"the stem's convolution must be 7 -> C with kernel 7, stride 2, padding 3, groups 1, dilation 1; got {conv}")
    if C < 8 or C % 8:
        raise ValueError(f"the stem's convolution must have a multiple of 8 output channels, got {C}")
    if not isinstance(pool, torch.nn.MaxPool2d) or (_pair(pool.kernel_size) != (3, 3) or _pair(pool.stride) != (2, 2)
                                                   or _pair(pool.padding) != (1, 1) or _pair(pool.dilation) != (1, 1) or pool.ceil_mode):
        raise ValueError(f"the stem's pool must be MaxPool2d(3, 2, 1) without ceil_mode, got {pool}")
    if not isinstance(act, torch.nn.LeakyReLU):
        raise ValueError(f"the stem's activation must be a LeakyReLU, got {type(act).__name__}")
    if not isinstance(bn, torch.nn.BatchNorm2d) or bn.num_features != C:
        raise ValueError(f"the stem's norm must be a BatchNorm2d over {C} channels, got {bn}")
    if bn.training or bn.running_mean is None or bn.running_var is None:
        raise ValueError("the stem's BatchNorm2d must be in eval() mode with running statistics: batch statistics couple the rows "
                         "of a batch, which the fused first layer cannot reproduce")
    weight, scale, shift = fold_doubles(conv, bn)
    return StemSpec(np.ascontiguousarray(weight, dtype=np.float32), scale.astype(np.float32), shift.astype(np.float32), float(act.negative_slope))


def fold_doubles(conv, bn):
    """``(weight [C, 7, 7, 7], scale [C], shift [C])`` in float64, before the one rounding to float: the fold alone, no checks."""
    import torch
    f64 = lambda t: t.detach().to("cpu", torch.float64).numpy()
    one = np.ones(int(conv.out_channels))
    gamma, beta = (f64(bn.weight), f64(bn.bias)) if bn.affine else (one, 0.0 * one)
    scale = gamma / np.sqrt(f64(bn.running_var) + float(bn.eps))
    shift = beta - f64(bn.running_mean) * scale
    if conv.bias is not None:
        shift = shift + scale * f64(conv.bias)
    return f64(conv.weight), scale, shift


def check_spec(spec) -> StemSpec:
    """``spec`` with contiguous float32 arrays of consistent shapes (``ValueError`` otherwise)."""
    w = np.ascontiguousarray(spec.weight, dtype=np.float32)
    s, b = np.ascontiguousarray(spec.scale, dtype=np.float32), np.ascontiguousarray(spec.shift, dtype=np.float32)
    if w.ndim != 4 or w.shape[1:] != (7, 7, 7) or w.shape[0] < 8 or w.shape[0] % 8 or s.shape != (w.shape[0],) or b.shape != s.shape:
        raise ValueError(f"StemSpec: weight {w.shape}, scale {s.shape}, shift {b.shape}; expected [C, 7, 7, 7], [C], [C] with C a multiple of 8")
    if not np.isfinite(float(spec.slope)):
        raise ValueError(f"StemSpec: slope = {spec.slope}")
    return StemSpec(w, s, b, float(spec.slope))


def split_network(net) -> Tuple[StemSpec, Callable]:
    """A module shaped like the reference's ``ConvMultiHypoNet(lite=True)`` -> ``(StemSpec, trunk)``: the stem is
    ``net.resnet34.stem.conv1`` = ``Sequential(Conv2d, BatchNorm2d, LeakyReLU)`` plus ``.pooling``; the trunk, a callable on
    ``[M, C, Hp, Wp]``, is ``layer1 .. layer4``, ``apool``, flatten, ``fc1``, ``leaky``, ``swarm`` of the same module (its
    parameters are shared with ``net``, not copied)."""
    def need(obj, path):
        for name in path.split("."):
            if not hasattr(obj, name):
                raise ValueError(f"split_network: the module has no {path!r} ({name!r} was not found)")
            obj = getattr(obj, name)
        return obj
    stem = need(net, "resnet34.stem")
    conv1, pool = need(net, "resnet34.stem.conv1"), need(net, "resnet34.stem.pooling")
    if getattr(stem, "deep", False):
        raise ValueError("split_network: 'resnet34.stem' is a deep stem (three 3 x 3 convolutions); only the 7 x 7 stem is fused")
    try:
        parts = list(conv1)
    except TypeError:
        parts = []
    if len(parts) != 3:
        raise ValueError("split_network: 'resnet34.stem.conv1' is not Sequential(Conv2d, BatchNorm2d, LeakyReLU)")
    spec = fold_stem(parts[0], parts[1], parts[2], pool)
    layers = [need(net, "resnet34." + n) for n in ("layer1", "layer2", "layer3", "layer4", "apool")]
    fc1, leaky, swarm = need(net, "fc1"), need(net, "leaky"), need(net, "swarm")

    def trunk(x):
        for layer in layers:
            x = layer(x)
        return swarm(leaky(fc1(x.reshape(x.shape[0], -1))))
    return spec, trunk
