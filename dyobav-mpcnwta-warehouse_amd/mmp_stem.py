"""The first layer of the multi-hypothesis predictor's network as the fused kernel takes it (``nmpc_mmp_stem_*``,
csrc/nmpc_mmp_stem.h): ``StemSpec`` = the convolution's weight and the norm folded into one scale and shift per channel.

A network that starts as the reference's ``ConvMultiHypoNet(lite=True)`` does -- ``Conv2d(7, C, 7, stride 2, padding 3)`` ->
``BatchNorm2d`` -> ``LeakyReLU`` -> ``MaxPool2d(3, 2, 1)`` (net_module/net.py:24-43, submodules.py:21-27) -- can hand these
four modules to the device stage and keep the rest, the trunk: ``split_network(net)`` does both for a module of that class's
shape, ``fold_stem`` for the four modules alone. ``BatchEvaluator(predictor="mmp", network=trunk, mmp_stem=spec)`` and
``MmpInterface(trunk, stem=spec)`` then never build the input stack.

The fold is done in float64 and rounded once to float: ``scale = gamma / sqrt(var + eps)``, ``shift = beta - mean * scale``
(+ ``scale * bias`` for a convolution with a bias). It is only valid for a norm in inference mode: batch statistics couple the
rows of a batch, which a per-pedestrian kernel cannot reproduce.

The four residual stages behind the stem (net_module/net.py:45-61) go the same way, one fused kernel per ``BasicBlock``;
``STAGES`` below is their table:

    resnet34   channels   blocks   spec         fold          kernel                 header                  plane (warehouse)
    layer1     16         3        BlockSpec    fold_block    nmpc_mmp_block_f32     csrc/nmpc_mmp_block.h   74 x 83
    layer2     32         4        Block2Spec   fold_block2   nmpc_mmp_block2_f32    csrc/nmpc_mmp_block2.h  37 x 42
    layer3     64         6        Block3Spec   fold_block3   nmpc_mmp_block3_f32    csrc/nmpc_mmp_block3.h  19 x 21
    layer4     128        3        Block4Spec   fold_block4   nmpc_mmp_block4_f32    csrc/nmpc_mmp_block4.h  10 x 11

A spec holds both 3 x 3 convolutions with their folded norms, the 1 x 1 projection of the stage's first block (``None`` for a block
that adds the identity) and the two slopes -- 0.1 inside the block (``compact_conv_layer``), 0.01 behind the addition (a default
``nn.LeakyReLU``). Layer1 runs at stride 1; the first block of each later stage halves the plane, so their specs also hold
``stride`` (1 or 2, of the first convolution and of the projection), and their float32 kernels are one, ``mmp_blkf_kernel``
(csrc/nmpc_mmp_block_f32.h), with a geometry per stage in the table's headers. ``check_blocks`` .. ``check_blocks4`` check one stage's specs
against what the stage in front gives. ``split_network_layer1`` .. ``split_network_layer4`` walk the table up to their stage and
return the stem, one tuple of specs per stage and the trunk, a callable made of whatever remains, for ``BatchEvaluator(...,
mmp_stem=spec, mmp_blocks=blocks, mmp_blocks2=blocks2, ..., network=trunk)`` and ``MmpInterface(trunk, stem=spec, blocks=blocks,
blocks2=blocks2, ...)``. The network's end -- ``AvgPool2d(2, 2)``, flatten,
``fc1 = Linear(F, 128)``, ``leaky``, ``swarm.layer_hypos = Linear(128, 2 K)`` -- is one launch (``nmpc_mmp_head_f32``,
csrc/nmpc_mmp_head.h): ``HeadSpec(w1, c1, slope, w2, c2)`` from ``fold_head``, and ``split_network_whole(net)`` returns the stem,
the four tuples of blocks and the head with NO trunk left, for ``BatchEvaluator(..., mmp_blocks4=blocks4, mmp_head=head)`` and
``MmpInterface(None, ..., blocks4=blocks4, head=head)``. Layer2, layer3 and layer4 also have
a kernel on binary16 MFMA operands (``nmpc_mmp_block{2,3,4}_f16``, one kernel with a geometry per stage: csrc/nmpc_mmp_block_f16.h;
``half=("layer3", "layer4")`` or, for all three, ``operands={"layer2": "f16", ...}`` in the callers, the mapping stage name ->
``"f32"`` or ``"f16"`` that generalises ``half=``): ``pack_block_f16`` rounds a stage's spec's weights once and packs them in the order
the kernel's lanes load them -- two, four or eight groups of sixteen output channels, one layout for both strides --,
``unpack_block_f16`` inverts it, ``round_f16`` is the rounding; ``pack_block{2,3,4}_f16`` and ``unpack_block{2,3,4}_f16`` are the
stages' names for them."""
from __future__ import annotations

import functools
from typing import Callable, NamedTuple, Optional, Tuple

import numpy as np


class StemSpec(NamedTuple):
    weight: np.ndarray      # [C, 7, 7, 7] float32
    scale: np.ndarray       # [C] float32
    shift: np.ndarray       # [C] float32
    slope: float


class BlockSpec(NamedTuple):
    w1: np.ndarray                  # [16, Cin, 3, 3] float32
    s1: np.ndarray                  # [16] float32
    b1: np.ndarray                  # [16] float32
    slope_mid: float
    w2: np.ndarray                  # [16, 16, 3, 3] float32
    s2: np.ndarray                  # [16]
    b2: np.ndarray                  # [16]
    wd: Optional[np.ndarray]        # [16, Cin] float32, or None: the identity (Cin == 16)
    sd: Optional[np.ndarray]        # [16] or None
    bd: Optional[np.ndarray]        # [16] or None
    slope_out: float


BLOCK_CHANNELS = 16                 # output channels of the fused block (csrc/nmpc_mmp_block.h)


# The strided stages' specs: BlockSpec's fields with C = 32 / 64 / 128 in place of 16 (the identity: Cin == C and stride == 1), then
# ``stride`` = 1 or 2, of the first convolution and of the projection. One class per stage: its name is what the messages print.
_STRIDED_FIELDS = [*BlockSpec.__annotations__.items(), ("stride", int)]
Block2Spec = NamedTuple("Block2Spec", _STRIDED_FIELDS)
Block3Spec = NamedTuple("Block3Spec", _STRIDED_FIELDS)
Block4Spec = NamedTuple("Block4Spec", _STRIDED_FIELDS)

BLOCK2_CHANNELS = 32                # output channels of the fused strided block (csrc/nmpc_mmp_block2.h)
BLOCK3_CHANNELS = 64                # output channels of the third stage's fused block (csrc/nmpc_mmp_block3.h)
BLOCK4_CHANNELS = 128               # output channels of the fourth stage's fused block (csrc/nmpc_mmp_block4.h)


class HeadSpec(NamedTuple):
    w1: np.ndarray                  # [128, F] float32: fc1 on the pooled planes flattened [c][h][w]
    c1: np.ndarray                  # [128] float32
    slope: float                    # of the LeakyReLU between the two layers
    w2: np.ndarray                  # [O, 128] float32: the hypothesis layer, O = 2 K
    c2: np.ndarray                  # [O] float32


HEAD_FEATURES = 128                 # outputs of the head's first linear layer (csrc/nmpc_mmp_head.h)


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
    for path in [*("resnet34." + n for n in _BODY), "fc1", "leaky", "swarm"]:
        need(net, path)
    return spec, _trunk(net, 0)


_BODY = ("layer1", "layer2", "layer3", "layer4", "apool")       # of ``net.resnet34``, behind the stem


def _trunk(net, n):
    """The network from the ``n`` th member of ``_BODY`` on as a callable on that member's input (parameters shared with ``net``)."""
    layers = [getattr(net.resnet34, name) for name in _BODY[n:]]
    fc1, leaky, swarm = net.fc1, net.leaky, net.swarm

    def trunk(x):
        for layer in layers:
            x = layer(x)
        return swarm(leaky(fc1(x.reshape(x.shape[0], -1))))
    return trunk


def _conv_norm(name, seq, n_parts):
    import torch
    try:
        parts = list(seq)
    except TypeError:
        parts = []
    if len(parts) != n_parts or not isinstance(parts[0], torch.nn.Conv2d) or not isinstance(parts[1], torch.nn.BatchNorm2d):
        raise ValueError(f"fold_block: '{name}' is not Sequential(Conv2d, BatchNorm2d{', LeakyReLU' if n_parts == 3 else ''})")
    conv, bn = parts[0], parts[1]
    if bn.num_features != conv.out_channels:
        raise ValueError(f"fold_block: the norm of '{name}' has {bn.num_features} channels, its convolution {conv.out_channels}")
    if bn.training or bn.running_mean is None or bn.running_var is None:
        raise ValueError(f"fold_block: the BatchNorm2d of '{name}' must be in eval() mode with running statistics: batch statistics "
                         "couple the rows of a batch, which the fused block cannot reproduce")
    return parts


def _conv_is(name, conv, kernel, padding):
    if (_pair(conv.kernel_size) != (kernel, kernel) or _pair(conv.stride) != (1, 1) or _pair(conv.padding) != (padding, padding)
            or conv.groups != 1 or _pair(conv.dilation) != (1, 1) or conv.padding_mode != "zeros"):
        raise ValueError(f"fold_block: '{name}' must have kernel {kernel}, stride 1, padding {padding}, groups 1, dilation 1 and "
                         f"zero padding; got {conv}")


def _slope(name, act) -> float:
    import torch
    if not isinstance(act, torch.nn.LeakyReLU):
        raise ValueError(f"fold_block: the activation '{name}' must be a LeakyReLU, got {type(act).__name__}")
    slope = float(act.negative_slope)
    if not np.isfinite(slope) or abs(slope) > 1.0:
        raise ValueError(f"fold_block: the slope of '{name}' is {slope}; it must be finite with |slope| <= 1")
    return slope


def fold_block(block) -> BlockSpec:
    """A module shaped like the reference's ``BasicBlock`` at stride 1 -- ``conv1 = Sequential(Conv2d 3 x 3, BatchNorm2d,
    LeakyReLU)``, ``conv2 = Sequential(Conv2d 3 x 3, BatchNorm2d)``, ``downsample = None | Sequential(Conv2d 1 x 1, BatchNorm2d)``,
    ``leaky = LeakyReLU`` -- -> :class:`BlockSpec`; ``ValueError`` for anything the kernel does not compute."""
    for name in ("conv1", "conv2", "downsample", "leaky"):
        if not hasattr(block, name):
            raise ValueError(f"fold_block: the module has no {name!r}")
    c1, n1, act = _conv_norm("conv1", block.conv1, 3)
    c2, n2 = _conv_norm("conv2", block.conv2, 2)
    _conv_is("conv1", c1, 3, 1)
    _conv_is("conv2", c2, 3, 1)
    Cin = int(c1.in_channels)
    if c1.out_channels != BLOCK_CHANNELS or c2.in_channels != BLOCK_CHANNELS or c2.out_channels != BLOCK_CHANNELS:
        raise ValueError(f"fold_block: the block must have {BLOCK_CHANNELS} output channels, got {c1.out_channels} and "
                         f"{c2.in_channels} -> {c2.out_channels}")
    if Cin < 8 or Cin > 256 or Cin % 8:
        raise ValueError(f"fold_block: the block must have a multiple of 8 input channels from 8 to 256, got {Cin}")
    slope_mid, slope_out = _slope("conv1[2]", act), _slope("leaky", block.leaky)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    wd = sd = bd = None
    if block.downsample is not None:
        cd, nd = _conv_norm("downsample", block.downsample, 2)
        _conv_is("downsample", cd, 1, 0)
        if cd.in_channels != Cin or cd.out_channels != BLOCK_CHANNELS:
            raise ValueError(f"fold_block: 'downsample' must be {Cin} -> {BLOCK_CHANNELS}, got {cd.in_channels} -> {cd.out_channels}")
        wd, sd, bd = fold_doubles(cd, nd)
        wd, sd, bd = f32(wd.reshape(BLOCK_CHANNELS, Cin)), f32(sd), f32(bd)
    elif Cin != BLOCK_CHANNELS:
        raise ValueError(f"fold_block: a block {Cin} -> {BLOCK_CHANNELS} without 'downsample' has no identity to add")
    w1, s1, b1 = fold_doubles(c1, n1)
    w2, s2, b2 = fold_doubles(c2, n2)
    return BlockSpec(f32(w1), f32(s1), f32(b1), slope_mid, f32(w2), f32(s2), f32(b2), wd, sd, bd, slope_out)


def check_block(spec) -> BlockSpec:
    """``spec`` with contiguous float32 arrays of consistent shapes (``ValueError`` otherwise)."""
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    C = BLOCK_CHANNELS
    w1, s1, b1, w2, s2, b2 = (f32(v) for v in (spec.w1, spec.s1, spec.b1, spec.w2, spec.s2, spec.b2))
    Cin = w1.shape[1] if w1.ndim == 4 else -1
    ok = (w1.ndim == 4 and w1.shape == (C, Cin, 3, 3) and 8 <= Cin <= 256 and Cin % 8 == 0 and w2.shape == (C, C, 3, 3)
          and all(v.shape == (C,) for v in (s1, b1, s2, b2)))
    proj = [v is not None for v in (spec.wd, spec.sd, spec.bd)]
    wd = sd = bd = None
    if ok and all(proj):
        wd, sd, bd = f32(spec.wd), f32(spec.sd), f32(spec.bd)
        ok = wd.shape == (C, Cin) and sd.shape == (C,) and bd.shape == (C,)
    elif ok:
        ok = not any(proj) and Cin == C
    if not ok:
        shp = lambda v: None if v is None else np.shape(v)
        raise ValueError(f"BlockSpec: w1 {w1.shape}, s1 {s1.shape}, b1 {b1.shape}, w2 {w2.shape}, s2 {s2.shape}, b2 {b2.shape}, wd {shp(spec.wd)}, "
                         f"sd {shp(spec.sd)}, bd {shp(spec.bd)}; expected [16, Cin, 3, 3], [16], [16], [16, 16, 3, 3], [16], [16] with Cin a "
                         "multiple of 8 from 8 to 256, and [16, Cin], [16], [16] or three None (Cin = 16)")
    for name in ("slope_mid", "slope_out"):
        if not np.isfinite(float(getattr(spec, name))) or abs(float(getattr(spec, name))) > 1.0:
            raise ValueError(f"BlockSpec: {name} = {getattr(spec, name)}")
    return BlockSpec(w1, s1, b1, float(spec.slope_mid), w2, s2, b2, wd, sd, bd, float(spec.slope_out))


def block2_plane(H: int, W: int, stride: int) -> Tuple[int, int]:
    """The output plane of a block of stride ``stride`` on an ``H x W`` input plane (3 x 3, padding 1 / 1 x 1, padding 0)."""
    return (int(H) - 1) // int(stride) + 1, (int(W) - 1) // int(stride) + 1


def _conv2_is(name, conv, kernel, padding, stride, fn="fold_block2"):
    if (_pair(conv.kernel_size) != (kernel, kernel) or _pair(conv.padding) != (padding, padding) or conv.groups != 1
            or _pair(conv.dilation) != (1, 1) or conv.padding_mode != "zeros"):
        raise ValueError(f"{fn}: '{name}' must have kernel {kernel}, padding {padding}, groups 1, dilation 1 and zero padding; got {conv}")
    if _pair(conv.stride) != (stride, stride):
        raise ValueError(f"{fn}: '{name}' must have stride {stride}, got stride {_pair(conv.stride)}")


def _fold_strided(block, fn, C, Spec):
    """``fold_block2`` / ``fold_block3``: one body; ``fn`` names the caller in the messages, ``C`` its output channels."""
    for name in ("conv1", "conv2", "downsample", "leaky"):
        if not hasattr(block, name):
            raise ValueError(f"{fn}: the module has no {name!r}")
    try:
        c1, n1, act = _conv_norm("conv1", block.conv1, 3)
        c2, n2 = _conv_norm("conv2", block.conv2, 2)
        parts_d = None if block.downsample is None else _conv_norm("downsample", block.downsample, 2)
    except ValueError as e:
        raise ValueError(str(e).replace("fold_block:", f"{fn}:")) from None
    stride = _pair(c1.stride)[0]
    if _pair(c1.stride) not in ((1, 1), (2, 2)):
        raise ValueError(f"{fn}: 'conv1' must have stride 1 or 2, got stride {_pair(c1.stride)}")
    _conv2_is("conv1", c1, 3, 1, stride, fn)
    _conv2_is("conv2", c2, 3, 1, 1, fn)
    Cin = int(c1.in_channels)
    if c1.out_channels != C or c2.in_channels != C or c2.out_channels != C:
        raise ValueError(f"{fn}: the block must have {C} output channels, got {c1.out_channels} and {c2.in_channels} -> {c2.out_channels}")
    if Cin < 8 or Cin > 256 or Cin % 8:
        raise ValueError(f"{fn}: the block must have a multiple of 8 input channels from 8 to 256, got {Cin}")
    try:
        slope_mid, slope_out = _slope("conv1[2]", act), _slope("leaky", block.leaky)
    except ValueError as e:
        raise ValueError(str(e).replace("fold_block:", f"{fn}:")) from None
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    wd = sd = bd = None
    if parts_d is not None:
        cd, nd = parts_d
        if _pair(cd.stride) != _pair(c1.stride):
            raise ValueError(f"{fn}: mismatched strides: 'conv1' has stride {_pair(c1.stride)}, 'downsample' {_pair(cd.stride)}")
        _conv2_is("downsample", cd, 1, 0, stride, fn)
        if cd.in_channels != Cin or cd.out_channels != C:
            raise ValueError(f"{fn}: 'downsample' must be {Cin} -> {C}, got {cd.in_channels} -> {cd.out_channels}")
        wd, sd, bd = fold_doubles(cd, nd)
        wd, sd, bd = f32(wd.reshape(C, Cin)), f32(sd), f32(bd)
    elif stride != 1:
        raise ValueError(f"{fn}: a block at stride 2 without 'downsample' has no identity of the output's shape to add")
    elif Cin != C:
        raise ValueError(f"{fn}: a block {Cin} -> {C} without 'downsample' has no identity to add")
    w1, s1, b1 = fold_doubles(c1, n1)
    w2, s2, b2 = fold_doubles(c2, n2)
    return Spec(f32(w1), f32(s1), f32(b1), slope_mid, f32(w2), f32(s2), f32(b2), wd, sd, bd, slope_out, int(stride))


def fold_block2(block) -> Block2Spec:
    """A module shaped like the reference's ``BasicBlock`` -- ``conv1 = Sequential(Conv2d 3 x 3 at stride 1 or 2, BatchNorm2d,
    LeakyReLU)``, ``conv2 = Sequential(Conv2d 3 x 3, BatchNorm2d)``, ``downsample = None | Sequential(Conv2d 1 x 1 at conv1's stride,
    BatchNorm2d)``, ``leaky = LeakyReLU`` -- with 32 output channels -> :class:`Block2Spec`, folded in float64 (``fold_doubles``) and
    rounded once; ``ValueError`` for anything the kernel does not compute."""
    return _fold_strided(block, "fold_block2", BLOCK2_CHANNELS, Block2Spec)


def fold_block3(block) -> Block3Spec:
    """As ``fold_block2`` for a block with 64 output channels -> :class:`Block3Spec`: the same fold in float64, the same refusals."""
    return _fold_strided(block, "fold_block3", BLOCK3_CHANNELS, Block3Spec)


def fold_block4(block) -> Block4Spec:
    """As ``fold_block2`` for a block with 128 output channels -> :class:`Block4Spec`: the same fold in float64, the same refusals."""
    return _fold_strided(block, "fold_block4", BLOCK4_CHANNELS, Block4Spec)


def _check_strided(spec, C, Spec):
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    w1, s1, b1, w2, s2, b2 = (f32(v) for v in (spec.w1, spec.s1, spec.b1, spec.w2, spec.s2, spec.b2))
    Cin = w1.shape[1] if w1.ndim == 4 else -1
    stride = spec.stride
    ok = (w1.ndim == 4 and w1.shape == (C, Cin, 3, 3) and 8 <= Cin <= 256 and Cin % 8 == 0 and w2.shape == (C, C, 3, 3)
          and all(v.shape == (C,) for v in (s1, b1, s2, b2)) and isinstance(stride, (int, np.integer)) and int(stride) in (1, 2))
    proj = [v is not None for v in (spec.wd, spec.sd, spec.bd)]
    wd = sd = bd = None
    if ok and all(proj):
        wd, sd, bd = f32(spec.wd), f32(spec.sd), f32(spec.bd)
        ok = wd.shape == (C, Cin) and sd.shape == (C,) and bd.shape == (C,)
    elif ok:
        ok = not any(proj) and Cin == C and int(stride) == 1
    if not ok:
        shp = lambda v: None if v is None else np.shape(v)
        raise ValueError(f"{Spec.__name__}: w1 {w1.shape}, s1 {s1.shape}, b1 {b1.shape}, w2 {w2.shape}, s2 {s2.shape}, b2 {b2.shape}, wd {shp(spec.wd)}, "
                         f"sd {shp(spec.sd)}, bd {shp(spec.bd)}, stride {stride!r}; expected [{C}, Cin, 3, 3], [{C}], [{C}], [{C}, {C}, 3, 3], [{C}], [{C}] "
                         f"with Cin a multiple of 8 from 8 to 256, stride 1 or 2, and [{C}, Cin], [{C}], [{C}] or three None (Cin = {C}, stride 1)")
    for name in ("slope_mid", "slope_out"):
        if not np.isfinite(float(getattr(spec, name))) or abs(float(getattr(spec, name))) > 1.0:
            raise ValueError(f"{Spec.__name__}: {name} = {getattr(spec, name)}")
    return Spec(w1, s1, b1, float(spec.slope_mid), w2, s2, b2, wd, sd, bd, float(spec.slope_out), int(stride))


def check_block2(spec) -> Block2Spec:
    """``spec`` with contiguous float32 arrays of consistent shapes and a stride of 1 or 2 (``ValueError`` otherwise)."""
    return _check_strided(spec, BLOCK2_CHANNELS, Block2Spec)


def check_block3(spec) -> Block3Spec:
    """As ``check_block2``, at 64 output channels."""
    return _check_strided(spec, BLOCK3_CHANNELS, Block3Spec)


def check_block4(spec) -> Block4Spec:
    """As ``check_block2``, at 128 output channels."""
    return _check_strided(spec, BLOCK4_CHANNELS, Block4Spec)


# layer2, layer3 and layer4 with binary16 MFMA operands (``nmpc_mmp_block{2,3,4}_f16``, csrc/nmpc_mmp_block_f16.h): the stage's spec with
# ``w1``, ``w2`` and ``wd`` rounded to binary16 and packed in the order the kernel's lanes load them, as uint16 bit patterns. With C
# output channels (32, 64, 128: 2, 4, 8 groups of sixteen) and KB = ceil(Cin / 32):
#   w1 [9, KB, C / 16, 64, 8]: [tap 3 ky + kx][K block kb][group g][lane l][j] = f16(w1[16 g + (l & 15), 32 kb + 8 (l >> 4) + j, ky, kx]),
#   zero where the input channel is >= Cin; w2 the same with Cin = C; wd [KB, C / 16, 64, 8] without the tap.
# Layer2's strided block has 16 input channels, half a K block, the other half packed zeros: one layout for both strides. The scales,
# the shifts, the slopes and the stride are the float32 spec's, unchanged.
# Layer1 (``nmpc_mmp_block_f16``, csrc/nmpc_mmp_block1_f16.h) under the same rule: C = 16 is one group, ``w1 [9, KB, 1, 64, 8]``, ``w2 [9, 1, 1,
# 64, 8]`` whose input channels 16 .. 31 (lanes 32 .. 63) are zeros -- the 16 channels of m are half a K block --, ``wd [KB, 1, 64, 8]``; the
# spec has ``BlockSpec``'s fields (no stride).
Block1F16Spec = NamedTuple("Block1F16Spec", list(BlockSpec.__annotations__.items()))
Block2F16Spec = NamedTuple("Block2F16Spec", _STRIDED_FIELDS)
Block3F16Spec = NamedTuple("Block3F16Spec", _STRIDED_FIELDS)
Block4F16Spec = NamedTuple("Block4F16Spec", _STRIDED_FIELDS)
_F16_SPECS = {BLOCK_CHANNELS: Block1F16Spec, BLOCK2_CHANNELS: Block2F16Spec, BLOCK3_CHANNELS: Block3F16Spec, BLOCK4_CHANNELS: Block4F16Spec}
F16_MAX = 65504.0


def round_f16(a) -> np.ndarray:
    """The rounding of the f16 kernels as numpy states it: clipped to +-65504 (the infinities with the finite values, NaN stays
    NaN), then rounded to nearest even with subnormals kept -> ``np.float16``."""
    return np.clip(np.asarray(a), -F16_MAX, F16_MAX).astype(np.float16)


def _pack_f16(w) -> np.ndarray:
    """``[C, Cin, T]`` -> ``[T, KB, C // 16, 64, 8]`` uint16 in fragment order (``C`` = 16, 32, 64 or 128 output channels: 1, 2, 4 or 8 groups)."""
    C, Cin, T = w.shape
    KB = (Cin + 31) // 32
    wp = np.zeros((C, 32 * KB, T), dtype=np.float16)
    wp[:, :Cin] = round_f16(w)
    # [g, row, kb, quad, j, t] -> [t, kb, g, quad, row, j]: lane = 16 quad + row
    return np.ascontiguousarray(wp.reshape(C // 16, 16, KB, 4, 8, T).transpose(5, 2, 0, 3, 1, 4)).reshape(T, KB, C // 16, 64, 8).view(np.uint16)


def _unpack_f16(p, Cin: int) -> np.ndarray:
    """``[T, KB, G, 64, 8]`` uint16 -> ``[16 G, Cin, T]`` float16: the inverse of ``_pack_f16`` (the padding channels dropped)."""
    T, KB, G = p.shape[:3]
    w = np.ascontiguousarray(p).view(np.float16).reshape(T, KB, G, 4, 16, 8).transpose(2, 4, 1, 3, 5, 0)
    return np.ascontiguousarray(w.reshape(16 * G, 32 * KB, T)[:, :Cin])


def _f16_stage(channels: int) -> "Stage":
    """The row of ``STAGES`` (below) whose blocks have ``channels`` output channels and an f16 kernel."""
    for st in STAGES:
        if st.channels == channels and channels in _F16_SPECS:
            return st
    raise ValueError(f"no f16 kernel for blocks of {channels} output channels")


def pack_block_f16(spec, channels: Optional[int] = None):
    """A stage's spec (:class:`BlockSpec`, :class:`Block2Spec`, :class:`Block3Spec`, :class:`Block4Spec`) -> its ``Block{1,2,3,4}F16Spec``: the three weight
    arrays rounded once (``round_f16``) and packed; everything else passed through. The stage is the one of ``channels`` output
    channels, by default the spec's own; ``ValueError`` for what that stage's checker refuses."""
    st = _f16_stage(np.shape(spec.w1)[0] if channels is None else channels)
    spec = st.check(spec)
    C, Cin = spec.w1.shape[:2]
    wd = None if spec.wd is None else _pack_f16(spec.wd.reshape(C, Cin, 1))[0]
    return _F16_SPECS[C](*spec._replace(w1=_pack_f16(spec.w1.reshape(C, Cin, 9)), w2=_pack_f16(spec.w2.reshape(C, C, 9)), wd=wd))


def unpack_block_f16(packed, Cin: int):
    """The inverse of ``pack_block_f16`` for a block of ``Cin`` input channels: the stage's float32 spec type whose ``w1``
    [C, Cin, 3, 3], ``w2`` and ``wd`` [C, Cin] are the ROUNDED weights as ``np.float16``."""
    C = 16 * np.shape(packed.w2)[2]
    wd = None if packed.wd is None else _unpack_f16(np.asarray(packed.wd)[None], Cin).reshape(C, Cin)
    return _f16_stage(C).Spec(*packed._replace(w1=_unpack_f16(np.asarray(packed.w1), Cin).reshape(C, Cin, 3, 3),
                                               w2=_unpack_f16(np.asarray(packed.w2), C).reshape(C, C, 3, 3), wd=wd))


# the stages' own names: a spec of another stage is refused by this stage's checker, in its words
pack_block1_f16 = functools.partial(pack_block_f16, channels=BLOCK_CHANNELS)
pack_block2_f16 = functools.partial(pack_block_f16, channels=BLOCK2_CHANNELS)
pack_block3_f16 = functools.partial(pack_block_f16, channels=BLOCK3_CHANNELS)
pack_block4_f16 = functools.partial(pack_block_f16, channels=BLOCK4_CHANNELS)
unpack_block1_f16 = unpack_block2_f16 = unpack_block3_f16 = unpack_block4_f16 = unpack_block_f16


def pack_activations_f16(x) -> np.ndarray:
    """Activations ``[M, C, H, W]`` (float, ``C % 8 == 0``) -> the octet form of binary16 activations in memory (include/nmpc_hip.h,
    csrc/nmpc_mmp_block_f16.h): uint16 bit patterns ``[M, C // 8, H, W, 8]`` with ``a[n, c // 8, y, x, c % 8] = round_f16(x[n, c, y, x])``,
    C-contiguous."""
    x = np.asarray(x)
    if x.ndim != 4 or x.shape[1] % 8 or x.shape[1] == 0:
        raise ValueError(f"pack_activations_f16: shape {x.shape} is no [M, C, H, W] with C a positive multiple of 8")
    M, C, H, W = x.shape
    return np.ascontiguousarray(round_f16(x).reshape(M, C // 8, 8, H, W).transpose(0, 1, 3, 4, 2)).view(np.uint16)


def unpack_activations_f16(a) -> np.ndarray:
    """The inverse of ``pack_activations_f16``: uint16 ``[M, C // 8, H, W, 8]`` -> float32 ``[M, C, H, W]``, exact (every binary16 value
    is a float32 value)."""
    a = np.asarray(a)
    if a.ndim != 5 or a.shape[4] != 8 or a.dtype != np.uint16:
        raise ValueError(f"unpack_activations_f16: {a.dtype} {a.shape} is no uint16 [M, C // 8, H, W, 8]")
    M, O, H, W, _ = a.shape
    return np.ascontiguousarray(np.ascontiguousarray(a).view(np.float16).transpose(0, 1, 4, 2, 3).reshape(M, 8 * O, H, W).astype(np.float32))


def _linear(fn, name, layer, n_in, n_out):
    """(weight [out, in], bias [out]) of a ``torch.nn.Linear`` -like ``layer`` as float32; a missing bias is zeros."""
    import torch
    w = getattr(layer, "weight", None)
    if not isinstance(layer, torch.nn.Linear):
        raise ValueError(f"{fn}: '{name}' must be a Linear, got {layer}")
    if (n_in is not None and w.shape[1] != n_in) or (n_out is not None and w.shape[0] != n_out):
        want = f"Linear({'F' if n_in is None else n_in}, {'O' if n_out is None else n_out})"
        raise ValueError(f"{fn}: '{name}' must be a {want}, got {w.shape[1]} -> {w.shape[0]}")
    f32 = lambda a: np.ascontiguousarray(a.detach().cpu().numpy(), dtype=np.float32)
    b = getattr(layer, "bias", None)
    return f32(w), (np.zeros(w.shape[0], dtype=np.float32) if b is None else f32(b))


def fold_head(apool, fc1, leaky, swarm) -> HeadSpec:
    """The network's end -> :class:`HeadSpec`: ``apool`` must be ``AvgPool2d(2, 2)`` with padding 0, no ``ceil_mode`` and no
    ``divisor_override``; ``fc1`` a ``Linear(F, 128)``; ``leaky`` a ``LeakyReLU``; ``swarm`` a ``Linear(128, O)`` or a module whose
    ``layer_hypos`` is one (the reference's swarm head). ``ValueError`` naming the offender otherwise; a missing bias folds to
    zeros."""
    import torch
    if (not isinstance(apool, torch.nn.AvgPool2d) or _pair(apool.kernel_size) != (2, 2)
            or _pair(apool.stride if apool.stride is not None else apool.kernel_size) != (2, 2)
            or _pair(apool.padding) != (0, 0) or apool.ceil_mode or apool.divisor_override is not None):
        raise ValueError(f"fold_head: 'apool' must be AvgPool2d(2, 2) with padding 0, no ceil_mode and no divisor_override; got {apool}")
    w1, c1 = _linear("fold_head", "fc1", fc1, None, HEAD_FEATURES)
    try:
        slope = _slope("leaky", leaky)
    except ValueError as e:
        raise ValueError(str(e).replace("fold_block:", "fold_head:")) from None
    hyp = getattr(swarm, "layer_hypos", swarm)
    try:
        w2, c2 = _linear("fold_head", "swarm", hyp, HEAD_FEATURES, None)
    except ValueError:
        raise ValueError(f"fold_head: 'swarm' must be a Linear(128, O) or have such a 'layer_hypos', got {swarm}") from None
    return check_head(HeadSpec(w1, c1, slope, w2, c2))


def check_head(spec) -> HeadSpec:
    """``spec`` with contiguous float32 arrays of consistent shapes, an even ``O`` from 2 to 512 and a finite slope of magnitude at most
    1 (``ValueError`` otherwise)."""
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    w1, c1, w2, c2 = (f32(v) for v in (spec.w1, spec.c1, spec.w2, spec.c2))
    O = w2.shape[0] if w2.ndim == 2 else -1
    if not (w1.ndim == 2 and w1.shape[0] == HEAD_FEATURES and w1.shape[1] >= 1 and c1.shape == (HEAD_FEATURES,)
            and w2.ndim == 2 and w2.shape[1] == HEAD_FEATURES and 2 <= O <= 512 and O % 2 == 0 and c2.shape == (O,)):
        raise ValueError(f"HeadSpec: w1 {w1.shape}, c1 {c1.shape}, w2 {w2.shape}, c2 {c2.shape}; expected [128, F], [128], [O, 128], [O] "
                         "with O even from 2 to 512")
    if not np.isfinite(float(spec.slope)) or abs(float(spec.slope)) > 1.0:
        raise ValueError(f"HeadSpec: slope = {spec.slope}")
    return HeadSpec(w1, c1, float(spec.slope), w2, c2)


def head_features(C: int, H: int, W: int) -> int:
    """F of the head on a ``[C, H, W]`` plane: the 2 x 2 pool drops an odd last row and column."""
    return int(C) * (int(H) // 2) * (int(W) // 2)


class Stage(NamedTuple):
    """One residual stage as the device runs it."""
    layer: str          # its attribute on ``net.resnet34``
    arg: str            # its specs in the callers' keywords (``mmp_`` + arg in ``BatchEvaluator``) and in the messages
    channels: int       # output channels of each of its blocks
    count: int          # blocks the reference's network has
    word: str           # ... in the messages
    Spec: type
    fold: Callable      # one block module -> Spec
    check: Callable     # one spec -> Spec, checked


STAGES = (Stage("layer1", "blocks", BLOCK_CHANNELS, 3, "three", BlockSpec, fold_block, check_block),
          Stage("layer2", "blocks2", BLOCK2_CHANNELS, 4, "four", Block2Spec, fold_block2, check_block2),
          Stage("layer3", "blocks3", BLOCK3_CHANNELS, 6, "six", Block3Spec, fold_block3, check_block3),
          Stage("layer4", "blocks4", BLOCK4_CHANNELS, 3, "three", Block4Spec, fold_block4, check_block4))


def check_stage(k: int, front, blocks) -> tuple:
    """The specs of ``STAGES[k]`` checked one by one and as a chain: the first block takes the channels that arrive from ``front`` --
    the (checked) ``StemSpec`` for layer1, the (checked) specs of ``STAGES[k - 1]`` otherwise --, each later one what a block gives."""
    st = STAGES[k]
    if k == 0:
        cin = int(front.weight.shape[0])
        arrives, gives = f"the stem has C = {cin}", f"every block gives {st.channels}"
    else:
        prev = STAGES[k - 1]
        if not front:
            raise ValueError(f"mmp_{st.arg}: the blocks of {prev.layer} are needed in front")
        cin, arrives, gives = prev.channels, f"{prev.layer} gives {prev.channels}", f"every block of {st.layer} gives {st.channels}"
    blocks = tuple(st.check(b) for b in blocks)
    if not blocks:
        raise ValueError(f"mmp_{st.arg}: at least one {st.Spec.__name__} is needed")
    for i, b in enumerate(blocks):
        if b.w1.shape[1] != cin:
            raise ValueError(f"mmp_{st.arg}: block {i} takes {b.w1.shape[1]} channels, but {cin} arrive ({arrives if i == 0 else gives})")
        cin = st.channels
    return blocks


def check_blocks(stem: StemSpec, blocks) -> Tuple[BlockSpec, ...]:
    """The blocks behind ``stem`` as a tuple of checked specs: the first takes the stem's channels, each later one is 16 -> 16."""
    return check_stage(0, stem, blocks)


def check_blocks2(blocks, blocks2) -> Tuple[Block2Spec, ...]:
    """The layer-2 blocks behind the (checked) layer-1 ``blocks``: the first takes the 16 channels layer1 gives, each later one is 32 -> 32."""
    return check_stage(1, blocks, blocks2)


def check_blocks3(blocks2, blocks3) -> Tuple[Block3Spec, ...]:
    """The layer-3 blocks behind the (checked) layer-2 ``blocks2``: the first takes 32 channels, each later one is 64 -> 64."""
    return check_stage(2, blocks2, blocks3)


def check_blocks4(blocks3, blocks4) -> Tuple[Block4Spec, ...]:
    """The layer-4 blocks behind the (checked) layer-3 ``blocks3``: the first takes 64 channels, each later one is 128 -> 128."""
    return check_stage(3, blocks3, blocks4)


def _walk(net, n: int, fn: Optional[str] = None) -> list:
    """``[StemSpec, specs of STAGES[0], ..., specs of STAGES[n - 1]]`` of a module shaped as ``split_network`` takes it. A refusal
    names the function that takes the offending stage off first, ``split_network_<layer>`` -- or ``fn`` for the last stage."""
    out = [split_network(net)[0]]
    for k, st in enumerate(STAGES[:n]):
        try:
            members = list(getattr(net.resnet34, st.layer))
        except TypeError:
            members = []
        if len(members) != st.count:
            raise ValueError(f"{fn if fn and k == n - 1 else 'split_network_' + st.layer}: 'resnet34.{st.layer}' is not a Sequential of "
                             f"{st.word} blocks")
        out.append(check_stage(k, out[-1], [st.fold(b) for b in members]))
    return out


def split_network_layer1(net) -> Tuple[StemSpec, Tuple[BlockSpec, BlockSpec, BlockSpec], Callable]:
    """As ``split_network``, with ``resnet34.layer1`` (three blocks, ``fold_block``) taken off the trunk as well:
    ``(StemSpec, (BlockSpec, BlockSpec, BlockSpec), trunk)``; the trunk, a callable on ``[M, 16, Hp, Wp]``, is ``layer2 .. layer4``,
    ``apool``, flatten, ``fc1``, ``leaky``, ``swarm`` (parameters shared with ``net``)."""
    return (*_walk(net, 1), _trunk(net, 1))


def split_network_layer2(net) -> Tuple[StemSpec, Tuple[BlockSpec, ...], Tuple[Block2Spec, ...], Callable]:
    """With ``resnet34.layer2`` (four blocks, ``fold_block2``) taken off as well: ``(StemSpec, blocks, blocks2, trunk)``; the trunk, a
    callable on ``[M, 32, H2, W2]``, starts at ``layer3``."""
    return (*_walk(net, 2), _trunk(net, 2))


def split_network_layer3(net) -> Tuple[StemSpec, Tuple[BlockSpec, ...], Tuple[Block2Spec, ...], Tuple[Block3Spec, ...], Callable]:
    """With ``resnet34.layer3`` (six blocks, ``fold_block3``) taken off as well: ``(StemSpec, blocks, blocks2, blocks3, trunk)``; the
    trunk, a callable on ``[M, 64, H3, W3]``, starts at ``layer4``."""
    return (*_walk(net, 3), _trunk(net, 3))


def split_network_layer4(net):
    """With ``resnet34.layer4`` (three blocks, ``fold_block4``) taken off as well: ``(StemSpec, blocks, blocks2, blocks3, blocks4,
    trunk)``; the trunk, a callable on ``[M, 128, H4, W4]``, is ``apool``, flatten, ``fc1``, ``leaky``, ``swarm``."""
    return (*_walk(net, 4), _trunk(net, 4))


def split_network_whole(net):
    """The whole network as folded weights, with no torch module left to call: ``(StemSpec, blocks, blocks2, blocks3, blocks4,
    HeadSpec)`` -- ``split_network_layer4`` with its trunk folded by ``fold_head``."""
    return (*_walk(net, 4, "split_network_whole"), fold_head(net.resnet34.apool, net.fc1, net.leaky, net.swarm))
