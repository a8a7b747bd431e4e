"""The multi-hypothesis predictor's WHOLE network as a torch module (test infrastructure; imports no device code), with weights
made by rule, for the tests that compare the folded chain -- restated in float64 or run on the device -- with the network it claims
to compute: tests/test_mmp_net_cpu.py, tests/test_gpu_mmp_net.py and the fixture tests/golden/mmp_net.json.

``Net(fc_input, K)`` is the reference's ``ConvMultiHypoNet(7, 2, fc_input, K, lite=True)`` written anew at full size: a 64-channel
7 x 7 / 2 stem with a 3 x 3 / 2 max-pool, stages of 3 / 4 / 6 / 3 residual blocks at 16 / 32 / 64 / 128 channels (each later stage
halves the plane in its first block, every first block has a 1 x 1 projection), a 2 x 2 average pool, ``fc1``, ``leaky`` and
``swarm.layer_hypos``, under the attribute names ``mmp_stem.split_network_whole`` reads. That it IS the reference's class --
the same 226 ``state_dict`` entries in the same order, the same float64 values at every stage -- is what the fixture pins.

No trained weights exist, so ``fill_by_rule`` makes some: every entry of ``state_dict()`` from ``hash_uniform``, a counter-based
integer hash (no library RNG: the values are the same on every machine and numpy version). The rule keeps the signal alive through
18 stages (``check_alive``): weights of variance 2 / fan_in, norm statistics of order one, gains of both signs, and the gain of
each block's second norm and of each projection's times 0.45 -- without it the residual additions let the activations grow about
fivefold per stage. A network whose activations vanish or explode tests nothing, so ``stages`` asserts the ranges.

The yardstick of every comparison is ``twin_error``: per stage, how far torch's own float32 module lies from the float64 module on
the same float32 input -- the reference's own float32 rounding."""
from __future__ import annotations

import copy
import zlib

import numpy as np
import torch

STAGE_NAMES = ("stem", "layer1", "layer2", "layer3", "layer4", "output")
LAYERS = (("layer1", 64, 16, 3, 1), ("layer2", 16, 32, 4, 2), ("layer3", 32, 64, 6, 2), ("layer4", 64, 128, 3, 2))
SHAPES = (dict(Hm=37, Wm=41, fc_input=128, K=3), dict(Hm=293, Wm=329, fc_input=3200, K=10))
BAR = 4.0                 # times the twin error: the project's margin over the reference's own float32 rounding
RMS, NEGATIVE = (0.25, 4.0), (0.1, 0.6)
_M64 = (1 << 64) - 1


def hash_uniform(n: int, salt: int) -> np.ndarray:
    """``n`` float64 values in [0, 1): splitmix64 of the counters ``1 .. n`` on a state that is itself the mix of ``salt``; the upper
    53 bits of each word. Integer arithmetic in ``np.uint64`` only (it wraps, as the generator is defined)."""
    def mix(z):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))
    gamma = np.uint64(0x9E3779B97F4A7C15)
    seed = mix(np.array([(int(salt) * 0x9E3779B97F4A7C15 + 0x9E3779B97F4A7C15) & _M64], dtype=np.uint64))
    z = mix(seed + gamma * np.arange(1, int(n) + 1, dtype=np.uint64))
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def _salt(name: str, k: int = 0) -> int:
    return zlib.crc32(name.encode()) + (k << 32)


def fill_by_rule(module):
    """Overwrite every entry of ``module.state_dict()`` by rule (salt: ``crc32`` of the entry's name) and return the module. Every
    value is rounded to float32 first, so that the module holds the same numbers in float32 and in float64.
      convolution and linear weights    uniform with variance 2 / fan_in; the hypothesis layer's (``layer_hypos``) times 0.25
      ``running_var``                   in [0.5, 1.5]
      ``running_mean``, biases          in +-0.2; the hypothesis layer's bias in 0.5 +- 0.1
      norm gains                        magnitude in [0.6, 1.4], about 15 % negative; those of ``conv2.1`` (a block's second norm) and
                                        ``downsample.1`` (its projection's) times 0.45
      ``num_batches_tracked``           an integer below 1000 (nothing reads it in ``eval()``)"""
    state = module.state_dict()
    for name, t in state.items():
        n = t.numel()
        u = hash_uniform(n, _salt(name))
        if name.endswith("num_batches_tracked"):
            v = np.floor(1000.0 * u)
        elif name.endswith("running_var"):
            v = 0.5 + u
        elif name.endswith("running_mean"):
            v = 0.4 * u - 0.2
        elif name.endswith(".bias"):
            v = 0.5 + 0.2 * (u - 0.5) if "layer_hypos" in name else 0.4 * u - 0.2
        elif t.dim() == 1:                                  # a norm's gain
            v = (0.6 + 0.8 * u) * np.where(hash_uniform(n, _salt(name, 1)) < 0.15, -1.0, 1.0)
            if ".conv2.1." in name or ".downsample.1." in name:
                v = 0.45 * v
        else:                                               # uniform on +-a has variance a^2 / 3
            v = (2.0 * u - 1.0) * np.sqrt(6.0 / (n // t.shape[0]))
            if "layer_hypos" in name:
                v = 0.25 * v
        v = v.astype(np.float32).astype(np.float64).reshape(tuple(t.shape))
        with torch.no_grad():
            t.copy_(torch.from_numpy(v).to(t.dtype))
    return module


def _conv(cin, cout, kernel, stride, padding, activate=True):
    nn = torch.nn
    parts = [nn.Conv2d(cin, cout, kernel, stride, padding, bias=False), nn.BatchNorm2d(cout)]
    return nn.Sequential(*parts, nn.LeakyReLU(0.1)) if activate else nn.Sequential(*parts)


class _Block(torch.nn.Module):
    def __init__(self, cin, cout, stride, project):
        super().__init__()
        self.conv1 = _conv(cin, cout, 3, stride, 1)
        self.conv2 = _conv(cout, cout, 3, 1, 1, activate=False)
        self.downsample = torch.nn.Sequential(torch.nn.Conv2d(cin, cout, 1, stride, bias=False), torch.nn.BatchNorm2d(cout)) if project else None
        self.leaky = torch.nn.LeakyReLU()

    def forward(self, x):
        return self.leaky(self.conv2(self.conv1(x)) + (x if self.downsample is None else self.downsample(x)))


class _Stem(torch.nn.Module):
    deep = False

    def __init__(self):
        super().__init__()
        self.conv1 = _conv(7, 64, 7, 2, 3)
        self.pooling = torch.nn.MaxPool2d(3, 2, 1)

    def forward(self, x):
        return self.pooling(self.conv1(x))


class _Body(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.stem = _Stem()
        for name, cin, cout, count, stride in LAYERS:
            setattr(self, name, torch.nn.Sequential(*[_Block(cin if i == 0 else cout, cout, stride if i == 0 else 1, i == 0) for i in range(count)]))
        self.apool = torch.nn.AvgPool2d(2, 2)

    def forward(self, x):
        x = self.stem(x)
        for name, *_ in LAYERS:
            x = getattr(self, name)(x)
        return self.apool(x)


class _Swarm(torch.nn.Module):
    def __init__(self, K):
        super().__init__()
        self.layer_hypos = torch.nn.Linear(128, 2 * K)

    def forward(self, x):
        return self.layer_hypos(x)


class Net(torch.nn.Module):
    def __init__(self, fc_input, K):
        super().__init__()
        self.resnet34 = _Body()
        self.fc1 = torch.nn.Linear(fc_input, 128)
        self.leaky = torch.nn.LeakyReLU()
        self.swarm = _Swarm(K)

    def forward(self, x):
        x = self.resnet34(x)
        return self.swarm(self.leaky(self.fc1(x.reshape(x.shape[0], -1))))


def made_net(shape) -> Net:
    """``Net`` of one of ``SHAPES`` in ``eval()`` with the rule's weights, in float32."""
    return fill_by_rule(Net(shape["fc_input"], shape["K"]).eval())


def in_double(net):
    """A float64 copy of ``net``: the same numbers (``fill_by_rule`` made them float32 values)."""
    return copy.deepcopy(net).double()


def finish(net, x, k: int):
    """The output of ``net`` for ``x`` = the tensor of ``STAGE_NAMES[k]`` (k = -1: the network's input), in the module's own dtype."""
    with torch.no_grad():
        body = net.resnet34
        parts = [body.stem] + [getattr(body, name) for name, *_ in LAYERS]
        for part in parts[k + 1:]:
            x = part(x)
        x = body.apool(x)
        return net.swarm(net.leaky(net.fc1(x.reshape(x.shape[0], -1))))


def check_alive(tensors):
    """The condition on the five activations in front of the head: finite, rms in [0.25, 4], 10 % to 60 % negative entries."""
    for name, t in zip(STAGE_NAMES, tensors[:5]):
        t = t.double()
        rms, neg = float(t.pow(2).mean().sqrt()), float((t < 0).double().mean())
        assert bool(torch.isfinite(t).all()), name
        assert RMS[0] <= rms <= RMS[1] and NEGATIVE[0] <= neg <= NEGATIVE[1], f"{name}: rms {rms:.3g}, {100 * neg:.0f} % negative: the rule's network is not alive here"
    assert bool(torch.isfinite(tensors[5]).all())


def stages(net, x):
    """The six tensors of ``STAGE_NAMES`` -- behind the stem, behind ``layer1`` .. ``layer4``, the output -- for the input ``x``
    ``[M, 7, Hm, Wm]`` (a tensor or an array; it is converted to the module's own dtype). Asserts ``check_alive``."""
    dtype = next(net.parameters()).dtype
    x = torch.as_tensor(np.asarray(x)).to(dtype)
    with torch.no_grad():
        body = net.resnet34
        out = [body.stem(x)]
        for name, *_ in LAYERS:
            out.append(getattr(body, name)(out[-1]))
        out.append(finish(net, out[-1], 4))
    check_alive(out)
    return out


def twin_error(net, x):
    """Per stage, max |float32 module - float64 module| on the same float32 input: six floats, in the order of ``STAGE_NAMES``."""
    x = np.asarray(x, dtype=np.float32)
    lo, hi = stages(copy.deepcopy(net).float(), x), stages(in_double(net), x)
    return [float((a.double() - b).abs().max()) for a, b in zip(lo, hi)]


def label_image(Hm: int, Wm: int) -> np.ndarray:
    """A grey label image by rule, float32: three quarters free (1.0), the rest one of 200 grey levels below 200 / 255. It is the
    warehouse's kind of image in units of 255: the rule's norms have statistics of order one, as a trained network's would have for
    its own inputs, and the kernels copy the image as it is."""
    u, g = hash_uniform(Hm * Wm, _salt("label")), hash_uniform(Hm * Wm, _salt("label", 1))
    return np.where(u < 0.25, np.floor(200.0 * g) / 255.0, 1.0).reshape(Hm, Wm).astype(np.float32)


def rule_input(Hm: int, Wm: int, M: int = 4) -> np.ndarray:
    """``[M, 7, Hm, Wm]`` float32, shaped as the predictor's input stack is: five Gaussian bumps (sigma 20 pixels, peak 1) around
    hashed centres on or near the map, ``label_image``, and a constant plane ``m + 1``."""
    c = hash_uniform(M * 5 * 2, _salt("centres")).reshape(M, 5, 2) * np.array([Wm + 8.0, Hm + 8.0]) - 4.0
    yy, xx = np.mgrid[0:Hm, 0:Wm].astype(np.float64)
    out = np.empty((M, 7, Hm, Wm), dtype=np.float32)
    for m in range(M):
        for k in range(5):
            out[m, k] = np.exp(-((xx - c[m, k, 0]) ** 2 + (yy - c[m, k, 1]) ** 2) / (2.0 * 20.0 ** 2))
        out[m, 5], out[m, 6] = label_image(Hm, Wm), m + 1.0
    return out


def sample_index(name: str, numel: int, n: int = 64) -> np.ndarray:
    """``n`` hashed flat positions of a tensor of ``numel`` elements (the fixture's samples of the stage ``name``)."""
    return np.minimum((hash_uniform(n, _salt("sample " + name)) * numel).astype(np.int64), numel - 1)
