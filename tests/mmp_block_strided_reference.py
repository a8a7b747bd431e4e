"""float64 restatement (test infrastructure) of one residual block of the multi-hypothesis predictor's strided residual stages
(layer2 .. layer4) as ``nmpc_mmp_block{2,3,4}_f32`` (csrc/nmpc_mmp_block_f32.h) fuse it, with
``torch.nn.functional.conv2d(stride=...)`` in double, stated once and parametrised by a ``Stage``; tests/mmp_block{2,3,4}_reference.py
are the stages under the names the tests import. The stride s (1 or 2) is the first convolution's and the projection's:

    m   = leaky(s1 conv3x3(x, w1; stride s, padding 1) + b1, slope_mid)        H x W -> H2 x W2 = ((H - 1) // s + 1, (W - 1) // s + 1)
    z   =       s2 conv3x3(m, w2; padding 1) + b2                             (m outside the H2 x W2 plane is 0)
    id  = x  |  sd conv1x1(x, wd; stride s) + bd
    out = leaky(z + id, slope_out)

``Stage.block`` returns ``(out, bound)``. The bound is the running first-order error analysis of tests/mmp_block_reference.py (see
there for the derivation: c(K) = K + 8 for a sum of K products with its affine and slope, u = 2^-24), with the sizes of a block of C
output channels, derived and not tuned:

    e_m   = c(9 Cin) u (|s1| conv(|x|, |w1|; stride s) + |b1|)                        (0 outside the plane: m is exactly 0 there)
    e_z   = |s2| conv(e_m, |w2|)                                                     the inherited error of m, through a linear map
            + c(9 C) u (|s2| conv(|m| + e_m, |w2|) + |b2|)                           the second convolution's own: 9 C products,
                                                                                     c(288), c(576), c(1152) for C = 32, 64, 128
    e_id  = 0  |  c(Cin) u (|sd| conv(|x|, |wd|; stride s) + |bd|)
    e_out = e_z + e_id + 2 u (|z| + |id| + e_z + e_id)                               the addition and the slope

Four wrong variants serve as controls (``block(..., wrong=...)``): ``"slope"`` applies ``slope_mid`` behind the addition;
``"halo"`` takes m on the ring outside the plane as ``leaky(b1)`` -- what the first convolution gives there on zero input --
instead of 0; ``"phase"`` (stride 2) lets the first convolution sample windows centred at the odd pixels 2 y + 1, which is what
a stride-2 convolution without the padding offset gives; ``"idphase"`` (stride 2) lets the projection read ``x[1::2, 1::2]``."""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24            # unit roundoff of float32
M_MAX = 3
case_id = lambda c: f"{c[0]}x{c[1]}-c{c[2]}-s{c[3]}"


def _c(K):
    return K + 8


def out_plane(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def random_x(M, Cin, H, W, seed):
    """Both signs, as the activations behind a LeakyReLU are."""
    return np.random.default_rng(seed).standard_normal((M, Cin, H, W)).astype(np.float32)


def _parts(x, spec):
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))
    v = lambda a: t(a)[None, :, None, None]
    return t(x), t(spec.w1), v(spec.s1), v(spec.b1), t(spec.w2), v(spec.s2), v(spec.b2)


def _proj(spec):
    wd = torch.as_tensor(np.asarray(spec.wd, dtype=np.float64))[:, :, None, None]
    sd, bd = (torch.as_tensor(np.asarray(a, dtype=np.float64))[None, :, None, None] for a in (spec.sd, spec.bd))
    return wd, sd, bd


def integer_units(x, spec):
    """For a stage's ``integer_block`` on integer x: the largest magnitude any partial sum or intermediate value can take, in units
    of its own last place (from the absolute-value convolutions, so for every order of summation); the reasoning of
    tests/mmp_block_reference.py ``integer_units``, with the stride. Below 2^24 float32 holds all of them, and every order of
    summation gives the same bits."""
    xt, w1, s1, b1, w2, s2, b2 = _parts(x, spec)
    s = int(spec.stride)
    S1 = F.conv2d(xt.abs(), w1.abs(), stride=s, padding=1)
    A1 = s1.abs() * S1 + b1.abs()
    S2 = F.conv2d(A1, w2.abs(), padding=1)
    A2 = s2.abs() * S2 + b2.abs()
    if spec.wd is None:
        AD = xt.abs()
    else:
        wd, sd, bd = _proj(spec)
        AD = sd.abs() * F.conv2d(xt.abs(), wd.abs(), stride=s) + bd.abs()
    return float(max(S1.max(), 16 * A1.max(), 16 * S2.max(), 32 * A2.max(), 2 * AD.max(), 128 * (A2 + AD).max()))


def torch_float32(x, spec):
    """torch's own float32 convolutions, affines and LeakyReLUs on the CPU: a correct fp32 implementation, as a control."""
    t = lambda a: torch.as_tensor(np.array(a, dtype=np.float32))
    v = lambda a: t(a)[None, :, None, None]
    xt, s = t(x), int(spec.stride)
    m = F.leaky_relu(F.conv2d(xt, t(spec.w1), stride=s, padding=1) * v(spec.s1) + v(spec.b1), float(spec.slope_mid))
    z = F.conv2d(m, t(spec.w2), padding=1) * v(spec.s2) + v(spec.b2)
    ident = xt if spec.wd is None else F.conv2d(xt, t(spec.wd)[:, :, None, None], stride=s) * v(spec.sd) + v(spec.bd)
    return F.leaky_relu(z + ident, float(spec.slope_out)).numpy()


class Stage:
    """One strided stage: ``n`` its number, ``C`` the output channels, ``TILE`` the outputs per tile of the kernel, ``spec`` the
    name of its spec class in mmp_stem, ``ternary`` what the integer block's weights are drawn from, ``x_max`` the range of the
    integer x, ``PLANES`` the input planes by stride, ``CHANNELS`` the (Cin, stride, projection) walked on them, ``REAL`` the
    warehouse planes (once each, M = 2), ``CHUNK`` the input channels per staged chunk where the cases are named from it."""

    def __init__(self, n, C, TILE, spec, ternary, x_max, PLANES, CHANNELS, REAL, CHUNK=None):
        self.n, self.C, self.TILE, self.spec, self.ternary, self.x_max = n, C, TILE, spec, ternary, x_max
        self.PLANES, self.CHANNELS, self.REAL, self.CHUNK = PLANES, CHANNELS, REAL, CHUNK
        self.CASES = tuple((H, W, Cin, s, proj) for Cin, s, proj in CHANNELS for H, W in PLANES[s])
        self.case = functools.lru_cache(maxsize=None)(self._case)

    def _spec(self, *a):
        from dyobav_mpcnwta_warehouse_amd import mmp_stem
        return getattr(mmp_stem, self.spec)(*a)

    def random_block(self, Cin, seed, stride, projection):
        """Seeded weights, scales of both signs, non-zero shifts, the reference's slopes 0.1 and 0.01."""
        C, rng = self.C, np.random.default_rng(seed)
        f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
        sign = lambda k: np.where((np.arange(C) + k) % 3 == 1, -1.0, 1.0)
        w1 = f32(rng.standard_normal((C, Cin, 3, 3)) / np.sqrt(9.0 * Cin))
        w2 = f32(rng.standard_normal((C, C, 3, 3)) / np.sqrt(9.0 * C))
        s1, s2, sd = (f32(rng.uniform(0.5, 1.5, C) * sign(k)) for k in range(3))
        b1, b2, bd = (f32(rng.uniform(0.25, 2.0, C) * sign(k + 1)) for k in range(3))
        wd = f32(rng.standard_normal((C, Cin)) / np.sqrt(Cin))
        if not projection:
            wd = sd = bd = None
        return self._spec(w1, s1, b1, 0.1, w2, s2, b2, wd, sd, bd, 0.01, stride)

    def integer_block(self, Cin, seed, stride, projection):
        """Weights in {-1, 0, 1}, scales in {+-1/2, +-1, +-2}, integer shifts, slopes 1/8 and 1/4: on integer x nothing rounds as
        long as the sums stay small (``integer_units``). The share of non-zero ternary weights falls with the number of terms: half
        in the 16-channel reference, a quarter at 32 channels (288 terms in the second convolution, 576 in the first at 64 input
        channels), an eighth at 64 (576, 1 152) and at 128 (1 152, 2 304)."""
        C, rng = self.C, np.random.default_rng(seed)
        f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
        scale = lambda: f32(rng.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], C))
        shift = lambda: f32(rng.integers(-3, 4, C))
        tern = lambda *shape: f32(rng.choice(self.ternary, shape))
        w1, w2, wd = tern(C, Cin, 3, 3), tern(C, C, 3, 3), tern(C, Cin)
        s1, b1, s2, b2, sd, bd = scale(), shift(), scale(), shift(), scale(), shift()
        if not projection:
            wd = sd = bd = None
        return self._spec(w1, s1, b1, 0.125, w2, s2, b2, wd, sd, bd, 0.25, stride)

    def doubling_block(self):
        """C -> C, stride 1: w1 and w2 the centre delta, scales 1, shifts 0, no projection: out = 2 x for x >= 0, exactly."""
        C = self.C
        w = np.zeros((C, C, 3, 3), dtype=np.float32)
        for c in range(C):
            w[c, c, 1, 1] = 1.0
        one, zero = np.ones(C, dtype=np.float32), np.zeros(C, dtype=np.float32)
        return self._spec(w, one, zero, 0.1, w.copy(), one.copy(), zero.copy(), None, None, None, 0.01, 1)

    def duplicate_and_double_block(self, Cin=None):
        """Cin -> C (by default from C / 2) at stride 2, exact: w1[c] and wd[c] the centre delta on channel c % Cin, w2 the delta, scales
        1, shifts 0: m = leaky(x[c % Cin, ::2, ::2]), z = m, id = x[c % Cin, ::2, ::2], so out = 2 cat(x, x, ...)[:, ::2, ::2] for x >= 0."""
        C, Cin = self.C, self.C // 2 if Cin is None else Cin
        w1, wd = np.zeros((C, Cin, 3, 3), dtype=np.float32), np.zeros((C, Cin), dtype=np.float32)
        for c in range(C):
            w1[c, c % Cin, 1, 1] = wd[c, c % Cin] = 1.0
        d = self.doubling_block()
        return d._replace(w1=w1, wd=wd, sd=d.s1.copy(), bd=d.b1.copy(), stride=2)

    def integer_x(self, M, Cin, H, W, seed):
        """Integers in [-x_max, x_max] as float32 ([-2, 2]; [-1, 1] at 128 channels: with 1 152 terms in the second convolution behind
        2 304 in the first the worst case of ``integer_units`` would pass 2^24 at 256 input channels)."""
        return np.random.default_rng(seed).integers(-self.x_max, self.x_max + 1, (M, Cin, H, W)).astype(np.float32)

    def block(self, x, spec, wrong=None):
        """x [M, Cin, H, W], spec the stage's spec (any float type, used as float64) -> (out, bound) [M, C, H2, W2] float64."""
        C = self.C
        xt, w1, s1, b1, w2, s2, b2 = _parts(x, spec)
        Cin, s = xt.shape[1], int(spec.stride)
        H2, W2 = out_plane(xt.shape[2], xt.shape[3], s)
        if wrong in ("phase", "idphase") and s != 2:
            raise ValueError(f"the wrong variant {wrong!r} exists at stride 2 only")
        slope_mid, slope_out = float(spec.slope_mid), float(spec.slope_mid if wrong == "slope" else spec.slope_out)
        if wrong == "phase":        # windows centred at 2 y + 1: rows 2 y .. 2 y + 2, zero behind the plane
            conv_x = F.conv2d(F.pad(xt, (0, 2 * W2 + 1 - xt.shape[3], 0, 2 * H2 + 1 - xt.shape[2])), w1, stride=2, padding=0)
        else:
            conv_x = F.conv2d(xt, w1, stride=s, padding=1)
        m = F.leaky_relu(s1 * conv_x + b1, slope_mid)
        assert m.shape[2:] == (H2, W2)
        e_m = _c(9 * Cin) * U * (s1.abs() * F.conv2d(xt.abs(), w1.abs(), stride=s, padding=1) + b1.abs())
        if wrong == "halo":
            ring = F.leaky_relu(b1, slope_mid).expand(m.shape[0], C, H2 + 2, W2 + 2).clone()
            ring[:, :, 1:-1, 1:-1] = m
            conv_m = F.conv2d(ring, w2, padding=0)
        else:
            conv_m = F.conv2d(m, w2, padding=1)
        z = s2 * conv_m + b2
        e_z = s2.abs() * F.conv2d(e_m, w2.abs(), padding=1) + _c(9 * C) * U * (s2.abs() * F.conv2d(m.abs() + e_m, w2.abs(), padding=1) + b2.abs())
        if spec.wd is None:
            ident, e_id = xt, torch.zeros_like(z)
        else:
            wd, sd, bd = _proj(spec)
            if wrong == "idphase":
                ident = sd * F.conv2d(F.pad(xt, (0, 2 * W2 - xt.shape[3], 0, 2 * H2 - xt.shape[2]))[:, :, 1::2, 1::2], wd) + bd
            else:
                ident = sd * F.conv2d(xt, wd, stride=s) + bd
            e_id = _c(Cin) * U * (sd.abs() * F.conv2d(xt.abs(), wd.abs(), stride=s) + bd.abs())
        out = F.leaky_relu(z + ident, slope_out)
        bound = e_z + e_id + 2 * U * (z.abs() + ident.abs() + e_z + e_id)
        return out.numpy(), bound.numpy()

    def _case(self, kind, H, W, Cin, stride, projection, M=M_MAX):
        """(x, spec, out, bound) of a seeded case, computed once and shared (read-only): ``kind`` = "random" or "integer". A call
        with fewer rows takes the first rows of x, so its reference is the head of this one."""
        seed = 1000 * H + 10 * W + Cin + stride
        if kind == "random":
            x, spec = random_x(M, Cin, H, W, seed), self.random_block(Cin, seed + 1, stride, projection)
        else:
            x, spec = self.integer_x(M, Cin, H, W, seed), self.integer_block(Cin, seed + 1, stride, projection)
        out, bound = self.block(x, spec)
        for a in (x, out, bound):
            a.setflags(write=False)
        return x, spec, out, bound

    def names(self):
        """What tests/mmp_block<n>_reference.py exports: the stage's own under the names the tests import, and the shared ones."""
        own = {f"{k}_block{self.n}": getattr(self, k + "_block") for k in ("random", "integer", "doubling", "duplicate_and_double")}
        own.update({k: getattr(self, k) for k in ("C", "TILE", "PLANES", "CHANNELS", "REAL", "CASES", "integer_x", "block", "case")})
        if self.CHUNK:
            own["CHUNK"] = self.CHUNK
        shared = {k: globals()[k] for k in ("U", "M_MAX", "case_id", "_c", "out_plane", "random_x", "_parts", "_proj", "integer_units", "torch_float32")}
        return {**shared, **own}


# The cases the tests walk. Planes are INPUT planes, chosen around the kernel's tile of OUTPUTS; (Cin, stride, projection).

# layer2, tile 8 x 44. Stride 2: smaller than a tile in both parities; 16 x 88 -> exactly one output tile; 17 x 89 -> 9 x 45, both
# parities changed and a remainder tile each way; 22 x 99 -> 11 x 50, two tiles both ways with remainders (even and odd side).
# Stride 1: the same list read as output planes. Cin = 64: eight streamed chunks.
LAYER2 = Stage(2, 32, (8, 44), "Block2Spec", [-1.0] + [0.0] * 6 + [1.0], 2,
               PLANES={2: ((3, 5), (4, 6), (16, 88), (17, 89), (22, 99)), 1: ((3, 5), (4, 6), (8, 44), (9, 45), (11, 50))},
               CHANNELS=((8, 2, True), (16, 2, True), (32, 1, False), (64, 1, True)),
               REAL=((74, 83, 16, 2, True), (37, 42, 32, 1, False)))

# layer3, tile 7 x 21. Stride 2: smaller than a tile in both parities; 14 x 42 -> exactly one output tile; 15 x 43 -> 8 x 22, both
# parities changed and a one-row, one-column sliver of a second tile each way; 30 x 7 -> 15 x 4, three tiles high. Stride 1: the
# same list read as output planes (30 x 7: five tiles high). Stride 2 streams chunks of 8 channels, stride 1 of 16: 128 are eight
# chunks, 24 one and a half (the kernel's only other path: a last chunk with channels missing).
LAYER3 = Stage(3, 64, (7, 21), "Block3Spec", [-1.0, 1.0] + [0.0] * 14, 2,
               PLANES={2: ((3, 5), (4, 6), (14, 42), (15, 43), (30, 7)), 1: ((3, 5), (4, 6), (7, 21), (8, 22), (30, 7))},
               CHANNELS=((8, 2, True), (32, 2, True), (64, 1, False), (128, 1, True), (24, 1, True)),
               REAL=((37, 42, 32, 2, True), (19, 21, 64, 1, False)))

# layer4, named from the kernel's tile: TILE = 10 x 11 outputs where the plane fits (kB4MH, kB4MW), TILE - 2 = 8 x 9 per tile along a
# longer side. Stride 2: smaller than a tile in both parities; 20 x 22 -> exactly one output tile; 21 x 23 -> 11 x 12, both parities
# changed and a second tile each way (rows 8 .. 10, columns 9 .. 11 of it: with 17 x 19 -> 9 x 10 it would still be one tile); 50 x 7
# -> 25 x 4, four tiles high and one wide without a halo. Stride 1: the same list read as output planes. Stride 2 streams chunks of
# 16 channels, stride 1 of 32 (CHUNK, the kernel's cc): 256 are eight chunks, 48 one and a half (a last chunk with channels missing).
_TH, _TW = 10, 11
LAYER4 = Stage(4, 128, (_TH, _TW), "Block4Spec", [-1.0, 1.0] + [0.0] * 14, 1,
               PLANES={2: ((3, 5), (4, 6), (2 * _TH, 2 * _TW), (2 * _TH + 1, 2 * _TW + 1), (50, 7)),
                       1: ((3, 5), (4, 6), (_TH, _TW), (_TH + 1, _TW + 1), (25, 4))},
               CHANNELS=((8, 2, True), (64, 2, True), (128, 1, False), (256, 1, True), (32 * 3 // 2, 1, True)),
               REAL=((19, 21, 64, 2, True), (10, 11, 128, 1, False)), CHUNK={1: 32, 2: 16})
