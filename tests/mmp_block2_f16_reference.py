"""float64 model (test infrastructure) of the layer2 block with binary16 MFMA operands, ``nmpc_mmp_block2_f16``
(csrc/nmpc_mmp_block2_f16.h), on top of tests/mmp_block2_reference.py, whose block, cases, wrong variants and ``integer_units`` it
keeps. The sibling of tests/mmp_block3_f16_reference.py, with this block's sizes in the bound.

The rule: whatever an MFMA reads is f16 -- ``x`` and the weights ``w1``, ``w2``, ``wd`` (clipped to +-65504, rounded to nearest even,
subnormals kept: ``mmp_stem.round_f16``), and ``m`` when it goes to LDS -- and nothing else is: the accumulation, the affines, the
LeakyReLUs, ``z + id`` and ``x`` as the identity are float32 in the kernel and exact here.

``block(x, spec) -> (out, bound)`` rounds ``x`` and the weights and does NOT round ``m``: the rounding of ``m`` is an error term of the
bound, like the float32 roundings. It does clip ``m`` to +-65504, as it clips ``x`` before it rounds: saturation is part of the rule,
and no multiple of an ulp covers it. With u = 2^-24, c(K) = K + 8 (tests/mmp_block_reference.py):

    e_m   = c(9 Cin) u (|s1| conv(|x_h|, |w1_h|; stride) + |b1|)
    e_mh  = e_m + 2^-11 (|m| + e_m) + 2^-25                        the rounding of m: half an ulp, or half a subnormal step
    e_z   = |s2| conv(e_mh, |w2_h|) + c(288) u (|s2| conv(|m| + e_mh, |w2_h|) + |b2|)
    e_id  = 0  |  c(Cin) u (|sd| conv(|x_h|, |wd_h|; stride) + |bd|)
    bound = e_z + e_id + 2 u (|z| + |id| + e_z + e_id)

(m outside the plane is exactly 0 and carries no error: the convolutions of e_mh pad with zeros.) ``model_chain`` is the rule with m
rounded as well, block after block, for the network-level tests; ``emulate`` is torch's float32 convolutions on the rounded operands
with m rounded: a correct implementation of the rule in another summation order, the control of the bound."""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

import mmp_block2_reference as b2
from dyobav_mpcnwta_warehouse_amd.mmp_stem import F16_MAX, pack_block2_f16, round_f16, unpack_block2_f16

U, C, _c = b2.U, b2.C, b2._c


def rounded(spec):
    """``spec`` with the weights the kernel gets: through ``pack_block2_f16`` and back (np.float16 arrays; the rest unchanged)."""
    return unpack_block2_f16(pack_block2_f16(spec), int(np.shape(spec.w1)[1]))


def block(x, spec, wrong=None, round_m=False):
    """x [M, Cin, H, W], spec a Block2Spec -> (out, bound) [M, 32, H2, W2] float64; ``wrong``: the variants of
    ``mmp_block2_reference.block``, on the rounded operands; ``round_m``: m rounded too (``model_chain``; the bound is then unused)."""
    xh = round_f16(x).astype(np.float64)
    sh = rounded(spec)
    if wrong is not None:
        return b2.block(xh, sh, wrong=wrong)[0], None
    xt, w1, s1, b1, w2, s2, b2_ = b2._parts(xh, sh)
    Cin, s = xt.shape[1], int(spec.stride)
    m = F.leaky_relu(s1 * F.conv2d(xt, w1, stride=s, padding=1) + b1, float(spec.slope_mid))
    e_m = _c(9 * Cin) * U * (s1.abs() * F.conv2d(xt.abs(), w1.abs(), stride=s, padding=1) + b1.abs())
    m = m.clamp(-F16_MAX, F16_MAX)                            # saturation is the rule, not an error of it (a contraction: e_m still holds)
    e_mh = e_m + 2.0 ** -11 * (m.abs() + e_m) + 2.0 ** -25
    if round_m:
        m = torch.as_tensor(round_f16(m.numpy()).astype(np.float64))
    z = s2 * F.conv2d(m, w2, padding=1) + b2_
    e_z = s2.abs() * F.conv2d(e_mh, w2.abs(), padding=1) + _c(9 * C) * U * (s2.abs() * F.conv2d(m.abs() + e_mh, w2.abs(), padding=1) + b2_.abs())
    if spec.wd is None:
        ident, e_id = torch.as_tensor(np.asarray(x, dtype=np.float64)), torch.zeros_like(z)       # read again, UNROUNDED
    else:
        wd, sd, bd = b2._proj(sh)
        ident = sd * F.conv2d(xt, wd, stride=s) + bd
        e_id = _c(Cin) * U * (sd.abs() * F.conv2d(xt.abs(), wd.abs(), stride=s) + bd.abs())
    out = F.leaky_relu(z + ident, float(spec.slope_out))
    bound = e_z + e_id + 2 * U * (z.abs() + ident.abs() + e_z + e_id)
    return out.numpy(), bound.numpy()


def model_chain(x, specs):
    """The rule in float64 with m rounded, block after block: the list of the blocks' outputs (each rounded to float32 on its way to
    the next block, as it is in memory)."""
    outs = []
    for spec in specs:
        x = block(x, spec, round_m=True)[0].astype(np.float32)
        outs.append(x)
    return outs


def emulate(x, spec):
    """torch's float32 convolutions, affines and LeakyReLUs on the rounded operands, with m rounded."""
    t = lambda a: torch.as_tensor(np.array(a, dtype=np.float32))
    v = lambda a: t(a)[None, :, None, None]
    sh, s = rounded(spec), int(spec.stride)
    xt = t(round_f16(x))
    m = F.leaky_relu(F.conv2d(xt, t(sh.w1), stride=s, padding=1) * v(sh.s1) + v(sh.b1), float(spec.slope_mid))
    m = t(round_f16(m.numpy()))
    z = F.conv2d(m, t(sh.w2), padding=1) * v(sh.s2) + v(sh.b2)
    ident = t(x) if spec.wd is None else F.conv2d(xt, t(sh.wd)[:, :, None, None], stride=s) * v(sh.sd) + v(sh.bd)
    return F.leaky_relu(z + ident, float(spec.slope_out)).numpy()


@functools.lru_cache(maxsize=None)
def case(kind, H, W, Cin, stride, projection, M=b2.M_MAX):
    """(x, spec, out, bound) of the seeded case of ``mmp_block2_reference.case`` under the rule, computed once and shared
    (read-only). The integer cases are exactly representable in f16, so their reference is the float32 one."""
    x, spec, _, _ = b2.case(kind, H, W, Cin, stride, projection, M)
    out, bound = block(x, spec)
    for a in (out, bound):
        a.setflags(write=False)
    return x, spec, out, bound
