"""float64 model (test infrastructure) of the residual block with binary16 MFMA operands, ``nmpc_mmp_block{2,3,4}_f16``
(csrc/nmpc_mmp_block_f16.h), stated once for the three stages: ``Model(b)`` stands on a stage's float32 reference module ``b``
(tests/mmp_block2_reference.py and its siblings), whose block, cases, wrong variants and output channels ``b.C`` it keeps.
tests/mmp_block{2,3,4}_f16_reference.py are ``Model(b)`` under the names the tests import.

The rule: whatever an MFMA reads is f16 -- ``x`` and the weights ``w1``, ``w2``, ``wd`` (``_h`` below: clipped to +-65504, rounded to
nearest even, subnormals kept: ``mmp_stem.round_f16``), and ``m`` when it goes to LDS -- and nothing else is: the accumulation, the
affines, the LeakyReLUs, ``z + id`` and ``x`` as the identity are float32 in the kernel and exact here.

``block(x, spec) -> (out, bound)`` rounds ``x`` and the weights and does NOT round ``m``: the rounding of ``m`` is an error term of the
bound, like the float32 roundings. It does clip ``m`` to +-65504, as it clips ``x`` before it rounds: saturation is part of the rule,
and no multiple of an ulp covers it. With u = 2^-24, c(K) = K + 8 (tests/mmp_block_reference.py):

    e_m   = c(9 Cin) u (|s1| conv(|x_h|, |w1_h|; stride) + |b1|)
    e_mh  = e_m + 2^-11 (|m| + e_m) + 2^-25                        the rounding of m: half an ulp, or half a subnormal step
    e_z   = |s2| conv(e_mh, |w2_h|) + c(9 C) u (|s2| conv(|m| + e_mh, |w2_h|) + |b2|)
    e_id  = 0  |  c(Cin) u (|sd| conv(|x_h|, |wd_h|; stride) + |bd|)
    bound = e_z + e_id + 2 u (|z| + |id| + e_z + e_id)

(m outside the plane is exactly 0 and carries no error: the convolutions of e_mh pad with zeros.) ``model_chain`` is the rule with m
rounded as well, block after block, for the network-level test; ``emulate`` is torch's float32 convolutions on the rounded operands
with m rounded: a correct implementation of the rule in another summation order, the control of the bound."""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

from dyobav_mpcnwta_warehouse_amd.mmp_stem import F16_MAX, pack_block_f16, round_f16, unpack_block_f16


def rounded(spec):
    """``spec`` with the weights the kernel gets: through ``pack_block_f16`` and back (np.float16 arrays; the rest unchanged)."""
    return unpack_block_f16(pack_block_f16(spec), int(np.shape(spec.w1)[1]))


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


class Model:
    """The model on the float32 reference module ``b`` of one stage: ``block``, ``model_chain``, ``emulate``, ``rounded`` and ``case``."""

    def __init__(self, b):
        self.b, self.U, self.C, self._c = b, b.U, b.C, b._c
        self.rounded, self.emulate = rounded, emulate
        self.case = functools.lru_cache(maxsize=None)(self._case)

    def block(self, x, spec, wrong=None, round_m=False):
        """x [M, Cin, H, W], spec the stage's spec -> (out, bound) [M, C, H2, W2] float64; ``wrong``: the variants of ``b.block``, on
        the rounded operands; ``round_m``: m rounded too (``model_chain``; the bound is then unused)."""
        b, U, C, _c = self.b, self.U, self.C, self._c
        xh = round_f16(x).astype(np.float64)
        sh = rounded(spec)
        if wrong is not None:
            return b.block(xh, sh, wrong=wrong)[0], None
        xt, w1, s1, b1, w2, s2, b2 = b._parts(xh, sh)
        Cin, s = xt.shape[1], int(spec.stride)
        m = F.leaky_relu(s1 * F.conv2d(xt, w1, stride=s, padding=1) + b1, float(spec.slope_mid))
        e_m = _c(9 * Cin) * U * (s1.abs() * F.conv2d(xt.abs(), w1.abs(), stride=s, padding=1) + b1.abs())
        m = m.clamp(-F16_MAX, F16_MAX)                            # saturation is the rule, not an error of it (a contraction: e_m still holds)
        e_mh = e_m + 2.0 ** -11 * (m.abs() + e_m) + 2.0 ** -25
        if round_m:
            m = torch.as_tensor(round_f16(m.numpy()).astype(np.float64))
        z = s2 * F.conv2d(m, w2, padding=1) + b2
        e_z = s2.abs() * F.conv2d(e_mh, w2.abs(), padding=1) + _c(9 * C) * U * (s2.abs() * F.conv2d(m.abs() + e_mh, w2.abs(), padding=1) + b2.abs())
        if spec.wd is None:
            ident, e_id = torch.as_tensor(np.asarray(x, dtype=np.float64)), torch.zeros_like(z)       # read again, UNROUNDED
        else:
            wd, sd, bd = b._proj(sh)
            ident = sd * F.conv2d(xt, wd, stride=s) + bd
            e_id = _c(Cin) * U * (sd.abs() * F.conv2d(xt.abs(), wd.abs(), stride=s) + bd.abs())
        out = F.leaky_relu(z + ident, float(spec.slope_out))
        bound = e_z + e_id + 2 * U * (z.abs() + ident.abs() + e_z + e_id)
        return out.numpy(), bound.numpy()

    def model_chain(self, x, specs):
        """The rule in float64 with m rounded, block after block: the list of the blocks' outputs (each rounded to float32 on its
        way to the next block, as it is in memory)."""
        outs = []
        for spec in specs:
            x = self.block(x, spec, round_m=True)[0].astype(np.float32)
            outs.append(x)
        return outs

    def _case(self, kind, H, W, Cin, stride, projection, M=None):
        """(x, spec, out, bound) of the seeded case of ``b.case`` (M rows, by default ``b.M_MAX``) under the rule, computed once and
        shared (read-only). The integer cases are exactly representable in f16, so their reference is the float32 one."""
        x, spec, _, _ = self.b.case(kind, H, W, Cin, stride, projection, self.b.M_MAX if M is None else M)
        out, bound = self.block(x, spec)
        for a in (out, bound):
            a.setflags(write=False)
        return x, spec, out, bound
