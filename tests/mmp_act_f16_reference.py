"""float64 model (test infrastructure) of the residual stages on binary16 operands WITH binary16 activations in memory
(``MmpFrontEnd(activations="f16")``, csrc/nmpc_mmp_block_f16.h): ``Model.model_chain`` of tests/mmp_block_f16_reference.py extended by
the one line the rounding rule gained -- the tensor between two blocks is binary16 where both blocks run on f16 operands; the
identity of a block without projection is then that binary16 value, and ``out`` is rounded once, after the last LeakyReLU.

``binary16_outputs`` states which tensors those are, from the operand types alone; ``model_chain`` rounds them. With nothing
binary16 it is the old ``model_chain``, call for call."""
from __future__ import annotations

import numpy as np

from dyobav_mpcnwta_warehouse_amd.mmp_stem import round_f16


def binary16_outputs(stages, operands, activations):
    """``stages``: (name, number of blocks) of the stages in network order; ``operands``: name -> ``"f32"`` / ``"f16"``. Returns name
    -> one bool per block: whether that block's output is binary16 in memory. It is where ``activations == "f16"`` and the block
    itself and the block that reads its output -- the next of its stage, or the first of the next stage -- both run on f16 operands;
    the last block of all writes float32."""
    on = [operands.get(name, "f32") == "f16" for name, count in stages for _ in range(count)]
    flags = [activations == "f16" and a and b for a, b in zip(on, on[1:] + [False])]
    out, k = {}, 0
    for name, count in stages:
        out[name] = tuple(flags[k:k + count])
        k += count
    return out


def model_chain(model, x, specs, out_f16=None):
    """``model.model_chain(x, specs)`` -- the rule in float64 with m rounded, block after block, each output rounded to float32 as
    it is in memory -- with the output of block ``i`` rounded to binary16 where ``out_f16[i]``: the value the next block stages,
    projects and, without a projection, adds as its identity. ``x`` is what is in memory in front of the first block (binary16
    values where that tensor is binary16)."""
    out_f16 = (False,) * len(specs) if out_f16 is None else tuple(out_f16)
    assert len(out_f16) == len(specs)
    outs = []
    for spec, half in zip(specs, out_f16):
        x = model.block(x, spec, round_m=True)[0].astype(np.float32)
        if half:
            x = round_f16(x).astype(np.float32)
        outs.append(x)
    return outs
