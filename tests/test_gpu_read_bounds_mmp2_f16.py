"""GPU test that the result of ``nmpc_mmp_block2_f16`` depends on no memory outside its arguments, as
tests/test_gpu_read_bounds.py shows it for the float32 entry (see tests/guarded_buffers.py): every array the entry point reads
lies between poisoned pads, with each poison in turn; the output must keep its bits and the pads must come back untouched.

    entry            structure               arrays read                                 arrays written only
    mmp_block2_f16   NmpcMmpBlock2F16Args    x w1 s1 b1 w2 s2 b2 wd sd bd                out

The packed arrays ``w1``, ``w2`` and ``wd`` are bit patterns (int16 here): their poisons are the bits of a binary16 NaN and of 65504,
and their pads keep the 16-byte alignment the entry demands (64 elements); ``x`` and the float arrays also take the odd pad."""
import ctypes

import numpy as np
import pytest
import torch

import dyobav_mpcnwta_warehouse_amd as nm
import mmp_block2_f16_reference as h2
import mmp_block2_reference as b2
from dyobav_mpcnwta_warehouse_amd import _capi
from dyobav_mpcnwta_warehouse_amd.mmp_stem import pack_block2_f16
from guarded_buffers import PADS, IntPoison, run_guarded

pytestmark = pytest.mark.gpu

BLOCK_WEIGHTS = ("w1", "s1", "b1", "w2", "s2", "b2", "wd", "sd", "bd")
PACKED = ("w1", "w2", "wd")


def test_the_table_matches_the_argument_block():
    assert PADS == (64, 61)
    assert {n for n, t in _capi.NmpcMmpBlock2F16Args._fields_ if t is ctypes.c_void_p} == set(("x",) + BLOCK_WEIGHTS) | {"out"}


@pytest.fixture(scope="module")
def handle():
    with nm.Handle(nm.default_config_struct()) as h:
        h.set_stream(torch.cuda.current_stream().cuda_stream)
        yield h


# One case per kernel, each on the plane one row and one column into a second tile: <2, true> with a quarter of a K block (Cin = 8:
# half of the staged chunk is zeros), <1, true> with two chunks (Cin = 64), <1, false> with the one whole K block.
BLOCK_CASES = [(17, 89, 8, 2, True), (9, 45, 64, 1, True), (9, 45, 32, 1, False)]


@pytest.mark.parametrize("c", BLOCK_CASES, ids=b2.case_id)
def test_mmp_block2_f16(handle, c):
    H, W, Cin, stride, projection = c
    assert c in b2.CASES
    x, spec, want, bound = h2.case("random", *c)
    packed = pack_block2_f16(spec)
    shape = (2, b2.C) + b2.out_plane(H, W, stride)
    inputs = {"x": np.array(x[:2], dtype=np.float32)}
    for k in BLOCK_WEIGHTS:
        v = getattr(packed, k)
        inputs[k] = None if v is None else np.ascontiguousarray(v).view(np.int16) if k in PACKED else np.array(v, dtype=np.float32)
    assert (inputs["wd"] is not None) == projection
    bits = IntPoison((0x7E00, 0x7BFF), -32768, 32767)

    def call(t):
        a = _capi.NmpcMmpBlock2F16Args()
        a.M, a.Cin, a.H, a.W, a.stride = 2, Cin, H, W, stride
        for k, v in t.items():
            setattr(a, k, None if v is None else v.data_ptr())
        a.slope_mid, a.slope_out = spec.slope_mid, spec.slope_out
        out = torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
        a.out = out.data_ptr()
        handle.mmp_block2_f16(a)
        torch.cuda.synchronize()
        return {"out": out}
    given = [k for k, v in inputs.items() if v is not None]
    got = run_guarded(call, inputs, device="cuda", int_poisons={k: bits for k in PACKED if k in given},
                      odd_pad=[k for k in given if k not in PACKED])["out"]
    assert np.isfinite(got).all() and (np.abs(got - want[:2]) <= bound[:2]).all()
