"""GPU tests that the results of ``nmpc_mmp_block4_f32`` and ``nmpc_mmp_head_f32`` depend on no memory outside their arguments, in
the manner of tests/test_gpu_read_bounds.py (see tests/guarded_buffers.py): every array the entry point reads lies between
poisoned pads of 64 and of 61 elements, with each real poison in turn; the outputs must keep their bits and the pads must come
back untouched.

    entry        structure            arrays read                                 arrays written only
    mmp_block4   NmpcMmpBlock4Args    x w1 s1 b1 w2 s2 b2 wd sd bd                out
    mmp_head     NmpcMmpHeadArgs      x w1 c1 w2 c2                               out

A region INSIDE an array that the header documents as not read (``run_poisoned_regions``): the odd last row and column of the
head's ``x``."""
import ctypes

import numpy as np
import pytest
import torch

import dyobav_mpcnwta_warehouse_amd as nm
import mmp_block4_reference as b4
import mmp_head_reference as hr
from dyobav_mpcnwta_warehouse_amd import _capi
from guarded_buffers import PADS, run_guarded, run_poisoned_regions

pytestmark = pytest.mark.gpu

BLOCK_WEIGHTS = ("w1", "s1", "b1", "w2", "s2", "b2", "wd", "sd", "bd")
HEAD_WEIGHTS = ("w1", "c1", "w2", "c2")


def test_the_table_matches_the_argument_blocks():
    assert PADS == (64, 61)
    for struct, read in ((_capi.NmpcMmpBlock4Args, ("x",) + BLOCK_WEIGHTS), (_capi.NmpcMmpHeadArgs, ("x",) + HEAD_WEIGHTS)):
        assert {n for n, t in struct._fields_ if t is ctypes.c_void_p} == set(read) | {"out"}


@pytest.fixture(scope="module")
def handle():
    with nm.Handle(nm.default_config_struct()) as h:
        h.set_stream(torch.cuda.current_stream().cuda_stream)
        yield h


def _ptr(t):
    return None if t is None else t.data_ptr()


# From CASES the plane one row and one column into a second tile, with and without a projection, with a last chunk of thirty-two
# with sixteen channels missing (Cin = 48) and with half a chunk at stride 2 (Cin = 8); and the smallest plane.
BLOCK_CASES = [(11, 12, 48, 1, True), (11, 12, 128, 1, False), (21, 23, 8, 2, True), (3, 5, 64, 2, True)]


@pytest.mark.parametrize("c", BLOCK_CASES, ids=b4.case_id)
def test_mmp_block4(handle, c):
    H, W, Cin, stride, projection = c
    assert c in b4.CASES
    x, spec, want, bound = b4.case("random", *c)
    shape = (2, b4.C) + b4.out_plane(H, W, stride)
    inputs = {"x": np.array(x[:2], dtype=np.float32)}
    inputs.update({k: None if getattr(spec, k) is None else np.array(getattr(spec, k), dtype=np.float32) for k in BLOCK_WEIGHTS})
    assert (inputs["wd"] is not None) == projection

    def call(t):
        a = _capi.NmpcMmpBlock4Args()
        a.M, a.Cin, a.H, a.W, a.stride = 2, Cin, H, W, stride
        for k, v in t.items():
            setattr(a, k, _ptr(v))
        a.slope_mid, a.slope_out = spec.slope_mid, spec.slope_out
        out = torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
        a.out = out.data_ptr()
        handle.mmp_block4(a)
        torch.cuda.synchronize()
        return {"out": out}
    got = run_guarded(call, inputs, device="cuda", odd_pad=[k for k, v in inputs.items() if v is not None])["out"]
    assert np.isfinite(got).all() and (np.abs(got - want[:2]) <= bound[:2]).all()


def _head_call(handle, spec, C, H, W, M):
    O = int(spec.w2.shape[0])

    def call(t):
        a = _capi.NmpcMmpHeadArgs()
        a.M, a.C, a.H, a.W, a.O, a.slope = M, C, H, W, O, spec.slope
        for k, v in t.items():
            setattr(a, k, _ptr(v))
        out = torch.full((M, O), float("nan"), dtype=torch.float32, device="cuda")
        a.out = out.data_ptr()
        handle.mmp_head(a)
        torch.cuda.synchronize()
        return {"out": out}
    return call


@pytest.mark.parametrize("c", [(8, 3, 3, 2), (16, 4, 7, 40), (128, 10, 11, 40)], ids=hr.case_id)
def test_mmp_head(handle, c):
    C, H, W, O = c
    assert c in hr.CASES
    M = hr.ROWS + 1                                          # a full group of rows and a group with one
    x, spec, want, bound = hr.case("random", *c)
    inputs = {"x": np.array(x[:M], dtype=np.float32)}
    inputs.update({k: np.array(getattr(spec, k), dtype=np.float32) for k in HEAD_WEIGHTS})
    got = run_guarded(_head_call(handle, spec, C, H, W, M), inputs, device="cuda", odd_pad=list(inputs))["out"]
    assert np.isfinite(got).all() and (np.abs(got - want[:M]) <= bound[:M]).all()


@pytest.mark.parametrize("c", [(8, 3, 3, 2), (16, 4, 7, 40), (16, 5, 6, 40)], ids=hr.case_id)
def test_mmp_head_does_not_read_the_odd_last_row_and_column(handle, c):
    C, H, W, O = c
    M = 3
    x, spec = hr.random_x(M, C, H, W, seed=11), hr.random_head(C, H, W, O, seed=12)
    inputs = {"x": x}
    inputs.update({k: np.array(getattr(spec, k), dtype=np.float32) for k in HEAD_WEIGHTS})
    mask = np.zeros(x.shape, dtype=bool)
    mask[:, :, H // 2 * 2:, :] = True
    mask[:, :, :, W // 2 * 2:] = True
    assert mask.any() and not mask.all()
    got = run_poisoned_regions(_head_call(handle, spec, C, H, W, M), inputs, {"x": mask}, device="cuda")["out"]
    want, bound = hr.head(x, spec)
    assert np.isfinite(got).all() and (np.abs(got - want) <= bound).all()
