"""GPU tests of the fused end of the multi-hypothesis predictor's network (nmpc_mmp_head_f32, csrc/nmpc_mmp_head.h: 2 x 2 average
pool, flatten, Linear(F, 128), LeakyReLU, Linear(128, O)) through the C ABI, against the float64 restatement of
tests/mmp_head_reference.py and its derived bound (see there; the controls of that bound are checked without a device in
tests/test_mmp_head_cpu.py).

The cases are ``mmp_head_reference.CASES``: the planes (8, 2, 2), (8, 3, 3) -- a row and a column dropped --, (16, 4, 7) and the
warehouse's (128, 10, 11), each with 2, 40 and 512 outputs, at M = 1, 3 and one more than two of the kernel's groups of 16 rows.
Every call writes into a buffer with 64 sentinel floats in front and behind.

Worst |out - ref| / bound measured on an MI355X: 0.0230 ((8, 3, 3), 512 outputs, M 33); 0.0001 on the warehouse plane."""
import ctypes

import numpy as np
import pytest
import torch

import dyobav_mpcnwta_warehouse_amd as nm
import mmp_head_reference as hr
import oracle
from conftest import config_for

pytestmark = pytest.mark.gpu

SENTINEL = -777.0
POINTERS = ("w1", "c1", "w2", "c2")


@pytest.fixture(scope="module")
def handle():
    with nm.Handle(config_for(oracle.Problem())) as h:
        h.set_stream(torch.cuda.current_stream().cuda_stream)
        yield h


def _head_args(x, spec):
    """NmpcMmpHeadArgs of x [M, C, H, W] (numpy) and a HeadSpec, everything uploaded; ``out`` is left to the caller."""
    a = nm._capi.NmpcMmpHeadArgs()
    keep = {"x": torch.from_numpy(np.array(x, dtype=np.float32)).cuda()}
    a.M, a.C, a.H, a.W = (int(v) for v in x.shape)
    a.O = int(spec.w2.shape[0])
    a.x = keep["x"].data_ptr()
    for name in POINTERS:
        keep[name] = torch.from_numpy(np.array(getattr(spec, name), dtype=np.float32)).cuda()
        setattr(a, name, keep[name].data_ptr())
    a.slope = spec.slope
    return a, keep


def _run(h, x, spec, shift=0):
    """The kernel's output [M, O] float32, ``shift`` floats into a buffer with 64 sentinel floats in front and behind, which must
    come back untouched."""
    a, keep = _head_args(x, spec)
    shape = (x.shape[0], int(spec.w2.shape[0]))
    n = int(np.prod(shape))
    buf = torch.full((64 + shift + n + 64,), SENTINEL, dtype=torch.float32, device="cuda")
    a.out = buf.data_ptr() + 4 * (64 + shift)
    h.mmp_head(a)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:64 + shift] == SENTINEL).all() and (got[64 + shift + n:] == SENTINEL).all(), "written outside the output"
    return got[64 + shift:64 + shift + n].reshape(shape)


@pytest.mark.parametrize("M", hr.ROWS_M)
@pytest.mark.parametrize("c", hr.CASES, ids=hr.case_id)
def test_kernel_against_the_restatement(handle, c, M):
    """The worst |out - ref| / bound is printed per case; the bound is a worst case over every order of summation."""
    assert hr.ROWS == nm._capi.MMP_HEAD_ROWS and M <= hr.M_MAX
    x, spec, want, bound = hr.case("random", *c)
    got = _run(handle, x[:M], spec)
    assert got.shape == (M, c[3]) and got.dtype == np.float32 and np.isfinite(got).all()
    ratio = np.abs(got - want[:M]) / bound[:M]
    print(f"{hr.case_id(c)} M {M}: worst |out - ref| / bound = {ratio.max():.4f}")
    assert ratio.max() <= 1.0


@pytest.mark.parametrize("c", hr.CASES, ids=hr.case_id)
def test_integer_head_is_exact(handle, c):
    x, spec, want, _ = hr.case("integer", *c)
    assert hr.integer_units(x, spec) < 2.0 ** 24              # no order of summation can round
    assert np.array_equal(x % 4, np.zeros_like(x)) and set(np.unique(spec.w1)) <= {-1.0, 0.0, 1.0} and spec.slope == 0.25
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    got = _run(handle, x, spec)
    assert np.array_equal(got, want.astype(np.float32)), (c, np.abs(got - want).max())


@pytest.mark.parametrize("c", [(16, 4, 7, 40), (128, 10, 11, 40)], ids=hr.case_id)
def test_bits_do_not_depend_on_batch_alignment_or_other_rows(handle, c):
    x, spec, _, _ = hr.case("random", *c)
    full = _run(handle, x, spec)
    for k in (0, 1, hr.ROWS - 1, hr.ROWS, hr.M_MAX - 1):     # a row alone sits in lane 0 of its group; in the batch anywhere
        assert np.array_equal(_run(handle, x[k:k + 1], spec)[0], full[k]), k
    for shift in (1, 2, 3):                                # out offset by 4, 8 and 12 bytes: with 0, four float alignments
        assert np.array_equal(_run(handle, x, spec, shift), full), shift
    other = x.copy()
    other[2] = hr.random_x(1, *x.shape[1:], seed=99)[0]
    got = _run(handle, other, spec)
    assert np.array_equal(np.delete(got, 2, axis=0), np.delete(full, 2, axis=0)) and not np.array_equal(got[2], full[2])


def test_errors(handle):
    C, H, W, O = 8, 5, 7, 40
    x, spec = hr.random_x(3, C, H, W, seed=1), hr.random_head(C, H, W, O, 2)
    n_out = 3 * O
    out = torch.full((64 + n_out + 64,), SENTINEL, dtype=torch.float32, device="cuda")
    o0 = out.data_ptr() + 256

    def make(**over):
        a, keep = _head_args(x, spec)
        a.out = o0
        for k, v in over.items():
            setattr(a, k, v)
        return a, keep

    def code(a):
        with pytest.raises(nm.NmpcError) as e:
            handle.mmp_head(a)
        assert str(e.value)                                # each refusal carries a message
        return e.value.code
    bad = {name + " = NULL": dict(**{name: None}) for name in ("x", "out") + POINTERS}
    bad.update({"H = 1": dict(H=1), "W = 1": dict(W=1), "H = 0": dict(H=0), "W < 0": dict(W=-2), "C = 0": dict(C=0), "C < 0": dict(C=-8),
                "O = 0": dict(O=0), "O = 1": dict(O=1), "O = 41": dict(O=41), "O = 514": dict(O=514), "O < 0": dict(O=-2), "M < 0": dict(M=-1),
                "slope = nan": dict(slope=float("nan")), "slope = inf": dict(slope=float("inf")), "slope = 1.5": dict(slope=1.5),
                "slope = -2": dict(slope=-2.0), "out misaligned": dict(out=o0 + 2)})
    a0, keep0 = make()
    bad.update({name + " misaligned": dict(**{name: getattr(a0, name) + 2}) for name in ("x",) + POINTERS})
    for what, over in bad.items():
        a, keep = make(**over)
        assert code(a) == -1, what
    # out overlapping x, by one float at either end, with the extents M C H W of x and M O of out
    a, keep = make()
    n_x = 3 * C * H * W
    for o in (a.x, a.x + n_x * 4 - 4, a.x - n_out * 4 + 4):
        a.out = o
        assert code(a) == -1, o - a.x
    # sizes the kernel's ints do not hold: refused as unsupported before anything is looked at on the device
    for over in (dict(H=2 ** 31 - 1), dict(W=2 ** 31 - 1), dict(C=2 ** 31 - 1), dict(C=2 ** 20, H=64, W=64)):
        a, keep = make(**over)
        assert code(a) == -4, over
    lib = nm.load_library()
    a, keep = make()
    assert lib.nmpc_mmp_head_f32(None, ctypes.byref(a)) == -1 and lib.nmpc_mmp_head_f32(handle._h, None) == -1
    # a host pointer is refused, not dereferenced
    host = np.zeros(128 * C * H * W, dtype=np.float32)
    for name in ("w1", "c2", "x"):
        a, keep = make(**{name: host.ctypes.data})
        assert code(a) == -1, name
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), "a refused call wrote to the output"
    a, keep = make(M=0)
    handle.mmp_head(a)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    a, keep = make()
    handle.mmp_head(a)
    torch.cuda.synchronize()
    assert bool((out[64:-64] != SENTINEL).all()) and bool((out[:64] == SENTINEL).all()) and bool((out[-64:] == SENTINEL).all())
