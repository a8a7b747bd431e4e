"""GPU tests of the fused residual block of the multi-hypothesis predictor's network (nmpc_mmp_block_f32, csrc/nmpc_mmp_block.h)
through the C ABI, against the float64 restatement of tests/mmp_block_reference.py and its derived bound (see there).

The planes are chosen around the kernel's tile of 15 x 28 outputs: 3 x 5 (smaller than a tile), 15 x 28 (one tile exactly),
16 x 29 (one row and one column more), 19 x 37 (two tiles each way with remainders), and the warehouse's 74 x 83 once. Input
channels: 8 and 64 with the projection (one and eight chunks of the streamed input), 16 without. Every call writes into a
buffer with 64 sentinel floats in front and behind.

Worst |out - ref| / bound measured on an MI355X: 0.0061 (19 x 37, Cin 8, M 3); 0.0007 on the 74 x 83 plane at Cin 64. The
bound is a worst case over every order of summation, so a correct kernel sits far below it (torch's own float32 ops on the
CPU: 0.0084); the two wrong variants of the controls exceed it by factors of more than 180."""
import ctypes

import numpy as np
import pytest
import torch

import dyobav_mpcnwta_warehouse_amd as nm
import mmp_block_reference as br
import oracle
from conftest import config_for

pytestmark = pytest.mark.gpu

SENTINEL = -777.0
POINTERS = ("w1", "s1", "b1", "w2", "s2", "b2", "wd", "sd", "bd")


@pytest.fixture(scope="module")
def handle():
    with nm.Handle(config_for(oracle.Problem())) as h:
        h.set_stream(torch.cuda.current_stream().cuda_stream)
        yield h


def _block_args(x, spec):
    """NmpcMmpBlockArgs of x [M, Cin, H, W] (numpy) and a BlockSpec, everything uploaded; ``out`` is left to the caller."""
    a = nm._capi.NmpcMmpBlockArgs()
    keep = {"x": torch.from_numpy(np.array(x, dtype=np.float32)).cuda()}
    a.M, a.Cin, a.H, a.W = (int(v) for v in x.shape)
    a.x = keep["x"].data_ptr()
    for name in POINTERS:
        v = getattr(spec, name)
        if v is not None:
            keep[name] = torch.from_numpy(np.array(v, dtype=np.float32)).cuda()
            setattr(a, name, keep[name].data_ptr())
    a.slope_mid, a.slope_out = spec.slope_mid, spec.slope_out
    return a, keep


def _run(h, x, spec, shift=0):
    """The kernel's output [M, 16, H, W] float32. It lies ``shift`` floats into a buffer with 64 sentinel floats in front and
    behind, which must come back untouched."""
    a, keep = _block_args(x, spec)
    shape = (x.shape[0], 16) + tuple(x.shape[2:])
    n = int(np.prod(shape))
    buf = torch.full((64 + shift + n + 64,), SENTINEL, dtype=torch.float32, device="cuda")
    a.out = buf.data_ptr() + 4 * (64 + shift)
    h.mmp_block(a)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:64 + shift] == SENTINEL).all() and (got[64 + shift + n:] == SENTINEL).all(), "written outside the output"
    return got[64 + shift:64 + shift + n].reshape(shape)


def _controls(x, spec, want, bound):
    """On the same inputs: torch's own float32 ops are admitted by the bound, each of the two wrong variants is not."""
    assert (np.abs(br.torch_float32(x, spec) - want) <= bound).all(), "the bound refuses torch's own float32 block"
    for wrong in ("slope", "halo"):
        bad, _ = br.block(x, spec, wrong=wrong)
        assert not (np.abs(bad - want) <= bound).all(), f"the bound admits the wrong variant {wrong!r}"


# ---- 1. the kernel against the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("Cin,projection", br.CHANNELS, ids=[f"c{c}" for c, _ in br.CHANNELS])
@pytest.mark.parametrize("plane", br.PLANES, ids=[f"{h}x{w}" for h, w in br.PLANES])
def test_kernel_against_the_restatement(handle, plane, Cin, projection, M):
    x, spec, want, bound = br.case("random", *plane, Cin, projection)
    assert (x < 0).any() and (x > 0).any() and (spec.s1 < 0).any() and (spec.s1 > 0).any() and (spec.b1 != 0).all()
    assert (spec.wd is not None) == projection and spec.slope_mid == 0.1 and spec.slope_out == 0.01
    got = _run(handle, x[:M], spec)
    assert got.shape == (M, 16) + plane and got.dtype == np.float32 and np.isfinite(got).all()
    ratio = np.abs(got - want[:M]) / bound[:M]
    print(f"{plane} Cin {Cin} M {M}: worst |out - ref| / bound = {ratio.max():.4f}")
    assert ratio.max() <= 1.0
    if M == 1:
        _controls(x, spec, want, bound)


def test_warehouse_plane_in_full(handle):
    H, W, Cin = 74, 83, 64
    x, spec = br.random_x(2, Cin, H, W, seed=74), br.random_block(Cin, 83, True)
    want, bound = br.block(x, spec)
    got = _run(handle, x, spec)
    ratio = np.abs(got - want) / bound
    print(f"74 x 83 Cin 64 M 2: worst |out - ref| / bound = {ratio.max():.4f}")
    assert got.shape == (2, 16, H, W) and np.isfinite(got).all() and ratio.max() <= 1.0
    _controls(x, spec, want, bound)


# ---- 2. exact: integer weights and inputs, every tap, both border rules and the channel mapping bit for bit -------------------------------
@pytest.mark.parametrize("Cin,projection", br.CHANNELS, ids=[f"c{c}" for c, _ in br.CHANNELS])
@pytest.mark.parametrize("plane", br.PLANES, ids=[f"{h}x{w}" for h, w in br.PLANES])
def test_integer_block_is_exact(handle, plane, Cin, projection):
    x, spec, want, _ = br.case("integer", *plane, Cin, projection)
    units = br.integer_units(x, spec)
    assert units < 2.0 ** 24, units                       # no order of summation can round
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want) and np.array_equal(x, np.round(x)) and np.abs(x).max() == 2
    assert spec.slope_mid == 0.125 and spec.slope_out == 0.25 and set(np.unique(spec.w1)) <= {-1.0, 0.0, 1.0}
    got = _run(handle, x, spec)
    assert np.array_equal(got, want.astype(np.float32)), (plane, Cin, np.abs(got - want).max())
    assert np.array_equal(br.torch_float32(x, spec), want.astype(np.float32))     # the control: torch's float32 is exact here too


def test_integer_block_is_exact_on_the_warehouse_plane(handle):
    """74 x 83 with M = 2 and Cin = 64: 5 x 3 tiles, the only plane here with tiles that have neighbours on all four sides."""
    x, spec, want, _ = br.case("integer", 74, 83, 64, True, 2)
    units = br.integer_units(x, spec)
    assert units < 2.0 ** 24, units
    assert x.shape == (2, 64, 74, 83) and np.array_equal(want.astype(np.float32).astype(np.float64), want) and np.abs(x).max() == 2
    got = _run(handle, x, spec)
    assert np.array_equal(got, want.astype(np.float32)), np.abs(got - want).max()


def test_doubling_block_doubles(handle):
    x = np.abs(br.random_x(2, 16, 16, 29, seed=5))
    got = _run(handle, x, br.doubling_block())
    assert np.array_equal(got, x + x)


# ---- 3. independence: the batch, the alignment of out and the other rows do not change a bit ----------------------------------------------
def test_bits_do_not_depend_on_batch_alignment_or_other_rows(handle):
    x, spec, _, _ = br.case("random", 19, 37, 64, True)
    full = _run(handle, x, spec)
    for k in range(3):
        assert np.array_equal(_run(handle, x[k:k + 1], spec)[0], full[k]), k
    for shift in (1, 2, 4):                                # out offset by 4, 8 and 16 bytes
        assert np.array_equal(_run(handle, x, spec, shift), full), shift
    other = x.copy()
    other[2] = br.random_x(1, 64, 19, 37, seed=99)[0]
    got = _run(handle, other, spec)
    assert np.array_equal(got[:2], full[:2]) and not np.array_equal(got[2], full[2])


# ---- 4. argument errors: refused on the host side, nothing is launched --------------------------------------------------------------------
def test_errors(handle):
    H, W = 16, 29
    x8, proj = br.random_x(2, 8, H, W, seed=1), br.random_block(8, 2, True)
    x16, plain = br.random_x(2, 16, H, W, seed=3), br.random_block(16, 4, False)
    out = torch.full((64 + 2 * 16 * H * W + 64,), SENTINEL, dtype=torch.float32, device="cuda")
    o0 = out.data_ptr() + 256

    def make(x_=x8, spec_=proj, **over):
        a, keep = _block_args(x_, spec_)
        a.out = o0
        for k, v in over.items():
            setattr(a, k, v)
        return a, keep

    def code(a):
        with pytest.raises(nm.NmpcError) as e:
            handle.mmp_block(a)
        return e.value.code
    bad = {name + " = NULL": dict(**{name: None}) for name in ("x", "out") + POINTERS}
    bad.update({"Cin = 0": dict(Cin=0), "Cin = 4": dict(Cin=4), "Cin = 12": dict(Cin=12), "Cin = 264": dict(Cin=264), "Cin < 0": dict(Cin=-8),
                "H = 0": dict(H=0), "W = 0": dict(W=0), "M < 0": dict(M=-1), "slope_mid = nan": dict(slope_mid=float("nan")),
                "slope_mid = inf": dict(slope_mid=float("inf")), "slope_out = nan": dict(slope_out=float("nan")),
                "slope_out = -inf": dict(slope_out=float("-inf")), "out misaligned": dict(out=o0 + 2)})
    for what, over in bad.items():
        a, keep = make(**over)
        assert code(a) == -1, what
    # wd = NULL above was refused because Cin = 8 has no identity; so is Cin = 64, and sd / bd only count with wd
    a, keep = make(x_=br.random_x(1, 64, H, W, seed=5), spec_=br.random_block(64, 6, False))
    assert code(a) == -1
    for name in ("x", "out", "w1", "s1", "b1", "w2", "s2", "b2"):
        a, keep = make(x_=x16, spec_=plain, **{name: None})
        assert code(a) == -1, name
    # out overlapping x: in place, and by one float at either end
    a, keep = make(x_=x16, spec_=plain)
    n_x = 2 * 16 * H * W * 4
    for o in (a.x, a.x + n_x - 4, a.x - n_x + 4):
        a.out = o
        assert code(a) == -1, o - a.x
    # more than 2^31 - 1 workgroups: refused as unsupported before anything is looked at on the device
    a, keep = make(M=1 << 16, H=4096, W=4096)
    assert code(a) == -4
    # (no int overflow on the way to the count: H + 14 and W + 27 do not fit an int here)
    for over in (dict(H=2 ** 31 - 1, W=4096), dict(H=4096, W=2 ** 31 - 1), dict(M=2 ** 31 - 1, H=2 ** 31 - 1, W=2 ** 31 - 1)):
        a, keep = make(**over)
        assert code(a) == -4, over
    lib = nm.load_library()
    a, keep = make()
    assert lib.nmpc_mmp_block_f32(None, ctypes.byref(a)) == -1 and lib.nmpc_mmp_block_f32(handle._h, None) == -1
    # a host pointer is refused, not dereferenced
    host = np.zeros(16 * 8 * 9, dtype=np.float32)
    for name in ("w1", "bd"):
        a, keep = make(**{name: host.ctypes.data})
        assert code(a) == -1, name
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), "a refused call wrote to the output"
    a, keep = make(M=0)
    handle.mmp_block(a)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    for x, spec in ((x8, proj), (x16, plain)):
        a, keep = make(x_=x, spec_=spec)
        handle.mmp_block(a)
        torch.cuda.synchronize()
        assert bool((out[64:-64] != SENTINEL).all()) and bool((out[:64] == SENTINEL).all()) and bool((out[-64:] == SENTINEL).all())
        out.fill_(SENTINEL)
