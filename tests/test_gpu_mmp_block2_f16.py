"""GPU tests of the layer2 block with binary16 MFMA operands (nmpc_mmp_block2_f16, csrc/nmpc_mmp_block2_f16.h) through the C ABI,
against the float64 model of tests/mmp_block2_f16_reference.py and its derived bound (the controls of that bound run without a
device in tests/test_mmp_block2_f16_cpu.py). The rule under test: whatever an MFMA reads is binary16 -- the weights (rounded once,
``mmp_stem.pack_block2_f16``), x as it is staged, m as it goes to LDS --, rounded to nearest even, saturated at +-65504, subnormals
kept; nothing else is.

The cases are those of tests/test_gpu_mmp_block2.py (``mmp_block2_reference.CASES`` and ``REAL``); every call writes into a buffer
with 64 sentinel floats in front and behind. What the result reads outside its arguments: tests/test_gpu_read_bounds_mmp2_f16.py.

Worst |out - ref| / bound measured on an MI355X: 0.2300 (4 x 6, Cin 8, stride 2, M 3; ``emulate`` on the CPU: the same 0.230); 0.1793
and 0.1602 on the two warehouse planes; 0.2679 with |x| up to 1e5. The subnormal test passes: the gfx950 MFMA keeps binary16
subnormals."""
import ctypes

import numpy as np
import pytest
import torch

import dyobav_mpcnwta_warehouse_amd as nm
import mmp_block2_f16_reference as h2
import mmp_block2_reference as b2
import oracle
from conftest import config_for
from dyobav_mpcnwta_warehouse_amd.mmp_stem import pack_block2_f16, round_f16

pytestmark = pytest.mark.gpu

SENTINEL = -777.0
POINTERS = ("w1", "s1", "b1", "w2", "s2", "b2", "wd", "sd", "bd")
PACKED = ("w1", "w2", "wd")


@pytest.fixture(scope="module")
def handle():
    with nm.Handle(config_for(oracle.Problem())) as h:
        h.set_stream(torch.cuda.current_stream().cuda_stream)
        yield h


def _upload(name, v):
    """A spec's array as the kernel takes it: the packed ones as int16 bit patterns, the others as float32."""
    return torch.from_numpy(np.ascontiguousarray(v).view(np.int16) if name in PACKED else np.array(v, dtype=np.float32)).cuda()


def _block_args(x, spec):
    """NmpcMmpBlock2F16Args of x [M, Cin, H, W] (numpy) and a Block2Spec (packed here), everything uploaded; ``out`` is left to the caller."""
    a = nm._capi.NmpcMmpBlock2F16Args()
    packed = pack_block2_f16(spec)
    keep = {"x": torch.from_numpy(np.array(x, dtype=np.float32)).cuda()}
    a.M, a.Cin, a.H, a.W = (int(v) for v in x.shape)
    a.stride = int(spec.stride)
    a.x = keep["x"].data_ptr()
    for name in POINTERS:
        v = getattr(packed, name)
        if v is not None:
            keep[name] = _upload(name, v)
            assert name not in PACKED or keep[name].data_ptr() % 16 == 0
            setattr(a, name, keep[name].data_ptr())
    a.slope_mid, a.slope_out = spec.slope_mid, spec.slope_out
    return a, keep


def _run(h, x, spec, shift=0):
    """The kernel's output [M, 32, H2, W2] float32. It lies ``shift`` floats into a buffer with 64 sentinel floats in front and
    behind, which must come back untouched."""
    a, keep = _block_args(x, spec)
    shape = (x.shape[0], 32) + b2.out_plane(x.shape[2], x.shape[3], spec.stride)
    n = int(np.prod(shape))
    buf = torch.full((64 + shift + n + 64,), SENTINEL, dtype=torch.float32, device="cuda")
    a.out = buf.data_ptr() + 4 * (64 + shift)
    h.mmp_block2_f16(a)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:64 + shift] == SENTINEL).all() and (got[64 + shift + n:] == SENTINEL).all(), "written outside the output"
    return got[64 + shift:64 + shift + n].reshape(shape)


# ---- 1. the kernel against the model -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("c", b2.CASES, ids=b2.case_id)
def test_kernel_against_the_model(handle, c, M):
    """Worst |out - ref| / bound measured on an MI355X over all cases: 0.2300 (printed per case). ``emulate``, torch's float32
    convolutions under the same rule on the CPU, lies at most 0.230 of the bound; the wrong variants exceed it 78 times and more
    (tests/test_mmp_block2_f16_cpu.py)."""
    H, W, Cin, stride, projection = c
    x, spec, want, bound = h2.case("random", *c)
    assert (x < 0).any() and (x > 0).any() and (spec.wd is not None) == projection and spec.stride == stride
    got = _run(handle, x[:M], spec)
    assert got.shape == (M, 32) + b2.out_plane(H, W, stride) and got.dtype == np.float32 and np.isfinite(got).all()
    ratio = np.abs(got - want[:M]) / bound[:M]
    print(f"{b2.case_id(c)} M {M}: worst |out - ref| / bound = {ratio.max():.4f}")
    assert ratio.max() <= 1.0


@pytest.mark.parametrize("c", b2.REAL, ids=b2.case_id)
def test_warehouse_planes_in_full(handle, c):
    """74 x 83 with Cin 16 at stride 2 and 37 x 42 with 32 -> 32, once each at M = 2. Measured on an MI355X: 0.1793 and 0.1602."""
    x, spec, want, bound = h2.case("random", *c, 2)
    got = _run(handle, x, spec)
    ratio = np.abs(got - want) / bound
    print(f"{b2.case_id(c)} M 2: worst |out - ref| / bound = {ratio.max():.4f}")
    assert got.shape == want.shape and np.isfinite(got).all() and ratio.max() <= 1.0


# a strided block stages half a K block per chunk: Cin = 32 is both halves of one K block, Cin = 64 two K blocks (tests only; the
# network's strided block has 16 channels, one chunk)
STRIDED_CHUNKS = [(17, 89, 32, 2, True), (16, 88, 64, 2, True)]


@pytest.mark.parametrize("c", STRIDED_CHUNKS, ids=b2.case_id)
def test_strided_block_with_more_than_one_chunk(handle, c):
    x, spec, want, bound = h2.case("random", *c, 2)
    got = _run(handle, x, spec)
    ratio = np.abs(got - want) / bound
    print(f"{b2.case_id(c)} M 2: worst |out - ref| / bound = {ratio.max():.4f}")
    assert got.shape == want.shape and np.isfinite(got).all() and ratio.max() <= 1.0
    xi, si, wi, _ = b2.case("integer", *c, 2)
    assert b2.integer_units(xi, si) < 2.0 ** 24 and np.array_equal(_run(handle, xi, si), wi.astype(np.float32))


# ---- 2. exact: every operand and every m of the integer cases is a binary16 value, so the float32 reference's bits ---------------------------
@pytest.mark.parametrize("c", b2.CASES + b2.REAL, ids=b2.case_id)
def test_integer_block_is_exact(handle, c):
    x, spec, want, _ = b2.case("integer", *c, 2 if c in b2.REAL else b2.M_MAX)
    assert b2.integer_units(x, spec) < 2.0 ** 24
    got = _run(handle, x, spec)
    assert np.array_equal(got, want.astype(np.float32)), (c, np.abs(got - want).max())


def test_exact_blocks_double_and_duplicate(handle):
    x = round_f16(np.abs(b2.random_x(2, 32, 9, 45, seed=5))).astype(np.float32)
    assert np.array_equal(_run(handle, x, b2.doubling_block2()), x + x)
    x = round_f16(np.abs(b2.random_x(2, 16, 17, 89, seed=6))).astype(np.float32)
    half = x[:, :, ::2, ::2]
    assert np.array_equal(_run(handle, x, b2.duplicate_and_double_block2()), np.concatenate([half + half, half + half], axis=1))


# ---- 3. the ends of binary16: subnormals are kept, large values saturate, a NaN stays in its row ----------------------------------------------
def _ternary_block(Cin, stride, projection, seed):
    """Ternary weights (a quarter non-zero), scales 1, shifts 0, both slopes 1: on x = k 2^-24 every product, every sum, m = conv1
    and the output are integer multiples of 2^-24 -- exact in float32, and m, below 2^-13, is a binary16 value, mostly a subnormal."""
    s = b2.integer_block2(Cin, seed, stride, projection)
    one, zero = np.ones(32, dtype=np.float32), np.zeros(32, dtype=np.float32)
    return s._replace(s1=one, b1=zero, s2=one, b2=zero, slope_mid=1.0, slope_out=1.0, **({"sd": one, "bd": zero} if projection else {}))


@pytest.mark.parametrize("c", [(17, 89, 16, 2, True), (9, 45, 32, 1, False)], ids=b2.case_id)
def test_subnormal_operands_are_kept(handle, c):
    """x = k 2^-24, |k| <= 2: binary16 subnormals. With ternary weights, unit scales and slopes 1, m is a small multiple of 2^-24 --
    a subnormal again -- and the exact result is the float64 one. A device that flushed f16 subnormals in the MFMA would give 0
    for z and for the projection."""
    H, W, Cin, stride, projection = c
    spec = _ternary_block(Cin, stride, projection, seed=3)
    x = (b2.integer_x(2, Cin, H, W, seed=4) * np.float32(2.0 ** -24)).astype(np.float32)
    want, _ = b2.block(x, spec)
    m_max = 2 * 9 * Cin * 2.0 ** -24
    assert m_max < 2.0 ** -13 and np.abs(want).max() > 0     # every multiple of 2^-24 below 2^-13 is a binary16 value; something is there to lose
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    got = _run(handle, x, spec)
    assert np.array_equal(got, want.astype(np.float32)), np.abs(got - want).max() / 2.0 ** -24


@pytest.mark.parametrize("c", [(17, 89, 16, 2, True), (9, 45, 32, 1, False), (9, 45, 24, 1, True)], ids=b2.case_id)
def test_large_values_saturate_and_stay_within_the_bound(handle, c):
    """Finite |x| up to 1e5 (a twentieth of the values beyond +-65504): the output is finite and within the model's bound; the
    model clips before it rounds."""
    x, spec, _, _ = b2.case("random", *c)
    rng = np.random.default_rng(17)
    x = x.copy()
    big = rng.random(x.shape) < 0.05
    x[big] = (rng.uniform(6e4, 1e5, x.shape) * rng.choice([-1.0, 1.0], x.shape)).astype(np.float32)[big]
    assert (np.abs(x) > 65504).any() and np.abs(x).max() <= 1e5
    want, bound = h2.block(x, spec)
    got = _run(handle, x, spec)
    ratio = np.abs(got - want) / bound
    print(f"{b2.case_id(c)}: worst |out - ref| / bound = {ratio.max():.4f} with |x| up to {np.abs(x).max():.0f}")
    assert np.isfinite(got).all() and ratio.max() <= 1.0


@pytest.mark.parametrize("c", [(17, 89, 16, 2, True), (9, 45, 32, 1, False)], ids=b2.case_id)
def test_a_nan_stays_in_its_row(handle, c):
    x, spec, _, _ = b2.case("random", *c)
    full = _run(handle, x, spec)
    bad = x.copy()
    bad[1, 3, 2, 4] = np.nan
    got = _run(handle, bad, spec)
    assert np.array_equal(got[0], full[0]) and np.array_equal(got[2], full[2]) and np.isnan(got[1]).any()


# ---- 4. independence: the batch, the alignment of out and the other rows do not change a bit ----------------------------------------------
@pytest.mark.parametrize("c", [(17, 89, 16, 2, True), (9, 45, 64, 1, True), (9, 45, 32, 1, False)], ids=b2.case_id)
def test_bits_do_not_depend_on_batch_alignment_or_other_rows(handle, c):
    x, spec, _, _ = b2.case("random", *c)
    full = _run(handle, x, spec)
    for k in range(3):
        assert np.array_equal(_run(handle, x[k:k + 1], spec)[0], full[k]), k
    for shift in (1, 2, 3):                                # out offset by 4, 8 and 12 bytes: with 0, four float alignments
        assert np.array_equal(_run(handle, x, spec, shift), full), shift
    other = x.copy()
    other[2] = b2.random_x(1, *x.shape[1:], seed=99)[0]
    got = _run(handle, other, spec)
    assert np.array_equal(got[:2], full[:2]) and not np.array_equal(got[2], full[2])


# ---- 5. argument errors: refused on the host side, nothing is launched --------------------------------------------------------------------
def test_errors(handle):
    H, W = 17, 29
    H2, W2 = b2.out_plane(H, W, 2)
    x8, proj = b2.random_x(2, 8, H, W, seed=1), b2.random_block2(8, 2, 2, True)
    x32, plain = b2.random_x(2, 32, H2, W2, seed=3), b2.random_block2(32, 4, 1, False)
    n_out = 2 * 32 * H2 * W2
    out = torch.full((64 + n_out + 64,), SENTINEL, dtype=torch.float32, device="cuda")
    o0 = out.data_ptr() + 256

    def make(x_=x8, spec_=proj, **over):
        a, keep = _block_args(x_, spec_)
        a.out = o0
        for k, v in over.items():
            setattr(a, k, v)
        return a, keep

    def code(a):
        with pytest.raises(nm.NmpcError) as e:
            handle.mmp_block2_f16(a)
        assert str(e.value)                                # each refusal carries a message
        return e.value.code
    bad = {name + " = NULL": dict(**{name: None}) for name in ("x", "out") + POINTERS}
    bad.update({"Cin = 0": dict(Cin=0), "Cin = 4": dict(Cin=4), "Cin = 12": dict(Cin=12), "Cin = 264": dict(Cin=264), "Cin < 0": dict(Cin=-8),
                "H = 0": dict(H=0), "W = 0": dict(W=0), "M < 0": dict(M=-1), "stride = 0": dict(stride=0), "stride = 3": dict(stride=3),
                "stride = -1": dict(stride=-1), "slope_mid = nan": dict(slope_mid=float("nan")),
                "slope_mid = inf": dict(slope_mid=float("inf")), "slope_out = nan": dict(slope_out=float("nan")),
                "slope_out = -inf": dict(slope_out=float("-inf")), "slope_mid = 1.5": dict(slope_mid=1.5), "slope_out = -2": dict(slope_out=-2.0),
                "out misaligned": dict(out=o0 + 2)})
    for what, over in bad.items():
        a, keep = make(**over)
        assert code(a) == -1, what
    # the packed arrays must be aligned to 16 bytes: every smaller alignment of each is refused
    for name in PACKED:
        for off in (2, 4, 8):
            a, keep = make()
            setattr(a, name, getattr(a, name) + off)
            assert code(a) == -1, (name, off)
    # wd = NULL above was refused because Cin = 8 at stride 2 has no identity; so are Cin = 64 at stride 1 and Cin = 32 at stride 2
    # (the packer itself refuses a spec 64 -> 32 without a projection: its projection is taken away here)
    a, keep = make(x_=b2.random_x(1, 64, H2, W2, seed=5), spec_=b2.random_block2(64, 6, 1, True), wd=None)
    assert code(a) == -1
    a, keep = make(x_=x32, spec_=plain, stride=2)
    assert code(a) == -1
    for name in ("x", "out", "w1", "s1", "b1", "w2", "s2", "b2"):      # sd / bd only count with wd
        a, keep = make(x_=x32, spec_=plain, **{name: None})
        assert code(a) == -1, name
    # out overlapping x, by one float at either end, with the extents M Cin H W of x and M 32 H2 W2 of out
    a, keep = make(x_=x32, spec_=plain)
    for o in (a.x, a.x + n_out * 4 - 4, a.x - n_out * 4 + 4):
        a.out = o
        assert code(a) == -1, o - a.x
    a, keep = make()                                       # stride 2: x has 2 * 8 * H * W floats, out 2 * 32 * H2 * W2
    n_x = 2 * 8 * H * W
    for o in (a.x, a.x + n_x * 4 - 4, a.x - n_out * 4 + 4):
        a.out = o
        assert code(a) == -1, o - a.x
    # more than 2^31 - 1 workgroups: refused as unsupported before anything is looked at on the device
    a, keep = make(M=1 << 16, H=4096, W=4096 * 4)
    assert code(a) == -4
    # (no int overflow on the way to the count, or in the kernel's pixel coordinates)
    for over in (dict(H=2 ** 31 - 1, W=4096), dict(H=4096, W=2 ** 31 - 1), dict(M=2 ** 31 - 1, H=2 ** 31 - 1, W=2 ** 31 - 1)):
        a, keep = make(**over)
        assert code(a) == -4, over
    lib = nm.load_library()
    a, keep = make()
    assert lib.nmpc_mmp_block2_f16(None, ctypes.byref(a)) == -1 and lib.nmpc_mmp_block2_f16(handle._h, None) == -1
    # a host pointer is refused, not dereferenced
    host = np.zeros(32 * 8 * 9 + 8, dtype=np.float32)
    aligned = host.ctypes.data + (-host.ctypes.data) % 16
    for name in ("w1", "bd"):
        a, keep = make(**{name: aligned})
        assert code(a) == -1, name
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), "a refused call wrote to the output"
    a, keep = make(M=0)
    handle.mmp_block2_f16(a)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    for x, spec in ((x8, proj), (x32, plain)):
        a, keep = make(x_=x, spec_=spec)
        handle.mmp_block2_f16(a)
        torch.cuda.synchronize()
        assert bool((out[64:-64] != SENTINEL).all()) and bool((out[:64] == SENTINEL).all()) and bool((out[-64:] == SENTINEL).all())
        out.fill_(SENTINEL)
