"""GPU tests of the layer1 block with binary16 MFMA operands (nmpc_mmp_block_f16, csrc/nmpc_mmp_block1_f16.h) through the C ABI,
against the float64 model of tests/mmp_block1_f16_reference.py and its derived bound (the controls of that bound run without a
device in tests/test_mmp_block1_f16_cpu.py). The rule under test is the one of tests/test_gpu_mmp_block2_f16.py: whatever an MFMA
reads is binary16 -- the weights (rounded once, ``mmp_stem.pack_block1_f16``), x as it is staged, m as it goes to LDS --, rounded to
nearest even, saturated at +-65504, subnormals kept; nothing else is.

The cases are those of tests/test_gpu_mmp_block.py (``mmp_block_reference.PLANES`` x ``CHANNELS``: Cin = 8 a quarter of a K block with
projection, 16 the identity kernel's half, 64 two chunks with projection) and the warehouse plane 74 x 83 once at M = 2 for 64 -> 16
and 16 -> 16; every call writes into a buffer with 64 sentinel floats in front and behind.

Worst |out - ref| / bound measured on an MI355X: 0.3108 (19 x 37, Cin 8; ``emulate`` on the CPU: the same 0.311); 0.1259 and 0.2472 on
the warehouse plane; 0.4092 with |x| up to 1e5 (16 x 29, Cin 8). The subnormal test passes."""
import ctypes

import numpy as np
import pytest
import torch

import dyobav_mpcnwta_warehouse_amd as nm
import mmp_block1_f16_reference as h1
import mmp_block_reference as br
import oracle
from conftest import config_for
from dyobav_mpcnwta_warehouse_amd import _capi
from dyobav_mpcnwta_warehouse_amd.mmp_stem import pack_block1_f16, round_f16
from guarded_buffers import IntPoison, run_guarded

pytestmark = pytest.mark.gpu

SENTINEL = -777.0
POINTERS = ("w1", "s1", "b1", "w2", "s2", "b2", "wd", "sd", "bd")
PACKED = ("w1", "w2", "wd")
C = br.C


@pytest.fixture(scope="module")
def handle():
    with nm.Handle(config_for(oracle.Problem())) as h:
        h.set_stream(torch.cuda.current_stream().cuda_stream)
        yield h


def _upload(name, v):
    """A spec's array as the kernel takes it: the packed ones as int16 bit patterns, the others as float32."""
    return torch.from_numpy(np.ascontiguousarray(v).view(np.int16) if name in PACKED else np.array(v, dtype=np.float32)).cuda()


def _block_args(x, spec):
    """NmpcMmpBlockF16Args of x [M, Cin, H, W] (numpy) and a BlockSpec (packed here), everything uploaded; ``out`` is left to the caller."""
    a = _capi.NmpcMmpBlockF16Args()
    packed = pack_block1_f16(spec)
    keep = {"x": torch.from_numpy(np.array(x, dtype=np.float32)).cuda()}
    a.M, a.Cin, a.H, a.W = (int(v) for v in x.shape)
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
    """The kernel's output [M, 16, H, W] float32. It lies ``shift`` floats into a buffer with 64 sentinel floats in front and behind,
    which must come back untouched."""
    a, keep = _block_args(x, spec)
    shape = (x.shape[0], C) + x.shape[2:]
    n = int(np.prod(shape))
    buf = torch.full((64 + shift + n + 64,), SENTINEL, dtype=torch.float32, device="cuda")
    a.out = buf.data_ptr() + 4 * (64 + shift)
    h.mmp_block_f16(a)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:64 + shift] == SENTINEL).all() and (got[64 + shift + n:] == SENTINEL).all(), "written outside the output"
    return got[64 + shift:64 + shift + n].reshape(shape)


# ---- 1. the kernel against the model -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("c", h1.CASES, ids=h1.case_id)
def test_kernel_against_the_model(handle, c, M):
    H, W, Cin, projection = c
    x, spec, want, bound = h1.case("random", *c)
    assert (x < 0).any() and (x > 0).any() and (spec.wd is not None) == projection
    got = _run(handle, x[:M], spec)
    assert got.shape == (M, C, H, W) and got.dtype == np.float32 and np.isfinite(got).all()
    ratio = np.abs(got - want[:M]) / bound[:M]
    print(f"{h1.case_id(c)} M {M}: worst |out - ref| / bound = {ratio.max():.4f}")
    assert ratio.max() <= 1.0


@pytest.mark.parametrize("c", h1.REAL, ids=h1.case_id)
def test_warehouse_plane_in_full(handle, c):
    """74 x 83 (3 x 5 tiles with remainders both ways) with 64 -> 16 and 16 -> 16, once each at M = 2."""
    x, spec, want, bound = h1.case("random", *c, 2)
    got = _run(handle, x, spec)
    ratio = np.abs(got - want) / bound
    print(f"{h1.case_id(c)} M 2: worst |out - ref| / bound = {ratio.max():.4f}")
    assert got.shape == want.shape and np.isfinite(got).all() and ratio.max() <= 1.0


# ---- 2. exact: every operand and every m of the integer cases is a binary16 value, so the float32 reference's bits ---------------------------
@pytest.mark.parametrize("c", h1.CASES + h1.REAL, ids=h1.case_id)
def test_integer_block_is_exact(handle, c):
    x, spec, want, _ = br.case("integer", *c, 2 if c in h1.REAL else br.M_MAX)
    assert br.integer_units(x, spec) < 2.0 ** 24
    got = _run(handle, x, spec)
    assert np.array_equal(got, want.astype(np.float32)), (c, np.abs(got - want).max())


def test_exact_block_doubles(handle):
    x = round_f16(np.abs(br.random_x(2, C, 16, 29, seed=5))).astype(np.float32)
    assert np.array_equal(_run(handle, x, br.doubling_block()), x + x)


# ---- 3. the ends of binary16: subnormals are kept, large values saturate, a NaN stays in its row ----------------------------------------------
def _ternary_block(Cin, projection, seed):
    """Ternary weights, scales 1, shifts 0, both slopes 1: on x = k 2^-24 every product, every sum, m = conv1 and the output are
    integer multiples of 2^-24 -- exact in float32, and m, below 2^-13, is a binary16 value, mostly a subnormal."""
    s = br.integer_block(Cin, seed, projection)
    one, zero = np.ones(C, dtype=np.float32), np.zeros(C, dtype=np.float32)
    return s._replace(s1=one, b1=zero, s2=one, b2=zero, slope_mid=1.0, slope_out=1.0, **({"sd": one, "bd": zero} if projection else {}))


ENDS = [(16, 29, 64, True), (16, 29, 16, False)]


@pytest.mark.parametrize("c", ENDS, ids=h1.case_id)
def test_subnormal_operands_are_kept(handle, c):
    """x = k 2^-24, |k| <= 2: binary16 subnormals; m is a small multiple of 2^-24 -- a subnormal again -- and the exact result is the
    float64 one. A device that flushed f16 subnormals in the MFMA would give 0 for z and for the projection."""
    H, W, Cin, projection = c
    spec = _ternary_block(Cin, projection, seed=3)
    x = (br.integer_x(2, Cin, H, W, seed=4) * np.float32(2.0 ** -24)).astype(np.float32)
    want, _ = br.block(x, spec)
    assert 2 * 9 * Cin * 2.0 ** -24 < 2.0 ** -13 and np.abs(want).max() > 0
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    got = _run(handle, x, spec)
    assert np.array_equal(got, want.astype(np.float32)), np.abs(got - want).max() / 2.0 ** -24


@pytest.mark.parametrize("c", ENDS + [(16, 29, 8, True)], ids=h1.case_id)
def test_large_values_saturate_and_stay_within_the_bound(handle, c):
    """Finite |x| up to 1e5 (a twentieth of the values beyond +-65504): the output is finite and within the model's bound; the model
    clips before it rounds."""
    x, spec, _, _ = h1.case("random", *c)
    rng = np.random.default_rng(17)
    x = x.copy()
    big = rng.random(x.shape) < 0.05
    x[big] = (rng.uniform(6e4, 1e5, x.shape) * rng.choice([-1.0, 1.0], x.shape)).astype(np.float32)[big]
    assert (np.abs(x) > 65504).any() and np.abs(x).max() <= 1e5
    want, bound = h1.block(x, spec)
    got = _run(handle, x, spec)
    ratio = np.abs(got - want) / bound
    print(f"{h1.case_id(c)}: worst |out - ref| / bound = {ratio.max():.4f} with |x| up to {np.abs(x).max():.0f}")
    assert np.isfinite(got).all() and ratio.max() <= 1.0


@pytest.mark.parametrize("c", ENDS, ids=h1.case_id)
def test_a_nan_stays_in_its_row(handle, c):
    x, spec, _, _ = h1.case("random", *c)
    full = _run(handle, x, spec)
    bad = x.copy()
    bad[1, 3, 2, 4] = np.nan
    got = _run(handle, bad, spec)
    assert np.array_equal(got[0], full[0]) and np.array_equal(got[2], full[2]) and np.isnan(got[1]).any()


# ---- 4. independence: the batch, the alignment of out and the other rows do not change a bit ----------------------------------------------
@pytest.mark.parametrize("c", [(19, 37, 8, True), (19, 37, 64, True), (19, 37, 16, False)], ids=h1.case_id)
def test_bits_do_not_depend_on_batch_alignment_or_other_rows(handle, c):
    x, spec, _, _ = h1.case("random", *c)
    full = _run(handle, x, spec)
    for k in range(3):
        assert np.array_equal(_run(handle, x[k:k + 1], spec)[0], full[k]), k
    for shift in (1, 2, 3):                                # out offset by 4, 8 and 12 bytes: with 0, four float alignments
        assert np.array_equal(_run(handle, x, spec, shift), full), shift
    other = x.copy()
    other[2] = br.random_x(1, *x.shape[1:], seed=99)[0]
    got = _run(handle, other, spec)
    assert np.array_equal(got[:2], full[:2]) and not np.array_equal(got[2], full[2])


# ---- 5. the result depends on no memory outside the arguments: one case per kernel of float32 memory -----------------------------------------
@pytest.mark.parametrize("c", [(16, 29, 64, True), (16, 29, 16, False)], ids=h1.case_id)
def test_the_result_depends_on_no_memory_outside_the_arguments(handle, c):
    """tests/guarded_buffers.py: every array the entry reads lies between poisoned pads, each poison in turn; the output keeps its
    bits and the pads come back untouched. (The kernels of binary16 memory: tests/test_gpu_mmp_block1_f16_io.py.)"""
    H, W, Cin, projection = c
    x, spec, want, bound = h1.case("random", *c)
    packed = pack_block1_f16(spec)
    inputs = {"x": np.array(x[:2], dtype=np.float32)}
    for k in POINTERS:
        v = getattr(packed, k)
        inputs[k] = None if v is None else np.ascontiguousarray(v).view(np.int16) if k in PACKED else np.array(v, dtype=np.float32)
    bits = IntPoison((0x7E00, 0x7BFF), -32768, 32767)

    def call(t):
        a = _capi.NmpcMmpBlockF16Args()
        a.M, a.Cin, a.H, a.W = 2, Cin, H, W
        for k, v in t.items():
            setattr(a, k, None if v is None else v.data_ptr())
        a.slope_mid, a.slope_out = spec.slope_mid, spec.slope_out
        out = torch.full((2, C, H, W), float("nan"), dtype=torch.float32, device="cuda")
        a.out = out.data_ptr()
        handle.mmp_block_f16(a)
        torch.cuda.synchronize()
        return {"out": out}
    given = [k for k, v in inputs.items() if v is not None]
    got = run_guarded(call, inputs, device="cuda", int_poisons={k: bits for k in PACKED if k in given},
                      odd_pad=[k for k in given if k not in PACKED])["out"]
    assert np.isfinite(got).all() and (np.abs(got - want[:2]) <= bound[:2]).all()


# ---- 6. argument errors: refused on the host side, nothing is launched --------------------------------------------------------------------
def test_errors(handle):
    H, W = 17, 29
    x8, proj = br.random_x(2, 8, H, W, seed=1), br.random_block(8, 2, True)
    x16, plain = br.random_x(2, 16, H, W, seed=3), br.random_block(16, 4, False)
    n_out = 2 * C * H * W
    out = torch.full((64 + n_out + 64,), SENTINEL, dtype=torch.float32, device="cuda")
    o0 = out.data_ptr() + 256

    def make(x_=x8, spec_=proj, **over):
        a, keep = _block_args(x_, spec_)
        a.out = o0
        for k, v in over.items():
            setattr(a, k, v)
        return a, keep

    def code(a, text="nmpc_mmp_block_f16"):
        with pytest.raises(nm.NmpcError) as e:
            handle.mmp_block_f16(a)
        assert text in str(e.value), str(e.value)
        return e.value.code
    bad = {name + " = NULL": dict(**{name: None}) for name in ("x", "out") + POINTERS}
    bad.update({"Cin = 0": dict(Cin=0), "Cin = 4": dict(Cin=4), "Cin = 12": dict(Cin=12), "Cin = 264": dict(Cin=264), "Cin < 0": dict(Cin=-8),
                "H = 0": dict(H=0), "W = 0": dict(W=0), "M < 0": dict(M=-1), "slope_mid = nan": dict(slope_mid=float("nan")),
                "slope_mid = inf": dict(slope_mid=float("inf")), "slope_out = nan": dict(slope_out=float("nan")),
                "slope_out = -inf": dict(slope_out=float("-inf")), "slope_mid = 1.5": dict(slope_mid=1.5), "slope_out = -2": dict(slope_out=-2.0),
                "out misaligned": dict(out=o0 + 2)})
    for what, over in bad.items():
        a, keep = make(**over)
        assert code(a) == -1, what
    a, keep = make(Cin=12)
    assert code(a, "is no multiple of 8") == -1
    for name in PACKED:                                    # the packed arrays must be aligned to 16 bytes
        for off in (2, 4, 8):
            a, keep = make()
            setattr(a, name, getattr(a, name) + off)
            assert code(a, "w1, w2 or wd is not aligned to 16 bytes") == -1, (name, off)
    # wd = NULL above was refused because Cin = 8 has no identity; so is Cin = 64
    a, keep = make(x_=br.random_x(1, 64, H, W, seed=5), spec_=br.random_block(64, 6, True), wd=None)
    assert code(a, "without a projection") == -1
    for name in ("x", "out", "w1", "s1", "b1", "w2", "s2", "b2"):      # sd / bd only count with wd
        a, keep = make(x_=x16, spec_=plain, **{name: None})
        assert code(a) == -1, name
    a, keep = make(x_=x16, spec_=plain)                    # out overlapping x, by one float at either end
    for o in (a.x, a.x + n_out * 4 - 4, a.x - n_out * 4 + 4):
        a.out = o
        assert code(a, "out overlaps x") == -1, o - a.x
    a, keep = make(M=1 << 16, H=4096, W=4096 * 4)          # more than 2^31 - 1 workgroups
    assert code(a) == -4
    for over in (dict(H=2 ** 31 - 1, W=4096), dict(H=4096, W=2 ** 31 - 1), dict(M=2 ** 31 - 1, H=2 ** 31 - 1, W=2 ** 31 - 1)):
        a, keep = make(**over)
        assert code(a) == -4, over
    lib = nm.load_library()
    a, keep = make()
    assert lib.nmpc_mmp_block_f16(None, ctypes.byref(a)) == -1 and lib.nmpc_mmp_block_f16(handle._h, None) == -1
    host = np.zeros(C * 8 * 9 + 8, dtype=np.float32)       # a host pointer is refused, not dereferenced
    aligned = host.ctypes.data + (-host.ctypes.data) % 16
    for name in ("w1", "bd"):
        a, keep = make(**{name: aligned})
        assert code(a) == -1, name
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), "a refused call wrote to the output"
    a, keep = make(M=0)
    handle.mmp_block_f16(a)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    for x, spec in ((x8, proj), (x16, plain)):
        a, keep = make(x_=x, spec_=spec)
        handle.mmp_block_f16(a)
        torch.cuda.synchronize()
        assert bool((out[64:-64] != SENTINEL).all()) and bool((out[:64] == SENTINEL).all()) and bool((out[-64:] == SENTINEL).all())
        out.fill_(SENTINEL)
