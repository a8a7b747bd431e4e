"""GPU tests of the residual blocks on binary16 MFMA operands with BINARY16 ACTIVATIONS in memory (``nmpc_mmp_block{2,3,4}_f16_io``,
csrc/nmpc_mmp_block_f16.h: ``x`` and / or ``out`` in the octet form ``[M][C / 8][H][W][8]``), through the C ABI.

The arithmetic and its order are those of ``nmpc_mmp_block{2,3,4}_f16`` on float32 memory, so there is no tolerance here: with
``K`` that entry, ``pack`` = ``mmp_stem.pack_activations_f16`` (the rule's rounding, on the host), ``x0`` a case's random float32
input and ``xr = float32(round_f16(x0))``,

    io(1, 0) on pack(xr) == K(xr)        io(0, 1) on x0 == pack(K(x0))        io(1, 1) on pack(xr) == pack(K(xr))        io(0, 0) == K

bit for bit (uint16 or float32 patterns; for NaN only the positions must agree). ``K`` itself is held to the float64 model by
tests/test_gpu_mmp_block{2,3,4}_f16.py. The cases are ``CASES`` and ``REAL`` of tests/mmp_block{2,3,4}_reference.py at M = 3 and
M = 2; every call writes into a buffer with 64 sentinel elements in front and behind."""
import ctypes

import numpy as np
import pytest
import torch

import dyobav_mpcnwta_warehouse_amd as nm
import mmp_block2_reference as b2
import mmp_block3_reference as b3
import mmp_block4_reference as b4
import oracle
from conftest import config_for
from dyobav_mpcnwta_warehouse_amd import _capi
from dyobav_mpcnwta_warehouse_amd.mmp_stem import pack_activations_f16, pack_block_f16, round_f16, unpack_activations_f16
from guarded_buffers import IntPoison, run_guarded

pytestmark = pytest.mark.gpu

POINTERS = ("w1", "s1", "b1", "w2", "s2", "b2", "wd", "sd", "bd")
PACKED = ("w1", "w2", "wd")
SENTINEL = {np.dtype(np.float32): -777.0, np.dtype(np.int16): -12345}
REFS = {2: b2, 3: b3, 4: b4}
ARGS = {2: _capi.NmpcMmpBlock2F16Args, 3: _capi.NmpcMmpBlock3F16Args, 4: _capi.NmpcMmpBlock4F16Args}
COMBOS = [(0, 1), (1, 0), (1, 1)]
ALL = [(n, c) for n, b in REFS.items() for c in b.CASES + b.REAL]
all_id = lambda t: f"layer{t[0]}-{b2.case_id(t[1])}"
HALF_BITS = IntPoison((0x7E00, 0x7BFF), -32768, 32767)       # the bits of a binary16 NaN and of 65504


@pytest.fixture(scope="module")
def handle():
    with nm.Handle(config_for(oracle.Problem())) as h:
        h.set_stream(torch.cuda.current_stream().cuda_stream)
        yield h


def _rounded(x):
    return round_f16(x).astype(np.float32)


def _same(a, b):
    """Identical bit patterns; for NaN only the positions must agree."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    fa, fb = (v.view(np.float16) if v.dtype == np.uint16 else v for v in (a, b))
    na, nb = np.isnan(fa), np.isnan(fb)
    return np.array_equal(na, nb) and a[~na].tobytes() == b[~nb].tobytes()


def _weights(n, spec):
    """The packed spec's arrays on the device, by name."""
    packed = pack_block_f16(spec, channels=REFS[n].C)
    up = lambda k, v: torch.from_numpy(np.ascontiguousarray(v).view(np.int16) if k in PACKED else np.array(v, dtype=np.float32)).cuda()
    return {k: up(k, getattr(packed, k)) for k in POINTERS if getattr(packed, k) is not None}


def _args(n, shape, spec, tensors):
    """The stage's struct for x of ``shape`` [M, Cin, H, W]; ``tensors``: name -> device tensor (``x`` and the weights)."""
    a = ARGS[n]()
    a.M, a.Cin, a.H, a.W = (int(v) for v in shape)
    a.stride, a.slope_mid, a.slope_out = int(spec.stride), spec.slope_mid, spec.slope_out
    for k, v in tensors.items():
        setattr(a, k, None if v is None else v.data_ptr())
    return a


def _launch(h, n, a, xh, oh, io=True):
    if io:
        getattr(h, f"mmp_block{n}_f16_io")(a, xh, oh)
    else:
        assert not xh and not oh
        getattr(h, f"mmp_block{n}_f16")(a)


def _run(h, n, x, spec, xh=0, oh=0, io=True, shift=0):
    """The block on float32 ``x`` [M, Cin, H, W] -- packed here where ``xh`` -- through the ``_io`` entry (``io=False``: through
    ``K``). Returns float32 [M, C, H2, W2], or with ``oh`` the uint16 octets [M, C / 8, H2, W2, 8]. The output lies ``shift``
    elements into a buffer with 64 sentinel elements in front and behind, which must come back untouched."""
    b = REFS[n]
    xs = torch.from_numpy(pack_activations_f16(x).view(np.int16) if xh else np.array(x, dtype=np.float32)).cuda()
    tensors = dict(_weights(n, spec), x=xs)
    a = _args(n, x.shape, spec, tensors)
    H2, W2 = b.out_plane(x.shape[2], x.shape[3], spec.stride)
    cnt = x.shape[0] * b.C * H2 * W2
    dt = torch.int16 if oh else torch.float32
    sentinel = SENTINEL[np.dtype(np.int16 if oh else np.float32)]
    buf = torch.full((64 + shift + cnt + 64,), sentinel, dtype=dt, device="cuda")
    a.out = buf.data_ptr() + buf.element_size() * (64 + shift)
    _launch(h, n, a, xh, oh, io)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:64 + shift] == sentinel).all() and (got[64 + shift + cnt:] == sentinel).all(), "written outside the output"
    got = got[64 + shift:64 + shift + cnt]
    return got.view(np.uint16).reshape(x.shape[0], b.C // 8, H2, W2, 8) if oh else got.reshape(x.shape[0], b.C, H2, W2)


def _inputs(n, c):
    x0, spec = REFS[n].case("random", *c, *((2,) if c in REFS[n].REAL else ()))[:2]
    return x0, _rounded(x0), spec


# ---- 1. the four forms against the kernel on float32 memory, bit for bit -------------------------------------------------------------------
@pytest.mark.parametrize("t", ALL, ids=all_id)
def test_every_form_gives_the_bits_of_the_float32_form(handle, t):
    n, c = t
    x0, xr, spec = _inputs(n, c)
    assert not np.array_equal(x0, xr)                                 # the rounding of x is something
    k0, kr = _run(handle, n, x0, spec, io=False), _run(handle, n, xr, spec, io=False)
    assert np.isfinite(k0).all() and k0.shape == (x0.shape[0], REFS[n].C) + REFS[n].out_plane(c[0], c[1], c[3])
    assert _same(_run(handle, n, xr, spec, 1, 0), kr)
    assert _same(_run(handle, n, x0, spec, 0, 1), pack_activations_f16(k0))
    assert _same(_run(handle, n, xr, spec, 1, 1), pack_activations_f16(kr))
    assert _same(_run(handle, n, x0, spec, 0, 0), k0)
    assert not np.array_equal(k0, unpack_activations_f16(pack_activations_f16(k0)))   # ... and so is that of out


# ---- 2. the ends of binary16 ---------------------------------------------------------------------------------------------------------------
def _smallest(n):
    """(H, W) of the stage's smallest plane at stride 1."""
    return REFS[n].PLANES[1][0]


@pytest.mark.parametrize("n", [2, 3, 4])
def test_outputs_beyond_the_range_saturate(handle, n):
    """The module's doubling block with both slopes 1: out = 2 x. |x| up to 6e4 doubles beyond +-65504, and +-inf, which only
    float32 memory holds, goes through the identity: a binary16 out holds +-65504 there, never an infinity."""
    b, (H, W) = REFS[n], _smallest(n)
    spec = getattr(b, f"doubling_block{n}")()._replace(slope_mid=1.0, slope_out=1.0)
    x = _rounded(b.random_x(3, b.C, H, W, seed=11) * 3e4)
    x[0, 0, 0, 0], x[1, 1, 1, 1], x[2, 2, 2, 2], x[0, 3, 1, 2] = 4e4, -4e4, 6e4, -6e4
    assert (np.abs(2 * x) > 65504).sum() >= 4 and np.isfinite(x).all()
    want = pack_activations_f16(2 * x)
    for xh in (0, 1):
        got = _run(handle, n, x, spec, xh, 1)
        assert _same(got, want) and _same(got, pack_activations_f16(_run(handle, n, x, spec, io=False)))
    f = unpack_activations_f16(want)
    assert f[0, 0, 0, 0] == 65504 and f[1, 1, 1, 1] == -65504 and np.isfinite(f).all()
    xi = x.copy()
    xi[0, 0, 0, 0], xi[1, 1, 1, 1] = np.inf, -np.inf
    k = _run(handle, n, xi, spec, io=False)
    assert k[0, 0, 0, 0] == np.inf and k[1, 1, 1, 1] == -np.inf
    got = _run(handle, n, xi, spec, 0, 1)
    assert _same(got, want) and _same(got, pack_activations_f16(k))


@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("xh", [0, 1])
def test_a_nan_stays_in_its_row_of_a_binary16_out(handle, n, xh):
    b, (H, W) = REFS[n], _smallest(n)
    spec = getattr(b, f"random_block{n}")(b.C, 5, 1, False)
    x = _rounded(b.random_x(3, b.C, H, W, seed=12))
    full = _run(handle, n, x, spec, xh, 1)
    bad = x.copy()
    bad[1, 3, 1, 2] = np.nan
    got = _run(handle, n, bad, spec, xh, 1)
    assert np.array_equal(got[0], full[0]) and np.array_equal(got[2], full[2])
    assert np.isnan(got[1].view(np.float16)).any() and not np.isnan(got[[0, 2]].view(np.float16)).any()
    assert _same(got, pack_activations_f16(_run(handle, n, bad, spec, io=False)))


@pytest.mark.parametrize("n", [2, 3, 4])
def test_subnormal_inputs_and_outputs_are_kept(handle, n):
    """x = k 2^-24, |k| <= 1: binary16 subnormals in memory. Ternary weights, unit scales and slopes 1: m is at most 9 C <= 1152
    units of 2^-24 -- below 2^-13, a binary16 value --, out a multiple of 2^-24, much of it below 2^-14: a binary16 subnormal again.
    A load or a store that flushed them would give zeros."""
    b, (H, W) = REFS[n], _smallest(n)
    s = getattr(b, f"integer_block{n}")(b.C, 3, 1, False)
    one, zero = np.ones(b.C, dtype=np.float32), np.zeros(b.C, dtype=np.float32)
    spec = s._replace(s1=one, b1=zero, s2=one, b2=zero, slope_mid=1.0, slope_out=1.0)
    x = (np.clip(b.integer_x(3, b.C, H, W, seed=4), -1, 1) * np.float32(2.0 ** -24)).astype(np.float32)
    assert np.array_equal(x, _rounded(x)) and (x != 0).any() and np.abs(x).max() < 2.0 ** -14
    k = _run(handle, n, x, spec, io=False)
    assert np.array_equal(k.astype(np.float64), b.block(x, spec)[0])             # exact in float32: nothing was flushed in K either
    want = pack_activations_f16(k)
    f = unpack_activations_f16(want)
    assert ((f != 0) & (np.abs(f) < 2.0 ** -14)).sum() > f.size // 8
    assert _same(_run(handle, n, x, spec, 1, 1), want) and _same(_run(handle, n, x, spec, 0, 1), want) and _same(_run(handle, n, x, spec, 1, 0), k)


# ---- 3. independence and bounds ------------------------------------------------------------------------------------------------------------
INDEPENDENT = {2: [(17, 89, 16, 2, True), (9, 45, 64, 1, True), (9, 45, 32, 1, False)],
               3: [(15, 43, 32, 2, True), (8, 22, 128, 1, True), (8, 22, 64, 1, False)],
               4: [(21, 23, 64, 2, True), (12, 13, 256, 1, True), (12, 13, 128, 1, False)]}     # each more than one tile both ways


@pytest.mark.parametrize("combo", COMBOS, ids=lambda v: f"x{v[0]}o{v[1]}")
@pytest.mark.parametrize("n", [2, 3, 4])
def test_bits_do_not_depend_on_batch_placement_or_other_rows(handle, n, combo):
    xh, oh = combo
    b = REFS[n]
    for c in INDEPENDENT[n]:
        x, spec = _rounded(b.random_x(3, c[2], c[0], c[1], seed=21)), getattr(b, f"random_block{n}")(c[2], 22, c[3], c[4])
        full = _run(handle, n, x, spec, xh, oh)
        for k in range(3):
            assert np.array_equal(_run(handle, n, x[k:k + 1], spec, xh, oh)[0], full[k]), (c, k)
        for shift in ((8, 16, 40) if oh else (1, 2, 3)):       # a binary16 out: every 16 bytes; a float32 out: every float
            assert np.array_equal(_run(handle, n, x, spec, xh, oh, shift=shift), full), (c, shift)
        other = x.copy()
        other[2] = _rounded(b.random_x(1, *x.shape[1:], seed=99))[0]
        got = _run(handle, n, other, spec, xh, oh)
        assert np.array_equal(got[:2], full[:2]) and not np.array_equal(got[2], full[2])


GUARDED = {2: (9, 45, 32, 1, False), 3: (15, 43, 32, 2, True), 4: (12, 13, 256, 1, True)}


@pytest.mark.parametrize("combo", COMBOS, ids=lambda v: f"x{v[0]}o{v[1]}")
@pytest.mark.parametrize("n", [2, 3, 4])
def test_the_result_depends_on_no_memory_outside_the_arguments(handle, n, combo):
    """tests/guarded_buffers.py: every array the entry reads lies between poisoned pads, each poison in turn; the output keeps its
    bits and the pads come back untouched. A binary16 x is bit patterns: its poisons are a binary16 NaN and 65504, its pad keeps
    the 16-byte alignment; a float32 x also takes the odd pad."""
    xh, oh = combo
    b, c = REFS[n], GUARDED[n]
    H, W, Cin, stride, projection = c
    x, spec = _rounded(b.random_x(2, Cin, H, W, seed=31)), getattr(b, f"random_block{n}")(Cin, 32, stride, projection)
    packed = pack_block_f16(spec, channels=b.C)
    inputs = {"x": pack_activations_f16(x).view(np.int16) if xh else x}
    for k in POINTERS:
        v = getattr(packed, k)
        inputs[k] = None if v is None else np.ascontiguousarray(v).view(np.int16) if k in PACKED else np.array(v, dtype=np.float32)
    H2, W2 = b.out_plane(H, W, stride)

    def call(t):
        a = _args(n, x.shape, spec, t)
        out = torch.zeros(2 * b.C * H2 * W2, dtype=torch.int16 if oh else torch.float32, device="cuda")
        a.out = out.data_ptr()
        _launch(handle, n, a, xh, oh)
        torch.cuda.synchronize()
        return {"out": out}
    given = [k for k, v in inputs.items() if v is not None]
    ints = [k for k in given if inputs[k].dtype == np.int16]
    got = run_guarded(call, inputs, device="cuda", int_poisons={k: HALF_BITS for k in ints}, odd_pad=[k for k in given if k not in ints])["out"]
    k = _run(handle, n, x, spec, io=False)
    assert _same(got.view(np.uint16).reshape(2, b.C // 8, H2, W2, 8), pack_activations_f16(k)) if oh else _same(got.reshape(k.shape), k)


# ---- 4. the new refusals: before the device is touched, nothing is launched ----------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 4])
def test_refusals_and_the_two_adjacent_placements(handle, n):
    b = REFS[n]
    H, W = 6, 10
    x, spec = _rounded(b.random_x(2, b.C, H, W, seed=41)), getattr(b, f"random_block{n}")(b.C, 42, 1, False)
    cnt = x.size                                                       # elements of x and of out alike: C -> C at stride 1
    weights = _weights(n, spec)
    # one allocation, in bytes: [256 | 4 cnt: x | 4 cnt: out | 256]; both regions begin on 16 bytes
    mem = torch.full((256 + 8 * cnt + 256,), 0x5A, dtype=torch.uint8, device="cuda")
    base = mem.data_ptr() + 256
    assert base % 16 == 0 and (4 * cnt) % 16 == 0
    launch = getattr(handle, f"mmp_block{n}_f16_io")
    name = f"nmpc_mmp_block{n}_f16_io"

    def make(x_at, out_at):
        a = _args(n, x.shape, spec, weights)
        a.x, a.out = x_at, out_at
        return a

    def refused(a, xh, oh, code, text):
        with pytest.raises(nm.NmpcError) as e:
            launch(a, xh, oh)
        assert e.value.code == code and name in str(e.value) and text in str(e.value), str(e.value)
    for xh, oh in ((2, 0), (0, 2), (-1, 1), (1, -1), (256, 0), (1, 3)):
        refused(make(base, base + 4 * cnt), xh, oh, -1, "(each is 0 or 1)")
    for off in (4, 8, 12):                                             # float-aligned, not 16-byte-aligned
        refused(make(base + off, base + 4 * cnt + 16), 1, 0, -1, "a binary16 x or out is not aligned to 16 bytes")
        refused(make(base, base + 4 * cnt + off), 0, 1, -1, "a binary16 x or out is not aligned to 16 bytes")
        refused(make(base + off, base + 4 * cnt + off), 1, 1, -1, "a binary16 x or out is not aligned to 16 bytes")
        a = make(base, base + 4 * cnt + off)                           # (a float32 side keeps needing 4 bytes only; one row fits
        a.M = 1                                                        # behind the offset)
        launch(a, 1, 0)
    # the overlap test counts 2 bytes per element on a binary16 side: one octet too close is refused, exactly adjacent is accepted
    x_end = base + 4 * cnt                                             # float32 x at base
    refused(make(base, x_end - 16), 0, 1, -1, "out overlaps x")
    refused(make(base, base), 0, 1, -1, "out overlaps x")
    refused(make(base + 2 * cnt, base + 16), 0, 1, -1, "out overlaps x")              # out [base + 16, base + 16 + 2 cnt) reaches into x
    refused(make(base, base + 2 * cnt - 16), 1, 0, -1, "out overlaps x")              # binary16 x [base, base + 2 cnt)
    refused(make(base, base + 2 * cnt - 16), 1, 1, -1, "out overlaps x")
    refused(make(base + 2 * cnt - 16, base), 1, 1, -1, "out overlaps x")
    torch.cuda.synchronize()
    lib = nm.load_library()
    a = make(base, x_end)
    assert getattr(lib, name)(None, ctypes.byref(a), 0, 0) == -1 and getattr(lib, name)(handle._h, None, 1, 1) == -1
    # ... and nothing was launched so far but the one accepted call per offset above, into the out region
    assert bool((mem[:256] == 0x5A).all()) and bool((mem[256:256 + 4 * cnt] == 0x5A).all()) and bool((mem[-256:] == 0x5A).all())
    k = _run(handle, n, x, spec, io=False)
    as_bytes = lambda v: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(-1)).cuda()
    # accepted: a binary16 out that begins exactly where a float32 x ends (with 4 bytes per element it would be no different;
    # with its END where x begins it is: out [base + 2 cnt, base + 4 cnt) in front of x at base + 4 cnt)
    for x_at, out_at in ((base, x_end), (x_end, base + 2 * cnt)):
        mem.fill_(0x5A)
        mem[x_at - base + 256:x_at - base + 256 + 4 * cnt] = as_bytes(x)
        launch(make(x_at, out_at), 0, 1)
        torch.cuda.synchronize()
        got = mem[out_at - base + 256:out_at - base + 256 + 2 * cnt].cpu().numpy().view(np.uint16).reshape(2, b.C // 8, H, W, 8)
        assert _same(got, pack_activations_f16(k))
        assert bool((mem[:256] == 0x5A).all()) and bool((mem[-256:] == 0x5A).all())
    # the reverse: a float32 out that begins exactly where a binary16 x ends
    mem.fill_(0x5A)
    mem[256:256 + 2 * cnt] = as_bytes(pack_activations_f16(x))
    launch(make(base, base + 2 * cnt), 1, 0)
    torch.cuda.synchronize()
    got = mem[256 + 2 * cnt:256 + 6 * cnt].cpu().numpy().view(np.float32).reshape(k.shape)
    assert _same(got, k) and bool((mem[256 + 6 * cnt:] == 0x5A).all()) and bool((mem[:256] == 0x5A).all())
    a = make(base, x_end)
    a.M = 0
    mem.fill_(0x5A)
    launch(a, 1, 1)
    torch.cuda.synchronize()
    assert bool((mem == 0x5A).all())
