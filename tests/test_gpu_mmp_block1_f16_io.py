"""GPU tests of the layer1 block on binary16 MFMA operands with BINARY16 ACTIVATIONS in memory (``nmpc_mmp_block_f16_io``,
csrc/nmpc_mmp_block1_f16.h on csrc/nmpc_mmp_block_f16.h: ``x`` and / or ``out`` in the octet form ``[M][C / 8][H][W][8]``), through the
C ABI; the sibling of tests/test_gpu_mmp_block_f16_io.py, which does the same for layer2 .. layer4.

The arithmetic and its order are those of ``nmpc_mmp_block_f16`` on float32 memory, so there is no tolerance here: with ``K`` that
entry, ``pack`` = ``mmp_stem.pack_activations_f16`` (the rule's rounding, on the host), ``x0`` a case's random float32 input and
``xr = float32(round_f16(x0))``,

    io(1, 0) on pack(xr) == K(xr)        io(0, 1) on x0 == pack(K(x0))        io(1, 1) on pack(xr) == pack(K(xr))        io(0, 0) == K

bit for bit. ``K`` itself is held to the float64 model by tests/test_gpu_mmp_block1_f16.py. Every call writes into a buffer with 64
sentinel elements in front and behind."""
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
from dyobav_mpcnwta_warehouse_amd.mmp_stem import pack_activations_f16, pack_block1_f16, round_f16, unpack_activations_f16
from guarded_buffers import IntPoison, run_guarded

pytestmark = pytest.mark.gpu

POINTERS = ("w1", "s1", "b1", "w2", "s2", "b2", "wd", "sd", "bd")
PACKED = ("w1", "w2", "wd")
SENTINEL = {np.dtype(np.float32): -777.0, np.dtype(np.int16): -12345}
COMBOS = [(0, 1), (1, 0), (1, 1)]
HALF_BITS = IntPoison((0x7E00, 0x7BFF), -32768, 32767)       # the bits of a binary16 NaN and of 65504
C = br.C
NAME = "nmpc_mmp_block_f16_io"


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


def _weights(spec):
    packed = pack_block1_f16(spec)
    up = lambda k, v: torch.from_numpy(np.ascontiguousarray(v).view(np.int16) if k in PACKED else np.array(v, dtype=np.float32)).cuda()
    return {k: up(k, getattr(packed, k)) for k in POINTERS if getattr(packed, k) is not None}


def _args(shape, spec, tensors):
    a = _capi.NmpcMmpBlockF16Args()
    a.M, a.Cin, a.H, a.W = (int(v) for v in shape)
    a.slope_mid, a.slope_out = spec.slope_mid, spec.slope_out
    for k, v in tensors.items():
        setattr(a, k, None if v is None else v.data_ptr())
    return a


def _launch(h, a, xh, oh, io=True):
    if io:
        h.mmp_block_f16_io(a, xh, oh)
    else:
        assert not xh and not oh
        h.mmp_block_f16(a)


def _run(h, x, spec, xh=0, oh=0, io=True, shift=0):
    """The block on float32 ``x`` [M, Cin, H, W] -- packed here where ``xh`` -- through the ``_io`` entry (``io=False``: through ``K``).
    Returns float32 [M, 16, H, W], or with ``oh`` the uint16 octets [M, 2, H, W, 8]. The output lies ``shift`` elements into a buffer
    with 64 sentinel elements in front and behind, which must come back untouched."""
    xs = torch.from_numpy(pack_activations_f16(x).view(np.int16) if xh else np.array(x, dtype=np.float32)).cuda()
    tensors = dict(_weights(spec), x=xs)                              # (kept alive until the launch has finished)
    a = _args(x.shape, spec, tensors)
    M, _, H, W = x.shape
    cnt = M * C * H * W
    sentinel = SENTINEL[np.dtype(np.int16 if oh else np.float32)]
    buf = torch.full((64 + shift + cnt + 64,), sentinel, dtype=torch.int16 if oh else torch.float32, device="cuda")
    a.out = buf.data_ptr() + buf.element_size() * (64 + shift)
    _launch(h, a, xh, oh, io)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:64 + shift] == sentinel).all() and (got[64 + shift + cnt:] == sentinel).all(), "written outside the output"
    got = got[64 + shift:64 + shift + cnt]
    return got.view(np.uint16).reshape(M, C // 8, H, W, 8) if oh else got.reshape(M, C, H, W)


# ---- 1. the four forms against the kernel on float32 memory, bit for bit -------------------------------------------------------------------
@pytest.mark.parametrize("c", h1.CASES + h1.REAL, ids=h1.case_id)
def test_every_form_gives_the_bits_of_the_float32_form(handle, c):
    x0, spec = br.case("random", *c, *((2,) if c in h1.REAL else ()))[:2]
    xr = _rounded(x0)
    assert not np.array_equal(x0, xr)                                 # the rounding of x is something
    k0, kr = _run(handle, x0, spec, io=False), _run(handle, xr, spec, io=False)
    assert np.isfinite(k0).all() and k0.shape == (x0.shape[0], C, c[0], c[1])
    assert _same(_run(handle, xr, spec, 1, 0), kr)
    assert _same(_run(handle, x0, spec, 0, 1), pack_activations_f16(k0))
    assert _same(_run(handle, xr, spec, 1, 1), pack_activations_f16(kr))
    assert _same(_run(handle, x0, spec, 0, 0), k0)
    assert not np.array_equal(k0, unpack_activations_f16(pack_activations_f16(k0)))   # ... and so is that of out


# ---- 2. the ends of binary16 ---------------------------------------------------------------------------------------------------------------
def test_outputs_beyond_the_range_saturate(handle):
    """The doubling block with both slopes 1: out = 2 x. |x| up to 6e4 doubles beyond +-65504, and +-inf, which only float32 memory
    holds, goes through the identity: a binary16 out holds +-65504 there, never an infinity."""
    spec = br.doubling_block()._replace(slope_mid=1.0, slope_out=1.0)
    x = _rounded(br.random_x(3, C, 16, 29, seed=11) * 3e4)
    x[0, 0, 0, 0], x[1, 1, 1, 1], x[2, 2, 2, 2], x[0, 3, 1, 2] = 4e4, -4e4, 6e4, -6e4
    assert (np.abs(2 * x) > 65504).sum() >= 4 and np.isfinite(x).all()
    want = pack_activations_f16(2 * x)
    for xh in (0, 1):
        got = _run(handle, x, spec, xh, 1)
        assert _same(got, want) and _same(got, pack_activations_f16(_run(handle, x, spec, io=False)))
    f = unpack_activations_f16(want)
    assert f[0, 0, 0, 0] == 65504 and f[1, 1, 1, 1] == -65504 and np.isfinite(f).all()
    xi = x.copy()
    xi[0, 0, 0, 0], xi[1, 1, 1, 1] = np.inf, -np.inf
    k = _run(handle, xi, spec, io=False)
    assert k[0, 0, 0, 0] == np.inf and k[1, 1, 1, 1] == -np.inf
    got = _run(handle, xi, spec, 0, 1)
    assert _same(got, want) and _same(got, pack_activations_f16(k))


@pytest.mark.parametrize("xh", [0, 1])
def test_a_nan_stays_in_its_row_of_a_binary16_out(handle, xh):
    spec = br.random_block(C, 5, False)
    x = _rounded(br.random_x(3, C, 16, 29, seed=12))
    full = _run(handle, x, spec, xh, 1)
    bad = x.copy()
    bad[1, 3, 1, 2] = np.nan
    got = _run(handle, bad, spec, xh, 1)
    assert np.array_equal(got[0], full[0]) and np.array_equal(got[2], full[2])
    assert np.isnan(got[1].view(np.float16)).any() and not np.isnan(got[[0, 2]].view(np.float16)).any()
    assert _same(got, pack_activations_f16(_run(handle, bad, spec, io=False)))


def test_subnormal_inputs_and_outputs_are_kept(handle):
    """x = k 2^-24, |k| <= 1: binary16 subnormals in memory. Ternary weights, unit scales and slopes 1: m is at most 9 x 16 units of
    2^-24, out a multiple of 2^-24, much of it below 2^-14: a binary16 subnormal again. A load or a store that flushed them would
    give zeros."""
    s = br.integer_block(C, 3, False)
    one, zero = np.ones(C, dtype=np.float32), np.zeros(C, dtype=np.float32)
    spec = s._replace(s1=one, b1=zero, s2=one, b2=zero, slope_mid=1.0, slope_out=1.0)
    x = (np.clip(br.integer_x(3, C, 16, 29, seed=4), -1, 1) * np.float32(2.0 ** -24)).astype(np.float32)
    assert np.array_equal(x, _rounded(x)) and (x != 0).any() and np.abs(x).max() < 2.0 ** -14
    k = _run(handle, x, spec, io=False)
    assert np.array_equal(k.astype(np.float64), br.block(x, spec)[0])             # exact in float32: nothing was flushed in K either
    want = pack_activations_f16(k)
    f = unpack_activations_f16(want)
    assert ((f != 0) & (np.abs(f) < 2.0 ** -14)).sum() > f.size // 8
    assert _same(_run(handle, x, spec, 1, 1), want) and _same(_run(handle, x, spec, 0, 1), want) and _same(_run(handle, x, spec, 1, 0), k)


# ---- 3. independence and bounds ------------------------------------------------------------------------------------------------------------
INDEPENDENT = [(19, 37, 64, True), (19, 37, 16, False)]      # more than one tile both ways; both kernels


@pytest.mark.parametrize("combo", COMBOS, ids=lambda v: f"x{v[0]}o{v[1]}")
def test_bits_do_not_depend_on_batch_placement_or_other_rows(handle, combo):
    xh, oh = combo
    for c in INDEPENDENT:
        x, spec = _rounded(br.random_x(3, c[2], c[0], c[1], seed=21)), br.random_block(c[2], 22, c[3])
        full = _run(handle, x, spec, xh, oh)
        for k in range(3):
            assert np.array_equal(_run(handle, x[k:k + 1], spec, xh, oh)[0], full[k]), (c, k)
        for shift in ((8, 16, 40) if oh else (1, 2, 3)):       # a binary16 out: every 16 bytes; a float32 out: every float
            assert np.array_equal(_run(handle, x, spec, xh, oh, shift=shift), full), (c, shift)
        other = x.copy()
        other[2] = _rounded(br.random_x(1, *x.shape[1:], seed=99))[0]
        got = _run(handle, other, spec, xh, oh)
        assert np.array_equal(got[:2], full[:2]) and not np.array_equal(got[2], full[2])


@pytest.mark.parametrize("c", [(16, 29, 64, True), (16, 29, 16, False)], ids=h1.case_id)
@pytest.mark.parametrize("combo", COMBOS, ids=lambda v: f"x{v[0]}o{v[1]}")
def test_the_result_depends_on_no_memory_outside_the_arguments(handle, combo, c):
    """tests/guarded_buffers.py, one case per kernel of binary16 memory: every array the entry reads lies between poisoned pads, each
    poison in turn; the output keeps its bits and the pads come back untouched. A binary16 x is bit patterns: its poisons are a
    binary16 NaN and 65504, its pad keeps the 16-byte alignment; a float32 x also takes the odd pad."""
    xh, oh = combo
    H, W, Cin, projection = c
    x, spec = _rounded(br.random_x(2, Cin, H, W, seed=31)), br.random_block(Cin, 32, projection)
    packed = pack_block1_f16(spec)
    inputs = {"x": pack_activations_f16(x).view(np.int16) if xh else x}
    for k in POINTERS:
        v = getattr(packed, k)
        inputs[k] = None if v is None else np.ascontiguousarray(v).view(np.int16) if k in PACKED else np.array(v, dtype=np.float32)

    def call(t):
        a = _args(x.shape, spec, t)
        out = torch.zeros(2 * C * H * W, dtype=torch.int16 if oh else torch.float32, device="cuda")
        a.out = out.data_ptr()
        _launch(handle, a, xh, oh)
        torch.cuda.synchronize()
        return {"out": out}
    given = [k for k, v in inputs.items() if v is not None]
    ints = [k for k in given if inputs[k].dtype == np.int16]
    got = run_guarded(call, inputs, device="cuda", int_poisons={k: HALF_BITS for k in ints}, odd_pad=[k for k in given if k not in ints])["out"]
    k = _run(handle, x, spec, io=False)
    assert _same(got.view(np.uint16).reshape(2, C // 8, H, W, 8), pack_activations_f16(k)) if oh else _same(got.reshape(k.shape), k)


# ---- 4. the refusals of the binary16 forms: before the device is touched, nothing is launched ------------------------------------------------
def test_refusals_and_the_two_adjacent_placements(handle):
    H, W = 6, 10
    x, spec = _rounded(br.random_x(2, C, H, W, seed=41)), br.random_block(C, 42, False)
    cnt = x.size                                                       # elements of x and of out alike: 16 -> 16
    weights = _weights(spec)
    # one allocation, in bytes: [256 | 4 cnt: x | 4 cnt: out | 256]; both regions begin on 16 bytes
    mem = torch.full((256 + 8 * cnt + 256,), 0x5A, dtype=torch.uint8, device="cuda")
    base = mem.data_ptr() + 256
    assert base % 16 == 0 and (4 * cnt) % 16 == 0
    launch = handle.mmp_block_f16_io

    def make(x_at, out_at):
        a = _args(x.shape, spec, weights)
        a.x, a.out = x_at, out_at
        return a

    def refused(a, xh, oh, code, text):
        with pytest.raises(nm.NmpcError) as e:
            launch(a, xh, oh)
        assert e.value.code == code and NAME in str(e.value) and text in str(e.value), str(e.value)
    for xh, oh in ((2, 0), (0, 2), (-1, 1), (1, -1), (256, 0), (1, 3)):
        refused(make(base, base + 4 * cnt), xh, oh, -1, "(each is 0 or 1)")
    for off in (4, 8, 12):                                             # float-aligned, not 16-byte-aligned
        refused(make(base + off, base + 4 * cnt + 16), 1, 0, -1, "a binary16 x or out is not aligned to 16 bytes")
        refused(make(base, base + 4 * cnt + off), 0, 1, -1, "a binary16 x or out is not aligned to 16 bytes")
        refused(make(base + off, base + 4 * cnt + off), 1, 1, -1, "a binary16 x or out is not aligned to 16 bytes")
        a = make(base, base + 4 * cnt + off)                           # (a float32 side keeps needing 4 bytes only; one row fits
        a.M = 1                                                        # behind the offset)
        launch(a, 1, 0)
    a = make(base, base + 4 * cnt)
    a.Cin = 12
    refused(a, 1, 1, -1, "is no multiple of 8")
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
    assert getattr(lib, NAME)(None, ctypes.byref(a), 0, 0) == -1 and getattr(lib, NAME)(handle._h, None, 1, 1) == -1
    assert bool((mem[:256] == 0x5A).all()) and bool((mem[256:256 + 4 * cnt] == 0x5A).all()) and bool((mem[-256:] == 0x5A).all())
    k = _run(handle, x, spec, io=False)
    as_bytes = lambda v: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(-1)).cuda()
    # accepted: a binary16 out that begins exactly where a float32 x ends, and one that ends exactly where x begins
    for x_at, out_at in ((base, x_end), (x_end, base + 2 * cnt)):
        mem.fill_(0x5A)
        mem[x_at - base + 256:x_at - base + 256 + 4 * cnt] = as_bytes(x)
        launch(make(x_at, out_at), 0, 1)
        torch.cuda.synchronize()
        got = mem[out_at - base + 256:out_at - base + 256 + 2 * cnt].cpu().numpy().view(np.uint16).reshape(2, C // 8, H, W, 8)
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
