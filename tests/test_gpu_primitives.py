"""The wavefront primitives (csrc/wave_ops.h) and the hand-written device math (csrc/nmpc_device.h), one function at a
time through nmpc_probe_*, value by value against host references (tests/wave_reference.py) -- not against device code,
and with the wave, lane and argument of every disagreement in the message.

Wave ops: bit-equal to the header's association restated in numpy of the same type; NaN / inf exactly where the
extended-precision sum has them; within gamma_63 * sum|x| of it. Scalar math: see each test for what is derived and what
was measured.
"""
import functools
from fractions import Fraction

import numpy as np
import pytest

import dyobav_mpcnwta_warehouse_amd as nm
from dyobav_mpcnwta_warehouse_amd._capi import PROBE_OPS
import wave_reference as wr

pytestmark = pytest.mark.gpu

WAVE_OPS = [op for op, spec in PROBE_OPS.items() if spec[0] <= PROBE_OPS["class_sums_by_wave_sum3"][0]]
DTYPES = [np.float32, np.float64]
IDS = ["f32", "f64"]


@pytest.fixture(scope="module")
def handle():
    h = nm.Handle(nm.default_config_struct())
    yield h
    h.close()


@functools.lru_cache(maxsize=None)
def _waves(dtype):
    x, where = wr.all_waves(dtype)
    x.setflags(write=False)
    return x, where


def _bits(a):
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _elementwise(h, op, dtype, args, chunk=1 << 16):
    """op on 1-D operand arrays of any length, in calls of at most `chunk` values (in: 1 MB, out: 1.5 MB in float), the
    block size alternating between 256 and 64 threads. Returns the op's result rows as 1-D arrays."""
    dtype = np.dtype(dtype)
    n = len(args[0])
    pad = (-n) % 64
    args = [np.concatenate([np.asarray(a, dtype), np.ones(pad, dtype)]) for a in args]
    outs = None
    for c, i in enumerate(range(0, n + pad, chunk)):
        got = h.probe(op, [a[i:i + chunk].reshape(-1, 64) for a in args], dtype, block_threads=(256, 64)[c % 2])
        got = [got] if isinstance(got, np.ndarray) else got
        outs = [[] for _ in got] if outs is None else outs
        for o, g in zip(outs, got):
            o.append(g.reshape(-1))
    return [np.concatenate(o)[:n] for o in outs]


# ---- wave ops ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block_threads", [64, 256])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("op", WAVE_OPS)
def test_wave_op_matches_its_restatements(handle, op, dtype, block_threads):
    """381 waves of their own data each (deltas, constants, NaN / inf in seven lanes, inf - inf, 1e30 cancellation across
    quad / row / row-pair boundaries, subnormals, 256 waves of scaled normals, the self-test's integers): 381 blocks of one
    wave, or 96 blocks of four with the last one part empty."""
    x, _ = _waves(dtype)
    xs = wr.operands(op, x, PROBE_OPS[op][2])
    got = handle.probe(op, xs, dtype, block_threads)
    got = [got] if isinstance(got, np.ndarray) else got
    bad = wr.check(op, dtype, xs, got)
    assert not bad, "\n".join(bad[:12])


@pytest.mark.parametrize("block_threads", [64, 256])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_class_sums_agree_bit_for_bit(handle, dtype, block_threads):
    """class3_sum1 = class3_sum2 = class3_issue1 + class3_finish1 on every family (the promise of wave_ops.h: a slot's E_j
    comes out bit-identical either way); a NaN in the same lanes."""
    x, _ = _waves(dtype)
    y = np.roll(x, 5, axis=1)
    one = [handle.probe("class3_sum1", v, dtype, block_threads) for v in (x, y)]
    two = handle.probe("class3_sum2", [x, y], dtype, block_threads)
    halves = [handle.probe("class3_issue1_finish1", v, dtype, block_threads) for v in (x, y)]
    for k in range(2):
        for name, other in (("class3_sum2", two[k]), ("class3_issue1 + class3_finish1", halves[k])):
            nan = np.isnan(one[k])
            assert np.array_equal(nan, np.isnan(other)), (name, k)
            diff = np.argwhere(~nan & (_bits(one[k]) != _bits(other)))
            assert len(diff) == 0, f"class3_sum1 != {name}, value {k}, first at wave {diff[0][0]} lane {diff[0][1]}: " \
                                   f"{one[k][tuple(diff[0])]!r} != {other[tuple(diff[0])]!r}"


# ---- sincos_medium / sincos_small ----------------------------------------------------------------------------------------------
def _old_selftest_arguments():
    """The 4 096 arguments of nmpc_selftest's sincos check, restated in float32 numpy (one rounding per operation)."""
    f = np.float32
    i = np.arange(4096, dtype=np.int64)
    x = (((i * 2654435761) % 2 ** 32) >> 8).astype(f) * f(1.0 / 16777216.0)
    sel = i & 3
    near = f(0.78539816) * ((i >> 2) % 17 - 8).astype(f) + (x - f(0.5)) * f(1e-4)
    return np.where(sel == 0, x * f(8) - f(4), np.where(sel == 1, (x - f(0.5)) * f(200), np.where(sel == 2, (x - f(0.5)) * f(2.6e5), near))).astype(f)


def _neighbours(centres, ulps=16):
    """Every float32 within +-ulps ulp of each centre (float32 array), through the sign-magnitude order of the bit patterns."""
    b = centres.astype(np.float32).view(np.int32).astype(np.int64)
    key = np.where(b < 0, -(b & 0x7fffffff), b)                              # monotone in the value; -0 and +0 coincide
    key = (key[:, None] + np.arange(-ulps, ulps + 1)[None, :]).reshape(-1)
    bits = np.where(key < 0, (-key) | 0x80000000, key).astype(np.uint32)
    return bits.view(np.float32)


@functools.lru_cache(maxsize=None)
def _sincos_arguments():
    rng = np.random.default_rng(1717)
    quarter = np.pi / 4
    k = np.arange(-2048, 2049)
    kmax = int(2.0 ** 17 / quarter)
    while kmax * quarter >= 2.0 ** 17:
        kmax -= 1
    far = rng.permutation(np.unique(np.exp(rng.uniform(np.log(2049), np.log(kmax), 2400)).astype(np.int64)))[:2046]
    far = np.concatenate([far * rng.choice([-1, 1], len(far)), [kmax, -kmax]])       # (log-uniform, random sign, and the last one)
    near = _neighbours(np.concatenate([k, far]).astype(np.float64) * quarter)
    rand = wr.random_exponent_floats(np.float32, 2 ** 20, -126, 17, rng)
    fi = np.finfo(np.float32)
    top = np.nextafter(np.float32(2.0 ** 17), np.float32(0))
    edges = np.array([0.0, -0.0, fi.smallest_subnormal, -fi.smallest_subnormal, fi.tiny, -fi.tiny, top, -top], np.float32)
    x = np.concatenate([near, rand, edges, _old_selftest_arguments()]).astype(np.float32)
    x = x[np.abs(x) < np.float32(2.0 ** 17)]
    gate = np.float32(0.785)
    below = (gate.view(np.uint32) - np.arange(1, 4097, dtype=np.uint32)).view(np.float32)
    small = np.concatenate([x[np.abs(x) < gate], below, -below]).astype(np.float32)
    assert np.all(np.abs(small) < gate) and len(near) == 33 * (4097 + 2048) and np.abs(x).max() == top
    x.setflags(write=False)
    small.setflags(write=False)
    return x, small


def _ulp_errors(x, s, c):
    xd = x.astype(np.float64)
    rs, rc = np.sin(xd), np.cos(xd)
    es = np.abs(s.astype(np.float64) - rs) / wr.ulp_of(rs, np.float32)
    ec = np.abs(c.astype(np.float64) - rc) / wr.ulp_of(rc, np.float32)
    return es, ec


def _check_sincos(handle, op, x):
    s, c, ls, lc = _elementwise(handle, op, np.float32, [x])
    for name, a, b in (("sin", s, ls), ("cos", c, lc)):
        diff = np.flatnonzero(_bits(a) != _bits(b))
        assert len(diff) == 0, f"{op}: {name} differs from the library's in {len(diff)} of {len(x)} arguments, first " + \
            ", ".join(f"x = {x[i]!r} ({_bits(x[i:i + 1])[0]:#010x}): {a[i]!r} vs {b[i]!r}" for i in diff[:6])
    es, ec = _ulp_errors(x, s, c)
    ls_, lc_ = _ulp_errors(x, ls, lc)
    worst, worst_lib = max(es.max(), ec.max()), max(ls_.max(), lc_.max())
    i, j = int(np.argmax(es)), int(np.argmax(ec))
    print(f"{op}: {len(x)} arguments; worst error sin {es.max():.4f} ulp at x = {x[i]!r}, cos {ec.max():.4f} ulp at x = {x[j]!r}; "
          f"library sin {ls_.max():.4f} ulp, cos {lc_.max():.4f} ulp")
    assert worst <= worst_lib, (worst, worst_lib)
    return worst, worst_lib


def test_sincos_medium_is_the_library_bit_for_bit(handle):
    """Every float32 within 16 ulp of k pi/4 for |k| <= 2048 and for ~2048 further k up to the last below 2^17, 2^20 floats
    of random exponent in [-126, 17), +-0, the smallest subnormal, min_pos, the last float below 2^17, the old self-test's
    4 096: sin and cos have the bits of the device library's sincosf on every one (the claim in nmpc_device.h), and so the
    hand-written path's worst error against numpy's float64 sin / cos of the same argument cannot exceed the library's.
    Worst over the 1 255 441 arguments, measured on an MI355X in float32 ulps of the true value: sin 1.3858 ulp at
    x = 184.84204, cos 1.4814 ulp at x = -1132.2936, for the hand-written path and for the library alike."""
    x, _ = _sincos_arguments()
    _check_sincos(handle, "sincos_medium", x)


def test_sincos_small_is_the_library_bit_for_bit(handle):
    """The same for sincos_small (the rollout's small-angle path) on the arguments above with |x| < float32(0.785), its
    gate in the rollout, and the 4 096 floats just below the gate on either side of zero.
    Finding: as first moved out of the rollout, the function returned sin(-0.0) = +0.0 where the library returns -0.0 (the
    one argument of 928 631 that differed): the library works on |x| and restores the sign, the polynomial on the signed
    argument ended in fma(-0, -0, -0) = +0. Fixed in sincos_small (the product r2 * t formed as fma(r2, t, +0)).
    Worst over the 928 631 arguments, measured on an MI355X: sin 0.6322 ulp at x = -0.25025105, cos 0.8519 ulp at
    x = 0.78494155, for the hand-written path and for the library alike."""
    _, small = _sincos_arguments()
    _check_sincos(handle, "sincos_small", small)


# ---- fast_rcp ------------------------------------------------------------------------------------------------------------------
BIG = {np.float32: np.float32(3.0e38), np.float64: np.float64(1.0e300)}


def _scenario_squared_radii(dtype):
    """(r + 1e-6)^2 in the kernel's type for the radii scenario generation can produce: 0.2 + 0.05 t along the horizon
    (t <= 64), with and without the vehicle / social margins the table adds, and the zero radius of a padding entry."""
    t = dtype(0.2) + dtype(0.05) * np.arange(65).astype(dtype)
    marg = np.concatenate([[0.0], np.arange(0.05, 1.55, 0.05)]).astype(dtype)
    r = np.concatenate([(t[:, None] + marg[None, :]).reshape(-1), [dtype(0)], np.arange(0.3, 6.0, 0.01).astype(dtype)]).astype(dtype)
    e = r + dtype(1e-6)
    return (e * e).astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fast_rcp_is_within_one_ulp_where_it_is_used(handle, dtype):
    """x and 1 / x normal, x <= big: random exponents over the whole normal range, powers of two, the squared radii of the
    scenarios, the clamp's edge. |fast_rcp(x) - 1/x| <= 1 ulp of the type at the true quotient -- derived: the hardware
    seed is good to 2^-23 (float) or ~2^-26 (double), so after the last Newton step the iteration error e^2 is below 2^-46
    (float) resp. far below 2^-53 (double) and what remains is the one rounding of the last fma (half an ulp) plus that.
    Float: against float64 division; double: exact rational arithmetic."""
    dtype_t = np.dtype(dtype).type
    fi = np.finfo(dtype)
    rng = np.random.default_rng(99)
    n = 2 ** 16 if dtype is np.float32 else 2 ** 14
    x = np.concatenate([wr.random_exponent_floats(dtype, n, fi.minexp, fi.maxexp, rng, signed=False),
                        np.ldexp(dtype_t(1), np.arange(fi.minexp, fi.maxexp)).astype(dtype),
                        _scenario_squared_radii(dtype_t), [BIG[dtype], np.nextafter(BIG[dtype], dtype_t(0)), fi.tiny]]).astype(dtype)
    with np.errstate(all="ignore"):
        q = 1.0 / x.astype(np.float64)
    x = x[(x <= BIG[dtype]) & (x >= fi.tiny) & (np.abs(q) >= float(fi.tiny)) & (np.abs(q) <= float(fi.max))]
    r, ieee = _elementwise(handle, "fast_rcp", dtype, [x])
    assert np.array_equal(ieee, (dtype_t(1) / x).astype(dtype)), "the device's IEEE quotient is not numpy's"
    if dtype is np.float32:
        ref = 1.0 / x.astype(np.float64)
        err = np.abs(r.astype(np.float64) - ref) / wr.ulp_of(ref, np.float32)
    else:
        err = np.empty(len(x))
        for i, (xi, ri, qi) in enumerate(zip(x.tolist(), r.tolist(), ieee.tolist())):
            err[i] = float(abs(Fraction(ri) - 1 / Fraction(xi)) / Fraction(float(wr.ulp_of(np.float64(qi), np.float64))))
    i = int(np.argmax(err))
    print(f"fast_rcp {np.dtype(dtype).name}: {len(x)} arguments, worst {err[i]:.4f} ulp at x = {x[i]!r}; "
          f"{np.count_nonzero(_bits(r) != _bits(ieee))} differ from the IEEE quotient")
    assert err[i] <= 1.0, (err[i], x[i], r[i])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fast_rcp_beyond_big_is_finite_and_out_of_reach(handle, dtype):
    """x > big -- nextafter(big), the largest finite value, +inf, an overflowed square -- gives a finite value of at most
    1/big (1 + 2u): the clamp's "out of reach" promise, where the unclamped Newton step would be NaN. Measured on an
    MI355X: 1e-300 in double; 0 in float, whose 1/big is subnormal and flushed by the hardware reciprocal."""
    dtype_t = np.dtype(dtype).type
    fi = np.finfo(dtype)
    with np.errstate(over="ignore"):
        sq = dtype_t(fi.max) * dtype_t(0.5)
        sq = sq * sq
    x = np.array([np.nextafter(BIG[dtype], dtype_t(np.inf)), fi.max, np.inf, sq, BIG[dtype] * dtype_t(1.1)], dtype)
    assert np.all(x > BIG[dtype]) and np.isinf(x[3])
    r, _ = _elementwise(handle, "fast_rcp", dtype, [x])
    lim = (1.0 / float(BIG[dtype])) * (1 + 2 * wr.unit_roundoff(dtype))
    assert np.all(np.isfinite(r)) and np.all(r >= 0) and np.all(r.astype(np.float64) <= lim), (x, r, lim)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fast_rcp_outside_its_domain_is_recorded(handle, dtype):
    """Zero, subnormals, an x whose reciprocal overflows, negative values, NaN: what the device returns next to the IEEE
    quotient, printed. nmpc_device.h promises nothing here except that the call sites cannot produce these arguments
    (x = (radius + margin + 1e-6)^2 >= 1e-12 for radii >= 0: unreachable, so the domain is stated in the function's comment
    and nothing is clamped), so all that is asserted is what that comment describes: NaN at +-0 where the quotient is
    +-inf, a NaN argument taken for `big` by fmin, negative normal arguments within 1 ulp like positive ones.
    Measured on an MI355X, fast_rcp(x) | the IEEE quotient:
                                    float                      double
      +-0                           NaN | +-inf                NaN | +-inf
      smallest subnormal            NaN | inf                  NaN | inf
      min_pos / 4, 1 / (2 max)      NaN | inf                  NaN | inf
      nextafter(min_pos, 0)         NaN | 8.50706e+37          4.494232837155791e+307 | the same
      NaN                           0.0 | NaN                  1e-300 | NaN
      -1, -3                        the quotient               the quotient
      -min_pos                      the quotient               -4.49423283715579e+307 | the same
      -big                          -0.0 | -3.333333e-39       -1e-300 | the same
      -inf                          NaN | -0.0                 NaN | -0.0
    Inside the domain (the test above) every one of 67 845 float and 20 761 double arguments came out equal to the IEEE
    quotient, worst error 0.5000 ulp."""
    dtype_t = np.dtype(dtype).type
    fi = np.finfo(dtype)
    x = np.array([0.0, -0.0, fi.smallest_subnormal, fi.tiny / 4, np.nextafter(fi.tiny, dtype_t(0)), 1 / float(fi.max) / 2,
                  np.nan, -1.0, -3.0, -float(fi.tiny), -float(BIG[dtype]), -np.inf], dtype)
    r, ieee = _elementwise(handle, "fast_rcp", dtype, [x])
    for xi, ri, qi in zip(x, r, ieee):
        print(f"fast_rcp {np.dtype(dtype).name}({xi!r}) = {ri!r}; IEEE 1/x = {qi!r}")
    assert np.isnan(r[0]) and np.isnan(r[1]) and np.isinf(ieee[0]) and np.isinf(ieee[1])
    assert np.isnan(ieee[6]) and 0 <= float(r[6]) <= (1.0 / float(BIG[dtype])) * (1 + 2 * wr.unit_roundoff(dtype))
    ref = 1.0 / x[7:9].astype(np.float64)
    assert np.all(np.abs(r[7:9].astype(np.float64) - ref) <= wr.ulp_of(ref, dtype))


# ---- ls_point ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_ls_point_rounds_every_operation(handle, dtype):
    """2^16 seeded quadruples: bit-equal to (u - (1 - tau) f) - tau d in numpy of the type, one rounding per operation. The
    set is checked on the host to hold thousands of quadruples on which contracting tau d into the last subtraction, or
    (1 - tau) f into the first, rounds differently -- the contraction ls_point switches off."""
    rng = np.random.default_rng(31)
    n = 2 ** 16
    t = np.dtype(dtype).type
    u, f, d = (rng.standard_normal(n) * 2.0 ** rng.integers(-3, 4, n)).astype(dtype), rng.standard_normal(n).astype(dtype), rng.standard_normal(n).astype(dtype)
    tau = np.where(rng.integers(0, 4, n) == 0, 2.0 ** -rng.integers(0, 12, n), rng.uniform(0, 1, n)).astype(dtype)
    a = (t(1) - tau) * f
    want = (u - a) - tau * d
    ext = np.longdouble
    fused_last = ((u - a).astype(ext) - tau.astype(ext) * d.astype(ext)).astype(dtype)        # (exact product for float32)
    fused_first = ((u.astype(ext) - (t(1) - tau).astype(ext) * f.astype(ext)).astype(dtype) - tau * d).astype(dtype)
    assert np.count_nonzero(_bits(fused_last) != _bits(want)) > 2000 and np.count_nonzero(_bits(fused_first) != _bits(want)) > 2000
    got, = _elementwise(handle, "ls_point", dtype, [u, f, d, tau])
    diff = np.flatnonzero(_bits(got) != _bits(want))
    assert len(diff) == 0, f"{len(diff)} of {n} differ, first (u, f, d, tau) = {(u[diff[0]], f[diff[0]], d[diff[0]], tau[diff[0]])!r}: " \
                           f"{got[diff[0]]!r} != {want[diff[0]]!r} (tau d fused: {fused_last[diff[0]]!r}, (1 - tau) f fused: {fused_first[diff[0]]!r})"


# ---- the entry point's own promises ----------------------------------------------------------------------------------------------
def test_probe_leaves_everything_outside_out_alone(handle):
    """Device buffers with 64 sentinel values in front of and behind `out`: they survive every op in both types at both
    block sizes, with 5 waves (two blocks of 256 threads, the second with three wavefronts past n_waves); n_waves = 0
    leaves `out` itself untouched; the refusals launch nothing."""
    import torch
    n_waves, sentinel = 5, -12345.0
    for dtype, tdt in ((np.float32, torch.float32), (np.float64, torch.float64)):
        x = torch.from_numpy(_waves(dtype)[0][64:64 + 4 * n_waves].reshape(n_waves, 4, 64).copy()).cuda()
        x[:, 1] = 4.0 * torch.arange(64, device="cuda", dtype=tdt)               # (bperm's addresses)
        size = x.element_size()
        for op, spec in PROBE_OPS.items():
            if spec[4] and dtype is np.float64:
                continue
            for bt in (64, 256):
                buf = torch.full((64 + n_waves * 6 * 64 + 64,), sentinel, dtype=tdt, device="cuda")
                torch.cuda.synchronize()
                handle.probe_raw(dtype, spec[0], bt, 0, x.data_ptr(), buf.data_ptr() + 64 * size)
                assert bool((buf == sentinel).all()), (op, bt, "n_waves = 0 wrote")
                for bad in ((len(PROBE_OPS), bt, n_waves), (spec[0], 96, n_waves), (spec[0], bt, -1)):
                    with pytest.raises(nm.NmpcError):
                        handle.probe_raw(dtype, bad[0], bad[1], bad[2], x.data_ptr(), buf.data_ptr() + 64 * size)
                assert bool((buf == sentinel).all()), (op, bt, "a refused call wrote")
                handle.probe_raw(dtype, spec[0], bt, n_waves, x.data_ptr(), buf.data_ptr() + 64 * size)
                host = buf.cpu().numpy()
                assert np.all(host[:64] == sentinel) and np.all(host[-64:] == sentinel), (op, bt)
                body = host[64:-64].reshape(n_waves, 6, 64)
                assert not np.any(body[:, :spec[3]] == sentinel), (op, bt, "a result row was not written")
    with pytest.raises(nm.NmpcError):
        handle.probe_raw(np.float64, PROBE_OPS["sincos_small"][0], 64, 1, x.data_ptr(), buf.data_ptr())
