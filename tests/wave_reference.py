"""Host restatements of the wavefront primitives of csrc/wave_ops.h, in two forms, and the data they are tested on.

(a) ``exact(op, xs)``: what the primitive means -- sums over the contributing lanes in extended precision (numpy
    ``longdouble``: 64 mantissa bits on x86, so 2^-64 per operation), moves as moves.
(b) ``ordered(op, xs)``: the association the header's comments promise, in numpy arithmetic of the kernel's own type, one
    rounding per operation. A kernel that keeps its promise is bit-equal to this on finite data.

Every function takes and returns arrays [n_waves, 64] (one wavefront per row, lane = column), a list of them where the op
has several operands / results. ``check(op, dtype, xs, got)`` is the comparison the GPU test applies to what
``Handle.probe`` returned and the CPU test applies to deliberately wrong restatements; it returns a list of messages that
name the wave, the lane and the values.
"""
import numpy as np

LANE = np.arange(64)
ROW = LANE >> 4
LPS = 3                                                        # lanes per horizon step of the compositions (kProbeLps)
CLASS3_LAST = np.array([[15, 13, 14], [30, 31, 29], [45, 46, 47], [63, 61, 62]])   # last lane of class r in row q
READ_LANES = (0, 16, 32, 48, 57, 63)
EXACT = np.longdouble
U_EXACT = 2.0 ** -64


def unit_roundoff(dtype):
    return {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}[np.dtype(dtype)]


def gamma(n, u):
    return n * u / (1 - n * u)


# ---- (b) ordered -------------------------------------------------------------------------------------------------------------
def _add_from(x, src, valid=None):
    """x + dpp(x): lane i adds lane src[i], or 0.0 where the DPP source is outside the row (bound_ctrl / old = 0)."""
    v = x[:, src % 64]
    if valid is not None:
        v = np.where(valid, v, x.dtype.type(0))
    return x + v


def _row_butterfly(x):
    for m in (1, 2, 7, 15):       # quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror
        x = _add_from(x, LANE ^ m)
    return x


def _row_shr(x, n):
    return _add_from(x, LANE - n, (LANE & 15) >= n)


def _row_shl(x, n):
    return _add_from(x, LANE + n, (LANE & 15) + n <= 15)


def _cross_rows(x, rows15=(1, 3), rows31=(2, 3)):
    """row_bcast:15 into rows15 (each from the last lane of the row below it), then row_bcast:31 into rows31."""
    y = x.copy()
    for q in rows15:
        y[:, 16 * q:16 * q + 16] = x[:, 16 * q:16 * q + 16] + x[:, 16 * q - 1:16 * q]
    z = y.copy()
    for q in rows31:
        z[:, 16 * q:16 * q + 16] = y[:, 16 * q:16 * q + 16] + y[:, 31:32]
    return z


def _bcast(v):
    return np.repeat(v[:, None], 64, axis=1)


def o_wave_sum(x, rows15=(1, 3)):
    return _bcast(_cross_rows(_row_butterfly(x), rows15=rows15)[:, 63])


def o_scan_incl(x, rows31=(2, 3)):
    for s in (1, 2, 4, 8):
        x = _row_shr(x, s)
    return _cross_rows(x, rows31=rows31)


def o_suffix_fix_rows(x):
    t1, t2, t3 = x[:, 16:17], x[:, 32:33], x[:, 48:49]
    c23 = t2 + t3
    c123 = t1 + c23
    zero = np.zeros_like(t3)
    add = np.where(ROW == 0, c123, np.where(ROW == 1, c23, np.where(ROW == 2, t3, zero)))
    return x + add


def o_scan_suffix_incl(x):
    for s in (1, 2, 4, 8):
        x = _row_shl(x, s)
    return o_suffix_fix_rows(x)


def o_class3(x, last=CLASS3_LAST):
    for s in (3, 6, 12):
        x = _row_shr(x, s)
    p = [x[:, last[q][LANE % 3]] for q in range(4)]
    return (p[0] + p[1]) + (p[2] + p[3])


def o_shift_up(x, s):
    out = np.zeros_like(x)
    out[:, s:] = x[:, :64 - s]
    return out


def o_shift_down(x, s):
    out = np.zeros_like(x)
    out[:, :64 - s] = x[:, s:]
    return out


def _masked(x, r):
    return np.where(LANE % 3 == r, x, x.dtype.type(0))


def _adjoint(xs, suffix, up, down):
    tail = LANE % LPS == LPS - 1
    outs = []
    for x in xs:
        g, a = x, x
        for _ in range(1, LPS):
            a = up(a, 1)
            g = g + a
        outs.append(suffix(np.where(tail, g, g.dtype.type(0))))
    return outs + [down(suffix(np.where(tail, o, o.dtype.type(0))), LPS) for o in outs]


def ordered(op, xs):
    """Form (b): list of results [n_waves, 64] of op on the operand list xs, in xs' own dtype."""
    x = xs[0]
    with np.errstate(all="ignore"):
        if op == "wave_sum":
            return [o_wave_sum(x)]
        if op in ("wave_sum2", "wave_sum3"):
            return [o_wave_sum(v) for v in xs]
        if op == "wave_scan_incl":
            return [o_scan_incl(x)]
        if op == "wave_scan_incl2":
            return [o_scan_incl(v) for v in xs]
        if op == "wave_scan_suffix_incl":
            return [o_scan_suffix_incl(x)]
        if op == "wave_scan_suffix_incl2":
            return [o_scan_suffix_incl(v) for v in xs]
        if op == "wave_suffix_fix_rows":
            return [o_suffix_fix_rows(x)]
        if op in ("class3_sum1", "class3_issue1_finish1"):
            return [o_class3(x)]
        if op == "class3_sum2":
            return [o_class3(v) for v in xs]
        if op == "class_sums_by_wave_sum3":
            return [o_wave_sum(_masked(x, r)) for r in range(3)]
        if op == "rollout_prefix":
            sc = o_scan_incl(x)
            return [o_shift_up(sc, LPS), sc]
        if op == "adjoint_suffix":
            return _adjoint(xs, o_scan_suffix_incl, o_shift_up, o_shift_down)
    return moves(op, xs)


def moves(op, xs):
    """The ops without arithmetic: the same in both forms."""
    x = xs[0]
    if op == "class3_addresses":
        return [np.repeat((4 * CLASS3_LAST[q][LANE % 3])[None, :], x.shape[0], axis=0).astype(x.dtype) for q in range(4)]
    if op == "wave_reverse":
        return [x[:, ::-1].copy()]
    if op == "read_lane":
        return [_bcast(x[:, l]) for l in READ_LANES]
    if op == "bperm":
        return [np.take_along_axis(x, (xs[1].astype(np.int64) // 4) % 64, axis=1)]
    if op.startswith("wave_shift_up_"):
        return [o_shift_up(x, int(op[-1]))]
    if op.startswith("wave_shift_down_"):
        return [o_shift_down(x, int(op[-1]))]
    raise KeyError(op)


MOVES = ("class3_addresses", "wave_reverse", "read_lane", "bperm", "wave_shift_up_1", "wave_shift_up_3", "wave_shift_down_1",
         "wave_shift_down_2", "wave_shift_down_3")


# ---- (a) exact ---------------------------------------------------------------------------------------------------------------
def e_sum(x):
    return _bcast(x.sum(axis=1))


def e_scan(x):
    return np.cumsum(x, axis=1)


def e_suffix(x):
    return np.cumsum(x[:, ::-1], axis=1)[:, ::-1]


def e_fix_rows(x):
    t = [x[:, 16 * q:16 * q + 1] for q in range(4)]
    zero = np.zeros_like(t[0])
    add = np.where(ROW == 0, t[1] + t[2] + t[3], np.where(ROW == 1, t[2] + t[3], np.where(ROW == 2, t[3], zero)))
    return x + add


def e_class3(x):
    return np.stack([x[:, r::3].sum(axis=1) for r in range(3)], axis=1)[:, LANE % 3]


def exact(op, xs):
    """Form (a), in longdouble, and the number of additions on the longest path of the kernel's sum (for the bound)."""
    if op in MOVES:
        return moves(op, xs), 0
    xs = [v.astype(EXACT) for v in xs]
    x = xs[0]
    with np.errstate(all="ignore"):
        if op in ("wave_sum", "wave_sum2", "wave_sum3"):
            return [e_sum(v) for v in xs], 63
        if op in ("wave_scan_incl", "wave_scan_incl2"):
            return [e_scan(v) for v in xs], 63
        if op in ("wave_scan_suffix_incl", "wave_scan_suffix_incl2"):
            return [e_suffix(v) for v in xs], 63
        if op == "wave_suffix_fix_rows":
            return [e_fix_rows(x)], 63
        if op in ("class3_sum1", "class3_issue1_finish1", "class3_sum2"):
            return [e_class3(v) for v in xs], 63
        if op == "class_sums_by_wave_sum3":
            return [e_sum(_masked(x, r)) for r in range(3)], 63
        if op == "rollout_prefix":
            sc = e_scan(x)
            return [o_shift_up(sc, LPS), sc], 63
        if op == "adjoint_suffix":   # two shifted additions, then two suffix sums one after the other
            return _adjoint(xs, e_suffix, o_shift_up, o_shift_down), 2 + 63 + 63
    raise KeyError(op)


def error_bound(op, dtype, xs):
    """gamma_n * sum |x_j| over the contributing lanes, weights included: every op is a sum with non-negative integer
    weights, so its exact form applied to |x| IS that sum; n = the additions on the longest path (63 for one primitive: the
    worst case over every summation order of 64 values). The extended-precision reference's own gamma is added."""
    ax, n = exact(op, [np.abs(v) for v in xs])
    g = gamma(n, unit_roundoff(dtype)) + gamma(n, U_EXACT) if n else 0.0
    with np.errstate(all="ignore"):
        return [g * a for a in ax]


# ---- the comparison ------------------------------------------------------------------------------------------------------------
def _bits(a):
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _where(mask, label, op, k, xs, got, want, out, limit=4):
    idx = np.argwhere(mask)
    for w, l in idx[:limit]:
        out.append(f"{op} result {k}: {label} at wave {w} lane {l}: got {got[w, l]!r}, expected {want[w, l]!r}; "
                   f"operand 0 of the wave: {xs[0][w].tolist()}")
    if len(idx) > limit:
        out.append(f"{op} result {k}: {label} in {len(idx)} lanes in all")


def check(op, dtype, xs, got):
    """Messages for everything wrong with `got` (list of [n_waves, 64] arrays) as the result of op on xs; [] if nothing is.
      * a NaN exactly where form (a) has one, +inf / -inf exactly where form (a) is infinite;
      * elsewhere bit-equal to form (b) -- zeros by value: `x + 0.0` turns -0.0 into +0.0 by design, in the lanes and rows
        whose DPP source is switched off, and which those are differs between the float and the double instruction sequence;
      * within the gamma bound of form (a)."""
    dtype = np.dtype(dtype)
    xs = [np.ascontiguousarray(v, dtype) for v in xs]
    want_b = ordered(op, xs)
    want_a, _ = exact(op, xs)
    bound = error_bound(op, dtype, xs)
    out = []
    assert len(got) == len(want_b), (op, len(got), len(want_b))
    for k, (g, b, a, bd) in enumerate(zip(got, want_b, want_a, bound)):
        g = np.asarray(g)
        assert g.dtype == dtype and g.shape == b.shape, (op, g.dtype, g.shape)
        a_nan, a_inf = np.isnan(a), np.isinf(a)
        _where(np.isnan(g) != a_nan, "NaN where the exact result has none, or none where it has one", op, k, xs, g, a, out)
        _where(a_inf & ~(g == a), "not the exact result's infinity", op, k, xs, g, a, out)
        _where(~a_nan & ~a_inf & np.isinf(g), "infinite where the exact result is finite", op, k, xs, g, a, out)
        fin = np.isfinite(a) & np.isfinite(g) & np.isfinite(b)
        same = (_bits(g) == _bits(b)) | ((g == 0) & (b == 0))
        _where(fin & ~same, "not the bits of the ordered restatement", op, k, xs, g, b, out)
        with np.errstate(all="ignore"):
            err = np.abs(g.astype(EXACT) - a)
        _where(fin & ~(err <= bd), "outside gamma * sum|x| of the exact result", op, k, xs, g, a, out)
    return out


# ---- data --------------------------------------------------------------------------------------------------------------------
NONFINITE_LANES = (0, 15, 16, 31, 47, 62, 63)


def integer_pattern(dtype, rounds=8):
    """The data of nmpc_selftest: (37 lane + 11 round) % 23 - 9."""
    return np.stack([((LANE * 37 + r * 11) % 23 - 9) for r in range(rounds)]).astype(dtype)


def families(dtype):
    """name -> [n_waves, 64] of the dtype. Each wave has its own data."""
    dtype = np.dtype(dtype)
    fi = np.finfo(dtype)
    rng = np.random.default_rng(20240607)
    fam = {}
    fam["deltas"] = np.eye(64, dtype=dtype)
    fam["constants"] = np.stack([np.zeros(64), -np.zeros(64), np.ones(64)]).astype(dtype)
    base = integer_pattern(dtype, 16) * dtype.type(0.75) + dtype.type(0.1)      # finite, inexact sums
    nan = base[:7].copy()
    inf = base[7:14].copy()
    for w, j in enumerate(NONFINITE_LANES):
        nan[w, j] = np.nan
        inf[w, j] = np.inf
    fam["one_nan"] = nan
    fam["one_inf"] = inf
    two = base[12:16].copy()
    two[0, 3], two[0, 9] = np.inf, -np.inf          # same row, different quads
    two[1, 5], two[1, 40] = np.inf, -np.inf         # different rows
    two[2, 20], two[2, 21] = -np.inf, np.inf        # same quad
    two[3, 15], two[3, 48] = np.inf, -np.inf        # row ends
    fam["inf_minus_inf"] = two
    big = dtype.type(1e30)
    canc = []
    for a, b, c in ((0, 1, 2), (2, 3, 4), (3, 4, 5), (14, 15, 16), (15, 16, 17), (30, 31, 32), (31, 32, 33), (46, 47, 48),
                    (47, 48, 49), (61, 62, 63), (0, 31, 63), (15, 47, 16)):
        w = np.zeros(64, dtype)
        w[a], w[b], w[c] = big, 1, -big
        canc.append(w)
        w = base[len(canc) % 16].copy()
        w[a], w[b], w[c] = -big, 1, big
        canc.append(w)
    canc.append(np.tile(np.array([big, 1, -big, 1], dtype), 16))
    canc.append(np.tile(np.array([big, 1, -big], dtype), 22)[:64])
    fam["cancellation"] = np.stack(canc)
    tiny, mp = fi.smallest_subnormal, fi.tiny
    sub = np.stack([np.full(64, tiny), tiny * ((LANE % 5) - 2), mp * (1 + fi.eps * ((LANE % 7) - 3)),
                    np.where(LANE % 2 == 0, mp, -mp + tiny), mp * dtype.type(0.5) * ((LANE % 3) - 1), mp - tiny * (LANE % 4)])
    fam["subnormal"] = sub.astype(dtype)
    k = rng.integers(-20, 21, size=(256, 64))
    fam["scaled_normal"] = (rng.standard_normal((256, 64)) * 2.0 ** k).astype(dtype)
    fam["integers"] = integer_pattern(dtype)
    return fam


def all_waves(dtype):
    """The families stacked: ([n_waves, 64], {name: slice of waves})."""
    fam = families(dtype)
    where, at = {}, 0
    for name, v in fam.items():
        where[name] = slice(at, at + v.shape[0])
        at += v.shape[0]
    return np.concatenate(list(fam.values())), where


def operands(op, x, n_in):
    """The operand list of op from one array of waves: the further operands are the first one rotated by lanes and by
    waves, so that every operand of a wave differs and a mix-up between them shows."""
    if op == "bperm":
        rng = np.random.default_rng(11)
        lanes = np.stack([rng.permutation(64) if w % 2 else rng.integers(0, 64, 64) for w in range(x.shape[0])])
        return [x, (4 * lanes).astype(x.dtype)]
    return [x] + [np.roll(np.roll(x, 5 * i, axis=1), i, axis=0) for i in range(1, max(n_in, 1))]


# ---- three wrong variants (each a restatement of a plausible slip in wave_ops.h) ---------------------------------------------
def wrong_scan_row_mask(x):
    """wave_scan_incl whose last row step has row_mask 0x8 instead of 0xc: row 2 never gets rows 0 + 1."""
    with np.errstate(all="ignore"):
        return o_scan_incl(x, rows31=(3,))


def wrong_class3_address(x):
    """class sum whose address of class 1 in row 1 is lane 30 instead of 31."""
    last = CLASS3_LAST.copy()
    last[1][1] = 30
    with np.errstate(all="ignore"):
        return o_class3(x, last)


def wrong_wave_sum_no_r3(x):
    """wave_sum without r3 += r2 (row_bcast:15 with row_mask 0x2)."""
    with np.errstate(all="ignore"):
        return o_wave_sum(x, rows15=(1,))


# ---- scalar helpers ----------------------------------------------------------------------------------------------------------
def ulp_of(ref, dtype):
    """The unit in the last place of dtype in the binade of |ref| (float64 array): 2^(e - p) for 2^(e-1) <= |ref| < 2^e."""
    p = {4: 24, 8: 53}[np.dtype(dtype).itemsize]
    _, e = np.frexp(np.abs(ref))
    emin = {4: -125, 8: -1021}[np.dtype(dtype).itemsize]
    return np.ldexp(1.0, np.maximum(e, emin) - p)


def random_exponent_floats(dtype, n, emin, emax, rng, signed=True):
    """n values with a uniformly random exponent in [emin, emax), a random mantissa and (signed) a random sign."""
    dtype = np.dtype(dtype)
    mant_bits = {4: 23, 8: 52}[dtype.itemsize]
    m = 1.0 + rng.integers(0, 2 ** mant_bits, n).astype(np.float64) / 2.0 ** mant_bits
    x = np.ldexp(m, rng.integers(emin, emax, n)).astype(dtype)
    return np.where(rng.integers(0, 2, n) == 1, -x, x) if signed else x
