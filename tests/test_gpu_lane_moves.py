"""The masked-row form of the suffix scans' cross-row step (csrc/wave_ops.h: wave_scan_suffix_incl_masked,
wave_scan_suffix_incl2_masked, wave_suffix_fix_rows_masked) against the select-tree form it replaces in the axis-aligned
fp32 register-table kernels, lane by lane as int32 views, and against numpy restatements in float32 -- through
nmpc_probe_f32, on 1, 2 and 4 wavefronts per workgroup and one to three workgroups per launch.

What is promised (wave_ops.h): the same additions of the same operands in rows 0..2 -- the same bits wherever the result is
no NaN, NaN in the same lanes; row 3 is left alone where the select tree adds 0.0, which shows in lane 48 alone, and only
with -0.0 in all of lanes 48..63 -- never on a call site's operand (+0.0 in every lane that is not a step's last). Both
halves of that sentence are tested.
The shifts by one step kept their DPP form (HISTORY.md, "Lane moves"): there is no second form of them to compare.
"""
import functools

import numpy as np
import pytest

import dyobav_mpcnwta_warehouse_amd as nm

pytestmark = pytest.mark.gpu

F = np.float32
LANE = np.arange(64)
NO_SOURCE_UP = [0, 1, 2]            # lanes a shift up by one step fills with 0.0
TOP = [60, 61, 62, 63]              # lanes 61..63: filled by a shift down by one step; 63 is no lane of any step
ROW_EDGES = [15, 16, 31, 32, 47, 48]
PZ, NZ = np.uint32(0), np.uint32(0x80000000)


@pytest.fixture(scope="module")
def handle():
    h = nm.Handle(nm.default_config_struct())
    yield h
    h.close()


def _i(a):
    return np.ascontiguousarray(a).view(np.int32)


def _f(bits):
    return np.ascontiguousarray(bits, dtype=np.uint32).view(F)


@functools.lru_cache(maxsize=None)
def _inputs():
    """name -> waves [n, 64] float32, read-only. `all_minus_zero_top` is the one family with the documented difference."""
    rng = np.random.default_rng(20240611)
    fam = {}
    fam["ramp"] = np.stack([LANE + 1, -(LANE + 1), 64 - LANE, (LANE + 1) * 0.37]).astype(F)
    normal = (rng.standard_normal((12, 64)) * np.exp2(rng.integers(-20, 21, (12, 64)))).astype(F)
    fam["random"] = normal
    z = (rng.standard_normal((8, 64)) + 3.0).astype(F)        # (nonzero everywhere before the zeros are placed)
    zb = z.view(np.uint32).copy()
    zb[0, NO_SOURCE_UP] = PZ
    zb[1, NO_SOURCE_UP] = NZ
    zb[2, TOP[1:]] = PZ
    zb[3, TOP[1:]] = NZ
    zb[4, ROW_EDGES] = PZ
    zb[5, ROW_EDGES] = NZ
    zb[6, ROW_EDGES] = [PZ, NZ, PZ, NZ, PZ, NZ]
    zb[7, ROW_EDGES] = [NZ, PZ, NZ, PZ, NZ, PZ]
    fam["zeros"] = _f(zb)
    sub = rng.integers(1, 0x800000, (4, 64)).astype(np.uint32) | (rng.integers(0, 2, (4, 64)).astype(np.uint32) << 31)
    fam["denormals"] = _f(sub)
    inf = (rng.standard_normal((6, 64)) + 2.0).astype(F)
    inf[0, [5, 40]] = np.inf
    inf[1, [17, 63]] = -np.inf
    inf[2, [0, 61]] = [np.inf, -np.inf]                        # (inf - inf in the scans: NaN in both forms)
    inf[3, [1, 2, 62]] = np.inf
    inf[4, ROW_EDGES] = [np.inf, 1.0, -np.inf, 1.0, 2.0, np.inf]
    inf[5, :] = np.inf
    fam["inf"] = inf
    # quiet and signalling NaNs, a payload of its own in every lane of every wave, both signs; wave 2: NaN in a few lanes only
    w = np.arange(4, dtype=np.uint32)[:, None]
    nb = np.uint32(0x7F800000) | ((w & 1) << 22) | (w << 8) | (LANE.astype(np.uint32) + 1)[None, :] | ((w >> 1) << 31)
    few = (rng.standard_normal((1, 64)) + 2.0).astype(F).view(np.uint32).copy()
    few[0, [0, 2, 16, 47, 61, 63]] = nb[0, [0, 2, 16, 47, 61, 63]] | np.uint32(0x00400000)
    fam["nan"] = _f(np.concatenate([nb, few]))
    # a call site's operand: a value in the last lane of every step (lane % 3 == 2, lanes 2 .. 59 at N = 20; 62 at N = 21), +0.0
    # in every other lane -- with ordinary values, with zeros of both signs and with -0.0 in every tail lane
    tail = LANE % 3 == 2
    site = np.zeros((5, 64), F)
    site[0] = np.where(tail & (LANE < 60), normal[0], 0)
    site[1] = np.where(tail, normal[1], 0)
    sb = site.view(np.uint32)
    sb[2] = np.where(tail, NZ, PZ)
    sb[3] = np.where(tail & (LANE >= 48), NZ, normal[2].view(np.uint32) * tail)
    sb[4] = np.where(tail & (LANE % 2 == 0), NZ, PZ)
    fam["call_site"] = site
    top = (rng.standard_normal((2, 64)) + 2.0).astype(F).view(np.uint32).copy()
    top[:, 48:] = NZ
    top[1, :48] = NZ
    fam["all_minus_zero_top"] = _f(top)
    for v in fam.values():
        v.setflags(write=False)
    return fam


def _all(fam):
    names = list(fam)
    return np.concatenate([fam[n] for n in names]), np.concatenate([[n] * len(fam[n]) for n in names])


def _launches(n_waves, waves_per_block):
    """Slices of the wave axis of 1, 2, 3, 1, 2, 3 ... workgroups each; every third slice one wave short where a workgroup
    has more than one wavefront (a last workgroup with wavefronts past n_waves)."""
    out, i, g = [], 0, 0
    while i < n_waves:
        n = waves_per_block * (g % 3 + 1) - (1 if waves_per_block > 1 and g % 3 == 2 else 0)
        out.append(slice(i, min(i + n, n_waves)))
        i += n
        g += 1
    return out


def _probe(h, op, xs, block_threads):
    xs = [xs] if isinstance(xs, np.ndarray) else xs
    n = xs[0].shape[0]
    outs = None
    launches = _launches(n, block_threads // 64)
    if n >= 6 * (block_threads // 64):
        assert {(-(-(s.stop - s.start) // (block_threads // 64))) for s in launches[:3]} == {1, 2, 3}
    for s in launches:
        got = h.probe(op, [x[s] for x in xs], F, block_threads)
        got = [got] if isinstance(got, np.ndarray) else got
        outs = [[] for _ in got] if outs is None else outs
        for o, g in zip(outs, got):
            o.append(g)
    return [np.concatenate(o) for o in outs]


# ---- numpy restatements (float32, one rounding per operation) --------------------------------------------------------------------
def ref_fix_rows_masked(x):
    """row 2 += lane 48; row 1 += lane 32 (by then t2 + t3); row 0 += lane 16 (by then t1 + (t2 + t3)); row 3 untouched."""
    y = x.copy()
    with np.errstate(all="ignore"):
        y[:, 32:48] = y[:, 32:48] + y[:, 48:49]
        y[:, 16:32] = y[:, 16:32] + y[:, 32:33]
        y[:, 0:16] = y[:, 0:16] + y[:, 16:17]
    return y


def ref_suffix_masked(x):
    """in each 16-lane row x_i += x_{i+s} for s = 1, 2, 4, 8, 0.0 past the end of the row; then the masked-row step."""
    with np.errstate(all="ignore"):
        for s in (1, 2, 4, 8):
            v = np.where((LANE & 15) + s <= 15, x[:, (LANE + s) % 64], F(0))
            x = x + v
    return ref_fix_rows_masked(x)


def _same_bits(got, want, names, what, lanes=slice(None)):
    """bit-equal where `want` is no NaN, NaN in the same lanes (numpy and the device choose a NaN's payload differently)."""
    g, w = got[:, lanes], want[:, lanes]
    nan = np.isnan(w)
    assert np.array_equal(np.isnan(g), nan), (what, "NaN in other lanes")
    diff = np.argwhere(~nan & (_i(g) != _i(w)))
    assert len(diff) == 0, f"{what}: {len(diff)} lanes differ, first in wave {diff[0][0]} ({names[diff[0][0]]}) at column {diff[0][1]}: " \
                           f"{g[tuple(diff[0])]!r} != {w[tuple(diff[0])]!r}"


def _identical(got, want, names, what, skip=None, nan_payload=True):
    """the same 32 bits in every lane, NaN payloads included -- or, for sums, NaN in the same lanes with whatever payload:
    which operand's payload NaN + NaN keeps follows the operand order of the instruction, which no form promises"""
    ne = _i(got) != _i(want)
    if not nan_payload:
        ne &= ~(np.isnan(got) & np.isnan(want))
    if skip is not None:
        ne &= ~skip
    diff = np.argwhere(ne)
    assert len(diff) == 0, f"{what}: {len(diff)} lanes differ, first in wave {diff[0][0]} ({names[diff[0][0]]}) lane {diff[0][1]}: " \
                           f"{int(_i(got)[tuple(diff[0])]) & 0xffffffff:#010x} != {int(_i(want)[tuple(diff[0])]) & 0xffffffff:#010x}"


# ---- the inputs themselves ---------------------------------------------------------------------------------------------------------
def test_inputs_hold_what_they_are_named_for():
    fam = _inputs()
    nan = fam["nan"].view(np.uint32)[:4]
    assert np.all(np.isnan(fam["nan"][:4])) and len(np.unique(nan)) == nan.size      # a payload of its own per lane and wave
    site = fam["call_site"].view(np.uint32)
    assert np.all(site[:, LANE % 3 != 2] == 0) and np.all(site[:, 63] == 0)
    z = fam["zeros"].view(np.uint32)
    assert np.all(z[4:6, ROW_EDGES] & 0x7fffffff == 0) and np.all(z[5, ROW_EDGES] == NZ) and np.all(z[6, ROW_EDGES[1::2]] == NZ)
    sub = fam["denormals"].view(np.uint32) & 0x7fffffff
    assert np.all((sub > 0) & (sub < 0x800000))
    for name in ("ramp", "random", "denormals", "call_site", "zeros"):
        assert np.all(np.isfinite(fam[name])), name


# ---- the scans -----------------------------------------------------------------------------------------------------------------------
def _lane48_exception(x):
    """[n, 64] mask: lane 48 of the waves with -0.0 in all of lanes 48..63"""
    m = np.zeros(x.shape, bool)
    m[:, 48] = np.all(x.view(np.uint32)[:, 48:] == NZ, axis=1)
    return m


@pytest.mark.parametrize("block_threads", [64, 128, 256])
def test_masked_row_suffix_scan_is_the_select_tree_scan(handle, block_threads):
    fam = _inputs()
    x, names = _all(fam)
    skip = _lane48_exception(x)
    assert skip.sum() == 2 and set(names[skip.any(axis=1)]) == {"all_minus_zero_top"}     # (no call-site operand among them)
    new, = _probe(handle, "wave_scan_suffix_incl_masked", x, block_threads)
    old, = _probe(handle, "wave_scan_suffix_incl", x, block_threads)
    _identical(new, old, names, "wave_scan_suffix_incl_masked != wave_scan_suffix_incl", skip, nan_payload=False)
    _same_bits(new, ref_suffix_masked(x), names, "wave_scan_suffix_incl_masked != its float32 restatement")
    # the documented difference, and nothing else: lane 48 keeps -0.0 where the select tree's + 0.0 makes it +0.0
    assert np.all(_i(new)[skip] == np.int32(-2 ** 31)) and np.all(_i(old)[skip] == 0)


@pytest.mark.parametrize("block_threads", [64, 128, 256])
def test_masked_row_suffix_scan_of_two_values(handle, block_threads):
    """two interleaved chains: each equal to the one-value scan of its operand, to the select-tree pair and to the restatement"""
    x, names = _all(_inputs())
    y = np.ascontiguousarray(np.roll(x, 7, axis=0)[:, ::-1])          # (another wave's values, lanes reversed)
    skip_x, skip_y = _lane48_exception(x), _lane48_exception(y)
    new = _probe(handle, "wave_scan_suffix_incl2_masked", [x, y], block_threads)
    old = _probe(handle, "wave_scan_suffix_incl2", [x, y], block_threads)
    for k, (v, skip) in enumerate(((x, skip_x), (y, skip_y))):
        one, = _probe(handle, "wave_scan_suffix_incl_masked", v, block_threads)
        _identical(new[k], one, names, f"value {k}: wave_scan_suffix_incl2_masked != wave_scan_suffix_incl_masked", nan_payload=False)
        _identical(new[k], old[k], names, f"value {k}: wave_scan_suffix_incl2_masked != wave_scan_suffix_incl2", skip, nan_payload=False)
        _same_bits(new[k], ref_suffix_masked(v), names, f"value {k}: wave_scan_suffix_incl2_masked != its float32 restatement")


@pytest.mark.parametrize("block_threads", [64, 128, 256])
def test_masked_row_step_alone(handle, block_threads):
    """wave_suffix_fix_rows_masked on arbitrary lanes: rows 0..2 as the select tree, row 3 the operand's own bits (signalling
    NaNs and -0.0 included: no arithmetic touches it)"""
    x, names = _all(_inputs())
    new, = _probe(handle, "wave_suffix_fix_rows_masked", x, block_threads)
    old, = _probe(handle, "wave_suffix_fix_rows", x, block_threads)
    row3 = np.zeros(x.shape, bool)
    row3[:, 48:] = True
    _identical(new, old, names, "rows 0..2: wave_suffix_fix_rows_masked != wave_suffix_fix_rows", row3, nan_payload=False)
    _identical(new, x, names, "row 3: wave_suffix_fix_rows_masked changed its operand", ~row3)
    _same_bits(new, ref_fix_rows_masked(x), names, "wave_suffix_fix_rows_masked != its float32 restatement")


def test_call_site_operands_have_no_exception(handle):
    """On operands shaped like the adjoint's (+0.0 in every lane that is not a step's last, lane 63 among them) the two forms
    agree in all 64 lanes -- with -0.0 in every tail lane too."""
    x = _inputs()["call_site"]
    names = np.array(["call_site"] * len(x))
    assert not _lane48_exception(x).any()
    new, = _probe(handle, "wave_scan_suffix_incl_masked", x, 64)
    old, = _probe(handle, "wave_scan_suffix_incl", x, 64)
    _identical(new, old, names, "call-site operand: masked-row scan != select-tree scan", nan_payload=False)
    assert np.all(_i(new)[:, 63] == 0)                                    # (+0.0 in lane 63: what the shift down by a step reads)
