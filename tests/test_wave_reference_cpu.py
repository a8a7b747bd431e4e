"""The host restatements of the wavefront primitives (tests/wave_reference.py) against each other, and the comparison
the GPU test relies on against three deliberately wrong restatements -- all without a GPU. Also: every primitive of
csrc/wave_ops.h has a probe op, and nmpc_probe_* refuses bad arguments before it needs a device."""
import ctypes
import os
import re

import numpy as np
import pytest

import dyobav_mpcnwta_warehouse_amd as nm
from dyobav_mpcnwta_warehouse_amd._capi import PROBE_OPS
import wave_reference as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVE_OPS = [op for op, spec in PROBE_OPS.items() if spec[0] <= PROBE_OPS["class_sums_by_wave_sum3"][0]]
DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module", params=DTYPES, ids=["f32", "f64"])
def waves(request):
    x, where = wr.all_waves(request.param)
    x.setflags(write=False)
    return request.param, x, where


@pytest.mark.parametrize("op", WAVE_OPS)
def test_ordered_form_passes_its_own_comparison(op, waves):
    """Form (b) agrees with form (a) within gamma_63 * sum|x_j| over the contributing lanes -- the worst case over every
    summation order, so no measurement is behind it -- with NaN and infinities in the same lanes, on every family."""
    dtype, x, _ = waves
    xs = wr.operands(op, x, PROBE_OPS[op][2])
    assert wr.check(op, dtype, xs, wr.ordered(op, xs)) == []


@pytest.mark.parametrize("op", WAVE_OPS)
def test_the_two_forms_are_equal_on_deltas_and_integers(op, waves):
    dtype, x, where = waves
    for name in ("deltas", "integers", "constants"):
        xs = wr.operands(op, x[where[name]], PROBE_OPS[op][2])
        for b, a in zip(wr.ordered(op, xs), wr.exact(op, xs)[0]):
            assert np.array_equal(b.astype(wr.EXACT), a), (op, name)


def test_deltas_show_which_lanes_see_which():
    d = np.eye(64, dtype=np.float32)                       # wave j: a 1 in lane j
    i, j = np.meshgrid(wr.LANE, wr.LANE)                   # [wave j, lane i]
    assert np.array_equal(wr.ordered("wave_sum", [d])[0], np.ones((64, 64)))
    assert np.array_equal(wr.ordered("wave_scan_incl", [d])[0], (i >= j))
    assert np.array_equal(wr.ordered("wave_scan_suffix_incl", [d])[0], (i <= j))
    assert np.array_equal(wr.ordered("class3_sum1", [d])[0], (i % 3 == j % 3))
    assert np.array_equal(wr.ordered("wave_shift_up_3", [d])[0], (i == j + 3))
    assert np.array_equal(wr.ordered("wave_shift_down_2", [d])[0], (i == j - 2))
    assert np.array_equal(wr.ordered("wave_suffix_fix_rows", [d])[0], (i == j) | ((j % 16 == 0) & (j // 16 > i // 16)))


WRONG = {
    "wave_scan_incl": wr.wrong_scan_row_mask,
    "class3_sum1": wr.wrong_class3_address,
    "wave_sum": wr.wrong_wave_sum_no_r3,
}


@pytest.mark.parametrize("op", sorted(WRONG))
def test_wrong_variants_fail_the_comparison(op, waves):
    """A prefix scan whose last row step misses row 2, a class sum with one wrong last-lane address, a wave_sum without
    r3 += r2: each must fail check() -- the function the GPU test calls -- on at least one family, the deltas among them."""
    dtype, x, where = waves
    failing = [name for name, sl in where.items() if wr.check(op, dtype, [x[sl]], [WRONG[op](x[sl])])]
    assert "deltas" in failing and "scaled_normal" in failing, (op, failing)
    msg = wr.check(op, dtype, [x[where["deltas"]]], [WRONG[op](x[where["deltas"]])])[0]
    assert re.search(r"wave \d+ lane \d+", msg), msg


def test_comparison_notices_a_change_of_association_only():
    """Summing the four row totals in another order is within the gamma bound but not the promised bits."""
    x = wr.families(np.float32)["scaled_normal"]
    r = [x[:, 16 * q:16 * q + 16] for q in range(4)]
    rs = [wr._row_butterfly(np.tile(v, 4))[:, 0] for v in r]
    other = wr._bcast(((rs[0] + rs[1]) + rs[2]) + rs[3])
    msgs = wr.check("wave_sum", np.float32, [x], [other])
    assert msgs and all("ordered restatement" in m for m in msgs), msgs[:2]


def test_comparison_notices_misplaced_nan_and_inf():
    fam = wr.families(np.float64)
    x = fam["one_nan"]
    good = wr.ordered("wave_scan_incl", [x])[0]
    assert wr.check("wave_scan_incl", np.float64, [x], [good]) == []
    bad = good.copy()
    bad[0, 0] = 1.0                                        # the NaN sat in lane 0: every lane of wave 0 must be NaN
    assert any("NaN" in m for m in wr.check("wave_scan_incl", np.float64, [x], [bad]))
    x = fam["one_inf"]
    bad = wr.ordered("wave_sum", [x])[0]
    bad[3, 5] = np.finfo(np.float64).max
    assert any("infinity" in m for m in wr.check("wave_sum", np.float64, [x], [bad]))


def test_every_primitive_of_wave_ops_h_has_a_probe_op():
    """A primitive added to wave_ops.h later cannot stay unprobed, and the table names nothing that is not there."""
    text = open(os.path.join(ROOT, "dyobav-mpcnwta-warehouse_amd", "csrc", "wave_ops.h")).read()
    text = re.sub(r"//[^\n]*", "", text)
    names = set(re.findall(r"__device__\s+(?:__forceinline__\s+|inline\s+)?[\w:<>]+[\s&*]+(\w+)\s*\(", text))
    assert {"wave_sum", "class3_addresses", "wave_suffix_fix_rows", "dpp_mov", "ref_wave_sum"} <= names, names
    primitives = {n for n in names if n != "dpp_mov" and not n.startswith("ref_")}
    device_h = open(os.path.join(ROOT, "dyobav-mpcnwta-warehouse_amd", "csrc", "nmpc_device.h")).read()
    scalar = {"sincos_medium", "sincos_small", "fast_rcp", "ls_point"}
    for n in scalar:
        assert re.search(r"__device__ __forceinline__ \w+ " + n + r"\(", device_h), n
    probed = {f for spec in PROBE_OPS.values() for f in spec[1]}
    assert probed - scalar == primitives, (sorted(primitives - probed), sorted(probed - scalar - primitives))
    assert scalar <= probed


def test_probe_table_matches_the_header_and_the_kernel():
    header = open(os.path.join(ROOT, "include", "nmpc_hip.h")).read()
    enum = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"NMPC_PROBE_(\w+) = (\d+)", header)}
    n_ops = enum.pop("n_ops")
    assert enum == {op: spec[0] for op, spec in PROBE_OPS.items()} and sorted(enum.values()) == list(range(n_ops))
    capi = open(os.path.join(ROOT, "dyobav-mpcnwta-warehouse_amd", "csrc", "nmpc_capi.hip")).read()
    for op in PROBE_OPS:
        assert f"OP == NMPC_PROBE_{op.upper()})" in capi, op
    assert "nmpc_probe_f32" in nm.EXPORTED_SYMBOLS and "nmpc_probe_f64" in nm.EXPORTED_SYMBOLS


def test_probe_refuses_bad_arguments_before_touching_the_device():
    """Every refusal comes before the handle is looked at, so it can be checked with no device: -1 and a message."""
    lib = nm.load_library()
    buf = (ctypes.c_double * (6 * 64))()
    p = ctypes.addressof(buf)
    for fn, float_only_refused in ((lib.nmpc_probe_f32, False), (lib.nmpc_probe_f64, True)):
        for args, word in (((-1, 64, 1, p, p), b"unknown op"), ((len(PROBE_OPS), 64, 1, p, p), b"unknown op"),
                           ((0, 0, 1, p, p), b"block_threads"), ((0, 32, 1, p, p), b"block_threads"),
                           ((0, 192, 1, p, p), b"block_threads"), ((0, 512, 1, p, p), b"block_threads"),
                           ((0, 64, -1, p, p), b"n_waves"), ((0, 64, 1, None, p), b"NULL"), ((0, 64, 1, p, None), b"NULL"),
                           ((0, 64, 0, None, None), b"NULL"), ((0, 256, 1, p, p), b"null handle"),
                           ((0, 64, 0, p, p), b"null handle")):
            assert fn(None, *args) == -1, args
            assert word in lib.nmpc_last_error(), (args, lib.nmpc_last_error())
        for op in ("sincos_medium", "sincos_small"):
            assert fn(None, PROBE_OPS[op][0], 64, 1, p, p) == -1
            assert (b"unknown op" in lib.nmpc_last_error()) == float_only_refused
    assert buf[0] == 0.0
