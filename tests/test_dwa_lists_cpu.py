"""tests/dwa_lists_reference.py -- the numpy restatement of the dynamic-window step over per-offset lists (nmpc_dwa_step_lists_*,
include/nmpc_hip.h) -- pinned without a device:

  1. with every count = H it is ``dwa_reference.run_step(..., dyn_mode=2)`` bit for bit on every recorded mode-2 call, in float64
     and as the float32 twin; the rows it must not read hold NaN
  2. a hand-made case checked point by point in plain python: an empty offset, an all-empty list, counts above R and below 0
  3. the argument block as the C compiler lays it out, the exported symbols, the refusals that need no device.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import dwa_cases as dc
import dwa_lists_reference as dl
import dwa_reference as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 20
KEYS = ("cost", "cand", "d_stc", "d_cur", "d_steps", "c_stc", "c_cur", "c_steps", "u", "traj")


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- 1. full lists are mode 2 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_full_lists_equal_mode_2_bit_for_bit(dtype):
    n_calls = 0
    for s, c, polys, cfg, rows in dc.recorded_calls():
        if s["dyn_mode"] != 2:
            continue
        H = rows.shape[0]
        want = dr.run_step(c["state"], s["goal"], c["last_u"], s["path"], polys, rows, 2, cfg, dtype)
        for R in (H, H + 3):                                   # rows beyond the counts are never looked at
            dyn = np.full((R, N + 1, 2), np.nan)
            dyn[:H] = rows
            got = dl.run_step(c["state"], s["goal"], c["last_u"], s["path"], polys, dyn, np.full(N + 1, H), cfg, dtype)
            assert (got["nv"], got["nw"], got["choice"]) == (want["nv"], want["nw"], want["choice"]), (s["name"], R)
            assert _same_bits(np.asarray(got["min_cost"]), np.asarray(want["min_cost"]))
            for k in KEYS:
                assert _same_bits(got[k], want[k]), (s["name"], R, k)
        n_calls += 1
    assert n_calls >= 10


# ---- 2. a hand-made case ------------------------------------------------------------------------------------------------------------
def _by_hand(r, obstacles, cfg, R):
    """(d_cur, d_steps) per candidate from the restatement's own trajectories, one python float at a time."""
    n = len(r["cost"])
    d_cur, d_steps = np.full(n, np.inf), np.full(n, np.inf)
    for j in range(n):
        for i in range(N + 1):
            x, y = float(r["traj"][j, i, 0]), float(r["traj"][j, i, 1])
            for ox, oy in obstacles[0][:R]:
                d_cur[j] = min(d_cur[j], math.hypot(x - ox, y - oy))
            if i < N:
                for ox, oy in obstacles[i + 1][:R]:
                    d_steps[j] = min(d_steps[j], math.sqrt(i + 1) * math.hypot(x - ox, y - oy))
    return d_cur, d_steps


def _term(d, first_inf):
    if first_inf:                                              # per-step: < 0.2 first
        return np.inf if d < 0.2 else 0.0 if d > 0.5 else 2.0 / d
    return 0.0 if d > 0.5 else np.inf if d < 0.2 else 2.0 / d  # offset 0: > 0.5 first


def test_hand_made_ragged_lists():
    cfg = dr.config()
    state, goal, last = np.array([0.0, 0.0, 0.0]), np.array([8.0, 0.5]), np.array([0.8, 0.0])
    path = np.array([[0.0, 0.0], [8.0, 0.5]])
    polys = np.zeros((0, 4, 2))
    R = 3
    rng = np.random.default_rng(3)
    ahead = lambda i: np.array([0.16 * i, 0.0])                # where the robot is after i steps at 0.8 m/s
    obstacles = [[(-0.35, 0.1)]]                               # offset 0: one position just behind the robot
    for t in range(1, N + 1):
        k = (0, 1, 2, 3, 5)[t % 5]                             # 0 .. 5 entries: empty offsets and more than R rows
        obstacles.append([tuple(ahead(t - 1) + rng.normal(0, 0.15, 2) + (0.0, 0.3)) for _ in range(k)])
    dyn, count = dl.lists_from(obstacles, R)
    assert count.max() == R and (count == 0).sum() == 4 and set(count.tolist()) == {0, 1, 2, 3} and np.isnan(dyn).any()
    r = dl.run_step(state, goal, last, path, polys, dyn, count, cfg)
    base = dr.run_step(state, goal, last, path, polys, None, 0, cfg)
    d_cur, d_steps = _by_hand(r, obstacles, cfg, R)
    assert np.allclose(r["d_cur"], d_cur, rtol=1e-12, atol=0) and np.allclose(r["d_steps"], d_steps, rtol=1e-12, atol=0)
    for j in range(len(r["cost"])):
        assert min(abs(d_cur[j] - t) for t in (0.2, 0.5)) > 1e-9 and min(abs(d_steps[j] - t) for t in (0.2, 0.5)) > 1e-9
        want = base["cost"][j] + (_term(d_steps[j], True) + _term(d_cur[j], False))
        assert (np.isinf(want) and np.isinf(r["cost"][j])) or abs(r["cost"][j] - want) <= 1e-12 * (1 + abs(want)), j
    fin = np.isfinite(r["cost"])
    assert np.isinf(r["cost"]).any() and (r["c_steps"][fin] > 0).any() and (r["c_cur"] > 0).any() and r["choice"] == int(np.argmin(r["cost"]))
    # counts above R are R, counts below 0 are 0: the rows beyond are not looked at
    wild = count.copy()
    wild[count == R] = R + 4
    wild[count == 0] = -2
    r2 = dl.run_step(state, goal, last, path, polys, dyn, wild, cfg)
    assert all(_same_bits(r[k], r2[k]) for k in KEYS) and r2["choice"] == r["choice"]
    # an offset emptied: its means stop counting
    t_hit = int(np.argmin([min([math.sqrt(i + 1) * math.hypot(*(r["traj"][r["choice"], i, :2] - np.array(o))) for o in obstacles[i + 1][:R]] or [np.inf])
                           for i in range(N)])) + 1
    less = count.copy()
    less[t_hit] = 0
    r3 = dl.run_step(state, goal, last, path, polys, dyn, less, cfg)
    assert (r3["d_steps"] >= r["d_steps"]).all() and (r3["d_steps"] > r["d_steps"]).any() and _same_bits(r3["d_cur"], r["d_cur"])
    # an all-empty list: the cost without a dynamic term, bit for bit; offset 0 alone: mode 1
    r4 = dl.run_step(state, goal, last, path, polys, dyn, np.zeros(N + 1, int), cfg)
    assert _same_bits(r4["cost"], base["cost"]) and r4["choice"] == base["choice"] and np.isinf(r4["d_steps"]).all() and np.isinf(r4["d_cur"]).all()
    only0 = np.zeros(N + 1, int)
    only0[0] = 1
    r5 = dl.run_step(state, goal, last, path, polys, dyn, only0, cfg)
    m1 = dr.run_step(state, goal, last, path, polys, np.nan_to_num(dyn[:1]), 1, cfg)
    assert _same_bits(r5["cost"], m1["cost"]) and not (r5["c_steps"] != 0).any()
    # offsets alone, nothing at offset 0
    no0 = count.copy()
    no0[0] = 0
    r6 = dl.run_step(state, goal, last, path, polys, dyn, no0, cfg)
    assert np.isinf(r6["d_cur"]).all() and not r6["c_cur"].any() and _same_bits(r6["d_steps"], r["d_steps"])


def test_lists_from_drops_entries_beyond_the_rows():
    obstacles = [[(float(t), float(k)) for k in range(t % 4)] for t in range(N + 1)]
    dyn, count = dl.lists_from(obstacles, 2)
    assert dyn.shape == (2, N + 1, 2) and count.tolist() == [min(t % 4, 2) for t in range(N + 1)]
    assert np.array_equal(dyn[1, 2], (2.0, 1.0)) and np.isnan(dyn[1, 1]).all() and np.isnan(dyn[0, 0]).all()


# ---- 3. the argument block and the symbols ----------------------------------------------------------------------------------------------
def test_lists_args_layout_matches_the_header(tmp_path):
    from dyobav_mpcnwta_warehouse_amd import _capi
    cc = next((c for c in ("cc", "gcc", "clang") if subprocess.run(["which", c], capture_output=True).returncode == 0), None)
    if cc is None:
        pytest.skip("no C compiler")
    names = [n for n, _ in _capi.NmpcDwaListsArgs._fields_]
    assert names[7] == "R" and names[-1] == "dyn_count" and [n for n in names[:-1] if n != "R"] == [n for n, _ in _capi.NmpcDwaArgs._fields_ if n != "reserved"]
    src = tmp_path / "l.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nmpc_hip.h"\nint main(void){printf("%zu %zu %d", sizeof(nmpc_dwa_lists_args), '
                   'sizeof(nmpc_dwa_args), NMPC_ABI_VERSION);\n' +
                   "".join(f'printf(" %zu", offsetof(nmpc_dwa_lists_args, {n}));\n' for n in names) + "return 0;}\n")
    exe = tmp_path / "l"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == ctypes.sizeof(_capi.NmpcDwaListsArgs) and out[1] == ctypes.sizeof(_capi.NmpcDwaArgs) and out[2] == 5
    assert out[3:] == [getattr(_capi.NmpcDwaListsArgs, n).offset for n in names]


def test_library_exports_the_entry_points_and_refuses_null():
    import dyobav_mpcnwta_warehouse_amd as nm
    from dyobav_mpcnwta_warehouse_amd import _capi
    lib = nm.load_library()
    for name in ("nmpc_dwa_step_lists_f32", "nmpc_dwa_step_lists_f64", "nmpc_hypotheses_to_ellipses_counts_f32", "nmpc_hypotheses_to_ellipses_counts_f64"):
        assert name in nm.EXPORTED_SYMBOLS and hasattr(lib, name), name
    a = _capi.NmpcDwaListsArgs()
    assert lib.nmpc_dwa_step_lists_f64(None, ctypes.byref(a)) == -1 and lib.nmpc_dwa_step_lists_f32(None, None) == -1
    assert lib.nmpc_hypotheses_to_ellipses_counts_f64(None, None, 1, None, 1, 0.2, 1.0, 2.0, 0.0, 1, None, None, None) == -1
    assert hasattr(nm.Handle, "dwa_step_lists")
