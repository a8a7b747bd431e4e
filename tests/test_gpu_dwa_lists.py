"""The dynamic-window tracker over PER-OFFSET LISTS -- ``dwa_step_lists_kernel`` (csrc/nmpc_dwa.h, entry points
nmpc_dwa_step_lists_*), what makes ``tracker="dwa"`` run on the multi-hypothesis predictor's cluster means -- through
``Handle.dwa_step_lists``, ``Handle.hypotheses_to_ellipses(..., counts=)``, ``BatchEvaluator(tracker="dwa", predictor="mmp")`` and the
drop-in ``DwaInterface``, against tests/dwa_lists_reference.py (pinned to the mode-2 restatement and by hand in
tests/test_dwa_lists_cpu.py) and the recordings of tests/golden/dwa_cases.json:

  1. full lists are mode 2: the recorded mode-2 sequences with R = H and counts = H, fp64 against the recording, fp32 against the twin
  2. ragged lists: R = 6, counts 0 .. R per offset, an all-empty scenario, counts above R and below 0, the fine grid (234 candidates);
     the rows and columns that must not be read hold NaN in one run and the robot's own position in the other
  3. a scenario gives the same bytes alone and among others through a permuted run list
  4. refusals, outputs untouched
  5. f2's per-offset counts on the recordings tests/test_gpu_hypotheses.py reads
  6. the evaluator call by call with a prescribed network: one, two and no cluster per offset; with compaction the same bytes
  7. the drop-in class.

Tolerances are those of tests/test_gpu_dwa.py for mode 2, unchanged: fp64 costs 1e-9 (1 + |cost|); fp32 four times ``delta_f32`` of
the fixture against the float32 twin, candidates within 4 delta_f32["dist"] of a threshold left out, at most 2 % of all candidates.
"""
import json
import os

import numpy as np
import pytest

import dwa_cases as dc
import dwa_lists_reference as dl
import dwa_reference as dr

pytestmark = pytest.mark.gpu

N, TS, R6 = 20, 0.2, 6
SENTINEL = -7.5e6
_handles = {}


def _handle():
    import torch
    import dyobav_mpcnwta_warehouse_amd as nm
    if "h" not in _handles:
        cfg = nm.default_config_struct()
        cfg.N_hor, cfg.ts = N, TS
        h = nm.Handle(cfg)
        h.set_stream(torch.cuda.current_stream().cuda_stream)
        _handles["h"] = h
    return _handles["h"]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for h in _handles.values():
        h.close()
    _handles.clear()


def _cap(cfg):
    cap = 1
    for rng, acc, res in ((cfg.lin_vel_max - cfg.lin_vel_min, cfg.lin_acc_max, cfg.vel_resolution), (2 * cfg.ang_vel_max, cfg.ang_acc_max, cfg.ang_resolution)):
        cap *= int(min(rng, 2 * acc * TS) / res * (1 + 1e-9)) + 1
    return cap


def lists_call(dtype, state_c, last_u_c, dyn, count, goal, path, plen, polys, cfg, run=None, cap=None, unread="nan", over=None, want_all=True):
    """One ``nmpc_dwa_step_lists`` call. ``state_c`` / ``last_u_c`` [n_run, ...] compact, ``dyn`` [n_run, R, N+1, 2] with ``count``
    [n_run, N+1], ``goal`` / ``path`` / ``plen`` [B, ...]. Everything of ``dyn_c`` that the entry must not read -- rows at or beyond the
    (clamped) count of their offset, columns 2:6 of every row -- holds NaN (``unread="nan"``) or the robot's own position (``"own"``:
    one read of it as an obstacle puts every candidate at distance 0 of it, i.e. at +inf). -> dict of numpy outputs, every one starting
    as SENTINEL (-9 for the integers). ``over``: fields of the argument block set last."""
    import torch
    from dyobav_mpcnwta_warehouse_amd import _capi
    dtype = np.dtype(dtype)
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    up = lambda x, dt=dtype: torch.as_tensor(np.ascontiguousarray(x, dtype=dt)).cuda()
    state_c, dyn, count = np.asarray(state_c, dtype=float), np.asarray(dyn, dtype=float), np.asarray(count)
    n_run, B, R = int(state_c.shape[0]), int(np.shape(goal)[0]), int(dyn.shape[1])
    cap = _cap(cfg) if cap is None else cap
    polys = np.asarray(polys, dtype=float).reshape(-1, 4, 2)
    own = np.tile(state_c[:, None, None, :2], (1, R, N + 1, 3))
    rows = np.full((n_run, R, N + 1, 6), np.nan) if unread == "nan" else own.copy()
    exists = np.arange(R)[None, :, None] < np.clip(count, 0, R)[:, None, :]
    rows[..., :2] = np.where(exists[..., None], dyn, rows[..., :2])
    t = dict(state_c=up(state_c), last_u_c=up(last_u_c), goal=up(goal), path=up(path), path_len=up(plen, np.int64), dyn_c=up(rows),
             dyn_count=up(count, np.int32))
    if polys.shape[0]:
        t["polys"] = up(polys)
    if run is not None:
        t["run"] = up(run, np.int64)
    out = dict(U_c=torch.full((n_run, 2 * N), SENTINEL, dtype=tdt, device="cuda"), min_cost=torch.full((n_run,), SENTINEL, dtype=tdt, device="cuda"),
               choice=torch.full((n_run,), -9, dtype=torch.int32, device="cuda"), counts=torch.full((n_run, 2), -9, dtype=torch.int32, device="cuda"))
    if want_all:
        out.update(cost_all=torch.full((n_run, cap), SENTINEL, dtype=tdt, device="cuda"), cand_all=torch.full((n_run, cap, 2), SENTINEL, dtype=tdt, device="cuda"))
    a = _capi.NmpcDwaListsArgs().set_config(cfg, 0.8)
    a.B, a.n_run, a.R, a.M, a.Pmax, a.cap = B, n_run, R, int(polys.shape[0]), int(np.shape(path)[1]), cap
    for k, v in {**t, **out}.items():
        assert v.is_contiguous()
        setattr(a, k, v.data_ptr())
    err = None
    for k, v in (over or {}).items():
        setattr(a, k, v)
    try:
        _handle().dwa_step_lists(dtype, a)
    except Exception as e:      # the caller looks at it; the outputs must be untouched
        err = e
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res["error"] = err
    return res


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _check_fp64(r, a, want, where, exact_choice=True):
    """Row ``a`` of an fp64 call against ``want`` (a restatement's dict, or a recorded call): counts, candidate bits, costs, choice, U_c."""
    n = want["nv"] * want["nw"]
    assert tuple(r["counts"][a]) == (want["nv"], want["nw"]), where
    assert _same_bits(r["cand_all"][a, :n], np.array(want["cand"], dtype=np.float64).reshape(n, 2)), where
    assert (r["cost_all"][a, n:] == SENTINEL).all(), where
    got, cost = r["cost_all"][a, :n], np.array(want["cost"], dtype=np.float64)
    assert np.array_equal(np.isfinite(got), np.isfinite(cost)) and not np.isnan(got).any(), (where, np.nonzero(np.isfinite(got) != np.isfinite(cost))[0])
    fin = np.isfinite(cost)
    err = np.abs(got[fin] - cost[fin]) / (1.0 + np.abs(cost[fin]))
    assert (err <= 1e-9).all(), (where, float(err.max()))
    ch = int(r["choice"][a])
    if exact_choice or dc.cost_gap(cost) > 1e-6:
        assert ch == want["choice"] and np.array_equal(r["U_c"][a, :2], np.array(want["u"])), (where, ch, want["choice"])
    assert np.array_equal(r["U_c"][a], np.tile(r["U_c"][a, :2], N)), where
    if want["choice"] < 0:
        assert ch == -1 and r["min_cost"][a] == np.inf and not r["U_c"][a].any(), where
    else:
        assert r["min_cost"][a] == got[ch] and abs(r["min_cost"][a] - want["min_cost"]) <= 1e-9 * (1 + abs(want["min_cost"])), where
    return n, int((~fin).sum()), float(err.max(initial=0.0))


def _check_fp32(r, a, tw, where, tol_c, tol_d):
    """Row ``a`` of an fp32 call against the float32 twin ``tw``, as tests/test_gpu_dwa.py does for mode 2. -> (candidates, left out)."""
    n = tw["nv"] * tw["nw"]
    assert tuple(r["counts"][a]) == (tw["nv"], tw["nw"]), where
    assert _same_bits(r["cand_all"][a, :n], tw["cand"]), where
    got, want = r["cost_all"][a, :n].astype(np.float64), tw["cost"].astype(np.float64)
    near = dr.near_threshold(tw, tol_d)
    ok = ~near
    assert np.array_equal(np.isfinite(got[ok]), np.isfinite(want[ok])) and not np.isnan(got).any(), where
    fin = ok & np.isfinite(want)
    err = np.abs(got[fin] - want[fin])
    assert (err <= tol_c).all(), (where, float(err.max()), tol_c)
    ch = int(r["choice"][a])
    if tw["choice"] < 0 and not near.any():
        assert ch == -1 and not r["U_c"][a].any() and r["min_cost"][a] == np.inf, where
    elif ch != tw["choice"]:
        assert ch >= 0 and (near[ch] or want[ch] <= float(tw["min_cost"]) + tol_c), (where, ch, tw["choice"])
    if ch >= 0:
        u = tw["cand"][ch].copy()
        if abs(u[0]) < np.float32(1e-3):
            u[1] = np.float32(-0.5)
        assert _same_bits(r["U_c"][a], np.tile(u, N)), where
    return n, int(near.sum()), float(err.max(initial=0.0))


# ---- 1. full lists are mode 2 ----------------------------------------------------------------------------------------------------
def _seq_lists_call(seq, dtype, rounded=False):
    """All calls of a recorded mode-2 sequence in one launch of the lists entry: R = H, every count = H."""
    calls = seq["calls"]
    B = len(calls)
    f = (lambda x: np.asarray(x, dtype=np.float32).astype(np.float64)) if rounded else (lambda x: np.asarray(x, dtype=np.float64))
    path = np.repeat(f(seq["path"])[None], B, axis=0)
    dyn = np.stack([f(dc.call_dyn(seq, c)) for c in calls])
    r = lists_call(dtype, f([c["state"] for c in calls]), f([c["last_u"] for c in calls]), dyn, np.full((B, N + 1), dyn.shape[1]),
                   np.repeat(f(seq["goal"])[None], B, axis=0), path, np.full(B, path.shape[1]), f(dc.seq_polys(seq)), dc.seq_config(seq))
    assert r["error"] is None, r["error"]
    return r


def test_full_lists_are_mode_2_fp64_against_the_recording():
    n_cand = n_inf = 0
    worst = 0.0
    for s in dc.golden()["sequences"]:
        if s["dyn_mode"] != 2:
            continue
        r = _seq_lists_call(s, np.float64)
        for a, c in enumerate(s["calls"]):
            n, ninf, err = _check_fp64(r, a, c, (s["name"], a))
            n_cand, n_inf, worst = n_cand + n, n_inf + ninf, max(worst, err)
    print(f"fp64, full lists: {n_cand} candidates ({n_inf} +inf), worst cost error {worst:.2e} (absolute + relative)")
    assert n_cand > 700 and n_inf > 20


def test_full_lists_are_mode_2_fp32_against_the_twin():
    g = dc.golden()
    tol_c, tol_d = 4 * g["delta_f32"]["cost"], 4 * g["delta_f32"]["dist"]
    n_cand = n_out = 0
    worst = 0.0
    for s in g["sequences"]:
        if s["dyn_mode"] != 2:
            continue
        r = _seq_lists_call(s, np.float32, rounded=True)
        for a, c in enumerate(s["calls"]):
            n, out, err = _check_fp32(r, a, dc.restate(s, c, np.float32, rounded=True), (s["name"], a), tol_c, tol_d)
            n_cand, n_out, worst = n_cand + n, n_out + out, max(worst, err)
    print(f"fp32, full lists: {n_cand} candidates, {n_out} left out near a threshold, worst cost error {worst:.3e} (bound {tol_c:.3e})")
    assert n_cand > 700 and n_out <= 0.02 * n_cand


# ---- 2. ragged lists ---------------------------------------------------------------------------------------------------------------
FINE = dict(vel_resolution=0.05, ang_resolution=0.04, ang_vel_max=0.51)        # 9 x 26 = 234 candidates (tests/test_gpu_dwa.py, edges)
N_RAGGED = 11


def ragged_cases(fine=False, seed=41):
    """Scenarios on the warehouse map (the start states, goals and node paths of the closed-loop fixture) with per-offset lists in
    R = 6 rows: 2 .. 4 current positions, 0 .. R means per offset. The means that matter are placed with the restatement, here on the
    CPU: next to point i of a candidate's trajectory at 0.1 .. 0.6 m / sqrt(i + 1), so that d_i falls around the thresholds of the
    per-step term; the others lie 1 .. 4 m away. Scenario 1 has every offset empty, scenario 2 has counts above R and below 0 (which
    mean R and 0). -> dict(cfg, state, last, goal, path, plen, polys, dyn [n, R, N+1, 2], count [n, N+1], want: the restatement's list)."""
    cfg = dr.config(**FINE) if fine else dr.config()
    n = 2 if fine else N_RAGGED
    s0, path, plen, _ = dc.loop_initial(dc.golden()["closed_loop"]["seed"], B=n)
    rng = np.random.default_rng([seed, int(fine)])
    polys = s0["polys"]
    state, goal = s0["robot"].copy(), s0["goal"].copy()
    if fine:
        v = next(v for v in np.arange(0.3, 1.0, 0.0125) if np.prod(dr.candidates([v, 0.0], cfg)[:2]) == 234)
        last = np.array([[v, 0.0]] * n)
    else:
        last = np.stack([rng.uniform(0.1, 1.2, n), rng.uniform(-0.3, 0.3, n)], axis=1)
    dyn = np.zeros((n, R6, N + 1, 2))
    count = np.zeros((n, N + 1), dtype=np.int32)
    unit = lambda: (lambda a: np.array([np.cos(a), np.sin(a)]))(rng.uniform(0, 2 * np.pi))
    for a in range(n):
        traj = dr.run_step(state[a], goal[a], last[a], path[a, :plen[a]], polys, None, 0, cfg)["traj"]
        count[a] = rng.integers(0, R6 + 1, N + 1)
        count[a, 0] = 2 + a % 3
        count[a, 1:7] = np.maximum(count[a, 1:7], 1)
        for t in range(N + 1):
            for r in range(R6):
                dyn[a, r, t] = state[a, :2] + unit() * rng.uniform(1.0, 4.0)
        for t in rng.choice(np.arange(2, 7), 2, replace=False):  # point i = t - 1 of some candidate
            j = rng.integers(0, traj.shape[0])
            dyn[a, rng.integers(0, count[a, t]), t] = traj[j, t - 1, :2] + unit() * rng.uniform(0.2, 0.6) / np.sqrt(t)
        dyn[a, 0, 0] = state[a, :2] + unit() * rng.uniform(0.45, 0.9)
    if not fine:
        count[1] = 0
        count[2, 8:] = np.where(np.arange(8, N + 1) % 2 == 0, R6 + 1 + np.arange(8, N + 1), -1 - np.arange(8, N + 1))
    return dict(cfg=cfg, state=state, last=last, goal=goal, path=path, plen=plen, polys=polys, dyn=dyn, count=count)


def _restate(c, dtype, rounded=False):
    f = (lambda x: np.asarray(x, dtype=np.float32).astype(np.float64)) if rounded else (lambda x: np.asarray(x, dtype=np.float64))
    return [dl.run_step(f(c["state"][a]), f(c["goal"][a]), f(c["last"][a]), f(c["path"][a, :c["plen"][a]]), f(c["polys"]), f(c["dyn"][a]),
                        c["count"][a], c["cfg"], dtype) for a in range(c["state"].shape[0])]


def _ragged_call(c, dtype, unread, rounded=False, **kw):
    f = (lambda x: np.asarray(x, dtype=np.float32).astype(np.float64)) if rounded else (lambda x: np.asarray(x, dtype=np.float64))
    return lists_call(dtype, f(c["state"]), f(c["last"]), f(c["dyn"]), c["count"], f(c["goal"]), f(c["path"]), c["plen"], f(c["polys"]), c["cfg"],
                      unread=unread, **kw)


@pytest.fixture(scope="module")
def ragged():
    """The cases and their restatements (fp64 and the float32 twin), computed once."""
    out = {}
    for fine in (False, True):
        c = ragged_cases(fine)
        out[fine] = (c, _restate(c, np.float64), _restate(c, np.float32, rounded=True))
    return out


def test_the_per_step_term_decides_in_the_ragged_cases(ragged):
    """On the CPU side of the fixture: the shares that make test 2 mean something."""
    n = n_mid = n_inf = 0
    for fine in (False, True):
        c, want, _ = ragged[fine]
        for w in want:
            n += len(w["cost"])
            n_mid += int((np.isfinite(w["c_steps"]) & (w["c_steps"] > 0)).sum())
            n_inf += int(np.isinf(w["c_steps"]).sum())
        assert max(w["nv"] * w["nw"] for w in want) == 234 if fine else 30 < max(w["nv"] * w["nw"] for w in want) <= _cap(c["cfg"]) == 55
    c = ragged[False][0]["count"]
    assert (c[1] == 0).all() and c[2].max() > R6 and c[2].min() < 0 and {int(v) for v in c[[0] + list(range(3, N_RAGGED)), 0]} == {2, 3, 4}
    assert len({int(v) for v in c[0, 1:]}) > 3 and (c[3:, 7:] == 0).any()
    print(f"ragged lists: {n} candidates, {n_mid} with a finite non-zero per-step cost, {n_inf} with +inf")
    assert n_mid > 0.25 * n and n_inf > 0.02 * n


@pytest.mark.parametrize("fine", [False, True], ids=["cap55", "cap234"])
def test_ragged_lists_fp64(ragged, fine):
    c, want, _ = ragged[fine]
    runs = [_ragged_call(c, np.float64, unread) for unread in ("nan", "own")]
    assert runs[0]["error"] is None and runs[1]["error"] is None
    for k in ("U_c", "min_cost", "choice", "counts", "cost_all", "cand_all"):
        assert _same_bits(runs[0][k], runs[1][k]), k
    worst = 0.0
    for a, w in enumerate(want):
        worst = max(worst, _check_fp64(runs[0], a, w, (fine, a), exact_choice=False)[2])
    print(f"fp64, ragged lists (fine = {fine}): worst cost error {worst:.2e}")
    if fine:
        assert int(np.prod(runs[0]["counts"][0])) == 234 > 64
    else:                               # every offset empty: the cost without a dynamic term
        base = dr.run_step(c["state"][1], c["goal"][1], c["last"][1], c["path"][1, :c["plen"][1]], c["polys"], None, 0, c["cfg"])
        n = base["nv"] * base["nw"]
        assert np.array_equal(np.isfinite(runs[0]["cost_all"][1, :n]), np.isfinite(base["cost"])) and runs[0]["choice"][1] == base["choice"]


def test_ragged_lists_fp32(ragged):
    g = dc.golden()
    tol_c, tol_d = 4 * g["delta_f32"]["cost"], 4 * g["delta_f32"]["dist"]
    n_cand = n_out = 0
    worst = 0.0
    for fine in (False, True):
        c, _, twin = ragged[fine]
        runs = [_ragged_call(c, np.float32, unread, rounded=True) for unread in ("nan", "own")]
        assert runs[0]["error"] is None and runs[1]["error"] is None
        for k in ("U_c", "min_cost", "choice", "counts", "cost_all", "cand_all"):
            assert _same_bits(runs[0][k], runs[1][k]), (fine, k)
        for a, tw in enumerate(twin):
            n, out, err = _check_fp32(runs[0], a, tw, (fine, a), tol_c, tol_d)
            n_cand, n_out, worst = n_cand + n, n_out + out, max(worst, err)
    print(f"fp32, ragged lists: {n_cand} candidates, {n_out} left out near a threshold, worst cost error {worst:.3e} (bound {tol_c:.3e})")
    assert n_out <= 0.02 * n_cand


# ---- 3. independence ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_scenario_gives_the_same_bytes_alone_or_among_others(ragged, dtype):
    c = ragged[False][0]
    full = _ragged_call(c, dtype, "nan")
    assert full["error"] is None and (full["choice"] >= 0).any()
    run = np.random.default_rng(5).permutation(N_RAGGED)[:7]
    sub = dict(c, state=c["state"][run], last=c["last"][run], dyn=c["dyn"][run], count=c["count"][run])
    part = _ragged_call(sub, dtype, "nan", run=run)
    assert part["error"] is None
    for k in ("U_c", "min_cost", "choice", "counts", "cost_all", "cand_all"):
        assert _same_bits(part[k], full[k][run]), k
    alone = _ragged_call(dict(c, state=c["state"][4:5], last=c["last"][4:5], dyn=c["dyn"][4:5], count=c["count"][4:5]), dtype, "own", run=np.array([4]),
                         want_all=False)
    for k in ("U_c", "min_cost", "choice", "counts"):
        assert _same_bits(alone[k], full[k][4:5]), k


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------
def test_lists_entry_refuses_bad_arguments(ragged):
    import torch
    import dyobav_mpcnwta_warehouse_amd as nm
    c = ragged[False][0]
    one = dict(c, state=c["state"][:1], last=c["last"][:1], dyn=c["dyn"][:1], count=c["count"][:1], goal=c["goal"][:1], path=c["path"][:1], plen=c["plen"][:1])
    spare = torch.zeros(64, dtype=torch.float64, device="cuda")
    host = np.zeros((1, N + 1), dtype=np.int32)
    INVALID, UNSUPPORTED = -1, -4
    bad = {"dyn_count = NULL": (dict(dyn_count=None), INVALID), "dyn_c = NULL": (dict(dyn_c=None), INVALID), "R = 0": (dict(R=0), INVALID),
           "R < 0": (dict(R=-3), INVALID), "misaligned dyn_count": (dict(dyn_count=spare.data_ptr() + 2), INVALID),
           "misaligned dyn_c": (dict(dyn_c=spare.data_ptr() + 4), INVALID), "misaligned U_c": (dict(U_c=spare.data_ptr() + 2), INVALID),
           "n_run > B": (dict(n_run=2), INVALID), "cap = 0": (dict(cap=0), INVALID),
           "R (N + 1) = 861 > 840": (dict(R=41), UNSUPPORTED), "cap too small": (dict(cap=_cap(c["cfg"]) - 1), UNSUPPORTED),
           "a host pointer": (dict(dyn_count=host.ctypes.data), INVALID)}
    for what, (over, code) in bad.items():
        r = _ragged_call(one, np.float64, "nan", over=over)
        e = r["error"]
        assert isinstance(e, nm.NmpcError) and e.code == code and "nmpc_dwa_step_lists" in str(e), (what, e)
        assert (r["cost_all"] == SENTINEL).all() and (r["min_cost"] == SENTINEL).all() and (r["U_c"] == SENTINEL).all() and (r["choice"] == -9).all(), what
    assert "device pointer" in str(_ragged_call(one, np.float64, "nan", over=dict(dyn_count=host.ctypes.data))["error"])
    with pytest.raises(nm.NmpcError):
        _handle().dwa_step_lists(np.float64, None)
    # R (N + 1) = 840 itself is taken: 40 rows, every count 0 but offset 0's
    big = dict(one, dyn=np.zeros((1, 40, N + 1, 2)) + one["state"][:, None, None, :2] + 3.0, count=np.array([[40] + [0] * N], dtype=np.int32))
    r = _ragged_call(big, np.float32, "own")
    assert r["error"] is None and r["choice"][0] >= -1 and (r["counts"][0] > 0).all()


# ---- 5. f2's counts -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_f2_reports_its_per_offset_counts(golden_dir, dt):
    import torch
    import dyobav_mpcnwta_warehouse_amd as nm
    cases = json.load(open(os.path.join(golden_dir, "hypotheses_cases.json")))
    tdt = torch.float32 if dt == np.float32 else torch.float64
    seen = set()
    for ndyn in (15, 3):
        cfg = nm.default_config_struct()
        cfg.N_hor, cfg.Ndynobs = N, ndyn
        with nm.Handle(cfg) as h:
            for c in cases:
                hyp, cur = torch.from_numpy(np.array(c["hypos"], dtype=dt)[None]).cuda(), torch.from_numpy(np.array(c["cur"], dtype=dt)[None]).cuda()
                if cur.shape[1] > ndyn:
                    continue
                outs = []
                for with_counts in (False, True):
                    dyn = torch.full((1, ndyn, N + 1, 6), float("nan"), dtype=tdt, device="cuda")
                    nobs = torch.full((1,), -9, dtype=torch.int32, device="cuda")
                    cnt = torch.full((1, N + 1), -9, dtype=torch.int32, device="cuda")
                    h.hypotheses_to_ellipses(dt, hyp, cur, dyn, nobs, counts=cnt if with_counts else None)
                    torch.cuda.synchronize()
                    outs.append((dyn.cpu().numpy(), nobs.cpu().numpy(), cnt.cpu().numpy()))
                (dyn0, nobs0, cnt0), (dyn1, nobs1, cnt1) = outs
                assert _same_bits(dyn0, dyn1) and _same_bits(nobs0, nobs1) and (cnt0 == -9).all()
                want = np.array(c["counts"])
                assert want[0] == cur.shape[1] and nobs1[0] == c["n_obs"] == want.max()
                assert np.array_equal(cnt1[0], np.minimum(want, ndyn)), (ndyn, cnt1[0], want)
                assert cnt1[0, 0] == min(cur.shape[1], ndyn)
                seen.update(int(v) for v in want)
    assert len(seen) > 3 and max(seen) > 3                       # unequal counts, and some that Ndynobs = 3 clamps


# ---- 6. the evaluator, call by call ----------------------------------------------------------------------------------------------------
HM, WM, EB, EH, EK, ESTEPS = 37, 41, 6, 2, 3, 8
PX = 0.8                                                         # metres per pixel: the 41 x 37 pixels cover the warehouse's 33 x 30 m


def _prescribed_network():
    """A callable in place of the network: row r of its input is pedestrian (r // N) % 2 at offset r % N + 1 (the evaluator's chunk
    holds whole scenarios). In pixels of 0.8 m (eps = 1.25 pixels), on a 1/8-pixel grid (exact in float32): at every fifth offset the
    six points of a scenario lie 2.5 pixels apart -- noise, no cluster; at the other odd offsets the pedestrians' groups lie 5 pixels
    apart -- two clusters; else all six within 0.5 pixels -- one. The groups start 0.2 .. 0.35 m beside the start of scenarios 0 and 3
    (8.5, 4.3) and move 0.1 m per offset along their way, so the per-step term is at work in their steps."""
    import torch

    def network(x):
        M = x.shape[0]
        assert x.dtype == torch.float32 and x.shape[1:] == (7, HM, WM) and M % (EH * N) == 0
        r = torch.arange(M, device=x.device)
        t, ped = r % N + 1, (r // N) % EH
        k = torch.arange(EK, device=x.device)
        centre = torch.stack([29.625 + 0.0 * t, 24.125 - 0.125 * t], dim=1)[:, None, :]               # [M, 1, 2]
        tight = torch.stack([0.125 * k[None, :] * (1 + ped[:, None]), 0.125 * ped[:, None] * torch.ones_like(k)[None, :]], dim=2)
        two = tight + torch.stack([5.0 * ped, 0.0 * ped], dim=1)[:, None, :]
        lone = torch.stack([-2.5 * (k[None, :] + EK * ped[:, None]), 2.5 * (k[None, :] % 2) + 0.0 * ped[:, None]], dim=2)
        fifth, odd = (t % 5 == 0)[:, None, None], (t % 2 == 1)[:, None, None]
        return (centre + torch.where(fifth, lone, torch.where(odd, two, tight))).to(torch.float32).reshape(M, EK * 2)
    return network


WANT_COUNT = np.array([EH] + [0 if t % 5 == 0 else 2 if t % 2 else 1 for t in range(1, N + 1)])


def _eval_scenarios(dead=None):
    import dyobav_mpcnwta_warehouse_amd as nm
    sc = nm.scenarios.make_reference_scenarios(EB, n_ped=EH)
    sc.pop("scenario_index")
    if dead is not None:     # scenario `dead` starts in the middle of the largest rectangle: it collides in its first step and leaves
        polys = sc["map_polygons"]
        e1, e3 = polys[:, 1] - polys[:, 0], polys[:, 3] - polys[:, 0]
        sc["robot_starts"] = sc["robot_starts"].copy()
        sc["robot_starts"][dead, :2] = polys[int(np.abs(e1[:, 0] * e3[:, 1] - e1[:, 1] * e3[:, 0]).argmax())].mean(axis=0)
    return sc


def _eval_run(dtype, sc, steps, **kw):
    """-> ((goal, node paths, path lengths), result, record) of one run of the pair on the all-free 37 x 41 map."""
    import dyobav_mpcnwta_warehouse_amd as nm
    from dyobav_mpcnwta_warehouse_amd.evaluate import BatchEvaluator
    from dyobav_mpcnwta_warehouse_amd.snap import WorldTransform
    ev = BatchEvaluator(nm.default_config_struct(), dtype=dtype, tracker="dwa", predictor="mmp", network=_prescribed_network(), mmp_hyp=EK,
                        ref_image=np.full((HM, WM), 255.0, dtype=np.float32), transform=WorldTransform(scale=PX, offsetx_after=-15.0, offsety_after=-15.0),
                        **kw, **sc)
    rec = []
    try:
        assert ev.dwa_cap == 55 and not hasattr(ev, "P") and ev.cfg.Ndynobs == 15
        res = ev.run(max_steps=steps, record=rec)
        host = (ev.goal.cpu().numpy().astype(np.float64), ev.node_path.cpu().numpy().astype(np.float64), ev.node_len.cpu().numpy())
    finally:
        ev.close()
    return host, res, rec


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_evaluator_call_by_call(dtype):
    g = dc.golden()
    tol_c, tol_d = 4 * g["delta_f32"]["cost"], 4 * g["delta_f32"]["dist"]
    sc = _eval_scenarios()
    ev, res, rec = _eval_run(dtype, sc, ESTEPS)
    goal, path, plen = ev
    assert len(rec) == ESTEPS and res.n_obs.shape == (ESTEPS, EB) and res.n_outside.shape == (ESTEPS, EB) and res.solve_ms == []
    assert res.steps.max() == ESTEPS and np.isfinite(res.trajectory).all()
    cfg, polys = dr.config(), np.asarray(sc["map_polygons"], dtype=np.float64)
    n_cand = n_out = n_checked = n_active = 0
    worst = 0.0
    for t, q in enumerate(rec):
        assert q["run"] is None and q["dyn"].shape == (EB, 15, N + 1, 6) and q["dyn"].dtype == dtype and q["dyn_count"].shape == (EB, N + 1)
        for b in np.nonzero(q["alive"])[0]:
            cnt = q["dyn_count"][b]
            assert np.array_equal(cnt, WANT_COUNT), (t, b, cnt)
            assert cnt[1:].max() == min(q["n_obs"][b], 15) == res.n_obs[t, b] and q["n_outside"][b] == 0 == res.n_outside[t, b]
            args = (q["state_c"][b].astype(np.float64), goal[b], q["last_u_c"][b].astype(np.float64), path[b, :plen[b]], polys,
                    q["dyn"][b].astype(np.float64)[..., :2], cnt, cfg)
            assert np.array_equal(q["state_c"][b], q["robot"][b]) and (t > 0 or not q["last_u_c"][b].any())
            if t > 0 and rec[t - 1]["alive"][b]:
                assert np.array_equal(q["last_u_c"][b], rec[t - 1]["U_c"][b, :2])
            ch, mc = int(q["choice"][b]), float(q["min_cost"][b])
            if dtype == np.float64:
                w = dl.run_step(*args)
                n_active += int((w["c_steps"] != 0).any())
                assert tuple(q["counts"][b]) == (w["nv"], w["nw"]), (t, b)
                if w["choice"] < 0:
                    assert ch == -1 and mc == np.inf and not q["U_c"][b].any()
                    continue
                assert abs(mc - w["min_cost"]) <= 1e-9 * (1 + abs(w["min_cost"])), (t, b, mc, w["min_cost"])
                worst = max(worst, abs(mc - w["min_cost"]) / (1 + abs(w["min_cost"])))
                if dc.cost_gap(w["cost"]) > 1e-6:
                    assert ch == w["choice"] and np.array_equal(q["U_c"][b], np.tile(w["u"], N)), (t, b, ch, w["choice"])
            else:
                tw = dl.run_step(*args, dtype=np.float32)
                n_active += int((tw["c_steps"] != 0).any())
                near = dr.near_threshold(tw, tol_d)
                n_cand, n_out = n_cand + len(near), n_out + int(near.sum())
                assert tuple(q["counts"][b]) == (tw["nv"], tw["nw"]), (t, b)
                want = tw["cost"].astype(np.float64)
                if tw["choice"] < 0 and not near.any():
                    assert ch == -1 and mc == np.inf and not q["U_c"][b].any()
                    continue
                assert ch >= 0 and (near[ch] or abs(mc - want[ch]) <= tol_c), (t, b, mc, want[ch])
                if ch != tw["choice"]:
                    assert near[ch] or want[ch] <= float(tw["min_cost"]) + tol_c, (t, b, ch, tw["choice"])
                u = tw["cand"][ch].copy()
                if abs(u[0]) < np.float32(1e-3):
                    u[1] = np.float32(-0.5)
                assert _same_bits(q["U_c"][b], np.tile(u, N)), (t, b)
                if not near[ch]:
                    worst = max(worst, abs(mc - want[ch]))
            n_checked += 1
    assert {0, 1, 2} == set(WANT_COUNT[1:].tolist()) and n_checked >= (EB - 1) * ESTEPS and n_active >= ESTEPS
    assert n_out <= 0.02 * max(n_cand, 1)
    print(f"evaluator, {np.dtype(dtype).name}: {n_checked} steps checked, {n_active} with a per-step cost, worst min_cost error {worst:.3e}")


def test_evaluator_with_compaction_gives_the_running_scenarios_the_same_bytes():
    """The compact buffers of the running scenarios (rows, counts, run list) through the lists step: a scenario that leaves in its first
    step does not change what the others get."""
    dead, steps = 1, 4
    sc = _eval_scenarios(dead=dead)
    (_, res_f, rec_f), (_, res_c, rec_c) = (_eval_run(np.float64, sc, steps, compact=c) for c in (False, True))
    assert res_c.collision[dead] and res_c.steps[dead] < steps and rec_c[-1]["run"] is not None and dead not in rec_c[-1]["run"]
    compared = 0
    for qf, qc in zip(rec_f, rec_c):
        assert np.array_equal(qf["alive"], qc["alive"]) and qf["run"] is None
        rows = np.arange(EB) if qc["run"] is None else qc["run"]
        for a, b in enumerate(rows):
            if qf["alive"][b]:
                assert np.array_equal(qc["dyn_count"][b], WANT_COUNT) and _same_bits(qc["dyn"][b], qf["dyn"][b])
                for k in ("U_c", "min_cost", "choice", "counts", "state_c", "last_u_c"):
                    assert _same_bits(qc[k][a], qf[k][b]), (k, b)
                compared += 1
    assert compared >= (EB - 1) * steps and np.array_equal(res_f.trajectory, res_c.trajectory)


def test_evaluator_still_refuses_the_pair_without_a_network():
    import dyobav_mpcnwta_warehouse_amd as nm
    from dyobav_mpcnwta_warehouse_amd.evaluate import BatchEvaluator
    sc = nm.scenarios.make_reference_scenarios(2, n_ped=EH)
    sc.pop("scenario_index")
    with pytest.raises(ValueError, match="network"):
        BatchEvaluator(nm.default_config_struct(), dtype=np.float64, tracker="dwa", predictor="mmp", **sc)


# ---- 7. the drop-in class --------------------------------------------------------------------------------------------------------------
def test_dropin_interface_takes_lists_of_unequal_length(ragged):
    from dyobav_mpcnwta_warehouse_amd.dwa_interface import DwaInterface
    import test_gpu_dwa as tg
    yaml_fp = os.path.join(dc.GOLDEN, "dwa_test.yaml")
    c = ragged[False][0]
    a = 3
    cnt = np.clip(c["count"][a], 0, R6)
    assert len(set(cnt.tolist())) > 2
    batched = _ragged_call(c, np.float64, "nan")
    itf = DwaInterface(yaml_fp, c["state"][a], static_obstacles=c["polys"])
    try:
        itf.update_global_path([tuple(p) for p in c["path"][a, :c["plen"][a]]])
        itf.past_actions = [c["last"][a].copy()]
        lists = [[tuple(c["dyn"][a, r, t]) for r in range(cnt[t])] for t in range(N + 1)]
        action, pred, cost = itf.run_step("work", lists)
        assert _same_bits(np.asarray(action), batched["U_c"][a, :2]) and cost == batched["min_cost"][a] and pred.shape == (N + 1, 3)
        # a rectangular list stays on mode 2: the bytes of nmpc_dwa_step with dyn_mode 2
        s = next(q for q in dc.golden()["sequences"] if q["dyn_mode"] == 2 and q["vel_resolution"] == 0.1 and q["polys"] == "warehouse")
        r2 = tg.seq_call(s, np.float64)
        itf2 = DwaInterface(yaml_fp, np.array(s["calls"][0]["state"]), static_obstacles=dc.seq_polys(s))
        try:
            itf2.update_global_path([tuple(p) for p in s["path"]])
            if any(s["calls"][0]["last_u"]):
                itf2.past_actions = [np.array(s["calls"][0]["last_u"])]
            for k, call in enumerate(s["calls"]):
                itf2.set_current_state(np.array(call["state"]))
                action, _, cost = itf2.run_step("work", call["dyn"])
                assert _same_bits(np.asarray(action), r2["U_c"][k, :2]) and cost == r2["min_cost"][k] and np.array_equal(action, call["u"]), k
        finally:
            itf2.close()
            for h in tg._handles.values():
                h.close()
            tg._handles.clear()
    finally:
        itf.close()
