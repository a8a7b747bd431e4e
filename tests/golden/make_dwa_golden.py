#!/usr/bin/env python3
"""Generate the fixture of the dynamic-window tracker stage (``nmpc_dwa_step_*``) by RUNNING THE REFERENCE'S OWN
``pkg_dwa_tracker.TrajectoryTracker`` (casadi is absent: ``_numeric_casadi.py`` stands in for its import line, as in
make_golden.py). Runs only where the reference tree is present; what it writes is data.

  dwa_cases.json   "sequences": every entry is one tracker object and the ``run_step`` calls made on it, in order; the
                   previous chosen control carries over between them through the tracker's own ``past_actions``. Between
                   two calls the state moves as main_base.py:320-322 moves it (no-backward clip, the reference's motion
                   model) and the pedestrians walk on.
      label "reference"                      dynamic obstacles None or a 2-D list: the reference alone
      label "reference, Euclidean per-step"  a 3-D list: the reference with ``calc_cost_dynamic_obstacles_steps`` -- which
                                             broadcasts its 1-D point along the wrong axis and raises for three or more
                                             pedestrians -- replaced by the Euclidean form of tests/dwa_reference.py
    per call: state, last_u, the pedestrians as given, (nv, nw) and the candidates from ``np.arange`` on the reference's
    window, every candidate's cost through the reference's ``calc_trajectory_cost`` on the reference's ``pred_trajectory``,
    its three deciding distances, and what ``run_step`` itself returned (control, min_cost).
  "closed_loop": the seed of the eight reference scenarios that tests/dwa_cases.py drives for thirty steps, chosen here so
                 that the best and the second-best cost stay more than 1e-6 apart in every step of every predictor.

Asserted here, on the CPU: the restatement agrees with every recording to 1e-12; no deciding distance within 1e-9 of a
threshold; best and second-best cost more than 1e-6 apart in every call; fewer than 1 % of the candidates within four times
the float32 twin's own distance error of a threshold. Floats are written by json (``float.__repr__``: they round-trip).

Usage:  python tests/golden/make_dwa_golden.py [out_dir]
"""
from __future__ import annotations

import contextlib
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.join(REF, "src"))

import _numeric_casadi as nc  # noqa: E402

nc.install()

import dwa_cases as dc  # noqa: E402
import dwa_reference as dr  # noqa: E402

SEED = 20263
N, TS = 20, 0.2
FINE = (0.05, 0.04)      # the yaml's commented "{Real}" resolutions
COARSE = (0.1, 0.1)


def make_tracker(res):
    from basic_motion_model.motion_model import UnicycleModel
    from configs import CircularRobotSpecification, DwaConfiguration
    from pkg_dwa_tracker.trajectory_tracker import TrajectoryTracker
    yaml_fp = os.path.join(REF, "config", "dwa_test.yaml")
    cfg, rob = DwaConfiguration.from_yaml(yaml_fp), CircularRobotSpecification.from_yaml(yaml_fp)
    want = dr.config()
    for k in dr.DEFAULTS:
        assert getattr(cfg if hasattr(cfg, k) else rob, k) == getattr(want, k), k
    cfg.vel_resolution, cfg.ang_resolution = res
    tr = TrajectoryTracker(cfg, rob, verbose=False)
    tr.load_motion_model(UnicycleModel(rob.ts))
    return tr


def euclid_steps(tr):
    """The replacement of calc_cost_dynamic_obstacles_steps: thresholds as written there, distances Euclidean."""
    def f(trajectory, dynamic_obstacles, thre: float = 0.2):
        d = float(dr.steps_distance(np.asarray(trajectory, dtype=float)[None], np.array(dynamic_obstacles, dtype=float), np.float64)[0])
        if d < thre:
            return np.inf
        if d > 0.5:
            return 0.0
        return 1.0 / d * tr.config.q_dyn_obstacle
    return f


def record_sequence(name, res, polys, path, state, last_u0, peds, vels, dyn_mode, n_calls):
    """``polys``: "warehouse", or [M,4,2]; ``peds`` / ``vels`` [H,2] (ignored with dyn_mode 0)."""
    from pkg_dwa_tracker import utils_geo
    tr = make_tracker(res)
    label = "reference"
    if dyn_mode == 2:
        tr.calc_cost_dynamic_obstacles_steps = euclid_steps(tr)
        label = "reference, Euclidean per-step"
    P = dc.warehouse_polys() if isinstance(polys, str) else np.asarray(polys, dtype=float).reshape(-1, 4, 2)
    static = [[tuple(map(float, v)) for v in q] for q in P] if P.shape[0] else None
    path = [tuple(map(float, p)) for p in path]
    state = np.array(state, dtype=float)
    tr.load_init_states(state, np.array(path[-1]))
    if last_u0 is not None:
        tr.past_actions = [np.array(last_u0, dtype=float)]
    peds, vels = np.array(peds, dtype=float).reshape(-1, 2), np.array(vels, dtype=float).reshape(-1, 2)
    calls = []
    for k in range(n_calls):
        if dyn_mode == 0:
            dyn = None
        elif dyn_mode == 1:
            dyn = peds.tolist()
        else:
            dyn = [(peds + vels * (TS * t)).tolist() for t in range(N + 1)]
        last_u = np.array(tr.past_actions[-1] if tr.past_actions else np.zeros(2), dtype=float).copy()
        tr.set_current_state(state.copy())
        with contextlib.redirect_stdout(io.StringIO()):
            best_u, _, min_cost = tr.run_step(path, static, dyn, mode="work")[:3]
        # every candidate again, one by one, through the reference's functions (base_speed is what run_step left)
        dw = tr.calc_dynamic_window(last_u[0], last_u[1])
        V, W = np.arange(dw[0], dw[1], res[0]), np.arange(dw[2], dw[3], res[1])
        cand, cost, d_stc, d_cur, d_steps = [], [], [], [], []
        for v in V:
            for w in W:
                u = np.array([v, w])
                traj = tr.pred_trajectory(state.copy(), u)
                cand.append([float(v), float(w)])
                cost.append(float(tr.calc_trajectory_cost(traj, u, np.array(path), tr.final_goal, static, dyn)))
                d_stc.append(min(float(np.min(utils_geo.lineseg_dists(traj[:, :2], np.array(o), np.array(o[1:] + [o[0]])))) for o in static)
                             if static else float("inf"))
                cur = peds if dyn_mode >= 1 else None
                d_cur.append(float(np.sqrt(((traj[:, None, :2] - cur[None]) ** 2).sum(-1)).min()) if cur is not None else float("inf"))
                d_steps.append(float(dr.steps_distance(traj[None], np.array(dyn[1:]), np.float64)[0]) if dyn_mode == 2 else float("inf"))
        finite = sorted(c for c in cost if np.isfinite(c))
        choice = -1
        for i, c in enumerate(cost):
            if c < (cost[choice] if choice >= 0 else np.inf):
                choice = i
        assert (min_cost == cost[choice]) if choice >= 0 else (min_cost == np.inf and not best_u.any()), (name, k)
        assert len(finite) < 2 or finite[1] - finite[0] > 1e-6, (name, k, "best and second-best cost too close")
        call = dict(state=state.tolist(), last_u=last_u.tolist(), dyn=dyn, nv=int(len(V)), nw=int(len(W)), cand=cand, cost=cost, d_stc=d_stc,
                    d_cur=d_cur, d_steps=d_steps, choice=choice, u=[float(best_u[0]), float(best_u[1])], min_cost=float(min_cost))
        for key, thr in dr.THRESHOLDS.items():
            d = np.array(call[key])
            assert all(np.abs(d[np.isfinite(d)] - t).min(initial=1.0) > 1e-9 for t in thr), (name, k, key)
        calls.append(call)
        action = np.array(best_u, dtype=float)
        if action[0] < 0:
            action = np.zeros(2)
        state = np.asarray(tr.motion_model(state, action, TS), dtype=float)
        peds = peds + vels * TS
    return dict(name=name, label=label, M=int(P.shape[0]), H=int(peds.shape[0]) if dyn_mode else 0, dyn_mode=dyn_mode, vel_resolution=res[0],
                ang_resolution=res[1], polys="warehouse" if isinstance(polys, str) else P.tolist(), path=[list(p) for p in path],
                goal=list(path[-1]), calls=calls)


def box(cx, cy, hx, hy):
    return [[cx + hx, cy + hy], [cx - hx, cy + hy], [cx - hx, cy - hy], [cx + hx, cy - hy]]


def sequences():
    rng = np.random.default_rng(SEED)
    with open(os.path.join(HERE, "warehouse_world.json")) as fh:
        w = json.load(fh)
    out = []

    def ahead(state, n, lo, hi):
        """n pedestrians lo..hi metres ahead of the robot, walking roughly towards it."""
        r, a = rng.uniform(lo, hi, n), state[2] + rng.uniform(-0.5, 0.5, n)
        p = np.stack([state[0] + r * np.cos(a), state[1] + r * np.sin(a)], axis=1)
        v = -np.stack([np.cos(a), np.sin(a)], axis=1) * rng.uniform(0.2, 1.2, (n, 1)) + rng.normal(0, 0.2, (n, 2))
        return p, v
    for k, (mode, res, u0, calls) in enumerate(((2, COARSE, None, 3), (1, COARSE, (0.9, 0.1), 3), (0, COARSE, (1.2, -0.2), 3), (2, FINE, (0.6, 0.0), 2))):
        s = w["scenarios"][str(k % 3)]
        st = np.array(s["robot_start_world"], dtype=float)
        p, v = ahead(st, 4, 1.0, 4.0)
        out.append(record_sequence(f"warehouse scenario {k % 3}, H = 4, mode {mode}", res, "warehouse", s["robot_path_world"], st, u0, p, v, mode, calls))
    st = np.array([0.3, -0.2, 0.4])
    path = [(0.0, 0.0), (4.0, 1.5), (7.0, 1.0)]
    one = [box(2.2, 0.2, 0.5, 0.4)]
    for name, res, polys, H, mode, u0, calls in (("no rectangle, H = 1, mode 2", COARSE, [], 1, 2, (0.5, 0.2), 3), ("one rectangle, H = 2, mode 2", COARSE, one, 2, 2, None, 3),
                                                 ("one rectangle, H = 1, mode 1", COARSE, one, 1, 1, (1.0, -0.3), 3), ("no rectangle, H = 2, mode 1", COARSE, [], 2, 1, (0.2, 0.5), 3),
                                                 ("one rectangle, H = 2, mode 1, fine grid", FINE, one, 2, 1, (0.8, 0.1), 2), ("no rectangle, no pedestrian, fine grid", FINE, [], 0, 0, (1.4, 0.3), 1)):
        p, v = ahead(st, max(H, 1), 0.8, 3.0)
        out.append(record_sequence(name, res, polys, path, st, u0, p[:H], v[:H], mode, calls))
    # near the goal: the base speed is lowered (distance to the goal < 0.8 * 1.5 * 20 * 0.2 = 4.8 m)
    p, v = ahead(np.array([5.2, 1.4, -0.1]), 1, 1.0, 2.0)
    out.append(record_sequence("near the goal, one rectangle, H = 1, mode 2", COARSE, one, path, [5.2, 1.4, -0.1], (0.7, 0.0), p, v, 2, 3))
    # boxed in: the robot sits 0.03 m from an edge, every candidate's first point is closer than 0.05 m
    out.append(record_sequence("boxed in: every candidate +inf", COARSE, [box(1.0, 0.53, 0.6, 0.5)], path, [1.0, 0.0, 0.0], None, [], [], 0, 2))
    # a wall 0.2 m ahead and one 0.2 m behind: only v = 0 survives, the stuck rule turns on the spot
    walls = [box(1.7, 0.0, 0.5, 2.0), box(-0.7, 0.0, 0.5, 2.0)]
    out.append(record_sequence("stuck: only standing still is finite", COARSE, walls, [(0.0, 0.0), (0.5, 3.0), (0.5, 6.0)], [0.5, 0.0, 0.0], None, [], [], 0, 3))
    stuck = out[-1]["calls"]
    assert all(abs(c["u"][0]) < 0.001 and c["u"][1] == -0.5 and c["cand"][c["choice"]][1] != -0.5 for c in stuck[:1]), "the stuck rule was not reached"
    assert any(c["choice"] == -1 for c in out[-2]["calls"]) and max(c["nv"] * c["nw"] for s in out for c in s["calls"]) > 64
    return out


def twin_figures(seqs):
    """Worst |float32 twin - fp64| of the restatement on the float32-rounded inputs (finite costs, finite deciding distances)
    and the share of candidates with a deciding distance within four times the latter of a threshold."""
    d_cost = d_dist = 0.0
    res = []
    for s in seqs:
        for c in s["calls"]:
            r64, r32 = dc.restate(s, c, np.float64, rounded=True), dc.restate(s, c, np.float32, rounded=True)
            assert r64["nv"] == r32["nv"] and r64["nw"] == r32["nw"]
            both = np.isfinite(r64["cost"]) & np.isfinite(r32["cost"])
            d_cost = max(d_cost, float(np.abs(r64["cost"][both] - r32["cost"][both].astype(np.float64)).max(initial=0.0)))
            for k in dr.THRESHOLDS:
                fin = np.isfinite(r64[k])
                d_dist = max(d_dist, float(np.abs(r64[k][fin] - r32[k][fin].astype(np.float64)).max(initial=0.0)))
            res.append(r64)
    near = sum(int(dr.near_threshold(r, 4 * d_dist).sum()) for r in res)
    total = sum(len(r["cost"]) for r in res)
    return d_cost, d_dist, near, total


def choose_closed_loop():
    # (seeds 13 .. 30 were tried when this was first recorded: each has a step in which two candidates cost the same to 1e-6)
    for seed in range(31, 60):
        gaps, outcomes = {}, {}
        for pred in dc.PREDICTORS:
            L = dc.closed_loop(seed, pred)
            gaps[str(pred)] = float(min(r["gap"].min() for r in L["recs"]))
            fin = L["recs"][-1]["post"]
            outcomes[str(pred)] = dict(collision=fin["collision"].tolist(), complete=fin["complete"].tolist(), steps=fin["steps"].tolist())
        if min(gaps.values()) > 1e-6:
            return dict(seed=seed, B=dc.LOOP_B, steps=dc.LOOP_STEPS, min_gap=gaps, outcomes=outcomes)
    raise AssertionError("no seed keeps the best and the second-best cost 1e-6 apart")


def main(out_dir=HERE):
    seqs = sequences()
    worst = 0.0
    for s in seqs:
        for k, c in enumerate(s["calls"]):
            r = dc.restate(s, c)
            assert (r["nv"], r["nw"], r["choice"]) == (c["nv"], c["nw"], c["choice"]), (s["name"], k)
            assert np.array_equal(r["cand"], np.array(c["cand"]).reshape(-1, 2)) and np.array_equal(r["u"], c["u"]), (s["name"], k)
            want = np.array(c["cost"])
            assert np.array_equal(np.isfinite(r["cost"]), np.isfinite(want)), (s["name"], k)
            fin = np.isfinite(want)
            for got, ref in ((r["cost"][fin], want[fin]), (r["d_stc"], c["d_stc"]), (r["d_cur"], c["d_cur"]), (r["d_steps"], c["d_steps"])):
                got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
                f2 = np.isfinite(ref)
                assert np.array_equal(np.isfinite(got), f2)
                worst = max(worst, float(np.abs(got[f2] - ref[f2]).max(initial=0.0)))
    assert worst <= 1e-12, worst
    d_cost, d_dist, near, total = twin_figures(seqs)
    assert near < 0.01 * total, (near, total)
    path = os.path.join(out_dir, "dwa_cases.json")
    with open(path, "w") as f:
        json.dump({"source": "pkg_dwa_tracker.TrajectoryTracker.run_step / calc_trajectory_cost, float64", "seed": SEED,
                   "delta_f32": {"cost": d_cost, "dist": d_dist, "near_threshold": near, "candidates": total},
                   "closed_loop": choose_closed_loop(), "sequences": seqs}, f)
    n = sum(len(s["calls"]) for s in seqs)
    print(f"{len(seqs)} sequences, {n} calls, {total} candidates, restatement worst {worst:.2e}, delta_f32 cost {d_cost:.3e} dist {d_dist:.3e}, "
          f"{near} near a threshold, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(*sys.argv[1:2])
