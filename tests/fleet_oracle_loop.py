"""The closed loop of ``BatchEvaluator(fleet=R)`` driven on the CPU: tests/step_reference.py around the fp64 oracle's solver, with
tests/fleet_reference.py between them -- no device, none of the package's kernels. It is what the geometry of the behavioural
test (tests/test_gpu_fleet_evaluate.py, case b) was chosen with: the oracle alone shows what the fleet terms buy.

One time step, for the robots still running (the evaluator's order):
  step_reference.pre -> fleet_reference.exchange (coupled arm only) -> oracle.assemble -> oracle.solve (multipliers carried,
  no warm start) -> step_reference.post -> fleet_reference.post.
"""
import os

import numpy as np

import fleet_reference as fr
import step_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HUMAN_SIZE, HUMAN_VMAX = 0.2, 1.5
TUNING = (0.0, 10.0, 0.0, 0.0, 0.0, 0.0, 0.0, 100.0, 10.0, 20.0)      # the evaluator's default weights ('work' mode)
LIP_STEP = 1e-4     # Lipschitz-estimator step on both sides (tests/test_gpu_evaluate.py)


def crossing_scenario():
    """G = 2 groups of R = 2 robots on crossing straight paths: member 0 drives 8 m along +x, member 1 crosses its line in the
    middle, 4 m from there, at ``angle`` and starts ``late`` metres further back -- each robot alone tracks its line at the base
    speed, so uncoupled they pass closer than vehicle_width. Group 0: 2.5 rad (nearly head-on), 0.25 m late; group 1, 20 m
    further along x: 60 degrees, 0.2 m late. Chosen by scanning angle and lateness with ``run`` below: the fleet terms act only
    inside vehicle_width and against a path weight of 100, so what they buy is small and depends on the discrete timing of the
    encounter; these two are the middles of ranges of lateness (0.21 .. 0.30 m and 0.19 .. 0.21 m) over which the oracle's gap
    keeps its size. One pedestrian per robot, parked 100 m away on its only way-point; one shelf far from everything.
    Returns the keyword arguments of ``BatchEvaluator``."""
    starts, paths = [], []
    for x0, angle, late in ((0.0, 2.5, 0.25), (20.0, np.pi / 3, 0.2)):
        d = np.array([np.cos(angle), np.sin(angle)])
        cross = np.array([x0 + 4.0, 0.0])
        sb, gb = cross - (4.0 + late) * d, cross + 4.0 * d
        starts += [[x0, 0.0, 0.0], [sb[0], sb[1], angle]]
        paths += [[(x0 + 8.0, 0.0)], [(float(gb[0]), float(gb[1]))]]
    starts = np.array(starts, dtype=np.float64)
    hstart = np.full((4, 1, 2), 100.0)
    hpath = np.full((4, 1, 1, 2), 100.0)
    box = np.array([[[61.0, 61.0], [60.0, 61.0], [60.0, 60.0], [61.0, 60.0]]])
    return dict(robot_starts=starts, robot_paths=paths, human_starts=hstart, human_paths=hpath, map_polygons=box)


def run(sc, R, coupling, max_steps, N=20, Nother=10, Nstc=10, Ndyn=15, ts=0.2, width=0.5, lin_vel_max=1.5, record=None):
    """-> dict(clearance_fleet, collision, collision_fleet, complete, steps, trajectory [B, T + 1, 3])."""
    import oracle
    from oracle.assemble import assemble
    from dyobav_mpcnwta_warehouse_amd.trajectory_tracker import TrajectoryTracker
    pr = oracle.Problem(N, Nother, Nstc, Ndyn, ts=ts, vehicle_width=width, lin_vel_max=lin_vel_max)
    opt = oracle.Options(lip_delta=LIP_STEP, lip_eps=LIP_STEP, hoist_trig=1)
    base_speed = lin_vel_max * 0.8
    starts = np.asarray(sc["robot_starts"], dtype=np.float64)
    B, H, W = starts.shape[0], sc["human_starts"].shape[1], sc["human_paths"].shape[2]
    trajs = [np.array(TrajectoryTracker.get_ref_traj(ts, list(p), tuple(s), base_speed)) for p, s in zip(sc["robot_paths"], starts)]
    Lmax = max(len(t) for t in trajs)
    z = lambda *shape, fill=0.0, dt=np.float64: np.full(shape, fill, dtype=dt)
    s = dict(robot=starts.copy(), last_u=z(B, 2), humans=np.array(sc["human_starts"], dtype=np.float64),
             hist=np.repeat(np.asarray(sc["human_starts"], dtype=np.float64)[:, :, None, :], 5, axis=2), hcount=z(B, H, fill=1, dt=np.int64),
             hidx=z(B, H, dt=np.int64), hpath=np.array(sc["human_paths"], dtype=np.float64),
             ref_traj=np.stack([np.concatenate([t, np.repeat(t[-1:], Lmax - len(t), axis=0)]) for t in trajs]),
             ref_len=np.array([len(t) for t in trajs], dtype=np.int64), idx_ref=z(B, dt=np.int64),
             goal=np.array([p[-1] for p in sc["robot_paths"]], dtype=np.float64), polys=np.array(sc["map_polygons"], dtype=np.float64),
             alive=z(B, fill=1, dt=np.uint8), collision=z(B, dt=np.uint8), complete=z(B, dt=np.uint8), steps=z(B, dt=np.int64),
             clr_dyn=z(B, fill=np.inf), clr_stc=z(B, fill=np.inf), dev_sum=z(B), dev_max=z(B), n_traj=z(B, fill=1.0),
             traj=z(B, max_steps + 1, 3), acts=z(B, max_steps, 2, fill=np.nan), U=z(B, 2 * N), y=z(B, 2 * N))
    s["traj"][:, 0] = starts
    fl = dict(clr_fleet=z(B, fill=np.inf), collision_fleet=z(B, dt=np.uint8))
    stcw = dynw = np.full(N, 10.0)
    n_run = 0
    for kt in range(max_steps):
        rows = np.nonzero(s["alive"])[0]
        if len(rows) == 0:
            break
        n_run = kt + 1
        pre, _ = sr.pre(s, N, ts, base_speed, lin_vel_max, HUMAN_SIZE, run=rows)
        s["idx_ref"] = pre["idx_ref"]
        other = None
        if coupling:
            other, _, _ = fr.exchange(s["robot"], s["U"] if kt > 0 else None, s["alive"], R, N, Nother, ts, run=rows)
        U_c, y_c, P = np.empty((len(rows), 2 * N)), np.empty((len(rows), 2 * N)), []
        for a, b in enumerate(rows):
            p = assemble(pre["last_u_c"][a], pre["state_c"][a], pre["refs_c"][a], pre["speed_c"][a], TUNING, None if other is None else other[a],
                         s["polys"], pre["dyn_c"][a], stcw, dynw, N, Nother, Nstc, Ndyn)
            U_c[a], y_c[a], _ = oracle.solve(pr, opt, p, u0=None, y0=s["y"][b] if kt > 0 else None)
            P.append(p)
        if record is not None:
            record.append(dict(rows=rows, robot=s["robot"].copy(), P=np.array(P), U=U_c.copy()))
        out, _ = sr.post(s, U_c, y_c, ts, HUMAN_SIZE, HUMAN_VMAX, kt, run=rows)
        s.update(out)
        new, _ = fr.post(s["robot"], R, width, fl["clr_fleet"], s["collision"], s["complete"], s["alive"], fl["collision_fleet"], run=rows)
        fl["clr_fleet"], fl["collision_fleet"] = new["clr_fleet"], new["collision_fleet"]
        s["collision"], s["complete"], s["alive"] = new["collision"], new["complete"], new["alive"]
    return dict(clearance_fleet=fl["clr_fleet"], collision=s["collision"].astype(bool) | s["alive"].astype(bool), collision_fleet=fl["collision_fleet"].astype(bool),
                complete=s["complete"].astype(bool), steps=s["steps"], trajectory=s["traj"][:, :n_run + 1])


if __name__ == "__main__":
    import sys
    sys.path.insert(0, ROOT)
    sc = crossing_scenario()
    for coupling in (False, True):
        r = run(sc, 2, coupling, 40)
        print("coupled  " if coupling else "uncoupled", "clearance_fleet", np.array2string(r["clearance_fleet"], precision=6),
              "collision_fleet", r["collision_fleet"].astype(int), "complete", r["complete"].astype(int), "steps", r["steps"])
