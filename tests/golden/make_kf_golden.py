#!/usr/bin/env python3
"""Generate the fixture of the Kalman-filter predictor stage (``nmpc_kf_predict_*``) by RUNNING THE REFERENCE'S OWN
``KfmpInterface`` and ``zfilter.KalmanFilter``. Runs only where the reference tree is present; what it writes is data.

  kf_cases.json   "sequences": every entry is one filter object and the calls made on it, in order
      kind "interface": ``KfmpInterface("mpc_default.yaml", Q=eye(4), R=eye(2))`` driven the way
                        ``MainBase.run_kf_prediction`` drives it (main_base.py:210-236): at every time step one
                        ``get_motion_prediction(past_traj)`` call per pedestrian h = 0 .. H-1 on the SAME object, past_traj
                        growing by one position per step while the pedestrian walks. H = 1, 3, 4; 12 steps; in every
                        sequence with H > 1 one pedestrian stops half-way; at the first step every trajectory has one point.
      kind "general":   ``zfilter.KalmanFilter`` with seeded non-diagonal SPD Q and R (eigenvalues of R >= 0.5), perturbed
                        A and C, P0 != I, ``set_init_state`` by the interface's rule and ``inference`` over three
                        trajectories one after the other on the same object.
    per call: the trajectory given, the N_hor predicted positions, the returned (P00, P11) and the whole P afterwards.

Floats are written by json (``float.__repr__``: they round-trip exactly).

Usage:  python tests/golden/make_kf_golden.py [out_dir]
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REF, "src"))

import kf_reference as kr  # noqa: E402

SEED = 20261
STEPS = 12


def walk(rng, steps, stop_after=None):
    """A pedestrian's past_traj after every time step: lists of positions, growing by one per step until it stops."""
    p = rng.uniform(-10, 10, 2)
    v = rng.uniform(-1.5, 1.5, 2) * 0.2
    traj, out = [p.tolist()], []
    for k in range(steps):
        if k > 0 and (stop_after is None or k <= stop_after):
            p = p + v + rng.normal(0, 0.03, 2)
            v = v + rng.normal(0, 0.02, 2)
            traj.append(p.tolist())
        out.append([list(q) for q in traj])
    return out


def spd(rng, n, floor):
    m = rng.normal(size=(n, n))
    w, v = np.linalg.eigh(m @ m.T)
    return (v * (floor + w / w.max())) @ v.T


def main(out_dir=HERE):
    import zfilter
    from interfaces.kfmp_interface import KfmpInterface

    rng = np.random.default_rng(SEED)
    sequences = []
    for H in (1, 3, 4):
        itf = KfmpInterface("mpc_default.yaml", Q=1 * np.eye(4), R=1 * np.eye(2))       # main_base.py:165
        N, ts = int(itf.config.N_hor), float(itf.config.ts)
        A, C, Q, R, P0 = kr.default_matrices(ts)
        assert np.array_equal(itf.state_space[0], A) and np.array_equal(itf.state_space[2], C)
        walks = [walk(rng, STEPS, stop_after=STEPS // 2 if (H > 1 and h == 1) else None) for h in range(H)]
        Pc = P0.copy()
        steps = []
        for k in range(STEPS):
            calls = []
            for h in range(H):
                traj = walks[h][k]
                pos, unc = itf.get_motion_prediction([tuple(q) for q in traj])
                assert len(pos) == N and all(u == unc[0] for u in unc)
                P = np.array(itf.kf.P)
                # the restatement must agree before anything is recorded
                want, Pc = kr.filter_traj(traj, Pc, A, C, Q, R, N)
                assert np.abs(want - np.array(pos)).max() < 1e-12 and np.abs(Pc - P).max() < 1e-12
                Pc = P.copy()
                calls.append(dict(traj=traj, positions=pos, std=list(unc[0]), P=P.tolist()))
            steps.append(calls)
        assert all(len(c["traj"]) == 1 for c in steps[0])
        sequences.append(dict(kind="interface", H=H, N=N, ts=ts, A=A.tolist(), C=C.tolist(), Q=Q.tolist(), R=R.tolist(),
                              P0=P0.tolist(), steps=steps))
    for g in range(3):
        N, ts = 20, 0.2
        A0, C0 = kr.model_cv(ts)
        A = A0 + rng.normal(0, 0.05, (4, 4))
        C = C0 + rng.normal(0, 0.05, (2, 4))
        Q, R, P0 = spd(rng, 4, 0.3), spd(rng, 2, 0.5), spd(rng, 4, 0.2)
        assert np.linalg.eigvalsh(R).min() >= 0.5 and np.abs(Q - np.diag(np.diag(Q))).max() > 0.05
        kf = zfilter.KalmanFilter([A, np.zeros((4, 1)), C, np.zeros((2, 1))], P0=P0.copy(), Q=Q, R=R, pred_offset=N)
        calls = []
        for L in (1, 7, 12):
            traj = walk(rng, L)[-1]
            t = np.array(traj)
            init = np.array([t[0, 0], t[0, 1], t[1, 0] - t[0, 0], t[1, 1] - t[0, 1]] if L > 1 else [t[0, 0], t[0, 1], 0, 0])
            kf.set_init_state(init.reshape(4, 1))                                        # kfmp_interface.py:44-51
            _, P = kf.inference(t)
            pos = kf.Xs[:2, L:].T
            assert pos.shape == (N, 2)
            calls.append(dict(traj=traj, positions=pos.tolist(), std=[float(P[0, 0]), float(P[1, 1])], P=np.array(P).tolist()))
        sequences.append(dict(kind="general", H=3, N=N, ts=ts, A=A.tolist(), C=C.tolist(), Q=Q.tolist(), R=R.tolist(),
                              P0=P0.tolist(), steps=[calls]))
    path = os.path.join(out_dir, "kf_cases.json")
    with open(path, "w") as f:
        json.dump({"source": "KfmpInterface.get_motion_prediction / zfilter.KalmanFilter.inference, float64", "seed": SEED,
                   "sequences": sequences}, f)
    print(f"{len(sequences)} sequences, {sum(len(c) for s in sequences for c in s['steps'])} calls, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(*sys.argv[1:2])
