"""CPU tests of tests/fleet_reference.py, the numpy statement of the fleet stage (csrc/nmpc_fleet.h): is its rollout the
reference's motion model, and is its block layout the builder's?

  a. rollout == the reference project's ``unicycle_model`` (basic_motion_model/motion_model.py:141-163), step by step, where the
     reference tree and casadi, which that module imports, are present (skipped otherwise; the closed form itself is derived in
     ``fleet_reference.unicycle_step`` and tied to the recording in b);
  b. rollout == the ``pred_states`` recorded in tests/golden/tracker_harness.json. The recording holds the ONE action taken per
     step, not the solution's N controls, so only ``pred_states[0]`` = model(state_out, action) can be replayed from recorded
     controls (the reference rolls the solution unshifted from the state after the step: the first control is applied again).
     For ``pred_states[1:]`` the controls are not in the file; they are recovered from two of the three state equations
     (w from theta, v from the displacement's length), and the third -- the displacement's direction -- is what is checked;
  c. a block written by ``fleet_reference.exchange`` and put into a golden parameter vector changes the fp64 oracle's cost by
     exactly the two fleet sums of mpc_builder.py:85-97, computed in numpy from ``cost_fleet_collision`` (weight 1000 against
     c_0 slots 1.., weight 10 per step against every slot of c, the zero ones at the origin included);
  d. selection: nearest first, ties to the lower index, never itself, capacity Nother - 1, slot 0 zero; epilogue: `<=`, a
     collision beats a completion, robots outside the run list untouched.
"""
import json
import os

import numpy as np
import pytest

import fleet_reference as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
# the reference's ``src`` directory: NMPC_REFERENCE_SRC, or a checkout named ``reference`` next to this repository
REFERENCE_SRC = os.environ.get("NMPC_REFERENCE_SRC") or os.path.join(os.path.dirname(ROOT), "reference", "src")


def _reference_unicycle():
    """The reference's ``unicycle_model``. Skipped only where the reference tree is absent or casadi, which its module imports, is
    not installed; anything else that goes wrong while loading it is an error."""
    path = os.path.join(REFERENCE_SRC, "basic_motion_model", "motion_model.py")
    if not os.path.exists(path):
        pytest.skip("the reference tree is not on this machine")
    import importlib.util
    if importlib.util.find_spec("casadi") is None:
        pytest.skip("casadi, which the reference's motion model imports, is not installed")
    spec = importlib.util.spec_from_file_location("_reference_motion_model", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.unicycle_model


def test_rollout_is_the_reference_motion_model_step_by_step():
    model = _reference_unicycle()
    rng = np.random.default_rng(41)
    worst = 0.0
    for _ in range(50):
        N = int(rng.integers(1, 25))
        ts = float(rng.choice([0.1, 0.2, 0.5]))
        s = np.array([rng.uniform(-20, 20), rng.uniform(-20, 20), rng.uniform(-4, 4)])
        U = np.stack([rng.uniform(-0.5, 1.5, N), rng.uniform(-0.5, 0.5, N)], axis=1).reshape(-1)
        got = fr.rollout(s, U, ts)
        for j in range(N):
            s = model(s, U[2 * j:2 * j + 2], ts, rk4=True)
            worst = max(worst, float(np.abs(got[j] - s).max()))
    print(f"rollout against the reference's unicycle_model: worst |error| {worst:.3e}")
    assert worst <= 1e-12 * 25      # 1e-12 x the coordinate scale


def test_rollout_against_the_recorded_pred_states():
    with open(os.path.join(GOLDEN, "tracker_harness.json")) as fh:
        rec = json.load(fh)
    ts = float(rec["get_ref_traj_case"]["ts"])
    n_first = n_rest = 0
    for st in rec["steps"]:
        pred = np.array(st["pred_states"], dtype=np.float64)
        assert len(st["actions"]) == 1      # the file holds the action taken, not the N controls of the solution
        # pred_states[0]: the solution's FIRST control applied again to the state after the step (unshifted)
        first = fr.rollout(st["state_out"], np.array(st["actions"][0], dtype=np.float64), ts)
        assert np.abs(first[0] - pred[0]).max() <= 1e-12, (first[0], pred[0])
        n_first += 1
        # pred_states[1:]: (v, w) recovered from theta and the displacement's length; the direction is the check
        for j in range(1, len(pred)):
            w = (pred[j, 2] - pred[j - 1, 2]) / ts
            unit = fr.unicycle_step(pred[j - 1], (1.0, w), ts)
            v = np.hypot(*(pred[j, :2] - pred[j - 1, :2])) / np.hypot(*(unit[:2] - pred[j - 1, :2]))
            v = v if np.dot(unit[:2] - pred[j - 1, :2], pred[j, :2] - pred[j - 1, :2]) >= 0 else -v
            got = fr.unicycle_step(pred[j - 1], (v, w), ts)
            assert np.abs(got - pred[j]).max() <= 1e-9, (j, got, pred[j])
            n_rest += 1
    assert n_first >= 4 and n_rest >= 4 * 19


def test_block_layout_is_the_builders(problem_n20):
    import oracle
    from dyobav_mpcnwta_warehouse_amd.scenarios import ParamLayout
    fx, pr = problem_n20
    N, No = pr.N, pr.Nother
    L = ParamLayout(N, No, pr.Nstc, pr.Ndyn)
    rng = np.random.default_rng(5)
    n_checked = 0
    for k in range(6):
        P = np.array(fx["P"][k], dtype=np.float64)
        U = np.array(fx["U"][k], dtype=np.float64)
        own = P[L.s0:L.s0 + 3]
        P[L.c0:L.c0 + fr.block_len(N, No)] = 0.0
        f_zero, _, _ = oracle.eval_problem(pr, U, P)
        # a group around the robot: peers on and near its predicted path, so that both hinges are active
        R = (2, 4, No, No + 3, 3, 5)[k]
        path = fr.rollout(own, U, pr.ts)
        robot = np.empty((R, 3))
        robot[0] = own
        for m in range(1, R):
            robot[m, :2] = path[int(rng.integers(N)), :2] + rng.uniform(-0.4, 0.4, 2)
            robot[m, 2] = rng.uniform(-3, 3)
        Uall = np.stack([rng.uniform(-0.2, 0.6, N), rng.uniform(-0.3, 0.3, N)], axis=-1).reshape(1, -1).repeat(R, axis=0)
        Uall[0] = U
        alive = np.ones(R, dtype=np.uint8)
        alive[R - 1] = 0 if k % 2 else 1
        blocks, peers, _ = fr.exchange(robot, Uall, alive, R, N, No, pr.ts, run=[0])
        assert len(peers[0]) == min(R - 1, No - 1)
        P[L.c0:L.c0 + fr.block_len(N, No)] = blocks[0]
        f_block, _, _ = oracle.eval_problem(pr, U, P)
        zero_sum = fr.fleet_cost(own, U, np.zeros(fr.block_len(N, No)), N, No, pr.ts, pr.vehicle_width)
        want = fr.fleet_cost(own, U, blocks[0], N, No, pr.ts, pr.vehicle_width) - zero_sum
        got = f_block - f_zero
        print(f"case {k}: R = {R}, fleet sums {want:.6f}, oracle's cost difference {got:.6f}")
        if R > 1:
            assert abs(want) > 1.0          # the hinges are active: the check sees the layout
        assert abs(got - want) <= 1e-9 * max(1.0, abs(f_block), abs(f_zero)), (k, got, want)
        n_checked += 1
    assert n_checked == 6


def test_selection_ties_capacity_and_slot_zero():
    # member 2 in the middle of mirror images on integer coordinates: members 0 and 4 tie, as do 1 and 3
    robot = np.array([[-2, 0, 0.1], [0, 1, 0.2], [0, 0, 0.3], [0, -1, 0.4], [2, 0, 0.5]], dtype=np.float64)
    N, No = 3, 3
    for dt in (np.float64, np.float32):
        out, peers, margins = fr.exchange(robot, None, np.ones(5, np.uint8), 5, N, No, 0.2, dtype=dt)
        assert peers[2] == [1, 3] and margins[2] == 0.0         # equal distances: the lower member index first
        assert peers[0] == [2, 1] and peers[4] == [2, 1]         # member 2 at distance 2, then sqrt(5) twice: the lower index
    out, peers, _ = fr.exchange(robot, None, np.ones(5, np.uint8), 5, N, No, 0.2)
    assert out.shape == (5, fr.block_len(N, No))
    for b in range(5):
        assert b not in peers[b] and len(peers[b]) == No - 1
        assert not out[b, 0:3].any()                                             # slot 0 of c_0
        assert not out[b, fr.c_index(0, 0, N, No):fr.c_index(1, 0, N, No)].any()  # slot 0 of c
        for s, m in enumerate(peers[b], start=1):
            assert np.array_equal(out[b, 3 * s:3 * s + 3], robot[m])
            for j in range(N):                                                   # at rest: the current state, N times
                i = fr.c_index(s, j, N, No)
                assert np.array_equal(out[b, i:i + 3], robot[m])
    # capacity 0: all zeros
    out, peers, _ = fr.exchange(robot, None, np.ones(5, np.uint8), 5, N, 1, 0.2)
    assert not out.any() and all(p == [] for p in peers)


def test_epilogue_rules():
    w = 0.5
    # group 0: exactly the width apart (collision, `<=`); group 1: one float above (none); group 2: a parked member is hit
    up = float(np.nextafter(np.float64(w), 1.0))
    # (-w / 2 and -w / 2 + up: the sum has the finer spacing of w / 2, so the difference is `up` exactly)
    robot = np.array([[0, 0, 0], [w, 0, 0], [3, -w / 2, 0], [3, -w / 2 + up, 0], [8, 8, 0], [8.2, 8, 0]], dtype=np.float64)
    assert robot[3, 1] - robot[2, 1] == up
    z = lambda v=0: np.full(6, v, dtype=np.uint8)
    complete = z()
    complete[0] = 1                                       # completion and collision in the same step: the collision wins
    alive = z(1)
    alive[0], alive[5] = 0, 0                             # 0 completed in loop_post just now (still in the run list); 5 is parked
    new, margins = fr.post(robot, 2, w, np.full(6, np.inf), z(), complete, alive, z(), run=[0, 1, 2, 3, 4])
    assert new["collision"].tolist() == [1, 1, 0, 0, 1, 0] and new["collision_fleet"].tolist() == [1, 1, 0, 0, 1, 0]
    assert new["complete"].tolist() == [0] * 6 and new["alive"].tolist() == [0, 0, 1, 1, 0, 0]
    assert new["clr_fleet"][:4].tolist() == [w, w, up, up]
    assert abs(new["clr_fleet"][4] - 0.2) < 1e-15 and np.isinf(new["clr_fleet"][5])     # the parked robot's record is not touched
    assert margins[0] == 0.0 and margins[2] > 0.0
