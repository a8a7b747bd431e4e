"""The fp64 reference of one closed-loop time step (tests/step_reference.py) is a reference and not a third opinion:
it reproduces the recordings of the reference project's own classes (tests/golden/evaluate_cases.json) to the 1e-12
the replays through ``evaluate.py``'s torch expressions use (tests/test_gpu_evaluate_reference.py). Also established
here, on the CPU, for the inputs tests/test_gpu_step_kernels.py uses: how often a decision's margin is too small to be
compared in fp32 / fp64, and the reference's own float32 rounding per output array (the yardstick of the fp32 kernels).
"""
import numpy as np
import pytest

import step_cases as sc
import step_reference as sr

TS, VMAX, HS = 0.2, 1.5, 0.2


@pytest.fixture(scope="module")
def cases():
    c = sc.golden_cases()
    assert c["ts"] == TS and c["human_vmax"] == VMAX
    return c


def test_reference_reproduces_recorded_walks(cases):
    """basic_agent.Human.run_step, state by state with the recorded stagger draws, including the steps after the path's end."""
    walks = cases["human_walks"]
    s = sc.walk_state(cases)
    T = len(walks[0]["moved"])
    U = np.zeros((len(walks), 40))
    for t in range(T):
        st = np.array([[w["stagger_draws"][t]] for w in walks])
        before = {k: s[k].copy() for k in ("humans", "hist", "hcount")}
        out, _ = sr.post(s, U, U, TS, HS, VMAX, t, stagger=st)
        s.update(out)
        want = np.array([w["states"][t + 1] for w in walks])
        np.testing.assert_allclose(s["humans"][:, 0], want, rtol=0, atol=1e-12, err_msg=f"step {t}")
        for b, w in enumerate(walks):
            moved = bool(w["moved"][t])
            assert (s["hcount"][b, 0] - before["hcount"][b, 0] == 1) == moved
            if not moved:     # run_step returned False: nothing is appended to past_traj
                assert np.array_equal(s["humans"][b], before["humans"][b]) and np.array_equal(s["hist"][b], before["hist"][b])
            else:
                assert np.array_equal(s["hist"][b, 0, 4], s["humans"][b, 0]) and np.array_equal(s["hist"][b, 0, :4], before["hist"][b, 0, 1:])
    assert not all(w["moved"][-1] for w in walks) and (s["hidx"].max() == s["hpath"].shape[2])


def test_reference_reproduces_recorded_cv_predictions(cases):
    cv = cases["cv_cases"]
    s = sc.cv_state(cases)
    out, _ = sr.pre(s, 20, TS, 1.2, 1.5, HS)
    rows = out["dyn_c"]
    for b, c in enumerate(cv):
        np.testing.assert_allclose(rows[b, 0, 0, :2], c["traj"][-1], rtol=0, atol=1e-12)
        np.testing.assert_allclose(rows[b, 0, 1:, :2], np.array(c["positions"]), rtol=0, atol=1e-12)
        assert (rows[b, 0, 1:, 2:4] == np.array(c["uncertainty"])).all() and (rows[b, 0, 0, 2:4] == HS).all()
        assert (rows[b, 0, :, 4] == 0).all() and (rows[b, 0, :, 5] == 1).all()
    assert sorted({len(c["traj"]) for c in cv})[0] == 1 and max(len(c["traj"]) for c in cv) > 5


def test_reference_reproduces_recorded_robot_steps(cases):
    s, U, want = sc.robot_step_state(cases)
    assert 0 < sum(r["action"][0] < 0 for r in cases["robot_steps"]) < len(cases["robot_steps"])
    out, _ = sr.post(s, U, U, TS, HS, VMAX, 0)
    np.testing.assert_allclose(out["robot"], want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(out["traj"][:, 1], want, rtol=0, atol=1e-12)
    assert np.array_equal(out["acts"][:, 0], U[:, :2]) and np.array_equal(out["last_u"], U[:, :2])


def test_reference_reproduces_recorded_metrics(cases):
    for m in cases["metric_cases"]:
        s, act = sc.metric_state(m)
        U = np.zeros((2, 40))
        for k, p in enumerate(act):
            s["robot"][0, :2] = p
            out, _ = sr.post(s, U, U, TS, HS, VMAX, k)
            s.update(out)
        assert s["n_traj"][0] == len(act) and s["alive"].all()
        assert s["dev_sum"][0] / s["n_traj"][0] == pytest.approx(m["deviation"][0], rel=1e-12)
        assert s["dev_max"][0] == pytest.approx(m["deviation"][1], rel=1e-12)
        assert s["clr_dyn"][1] == pytest.approx(m["min_dyn_distance"], rel=1e-12)


# ---- the inputs of the GPU comparisons: which decisions can be compared, and the reference's own float32 rounding ----------
PRE_ARRAYS = ("dyn_c", "refs_c", "speed_c", "state_c", "last_u_c", "y_c")
POST_ARRAYS = ("robot", "last_u", "humans", "hist", "clr_dyn", "clr_stc", "dev_sum", "dev_max", "n_traj", "traj", "acts", "U", "y")
POST_EXACT = ("hcount", "hidx", "alive", "collision", "complete", "steps")
TRIG_ARRAYS = ("dyn_c", "robot", "traj")      # go through float32 sin / cos, whose last bit may differ between numpy builds / CPUs


def fuzz_twin_errors(verbose=True):
    """The fuzz set of tests/step_cases.py evaluated by the reference in float32 against itself in fp64 on the same
    (float32-rounded) inputs: {array: worst absolute error}, and the shares of decisions excluded at 16 eps32."""
    eps = float(np.finfo(np.float32).eps)
    worst, total = {}, {}
    for g in range(len(sc.FUZZ_GROUPS)):
        case = sc.round_inputs(sc.fuzz_group(g), np.float32)
        s = case["state"]
        rows = np.arange(sc.FUZZ_B) if case["run"] is None else case["run"]
        (op, mp), (oq, mq) = sc.ref_pre(case), sc.ref_post(case)
        thr = 16 * eps * sc.coord_max(s)
        low_p, low_q = sc.low_margins(mp, thr), sc.low_margins(mq, thr)
        sc.add_shares(total, sc.shares(low_p, low_q, rows, s))
        # the twin takes the fp64 decisions where the margin is low (there its own may legitimately differ) ...
        f = sc.forced(sc.decisions(case, op, oq), low_p, low_q)
        tp, _ = sc.ref_pre(case, np.float32, force=f)
        tq, _ = sc.ref_post(case, np.float32, force=f)
        # ... and everywhere else arrives at them by itself
        assert np.array_equal(tp["idx_ref"], op["idx_ref"]), g
        for k in POST_EXACT:
            assert np.array_equal(tq[k], oq[k]), (g, k)
        for k in PRE_ARRAYS + POST_ARRAYS:
            a, b = (tp, op) if k in PRE_ARRAYS else (tq, oq)
            if a[k] is None:
                continue
            fin = np.isfinite(b[k])
            assert np.array_equal(fin, np.isfinite(a[k])) and np.array_equal(a[k][~fin], b[k][~fin].astype(np.float32)), (g, k)
            err = float(np.abs(a[k].astype(np.float64)[fin] - b[k][fin]).max()) if fin.any() else 0.0
            worst[k] = max(worst.get(k, 0.0), err)
    if verbose:
        print("float32 twin of the reference, worst absolute error per array over the fuzz set:")
        print("    " + ", ".join(f'"{k}": {v:.3e}' for k, v in worst.items()))
    return worst, total


def test_fuzz_inputs_keep_the_decisions_comparable_and_twin_errors_match_the_committed_bounds():
    """The fuzz set (seed step_cases.FUZZ_SEED, 12 groups x 210 scenarios): at most 1 % of the scenarios and of the
    instances of any decision kind have a margin under 16 eps x the largest coordinate, in either type; and the float32
    twin errors are the constants committed in tests/test_gpu_step_kernels.py (to the printed digits; the three arrays
    behind a float32 sin / cos, whose last bit is the numpy build's, to a quarter). Figures: end of this file."""
    import test_gpu_step_kernels as g
    worst, total = fuzz_twin_errors()
    sc.check_shares(total, "fuzz, 16 eps32")
    assert set(worst) == set(g.TWIN_ERROR_F32)
    for k, v in worst.items():
        c = g.TWIN_ERROR_F32[k]
        if k in TRIG_ARRAYS:
            assert abs(v - c) <= 0.25 * c, (k, v, c)
        else:
            assert float(f"{v:.3e}") == c, (k, v, c)
        assert g.BOUND_F32[k] == 4 * c
    # fp64: the same inputs unrounded, 16 eps64
    total = {}
    for gi in range(len(sc.FUZZ_GROUPS)):
        case = sc.fuzz_group(gi)
        rows = np.arange(sc.FUZZ_B) if case["run"] is None else case["run"]
        (_, mp), (_, mq) = sc.ref_pre(case), sc.ref_post(case)
        thr = 16 * float(np.finfo(np.float64).eps) * sc.coord_max(case["state"])
        sc.add_shares(total, sc.shares(sc.low_margins(mp, thr), sc.low_margins(mq, thr), rows, case["state"]))
    sc.check_shares(total, "fuzz, 16 eps64")
    assert total["scenario"][1] >= 2000


def test_fuzz_inputs_populate_every_branch():
    counts = sc.fuzz_population(verbose=True)
    for k, v in counts.items():
        assert v > 0, k


@pytest.mark.parametrize("family", ["reference", "corridor"])
def test_sixty_step_inputs_end_every_way_and_keep_the_decisions_comparable(family):
    s0, seq, recs = sc.sixty_reference(family)
    fin = recs[-1]["post"]
    print(f"{family}: {len(recs)} steps, collisions {int(fin['collision'].sum())}, completions {int(fin['complete'].sum())}, "
          f"survivors {int(fin['alive'].sum())}")
    assert fin["collision"].sum() > 10 and fin["complete"].sum() > 10 and fin["alive"].sum() > 10
    assert any(r["run"] is not None for r in recs) and recs[0]["run"] is None
    B = s0["robot"].shape[0]
    out64, tot32 = np.zeros(B, bool), {}
    prev = s0
    for r in recs:
        rows = np.arange(B) if r["run"] is None else r["run"]
        one = np.ones(B)
        for m in (sc.low_margins(r["pre_mar"], 1e-9 * one), sc.low_margins(r["post_mar"], 1e-9 * one)):
            for v in m.values():
                out64 |= v if v.ndim == 1 else v.any(axis=1)
        thr = 16 * float(np.finfo(np.float32).eps) * sc.coord_max(prev)
        sc.add_shares(tot32, sc.shares(sc.low_margins(r["pre_mar"], thr), sc.low_margins(r["post_mar"], thr), rows, prev))
        prev = r["post"]
    print(f"{family}: scenarios with a margin under 1e-9 somewhere along the run: {int(out64.sum())} of {B}")
    assert out64.sum() <= 0.01 * B
    sc.check_shares(tot32, f"sixty steps ({family}), 16 eps32 along the fp64 run")


# Output of `pytest -s -m "not gpu" tests/test_step_reference_cpu.py` (numpy 2.2, x86-64), the figures the GPU module relies on:
#
# float32 twin of the reference, worst absolute error per array over the fuzz set:
#     dyn_c 3.711e-06, refs_c 0, speed_c 1.159e-07, state_c 0, last_u_c 0, robot 9.402e-07, last_u 0, humans 9.813e-07,
#     hist 9.813e-07, clr_dyn 1.993e-06, clr_stc 1.720e-06, dev_sum 7.657e-06, dev_max 8.850e-07, n_traj 0, traj 9.402e-07,
#     acts 0, U 0, y 0, y_c 0
# fuzz, 16 eps32: excluded argmin 0/2100, col_dyn 0/1899, col_stc 1/1899 = 0.053 %, done_x 0/1899, done_y 0/1899, near 0/2100,
#     wp 3/31042 = 0.010 %, scenario 4/2100 = 0.190 %
# fuzz, 16 eps64: nothing excluded (2100 scenarios, 31042 way-point decisions)
# sixty steps (reference): collisions 150, completions 46, survivors 60; margins under 1e-9 along the fp64 run: 0 of 256;
#     at 16 eps32 along the fp64 run: argmin 13/10763 = 0.121 %, col_stc 5/10763 = 0.046 %, others 0, scenario 18/10763 = 0.167 %
# sixty steps (corridor): collisions 108, completions 90, survivors 58; margins under 1e-9: 0 of 256;
#     at 16 eps32: argmin 5/10070 = 0.050 %, others 0, scenario 5/10070 = 0.050 %
# (the arg-min share is what a robot within 1 m of a path with points 0.24 m apart gives: ~0.1 % at 16 eps32 x 30 m)
