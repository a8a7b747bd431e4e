"""``BatchEvaluator(fleet=R)``: several robots in one world (csrc/nmpc_fleet.h around the unchanged solve).

  a. ``fleet=1`` against ``fleet=None``: B = 4, 6 steps, the dimensions and robot of config/mpc_fast.yaml -- ``P``, ``U``,
     trajectories and flags are ``array_equal``: a group of one launches an exchange that writes zeros, the default of the block.
  b. behaviour: ``fleet=2``, G = 2, pedestrians parked 100 m away, stagger 0, at most 40 steps, on
     ``fleet_oracle_loop.crossing_scenario()``: two robots on crossing straight paths that pass closer than vehicle_width when each
     ignores the other. The recorded ``P`` of a middle step holds the peer's state in slot 1 of c_0, and ``clearance_fleet`` of
     the coupled run is STRICTLY LARGER than that of the ``fleet_coupling=False`` run -- no margin beyond that is asserted, and
     "no collision" is not: the fleet terms act only inside vehicle_width, what they buy is measured.
     The geometry was chosen with the CPU oracle alone driving the same loop in numpy (tests/fleet_oracle_loop.py). Its
     clearances, fp64 (``test_the_oracle_alone_shows_the_gap`` recomputes them without a GPU):
         group 0 (2.5 rad, 0.25 m late):   uncoupled 0.148726   coupled 0.474936   gap +0.326
         group 1 (60 deg, 0.20 m late):    uncoupled 0.333743   coupled 0.431585   gap +0.098
     and the device's (MI355X, fp64, this test's run; printed by it):
         group 0:   uncoupled 0.148757   coupled 0.476357   gap +0.328
         group 1:   uncoupled 0.332750   coupled 0.423175   gap +0.090
     (the solver's kernels and the oracle agree to rounding per solve; twenty closed-loop steps amplify that to the 1e-3 .. 1e-2 seen).
     In all four arms the pair ends in a robot-robot collision (distance <= 0.5 m): coupled, the robots meet later and further
     apart, they do not avoid each other: since a robot stops where it collides, ``clearance_fleet`` here is the first distance at
     or below 0.5 m, so "strictly larger" measures the timing and geometry of the encounter under the fleet terms, not avoidance.
  c. the refusals, one assert each (no GPU work: they come before the handle is made).
  d. ``make_fleet_scenarios`` through the MPC tracker with each of the three predictors; compaction on.
"""
import numpy as np
import pytest

import fleet_oracle_loop as fo
import fleet_reference as fr

ORACLE_CLEARANCE = {False: (0.148726, 0.333743), True: (0.474936, 0.431585)}     # [coupling] -> (group 0, group 1)


def _fast_config():
    import os
    import dyobav_mpcnwta_warehouse_amd as nm
    from dyobav_mpcnwta_warehouse_amd.configs import CircularRobotSpecification, MpcConfiguration
    from dyobav_mpcnwta_warehouse_amd.solver import make_config
    yaml = os.path.join(fo.ROOT, "config", "mpc_fast.yaml")
    # (time_cap none: iteration caps only, as the oracle; the Lipschitz step of tests/test_gpu_evaluate.py on both sides)
    cfg = make_config(MpcConfiguration.from_yaml(yaml), CircularRobotSpecification.from_yaml(yaml), time_cap="none")
    cfg.lip_delta_f64 = cfg.lip_eps_f64 = fo.LIP_STEP
    assert (cfg.N_hor, cfg.Nother, cfg.vehicle_width) == (20, 10, 0.5) and isinstance(cfg, nm.NmpcConfigStruct)
    return cfg


def _run(sc, steps, **kw):
    from dyobav_mpcnwta_warehouse_amd.evaluate import BatchEvaluator
    ev = BatchEvaluator(_fast_config(), dtype=np.float64, **kw, **sc)
    rec = []
    try:
        res = ev.run(max_steps=steps, record=rec)
    finally:
        ev.close()
    return res, rec


@pytest.mark.gpu
def test_a_group_of_one_is_the_present_evaluator_bit_for_bit():
    import dyobav_mpcnwta_warehouse_amd as nm
    sc = nm.scenarios.make_reference_scenarios(4)
    sc.pop("scenario_index")
    for compact in (False, True):
        a, ra = _run(sc, 6, human_stagger=0.5, seed=3, compact=compact)
        b, rb = _run(sc, 6, human_stagger=0.5, seed=3, compact=compact, fleet=1)
        assert len(ra) == len(rb) == 6
        for x, y in zip(ra, rb):
            for k in ("P", "U", "robot", "humans", "alive", "y_in"):
                assert np.array_equal(x[k], y[k]), (compact, k)
        for k in ("collision", "complete", "steps", "trajectory", "actions", "clearance", "clearance_dyn", "deviation"):
            assert np.array_equal(getattr(a, k), getattr(b, k), equal_nan=True), (compact, k)
        assert a.clearance_fleet is None and a.collision_fleet is None
        assert np.isinf(b.clearance_fleet).all() and not b.collision_fleet.any()


def test_the_oracle_alone_shows_the_gap():
    """The CPU side of case b: the oracle-driven numpy loop on the same scenario gives the clearances of the module text."""
    sc = fo.crossing_scenario()
    got = {c: fo.run(sc, 2, c, 40)["clearance_fleet"] for c in (False, True)}
    print("oracle: uncoupled", got[False], "coupled", got[True])
    for c in (False, True):
        assert np.array_equal(got[c][0::2], got[c][1::2])                 # a distance belongs to both robots of a pair
        assert np.abs(got[c][0::2] - ORACLE_CLEARANCE[c]).max() < 1e-4, (c, got[c])
    assert (got[True] > got[False]).all()


@pytest.mark.gpu
def test_coupled_robots_keep_more_clearance_than_uncoupled_ones():
    sc = fo.crossing_scenario()
    cpl, rec = _run(sc, 40, human_stagger=0.0, fleet=2)
    unc, rec_u = _run(sc, 40, human_stagger=0.0, fleet=2, fleet_coupling=False)
    print("device: uncoupled", unc.clearance_fleet, "coupled", cpl.clearance_fleet)
    print("        robot-robot collisions uncoupled", unc.collision_fleet.astype(int), "coupled", cpl.collision_fleet.astype(int))
    # a middle step: slot 1 of c_0 holds the peer's current state, slot 0 and slots 2.. are zero; c holds its previous solution rolled
    # out from that state
    from dyobav_mpcnwta_warehouse_amd.scenarios import ParamLayout
    L = ParamLayout(20, 10, 10, 15)
    kt = 8
    r = rec[kt]
    assert r["alive"].all()
    for b in range(4):
        peer = b ^ 1
        block = r["P"][b, L.c0:L.c0 + fr.block_len(20, 10)]
        assert np.array_equal(block[3:6], r["robot"][peer]), b
        assert not block[0:3].any() and not block[6:30].any()
        want, peers, _ = fr.exchange(r["robot"], rec[kt - 1]["U"], r["alive"], 2, 20, 10, 0.2, run=[b])
        assert peers[0] == [peer] and np.abs(block - want[0]).max() <= 1e-12 * 25
        assert not rec_u[kt]["P"][b, L.c0:L.c0 + fr.block_len(20, 10)].any()          # the uncoupled arm: the blocks stay zeros
    # the first step has no previous solution: the peer at rest
    block = rec[0]["P"][0, L.c0:L.c0 + fr.block_len(20, 10)]
    assert np.array_equal(block[fr.c_index(1, 0, 20, 10):fr.c_index(2, 0, 20, 10)], np.tile(rec[0]["robot"][1], 20))
    assert np.isfinite(cpl.clearance_fleet).all() and np.isfinite(unc.clearance_fleet).all()
    assert (cpl.clearance_fleet > unc.clearance_fleet).all(), (cpl.clearance_fleet, unc.clearance_fleet)
    # collision now also counts robot-robot hits, and the flag tells them apart
    for res in (cpl, unc):
        assert (res.collision | ~res.collision_fleet).all() and not (res.complete & res.collision_fleet).any()
        assert np.array_equal(res.collision_fleet, res.clearance_fleet <= 0.5)


def test_refusals():
    import dyobav_mpcnwta_warehouse_amd as nm
    from dyobav_mpcnwta_warehouse_amd.evaluate import BatchEvaluator
    sc = fo.crossing_scenario()
    cfg = nm.default_config_struct()
    with pytest.raises(ValueError, match="fused = True"):
        BatchEvaluator(cfg, fleet=2, fused=False, **sc)
    with pytest.raises(ValueError, match="tracker = 'mpc'"):
        BatchEvaluator(cfg, fleet=2, tracker="dwa", **sc)
    with pytest.raises(ValueError, match="whole number of groups"):
        BatchEvaluator(cfg, fleet=3, **sc)
    with pytest.raises(ValueError, match="1 .. 64"):
        BatchEvaluator(cfg, fleet=0, **sc)
    with pytest.raises(ValueError, match="1 .. 64"):
        BatchEvaluator(cfg, fleet=65, **sc)


def test_fleet_scenarios_are_deterministic_separated_and_share_pedestrians():
    import dyobav_mpcnwta_warehouse_amd as nm
    G, R = 5, 6
    a, b = nm.scenarios.make_fleet_scenarios(G, R, seed=4), nm.scenarios.make_fleet_scenarios(G, R, seed=4)
    base = nm.scenarios.make_reference_scenarios(G, seed=4)
    assert all(np.array_equal(a[k], b[k]) for k in ("robot_starts", "human_starts", "human_paths")) and a["robot_paths"] == b["robot_paths"]
    assert a["robot_starts"].shape == (G * R, 3) and len(a["robot_paths"]) == G * R and a["human_starts"].shape[0] == G * R
    for g in range(G):
        assert np.array_equal(a["robot_starts"][g * R], base["robot_starts"][g]) and a["robot_paths"][g * R] == base["robot_paths"][g]
        xy = a["robot_starts"][g * R:(g + 1) * R, :2]
        d = np.linalg.norm(xy[:, None] - xy[None], axis=-1) + np.eye(R) * 1e9
        assert d.min() > 0.5                                        # farther apart than vehicle_width
        for i in range(R):
            assert np.array_equal(a["human_starts"][g * R + i], base["human_starts"][g])
            assert np.array_equal(a["human_paths"][g * R + i], base["human_paths"][g])
    assert not np.array_equal(nm.scenarios.make_fleet_scenarios(G, R, seed=5)["robot_starts"], a["robot_starts"])


@pytest.mark.gpu
@pytest.mark.parametrize("predictor", ["cvmp", "kfmp", "mmp"])
def test_fleet_scenarios_run_with_every_predictor(predictor):
    import torch
    import dyobav_mpcnwta_warehouse_amd as nm
    from dyobav_mpcnwta_warehouse_amd.evaluate import BatchEvaluator
    from dyobav_mpcnwta_warehouse_amd.snap import WorldTransform
    G, R, steps = 3, 4, 5
    sc = nm.scenarios.make_fleet_scenarios(G, R, seed=2, n_ped=2)
    sc.pop("scenario_index")
    sc.pop("group")
    kw = {}
    if predictor == "mmp":      # a callable in place of the network: three hypotheses around one free pixel of an all-free map
        K = 3
        kw = dict(network=lambda x: torch.tensor([10.0, 10.0, 10.25, 10.0, 10.0, 10.25], device=x.device).repeat(x.shape[0], 1), mmp_hyp=K,
                  ref_image=np.full((37, 41), 255.0, dtype=np.float32), transform=WorldTransform(scale=0.8, offsetx_after=-15.0, offsety_after=-15.0))
    ev = BatchEvaluator(nm.default_config_struct(), dtype=np.float32, predictor=predictor, human_stagger=0.5, seed=1, fleet=R, compact=True, **kw, **sc)
    ev.time_fleet = True
    rec = []
    try:
        res = ev.run(max_steps=steps, record=rec)
    finally:
        ev.close()
    assert len(rec) == steps and res.clearance_fleet.shape == (G * R,) and res.collision_fleet.shape == (G * R,)
    assert np.isfinite(res.clearance_fleet).all() and (res.clearance_fleet > 0).all() and np.isfinite(res.trajectory).all()
    assert len(ev.fleet_ms["exchange"]) == len(ev.fleet_ms["post"]) == steps and all(m > 0 for m in ev.fleet_ms["exchange"] + ev.fleet_ms["post"])
    # the members of a group see the same pedestrians at every step
    for r in rec:
        h = r["humans"].reshape(G, R, -1)
        assert np.array_equal(h, np.repeat(h[:, :1], R, axis=1))
    # the blocks in P are what the numpy statement makes of the recorded states (step 2: previous solutions exist)
    from dyobav_mpcnwta_warehouse_amd.scenarios import ParamLayout
    L = ParamLayout(20, 10, 10, 15)
    r = rec[2]
    rows = np.nonzero(r["alive"])[0]
    want, _, margins = fr.exchange(r["robot"].astype(np.float64), rec[1]["U"].astype(np.float64), r["alive"], R, 20, 10, 0.2, run=rows)
    got = r["P"][rows][:, L.c0:L.c0 + fr.block_len(20, 10)].astype(np.float64)
    # the bar of tests/test_gpu_fleet_kernels.py: four times the float32 error of the numpy statement against its float64 self on
    # the same (float32) inputs, measured here; a robot whose ranking another rounding could change is left out
    twin, tp, _ = fr.exchange(r["robot"], rec[1]["U"], r["alive"], R, 20, 10, 0.2, run=rows, dtype=np.float32)
    _, peers, _ = fr.exchange(r["robot"].astype(np.float64), rec[1]["U"].astype(np.float64), r["alive"], R, 20, 10, 0.2, run=rows)
    sure = (margins > 16 * float(np.finfo(np.float32).eps) * 25) & np.array([a == b for a, b in zip(tp, peers)])
    bound = 4 * float(np.abs(twin[sure].astype(np.float64) - want[sure]).max())
    err = float(np.abs(got[sure] - want[sure]).max())
    print(f"{predictor}: blocks of step 2 in P, worst |error| {err:.3e}, bound {bound:.3e}")
    assert sure.any() and bound > 0 and err <= bound
