"""Warm starts through every solve plan. From its second time step on, the closed loop (evaluate.py, TrajectoryTracker)
sends the previous solution shifted by one step as u0, the previous multipliers as y (y_is_input = 1) and the previous
penalty as c0. The plans of run_solve -- dispatch order from one evaluation or from a pilot launch, the resumable solve,
the tail hand-off with its deep parks -- restore those inputs by paths of their own, so each plan is checked against one
plain launch (index order, no hand-off) of the same warm-started batch: every result array identical, bit for bit. The
batch sizes follow the device's SIMD count and the plan thresholds of csrc/nmpc_plan.h; nmpc_last_launch_info shows that the
intended plan ran.

Edge warm starts (multipliers outside the box Y = [-1e12, 1e12], zero multipliers passed as input, penalties below 1,
initial guesses outside the control box) are checked against the fp64 oracle on the iterate path."""
import numpy as np
import pytest

import dyobav_mpcnwta_warehouse_amd as nm
import oracle
from conftest import config_for
from plan_cases import HINT, LAY, PLAIN, PLAN_IDS, check_plan, n_simd, plan_batch, plan_cfg, plans, same  # noqa: F401  (other test modules take them from here)

pytestmark = pytest.mark.gpu


def warm_start(prev):
    """What the closed loop sends at the next time step: U shifted by one step (last step repeated), y, the penalty."""
    U = prev["U"]
    u0 = np.concatenate([U[:, 2:], U[:, -2:]], axis=1)
    return np.nan_to_num(u0), np.nan_to_num(prev["y"]), np.nan_to_num(prev["info"][:, 3], nan=10.0)


@pytest.mark.parametrize("idx", range(5), ids=PLAN_IDS)
def test_warm_start_through_the_plan_matches_one_plain_launch(idx):
    name, dtype, B, want, two_waves = plans()[idx]
    assert name == PLAN_IDS[idx]
    P = plan_batch(B, dtype, seed=100 + idx)
    with nm.Handle(plan_cfg(**PLAIN)) as h:
        cold = h.solve(P)
        u0, y0, c0 = warm_start(cold)
        plain = h.solve(P, u0=u0, y0=y0, c0=c0)
        li = h.last_launch_info()
        assert li["order_source"] == 0 and li["tail_handed_off"] == 0 and li["staged_outer_iterations"] == 0, li
    assert (np.abs(y0) > 0).any() and (c0 > 10).any()               # (the warm start carries multipliers and raised penalties)
    with nm.Handle(plan_cfg()) as h:
        r = h.solve(P, u0=u0, y0=y0, c0=c0)
        li = h.last_launch_info()
    print("plan:", name, B, li)
    check_plan(li, want)
    assert li["deep_parked"] <= li["tail_handed_off"]
    if two_waves:
        assert (r["info"][:, 7] == 2).all()
    if want["tail_handed_off"]:
        assert (r["info"][:, 7] > 0).any()                          # (some instance was finished by the tail member)
    same(r, plain, name)
    # ... and warm starts are not ignored: the answers differ from the cold solve's
    assert not np.array_equal(r["iters"], cold["iters"])


def _edge_warm_starts(pr, B, rng):
    """u0 partly outside the control box; y0 with entries of +-1e13 (outside Y), y0 = 0 passed as input, c0 < 1."""
    n, N = 2 * pr.N, pr.N
    u0 = np.empty((B, n))
    u0[:, 0::2] = rng.uniform(0.0, 1.2, (B, N))
    u0[:, 1::2] = rng.uniform(-0.5, 0.5, (B, N))
    y0 = rng.normal(size=(B, n)) * 5
    c0 = rng.uniform(5, 50, B)
    for b in range(B):
        kind = b % 4
        if kind == 0:                                   # multipliers outside [-1e12, 1e12]
            j = rng.choice(n, 4, replace=False)
            y0[b, j] = np.array([1e13, -1e13, 1e13, -1e13])
        elif kind == 1:                                 # zero multipliers, passed as input
            y0[b] = 0
        elif kind == 2:                                 # penalty below 1 (1 / max(c, 1) in the penalty terms)
            c0[b] = rng.uniform(0.05, 0.9)
        else:                                           # initial guess outside the control box
            u0[b, 0::2] = rng.uniform(-1.0, 3.0, N)
            u0[b, 1::2] = rng.uniform(-3.0, 3.0, N)
    return u0, y0, c0


@pytest.mark.parametrize("latency_waves", [1, 4], ids=["throughput-kernel", "latency-kernel"])
@pytest.mark.parametrize("outer,inner", [(1, 10), (2, 5)])
def test_edge_warm_starts_match_oracle_f64(latency_waves, outer, inner):
    """Iterate-path protocol of test_gpu_parity.py (Lipschitz step 1e-4 on both sides, short solves): identical status and
    iteration counts everywhere. Zero multipliers, penalties below 1, guesses outside the box: max|u - u_ref| < 1e-7, and
    since the ALM update y+ = y + c (F1(u) - Proj(F1(u) + y / c)) moves y by at most c * (2 / ts) * |du| when u moves by
    |du| (F1 = differences of consecutive controls over ts), |y - y_ref| <= 1e-9 * max(1, |y_ref|) + c * (2 / ts) * max|du|
    with c the final penalty (info[:, 3]).
    Multipliers of +-1e13: both sides project them on [-1e12, 1e12] before the first inner solve, as before every outer
    iteration. psi is then ~1e23, its rounding exceeds the differences the line search compares, and the iterate path is
    decided by the order of the sums -- the oracle against its own reassociated build differs by up to 1.7 in u on these
    instances -- so u is not compared there. The multipliers are: |y - y_ref| <= 1e-9 * max|y_ref| (unprojected input would
    be off by ~9e12), and the kernel's answer equals, bit for bit, its answer to the input projected by the caller."""
    pr = oracle.Problem()
    B = 24
    P = nm.scenarios.make_batch(B, nm.scenarios.ParamLayout(), seed=50 + outer)
    u0, y0, c0 = _edge_warm_starts(pr, B, np.random.default_rng(7 + outer))
    cfg = config_for(pr, latency_waves=latency_waves, max_outer_iterations=outer, max_inner_iterations=inner,
                     lip_delta_f64=1e-4, lip_eps_f64=1e-4)
    with nm.Handle(cfg) as h:
        r = h.solve(P, u0=u0, y0=y0, c0=c0)
        pre = h.solve(P, u0=u0, y0=np.clip(y0, -1e12, 1e12), c0=c0)
    same(r, pre, "input multipliers projected by the caller")
    op = oracle.Options(max_outer=outer, max_inner=inner, lip_delta=1e-4, lip_eps=1e-4)
    worst, bad = np.zeros(3), []
    for b in range(B):
        op_b = oracle.Options(**{**op.__dict__, "initial_penalty": float(c0[b])})
        u, y, res = oracle.solve(pr, op_b, P[b], u0=u0[b], y0=y0[b])
        du = np.abs(r["U"][b] - u).max()
        dy = np.abs(r["y"][b] - y).max()
        if b % 4 == 0:
            ok = dy <= 1e-9 * np.abs(y).max()
        else:
            tol_y = 1e-9 * max(1.0, np.abs(y).max()) + r["info"][b, 3] * (2 / pr.ts) * du
            ok = du < 1e-7 and dy <= tol_y
            worst = np.maximum(worst, (du, dy, dy / tol_y))
        ok = ok and r["status"][b] == res["status"] and r["iters"][b, 0] == res["outer_iters"] and r["iters"][b, 1] == res["inner_iters"]
        if not ok:
            bad.append((b, b % 4, du, dy, int(r["status"][b]), int(res["status"]), tuple(r["iters"][b]), int(res["outer_iters"]), int(res["inner_iters"])))
    print("edge warm starts, max |du|, max |dy|, max dy / tol:", worst)
    assert not bad, bad
