"""CPU tests of the oracle's solver restatement (OpEn PANOC + ALM; "parity unpinned", see oracle/nmpc_oracle.h):
solver-independent properties only."""
import numpy as np
import pytest
from scipy.optimize import minimize

import dyobav_mpcnwta_warehouse_amd as nm
import oracle


def _batch(B, **kw):
    L = nm.scenarios.ParamLayout()
    return L, nm.scenarios.make_batch(B, L, seed=11, **kw)


def test_param_layout_matches_oracle():
    for dims in ((20, 10, 10, 15), (20, 10, 10, 40), (40, 10, 10, 160), (6, 3, 2, 4)):
        assert nm.scenarios.ParamLayout(*dims).np_ == oracle.Problem(*dims).np_
    assert nm.scenarios.ParamLayout().np_ == 2778
    assert nm.scenarios.ParamLayout(20, 10, 10, 40).np_ == 5928
    assert nm.scenarios.ParamLayout(40, 10, 10, 160).np_ == 40968


def test_solution_is_feasible_and_stationary():
    _, P = _batch(8, n_ped=0, n_boxes=0)
    pr, op = oracle.Problem(), oracle.Options()
    U, res = oracle.solve_batch(pr, op, P, nthreads=4)
    assert (res["outer_iters"] >= 2).all()          # ALM criterion 1 needs iteration > 0
    for b in range(8):
        u = U[b]
        assert (u[0::2] >= pr.lin_vel_min - 1e-12).all() and (u[0::2] <= pr.lin_vel_max + 1e-12).all()
        assert (np.abs(u[1::2]) <= pr.ang_vel_max + 1e-12).all()
        f, F1, F2 = oracle.eval_problem(pr, u, P[b])
        assert f == pytest.approx(res["cost"][b], rel=1e-12)
        if res["status"][b] == 0:
            assert np.linalg.norm(F2) <= 1e-4 + 1e-12
            assert res["last_fpr"][b] < 1e-4


def test_inner_problem_minimiser_agrees_with_scipy():
    """Fixed (c, y): PANOC's fixed point must be the L-BFGS-B minimiser of the same psi over the box U."""
    _, P = _batch(3, n_ped=0, n_boxes=0)
    pr = oracle.Problem()
    op = oracle.Options(max_outer=1, max_inner=5000, tolerance=1e-9, initial_tolerance=1e-9)
    n = 2 * pr.N
    bounds = [(pr.lin_vel_min, pr.lin_vel_max), (-pr.ang_vel_max, pr.ang_vel_max)] * pr.N
    for b in range(3):
        u, _, res = oracle.solve(pr, op, P[b])

        def fun(x):
            v, g = oracle.psi(pr, x, op.initial_penalty, np.zeros(n), P[b])
            return v, g

        ref = minimize(fun, np.zeros(n), jac=True, bounds=bounds, method="L-BFGS-B",
                       options=dict(maxiter=20000, ftol=1e-15, gtol=1e-10))
        vu, _ = oracle.psi(pr, u, op.initial_penalty, np.zeros(n), P[b], grad=False)
        assert vu <= ref.fun + 1e-6 * abs(ref.fun)
        assert np.abs(u - ref.x).max() < 5e-3


def test_fp32_oracle_tracks_fp64():
    _, P = _batch(16, n_ped=0, n_boxes=0)
    pr = oracle.Problem()
    U64, r64 = oracle.solve_batch(pr, oracle.Options(lip_delta=1e-4, lip_eps=1e-4), P, nthreads=4)
    U32, r32 = oracle.solve_batch(pr, oracle.Options(lip_delta=1e-4, lip_eps=1e-4), P, nthreads=4, dtype=np.float32)
    both = (r64["status"] == 0) & (r32["status"] == 0)
    assert both.sum() >= 4
    assert np.median(np.abs(U64 - U32).max(axis=1)[both]) < 2e-2


def test_oracle_wall_clock_cap_like_the_reference():
    """orc_options.max_time_s (the reference builds its solver with_max_duration_micros = 0.1 s, mpc_builder.py:189): a
    budget that is used up ends the solve NotConvergedOutOfTime; a generous one changes nothing."""
    import dyobav_mpcnwta_warehouse_amd as nm
    lay = nm.scenarios.ParamLayout()
    P = nm.scenarios.make_batch(6, lay, seed=3)
    pr = oracle.Problem()
    U0, r0 = oracle.solve_batch(pr, oracle.Options(), P, nthreads=2)
    U1, r1 = oracle.solve_batch(pr, oracle.Options(max_time_s=1e-4), P, nthreads=2)
    U2, r2 = oracle.solve_batch(pr, oracle.Options(max_time_s=600.0), P, nthreads=2)
    assert (r1["status"] == 2).all() and (r1["inner_iters"] < r0["inner_iters"]).all()
    assert np.array_equal(U0, U2) and np.array_equal(r0["status"], r2["status"])


def test_oracle_evaluation_budget_is_deterministic_and_counts_like_the_kernels():
    """orc_options.max_evals = the reference's max_solver_time as a COUNT (what nmpc_config.max_evaluations does on the device;
    tests/test_gpu_options.py compares the two sides exactly). n_points counts the arguments at which psi is formed --
    every gradient call, every psi(u_half) of the Lipschitz test, one F1 / F2 evaluation per outer iteration:
    n_points = n_grad + (cost calls at new points) + outer iterations, and cost calls = gradient calls - 1 init + 2 per step."""
    lay = nm.scenarios.ParamLayout()
    P = nm.scenarios.make_batch(12, lay, seed=3)
    pr = oracle.Problem()
    U0, r0 = oracle.solve_batch(pr, oracle.Options(), P, nthreads=4)
    # the count itself: gradient calls (each at a new point) + the Lipschitz test's psi(u_half) calls + one per outer iteration
    lip_calls = r0["n_points"] - r0["n_grad_evals"] - r0["outer_iters"]
    assert (lip_calls >= r0["inner_iters"]).all()        # at least one psi(u_half) per started step
    assert (r0["n_points"] > 0).all() and (r0["n_points"] <= r0["n_cost_evals"] + r0["outer_iters"]).all()
    # a generous budget changes nothing; the twin and the fp32 instantiation take the option too
    U9, r9 = oracle.solve_batch(pr, oracle.Options(max_evals=10**8), P, nthreads=4)
    assert np.array_equal(U0, U9) and all(np.array_equal(r0[k], r9[k]) for k in ("status", "inner_iters", "n_points"))
    for E in (1, 40, 400, 2500):
        U1, r1 = oracle.solve_batch(pr, oracle.Options(max_evals=E), P, nthreads=4)
        U2, r2 = oracle.solve_batch(pr, oracle.Options(max_evals=E), P, nthreads=1)          # deterministic: threads, order
        assert np.array_equal(U1, U2) and np.array_equal(r1["n_points"], r2["n_points"])
        cut = r0["n_points"] > E + 45
        assert cut.any() or E == 2500
        # cut off: status 2, the budget overshot by at most two iterations (1 + 10 Lipschitz + 11 line-search evaluations
        # each: like OpEn's `while step() && flags`, the step that follows the failed test still runs) + the F1 / F2
        # evaluation behind them; never more work than the unbudgeted solve
        assert (r1["status"][cut] == 2).all()
        assert (r1["n_points"][cut] >= E).all() and (r1["n_points"][cut] <= max(E, 3) + 45).all(), (E, r1["n_points"][cut])
        assert (r1["n_points"] <= r0["n_points"]).all()
        # not cut off (finished within the budget): identical to the unbudgeted solve
        free = r0["n_points"] < E
        assert np.array_equal(U1[free], U0[free]) and np.array_equal(r1["status"][free], r0["status"][free])
        assert np.isfinite(U1).all()
        # the truncated answer is a prefix of the same iterate path: a larger budget continues it
        Ur, rr = oracle.solve_batch(pr, oracle.Options(max_evals=E), P, nthreads=4, reassoc=True)
        assert (rr["status"][cut] == 2).all()
    U32, r32 = oracle.solve_batch(pr, oracle.Options(max_evals=400, lip_delta=1e-4, lip_eps=1e-4), P, nthreads=4, dtype=np.float32)
    assert (r32["n_points"] <= 445).all() and ((r32["status"] == 2) | (r32["n_points"] < 400)).all()


def test_evaluation_budget_from_the_yaml_time_cap():
    """solver.evaluation_budget: yaml max_solver_time [us] -> nmpc_config.max_evaluations, scaled by the work of one
    evaluation at the yaml's dimensions (SURVEY 8d's F_fwd) and the measured CPU rate."""
    from dyobav_mpcnwta_warehouse_amd.solver import CPU_FORWARD_FLOPS_PER_S, evaluation_budget, forward_flops, make_config
    from dyobav_mpcnwta_warehouse_amd.configs import CircularRobotSpecification, MpcConfiguration
    import os
    assert forward_flops(20, 10, 10, 15) == 32340 and forward_flops(20, 10, 10, 40) == 63340
    assert evaluation_budget(0, 20, 10, 10, 15) == 0
    assert evaluation_budget(1e5, 20, 10, 10, 15) == round(0.1 * CPU_FORWARD_FLOPS_PER_S / 32340)
    assert evaluation_budget(5e5, 20, 10, 10, 15) == round(0.5 * CPU_FORWARD_FLOPS_PER_S / 32340)
    assert evaluation_budget(1e5, 20, 10, 10, 40) < evaluation_budget(1e5, 20, 10, 10, 15)          # more work per evaluation
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name, us in (("mpc_fast.yaml", 1e5), ("mpc_default.yaml", 5e5)):
        y = os.path.join(root, "config", name)
        mpc, rob = MpcConfiguration.from_yaml(y), CircularRobotSpecification.from_yaml(y)
        cfg = make_config(mpc, rob)                                     # default: the deterministic form
        assert cfg.max_evaluations == evaluation_budget(us, 20, 10, 10, 15) and cfg.max_solver_time_us == 0.0
        cfg = make_config(mpc, rob, time_cap="wall_clock")              # B = 1 latency bound, behind a flag
        assert cfg.max_evaluations == 0 and cfg.max_solver_time_us == us
        cfg = make_config(mpc, rob, time_cap="none")
        assert cfg.max_evaluations == 0 and cfg.max_solver_time_us == 0.0
    with pytest.raises(ValueError):
        make_config(time_cap="sometimes")


def test_hoisted_trigonometry_gives_the_same_bits():
    """orc_options.hoist_trig = 1 (cos / sin of the ellipse angles once per solve instead of on every evaluation, as a hand-tuned
    CPU solver would; the default recomputes them like the reference's CasADi-generated code) changes the time, not one bit of
    the result -- controls, statuses, every count -- for axis-aligned and rotated ellipses, in fp64, in the re-associated twin and
    in fp32. It is the CPU-baseline speed option of bench.py (`value_trig_hoisted`) and what the GPU suite's CPU-bound legs use."""
    for dims, n in (((20, 10, 10, 15), 10), ((20, 10, 10, 40), 6)):
        lay = nm.scenarios.ParamLayout(*dims)
        P = nm.scenarios.make_batch(n, lay, seed=17, n_ped=dims[3] // 5, n_hyp=5, ped_mode="passing")
        rows = P[:, lay.od:lay.od + lay.Ndyn * (lay.N + 1) * 6].reshape(n, lay.Ndyn, lay.N + 1, 6)
        rows[n // 2:, ::2, :, 4] = 0.37                       # half of the instances: every other ellipse rotated
        pr = oracle.Problem(*dims)
        for kw in (dict(), dict(reassoc=True), dict(dtype=np.float32)):
            opts = dict(lip_delta=1e-4, lip_eps=1e-4) if kw.get("dtype") is np.float32 else {}
            U0, r0 = oracle.solve_batch(pr, oracle.Options(**opts), P, nthreads=4, **kw)
            U1, r1 = oracle.solve_batch(pr, oracle.Options(hoist_trig=1, **opts), P, nthreads=4, **kw)
            assert np.array_equal(U0, U1), (dims, kw)
            assert all(np.array_equal(r0[k], r1[k]) for k in r0.dtype.names), (dims, kw)
        u, y, res, head, Ut = oracle.solve_trace(pr, oracle.Options(hoist_trig=1), P[-1])
        u0, y0, res0, head0, Ut0 = oracle.solve_trace(pr, oracle.Options(), P[-1])
        assert np.array_equal(u, u0) and np.array_equal(head, head0) and np.array_equal(Ut, Ut0)


def test_fp32_twin_takes_the_same_decisions_at_the_wide_lipschitz_step():
    """The fp32 noise floor: orc_*_r32 is the fp32 solver with its sums associated differently (ORC_REASSOC). At the fp32
    default Lipschitz step (1e-4) the finite-difference estimate is itself noisy to ~1e-3 in fp32 and the two builds part
    on a few instances within one iteration; at a step of 1e-2 they take the same decisions on 1 x 1 and 1 x 3 paths for
    every instance of every family and agree to ~1e-5 -- the bar tests/test_gpu_fp32_paths.py holds the fp32 kernels to.
    Measured (96 instances per family, seed 21): du q90 <= 3.6e-5, max <= 1.4e-3; no instance bit-identical."""
    lay = nm.scenarios.ParamLayout()
    pr = oracle.Problem()
    families = dict(free=dict(n_ped=0, n_boxes=0), boxes=dict(n_ped=0), oncoming=dict(ped_mode="oncoming"),
                    toward_robot=dict(), passing=dict(ped_mode="passing"))
    for fam, kw in families.items():
        P = nm.scenarios.make_batch(96, lay, seed=21, **kw).astype(np.float32)
        for max_inner in (1, 3):
            op = oracle.Options(max_outer=1, max_inner=max_inner, lip_delta=1e-2, lip_eps=1e-2)
            U, r = oracle.solve_batch(pr, op, P, nthreads=4, dtype=np.float32)
            Ur, rr = oracle.solve_batch(pr, op, P, nthreads=4, dtype=np.float32, reassoc=True)
            for k in ("status", "outer_iters", "inner_iters", "n_points", "n_grad_evals"):
                assert np.array_equal(r[k], rr[k]), (fam, max_inner, k)
            du = np.abs(U.astype(np.float64) - Ur).max(axis=1)
            assert np.quantile(du, 0.9) < 1e-4 and du.max() < 5e-3, (fam, max_inner, np.quantile(du, 0.9), du.max())
            assert (du > 0).any(), (fam, max_inner)             # the twin really rounds differently
