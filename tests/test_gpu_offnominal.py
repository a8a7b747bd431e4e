"""The solve and evaluation kernels away from the one point the rest of the suite runs at (the robot constants of
config/mpc_fast.yaml, OpEn's default solver options), against the oracle. Inputs, oracle sides and the conditions that need
no device are in tests/offnominal_cases.py / tests/test_offnominal_cpu.py; the oracle itself is pinned at these constants by
tests/golden/problem_offnominal.npz, recorded from the reference (tests/test_oracle_golden.py).

Part 2, psi / grad psi at off-nominal robot constants, every table variant. Bars: on the recorded instances those of
test_gpu_parity.py::test_psi_and_gradient_match_oracle_on_golden_inputs (fp64 1e-11 of |psi| and of max |grad|; fp32 2e-5 and
2e-4; ||F2||^2 and, at c = 0, psi against the RECORDED F2 and f); at the table boundaries those of test_gpu_dims_sweep.py
(fp64 1e-11 / 1e-10 max(1, |grad|), fp32 5e-5 / 5e-4).

Part 3, iterate paths at off-nominal constants (fp64: 3 x 6, Lipschitz step 1e-4; fp32: 1 x 3 and 1 x 10, step 1e-2, on the
14- and 4-slot register tables): status, outer / inner iterations, points and gradient evaluations equal the oracle's,
every control inside the OFF-NOMINAL box exactly; the `reversing` family starts outside the box and ends on the lin_vel_min
face. fp32: exactly the 1 x 3 and 1 x 10 bars of test_gpu_fp32_paths.py.

Part 4, the solver options one at a time (fp64, step 1e-4; L-BFGS memory 1, 2, 3, 5 at 1 x 12; eight ALM / line-search
cases at 3 x 6 or 5 x 40). The bar is taken from the oracle and its re-associated twin, not from the kernels: the kernels'
counts equal the oracle's on every instance for which the twin's do; du (= max |u - u_oracle| of an instance) q90 <=
max(1e-9, 10 x the twin's q90) and max <= 1e-6 over the instances the twin reproduces to 1e-7, which must be 90 % or more.
fp32 at memory 1 and 3: the 1 x 10 bars of test_gpu_fp32_paths.py. Memory 3 through one staged and one tail-hand-off plan
equals one plain launch, as tests/test_gpu_plan_warmstart.py asserts at memory 10.

Measured on an MI355X:
  * psi / grad psi, recorded instances: fp64 1.3e-15 (psi), 4.7e-15 (grad), 1.3e-15 (||F2||^2); fp32 3.7e-7, 2.1e-6, 7.4e-7.
    Table boundaries: fp64 <= 7.3e-15 (psi), <= 1.3e-14 (grad); fp32 <= 8.8e-7 (psi), <= 4.0e-6 (grad).
  * fp64 cases, one line each: kernel du q90, max | twin du q90, max, share of instances the twin reproduces (all over
    the reproduced instances; the oracle's counts on EVERY instance of every case and kernel). Throughput kernel; the
    latency kernels give the same digits, the cooperative kernel differs in four cases, given in brackets.
      path 3 x 6, boxes                            2.56e-11  5.6e-11  | 3.25e-11  7.8e-11  1.000
      path 3 x 6, oncoming                         2.01e-11  8.6e-10  | 3.12e-11  5.6e-10  1.000   [cooperative 2.00e-11  8.6e-10]
      path 3 x 6, toward_robot                     3.43e-11  2.7e-08  | 3.13e-11  2.0e-08  1.000   [cooperative 2.60e-11  2.7e-08]
      path 3 x 6, reversing                        1.83e-12  3.5e-12  | 1.86e-12  2.9e-12  1.000
      path 1 x 1, reversing (projection)           7.58e-13  1.6e-12  | 7.65e-13  1.4e-12  1.000
      memory 1, free                               4.73e-11  7.8e-11  | 6.87e-11  1.0e-10  1.000
      memory 2, free                               4.62e-11  9.5e-11  | 3.55e-11  6.0e-11  1.000
      memory 3, free                               1.34e-11  3.5e-11  | 1.18e-11  2.8e-11  1.000
      memory 5, free                               2.97e-11  4.8e-11  | 2.32e-11  3.8e-11  1.000
      memory 1, boxes                              1.10e-10  5.2e-09  | 9.79e-11  3.1e-09  1.000
      memory 2, boxes                              8.52e-11  1.4e-09  | 4.63e-11  2.8e-10  1.000
      memory 3, boxes                              1.40e-11  2.2e-08  | 1.97e-11  1.3e-08  1.000
      memory 5, boxes                              6.91e-11  7.5e-10  | 5.97e-11  4.5e-10  1.000
      memory 1, oncoming                           5.03e-10  2.9e-09  | 1.59e-09  9.1e-09  1.000
      memory 2, oncoming                           6.96e-10  5.4e-09  | 4.72e-10  2.6e-08  1.000
      memory 3, oncoming                           5.11e-10  1.7e-09  | 1.10e-09  4.2e-09  1.000
      memory 5, oncoming                           7.57e-10  3.5e-09  | 1.10e-09  2.0e-09  1.000
      memory 1, toward_robot                       1.49e-09  5.7e-09  | 1.10e-09  5.5e-09  1.000
      memory 2, toward_robot                       8.68e-10  1.0e-09  | 9.19e-10  1.7e-09  1.000
      memory 3, toward_robot                       7.41e-10  1.4e-09  | 8.05e-10  1.1e-09  1.000
      memory 5, toward_robot                       8.00e-10  1.7e-09  | 9.14e-10  1.7e-09  1.000
      initial_penalty, boxes                       3.40e-11  1.1e-10  | 3.19e-11  1.6e-10  1.000
      initial_penalty, oncoming                    1.18e-10  3.3e-10  | 3.37e-11  3.7e-09  1.000
      penalty_update_factor, boxes                 4.02e-11  3.0e-08  | 6.33e-11  2.9e-08  1.000
      penalty_update_factor, oncoming              2.84e-09  5.8e-09  | 1.97e-09  1.1e-08  1.000   [cooperative 3.19e-09  5.8e-09]
      sy_epsilon, boxes                            9.68e-12  5.9e-10  | 4.99e-12  5.7e-10  1.000
      sy_epsilon, oncoming                         7.35e-12  2.3e-10  | 5.88e-12  3.2e-10  1.000
      cbfgs_epsilon, boxes                         5.35e-11  7.6e-10  | 4.98e-11  6.2e-10  1.000
      cbfgs_epsilon, oncoming                      2.44e-10  4.4e-09  | 2.43e-10  2.9e-09  0.938   [cooperative 2.45e-10  4.4e-09]
      cbfgs_epsilon_alpha, boxes                   1.44e-10  3.6e-09  | 1.30e-10  3.5e-09  1.000
      cbfgs_epsilon_alpha, oncoming                1.74e-09  7.5e-08  | 5.04e-09  5.8e-08  1.000
      sufficient_decrease_coeff, boxes             1.79e-10  3.6e-09  | 2.69e-10  3.5e-09  1.000
      tolerances, free                             8.24e-11  9.8e-10  | 6.30e-11  7.7e-10  1.000
      delta_tolerance, free                        3.76e-09  3.1e-08  | 3.80e-10  2.6e-08  0.938
    The twin strays on two instances of `cbfgs_epsilon` / `oncoming` and of `delta_tolerance` / `free`; its q90 over ALL
    instances is 2.06e-9 and 1.60e-8 there. The bars use the reproduced instances only: 2.43e-9 and 3.80e-9 -- the
    `delta_tolerance` case (5 x 40 iterations) meets its bar by 1 %.
    Active faces of the 3 x 6 paths: lin_vel_max 100 % and +-ang_vel_max 37..53 % of `boxes` / `oncoming` /
    `toward_robot`, lin_vel_min 100 % of `reversing`. Every case ran the kernel it names (launch family and info[7]).
  * fp32 paths: 1 x 3 the oracle's counts on all 128 instances, du q90 2.1e-5 (14-slot; twin 1.4e-5) and 9.0e-6 (4-slot;
    twin 8.9e-6), max 2.2e-4; 1 x 10 shares 0.992 / 1.000 (twin the same), du q90 1.4e-4 / 1.1e-4 (twin 1.2e-4 / 1.0e-4).
  * L-BFGS memory in fp32, 1 x 10 (96 instances; 6-slot throughput and latency kernels, the latency kernel with the tail
    member, the cooperative LDS kernel): share with the oracle's counts 0.969 (twin 0.969 at memory 1, 0.979 at 3), du q90
    2.6e-4 (memory 1; twin 2.1e-4) and 6.8e-4 (memory 3; twin 4.9e-4). Plans at memory 3: 5 120 instances, 256 handed to the
    tail member, 231 of them deep parks; 384 fp64 instances through the pilot (staged) plan -- both bit for bit the plain
    launch.
"""
import ctypes

import numpy as np
import pytest

import dyobav_mpcnwta_warehouse_amd as nm
import oracle
import offnominal_cases as oc

pytestmark = pytest.mark.gpu

SOLVE_KERNELS = ("throughput", "latency", "cooperative")
# kernel name -> (family of nmpc_last_launch_info, info[7] of every instance: 0 throughput kernel, W wavefronts of the
# latency kernel, -W of the cooperative one), as tests/test_gpu_fp32_paths.py reads them
RAN = {"throughput": ("throughput", 0), "latency": ("latency", 4), "latency3": ("latency", 3), "cooperative": ("cooperative", -4)}


def solve_on(kernel, cfg, P, u0=None):
    """Solve with `cfg` and show that the kernel the case names is the one that ran, and no other."""
    fam, w = RAN[kernel]
    with nm.Handle(cfg) as h:
        r = h.solve(P, u0=u0)
        li = h.last_launch_info()
    assert li["family"] == fam and (r["info"][:, 7] == w).all(), (kernel, li, np.unique(r["info"][:, 7]))
    return r


# ---- part 2 ----------------------------------------------------------------------------------------------------------
EVAL_MODES = {"throughput": dict(latency_waves=1), "throughput-lds-table": dict(latency_waves=1, reg_table=-1),
              "latency": dict(latency_waves=4), "latency-lds-table": dict(latency_waves=4, reg_table=-1),
              "cooperative": dict(latency_waves=1, coop_waves=4, reg_table=-1)}


@pytest.mark.parametrize("mode", list(EVAL_MODES))
def test_psi_and_gradient_on_the_recorded_offnominal_instances(mode):
    inp = oc.eval_inputs_fixture()
    pr, P, U, Y, C = (inp[k] for k in ("pr", "P", "U", "Y", "C"))
    want = oc.memo("psi-fixture", lambda: oc.oracle_psi(inp))
    with nm.Handle(oc.config_for(pr, **EVAL_MODES[mode])) as h:
        for dtype, rp, rg in ((np.float64, 1e-11, 1e-11), (np.float32, 2e-5, 2e-4)):
            r = h.eval(P, U, Y, C, dtype=dtype)
            worst = np.zeros(3)
            for i, (v, g) in enumerate(want):
                f2 = float(np.sum(inp["F2"][i] ** 2))
                worst = np.maximum(worst, (abs(r["psi"][i] - v) / abs(v), np.abs(r["grad"][i] - g).max() / np.abs(g).max(),
                                           abs(r["f2sq"][i] - f2) / f2))
            print(mode, np.dtype(dtype).name, "worst relative error of psi, grad (of max |grad|), f2sq:", worst)
            for i, (v, g) in enumerate(want):
                assert r["psi"][i] == pytest.approx(v, rel=rp), (mode, dtype, i)
                np.testing.assert_allclose(r["grad"][i], g, rtol=0, atol=rg * np.abs(g).max())
                assert r["f2sq"][i] == pytest.approx(float(np.sum(inp["F2"][i] ** 2)), rel=10 * rp, abs=1e-12)
            for i in range(2):
                assert C[i] == 0.0 and r["psi"][i] == pytest.approx(inp["f"][i], rel=rp)


@pytest.mark.parametrize("idx", range(len(oc.DIMS_CASES)), ids=oc.DIMS_IDS)
def test_psi_and_gradient_at_the_table_boundaries_with_offnominal_constants(idx):
    N, Ndyn, n_ped, n_hyp, ov = oc.DIMS_CASES[idx]
    inp = oc.eval_inputs_dims(N, Ndyn, n_ped, n_hyp)
    pr, P, U, Y, C = (inp[k] for k in ("pr", "P", "U", "Y", "C"))
    want = oc.memo(("psi-dims", N, Ndyn), lambda: oc.oracle_psi(inp))
    if N == 40:      # the streamed table: the cooperative pair member asked for, and the throughput kernel's general table
        modes = [dict(coop_waves=4, latency_waves=1, reg_table=-1, **ov), dict(coop_waves=1, latency_waves=1, reg_table=-1)]
    else:
        modes = [dict(reg_table=0), dict(reg_table=-1)]
        slots = {12: 4, 13: 6, 43: 0}.get(Ndyn) if N == 20 else 0
        assert nm.layout_info(oc.config_for(pr)).reg_slots_f32 == slots           # the table this row count is the edge of
    for m in modes:
        with nm.Handle(oc.config_for(pr, **m)) as h:
            for dtype, tp, tg in ((np.float64, 1e-11, 1e-10), (np.float32, 5e-5, 5e-4)):
                r = h.eval(P, U, Y, C, dtype=dtype)
                if "axis_aligned" in m:
                    li = h.last_launch_info()
                    assert li["family"] == "cooperative" and li["axis_aligned"] == {1: 1, -1: 0}[m["axis_aligned"]], li
                worst = np.zeros(2)
                for i, (v, g) in enumerate(want):
                    worst = np.maximum(worst, (abs(r["psi"][i] - v) / abs(v), np.abs(r["grad"][i] - g).max() / max(1.0, np.abs(g).max())))
                print(oc.DIMS_IDS[idx], m, np.dtype(dtype).name, "worst error of psi (relative), grad (of max(1, |grad|)):", worst)
                for i, (v, g) in enumerate(want):
                    assert r["psi"][i] == pytest.approx(v, rel=tp), (m, dtype, i)
                    np.testing.assert_allclose(r["grad"][i], g, rtol=0, atol=tg * max(1.0, np.abs(g).max()))


# ---- the bar of parts 3 and 4 (fp64) -----------------------------------------------------------------------------------
def check_against_oracle_and_twin(what, r, oracle_side, twin_side, exact_counts=False):
    """Counts equal the oracle's wherever the twin's do (`exact_counts`: on every instance); du q90 <= max(1e-9, 10 x the
    twin's) and max <= 1e-6 over the instances the twin reproduces to 1e-7 -- at least 90 % of them. Both
    q90 are taken over those reproduced instances; the twin's q90 over the whole case is printed beside it."""
    (Uo, ro), (Ut, rt) = oracle_side, twin_side
    twin_same, rep = oc.twin_floor(Uo, ro, Ut, rt)
    hip = oc.as_record(r)
    same = oc.same_counts(hip, ro)
    d, dt = oc.du(r["U"], Uo), oc.du(Ut, Uo)
    msg = (what, f"same counts {same.mean():.3f} (twin {twin_same.mean():.3f}, reproduces {rep.mean():.3f})",
           f"du q90 {np.quantile(d[rep], 0.9):.2e} max {d[rep].max():.1e} | twin q90 {np.quantile(dt[rep], 0.9):.2e} max {dt[rep].max():.1e} (q90 of all instances {np.quantile(dt, 0.9):.2e})")
    print(*msg)
    assert np.isfinite(r["U"]).all(), msg
    assert rep.mean() >= 0.9, msg
    bad = np.flatnonzero(~same & (True if exact_counts else twin_same))
    assert bad.size == 0, msg + ({k: (hip[k][bad[:4]], ro[k][bad[:4]]) for k in oc.COUNTS},)
    assert np.quantile(d[rep], 0.9) <= max(1e-9, 10 * np.quantile(dt[rep], 0.9)), msg
    assert d[rep].max() <= 1e-6, msg


# ---- part 3 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", SOLVE_KERNELS)
@pytest.mark.parametrize("family", oc.PATH_FAMILIES)
def test_iterate_path_at_offnominal_constants_f64(family, kernel):
    pr, P, u0 = oc.path_case(family)
    o = oc.oracle_solve(("path", family), pr, P, u0=u0, **oc.PATH_CAPS)
    t = oc.oracle_solve(("path", family), pr, P, u0=u0, reassoc=True, **oc.PATH_CAPS)
    r = solve_on(kernel, oc.config_for(pr, **oc.KERNELS[kernel], **oc.config_options(**oc.PATH_CAPS)), P, u0)
    check_against_oracle_and_twin(("path", family, kernel), r, o, t, exact_counts=True)
    assert oc.inside_box(r["U"], pr)
    act = oc.face_activity(r["U"], pr)
    print(family, kernel, "active faces:", act)
    if family == "reversing":
        assert act["lin_vel_min"] >= 0.1
    else:
        assert act["lin_vel_max"] >= 0.1 and act["ang_vel_max"] >= 0.1


def test_projection_of_a_guess_outside_the_offnominal_box():
    """1 x 1 from the `reversing` warm start (speeds below lin_vel_min, turn rates beyond +-ang_vel_max): counts and first
    iterate against the oracle, every kernel."""
    pr, P, u0 = oc.path_case("reversing")
    caps = dict(max_outer=1, max_inner=1)
    o = oc.oracle_solve(("path", "reversing"), pr, P, u0=u0, **caps)
    t = oc.oracle_solve(("path", "reversing"), pr, P, u0=u0, reassoc=True, **caps)
    for kernel in SOLVE_KERNELS:
        r = solve_on(kernel, oc.config_for(pr, **oc.KERNELS[kernel], **oc.config_options(**caps)), P, u0)
        check_against_oracle_and_twin(("projection", kernel), r, o, t, exact_counts=True)
        assert oc.inside_box(r["U"], pr) and (r["U"][:, 0::2] == pr.lin_vel_min).any(axis=1).all()


F32_TABLES = {"reg14": ((4, 10), 40, 14), "reg4": ((2, 5), 12, 4)}      # rows (n_ped, n_hyp), max_active_dynobs, slots
F32_KERNELS = {"throughput": dict(latency_waves=1, coop_waves=1), "latency": dict(latency_waves=4, coop_waves=1)}


def _f32_batch(table):
    """The four families of part 3 (32 instances each) at Ndynobs = 40 in fp32; zero start except `reversing`."""
    def make():
        rows = F32_TABLES[table][0]
        Ps, u0s = [], []
        for fam in oc.PATH_FAMILIES:
            pr, P, u0 = oc.path_case(fam, np.float32, 40, rows, 32)
            Ps.append(P)
            u0s.append(np.zeros((32, 40), dtype=np.float32) if u0 is None else u0)
        return pr, np.concatenate(Ps), np.concatenate(u0s)
    return oc.memo(("f32-batch", table), make)


@pytest.mark.parametrize("kernel", list(F32_KERNELS))
@pytest.mark.parametrize("table", list(F32_TABLES))
def test_iterate_path_at_offnominal_constants_f32(table, kernel):
    """The fp32 register-table kernels against the fp32 oracle at the off-nominal constants: the 1 x 3 and 1 x 10 bars of
    test_gpu_fp32_paths.py::test_iterate_path_matches_the_fp32_oracle with the twin as the noise floor."""
    rows, hint, slots = F32_TABLES[table]
    pr, P, u0 = _f32_batch(table)
    for outer, inner in ((1, 3), (1, 10)):
        caps = dict(max_outer=outer, max_inner=inner)
        cfg = oc.config_for(pr, max_active_dynobs=hint, **F32_KERNELS[kernel], **oc.config_options(np.float32, **caps))
        assert nm.layout_info(cfg).reg_slots_f32 == slots
        r = solve_on(kernel, cfg, P, u0)
        Uo, ro = oc.oracle_solve(("path32", table), pr, P, np.float32, u0=u0, **caps)
        Ut, rt = oc.oracle_solve(("path32", table), pr, P, np.float32, u0=u0, reassoc=True, **caps)
        hip = oc.as_record(r)
        same, twin = oc.same_counts(hip, ro), oc.same_counts(rt, ro)
        d, d_t = oc.du(r["U"], Uo), oc.du(Ut, Uo)
        floor = ~twin | (d_t > 1e-3)
        near = same & ~floor
        msg = (table, kernel, outer, inner, f"same {same.mean():.3f} (twin {twin.mean():.3f})",
               f"du q90 {np.quantile(d[same], 0.9):.2e} max {d[near].max():.2e} | twin q90 {np.quantile(d_t[twin], 0.9):.2e} max {d_t[twin & ~floor].max():.2e}")
        print(*msg)
        assert np.isfinite(r["U"]).all() and oc.inside_box(r["U"], pr, np.float32), msg
        if inner == 3:
            bad = np.flatnonzero(~same)
            assert bad.size <= 1 and floor[bad].all(), msg + ({k: (hip[k][bad[:4]], ro[k][bad[:4]]) for k in oc.COUNTS},)
            assert np.quantile(d[same], 0.9) <= max(1e-4, 2 * np.quantile(d_t[twin], 0.9)), msg
            assert d[near].max() <= 5e-3, msg
        else:
            assert same.mean() >= twin.mean() - 0.1 and same.any(), msg
            for q in (0.5, 0.9):
                assert np.quantile(d[same], q) <= 10 * max(np.quantile(d_t[twin], q), 1e-6), (q,) + msg
        rev = slice(96, 128)
        assert (r["U"][rev, 0::2] == np.float32(pr.lin_vel_min)).any(axis=1).mean() >= 0.1


# ---- part 4: L-BFGS memory ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ("throughput", "latency3", "latency", "cooperative"))
@pytest.mark.parametrize("family", oc.MEM_FAMILIES)
def test_lbfgs_memory_against_the_oracle_f64(family, kernel):
    pr, P = oc.mem_case(family)
    for mem in oc.MEMORIES:
        op = dict(lbfgs_mem=mem, **oc.MEM_CAPS)
        o = oc.oracle_solve(("mem", family), pr, P, **op)
        t = oc.oracle_solve(("mem", family), pr, P, reassoc=True, **op)
        r = solve_on(kernel, oc.config_for(pr, **oc.KERNELS[kernel], **oc.config_options(**op)), P)
        check_against_oracle_and_twin(("memory", mem, family, kernel), r, o, t)
        U10, r10 = oc.oracle_solve(("mem", family), pr, P, lbfgs_mem=10, **oc.MEM_CAPS)
        assert oc.moved(r["U"], oc.as_record(r), U10, r10) >= 0.5          # (the memory matters: not memory 10's answer)


MEM32_KERNELS = {"throughput-reg6": ("throughput", dict(latency_waves=1, coop_waves=1)),
                 "latency-reg6": ("latency", dict(latency_waves=4, coop_waves=1)),
                 "latency-reg6-tail": ("latency", dict(latency_waves=4, coop_waves=1, batch_invariant=1)),
                 "cooperative-lds": ("cooperative", dict(latency_waves=1, coop_waves=4, reg_table=-1))}


@pytest.mark.parametrize("kernel", list(MEM32_KERNELS))
def test_lbfgs_memory_against_the_fp32_oracle(kernel):
    """Memory 1 and 3 in fp32 (the register-table kernels and the tail members exist in fp32 only), 1 x 10 bars of
    test_gpu_fp32_paths.py; the four families of the fp64 test in one batch of 96."""
    pr = oracle.Problem()
    P = np.concatenate([oc.mem_case(f, np.float32)[1] for f in oc.MEM_FAMILIES])
    caps = dict(max_outer=1, max_inner=10)
    for mem in (1, 3):
        ran, ov = MEM32_KERNELS[kernel]
        cfg = oc.config_for(pr, **ov, **oc.config_options(np.float32, lbfgs_mem=mem, **caps))
        assert nm.layout_info(cfg).reg_slots_f32 == (0 if "lds" in kernel else 6)
        r = solve_on(ran, cfg, P)
        Uo, ro = oc.oracle_solve("mem32", pr, P, np.float32, lbfgs_mem=mem, **caps)
        Ut, rt = oc.oracle_solve("mem32", pr, P, np.float32, reassoc=True, lbfgs_mem=mem, **caps)
        U10, r10 = oc.oracle_solve("mem32", pr, P, np.float32, lbfgs_mem=10, **caps)
        same, twin = oc.same_counts(oc.as_record(r), ro), oc.same_counts(rt, ro)
        d, d_t = oc.du(r["U"], Uo), oc.du(Ut, Uo)
        msg = (kernel, mem, f"same {same.mean():.3f} (twin {twin.mean():.3f})",
               f"du q50 {np.quantile(d[same], 0.5):.2e} q90 {np.quantile(d[same], 0.9):.2e} | twin q50 {np.quantile(d_t[twin], 0.5):.2e} q90 {np.quantile(d_t[twin], 0.9):.2e}")
        print(*msg)
        assert np.isfinite(r["U"]).all(), msg
        assert same.mean() >= twin.mean() - 0.1 and same.any(), msg
        for q in (0.5, 0.9):
            assert np.quantile(d[same], q) <= 10 * max(np.quantile(d_t[twin], q), 1e-6), (q,) + msg
        assert oc.moved(r["U"], oc.as_record(r), U10, r10, tol=1e-3) >= 0.5, msg


@pytest.mark.parametrize("plan", ["throughput-evaluation-order-tail", "fp64-pilot"])
def test_lbfgs_memory_3_through_a_tail_hand_off_and_a_staged_plan_matches_one_plain_launch(plan):
    """tests/test_gpu_plan_warmstart.py at lbfgs_memory = 3: the ring (lb_head / lb_active and three of the ten slots) goes
    through the deep park of the tail hand-off, and through the resumable solve of the staged plan, and the warm-started
    batch comes out bit for bit as from one plain launch."""
    import test_gpu_plan_warmstart as pw
    idx = pw.PLAN_IDS.index(plan)
    name, dtype, B, want, _ = pw.plans()[idx]
    assert name == plan and (want["tail_handed_off"] > 0 or want["staged_outer_iterations"] > 0)
    P = pw.plan_batch(B, dtype, seed=100 + idx)
    with nm.Handle(pw.plan_cfg(lbfgs_memory=3, **pw.PLAIN)) as h:
        cold = h.solve(P)
        u0, y0, c0 = pw.warm_start(cold)
        plain = h.solve(P, u0=u0, y0=y0, c0=c0)
        li = h.last_launch_info()
        assert li["order_source"] == 0 and li["tail_handed_off"] == 0 and li["staged_outer_iterations"] == 0, li
    with nm.Handle(pw.plan_cfg(lbfgs_memory=3)) as h:
        r = h.solve(P, u0=u0, y0=y0, c0=c0)
        li = h.last_launch_info()
    print("plan:", name, B, li)
    pw.check_plan(li, want)
    if want["tail_handed_off"]:
        assert (r["info"][:, 7] > 0).any()
    pw.same(r, plain, name)
    with nm.Handle(pw.plan_cfg(**pw.PLAIN)) as h:           # ... and it is memory 3's answer, not memory 10's
        ten = h.solve(P, u0=u0, y0=y0, c0=c0)
    assert np.mean(np.any(ten["iters"] != r["iters"], axis=1)) >= 0.2


# ---- part 4: ALM and line-search options -------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", SOLVE_KERNELS)
@pytest.mark.parametrize("name", list(oc.OPTION_CASES))
def test_solver_option_against_the_oracle_f64(name, kernel):
    op, families, caps = oc.OPTION_CASES[name]
    for family in families:
        pr, P = oc.option_case(family)
        o = oc.oracle_solve(("opt", family), pr, P, **caps, **op)
        t = oc.oracle_solve(("opt", family), pr, P, reassoc=True, **caps, **op)
        r = solve_on(kernel, oc.config_for(pr, **oc.KERNELS[kernel], **oc.config_options(**caps, **op)), P)
        check_against_oracle_and_twin((name, family, kernel), r, o, t)
        Ub, rb = oc.oracle_solve(("opt", family), pr, P, **caps)
        assert oc.moved(r["U"], oc.as_record(r), Ub, rb) >= 0.2           # (the option bites on the device too)


def test_lbfgs_memory_argument_checks():
    lib = nm.load_library()
    cfg = nm.default_config_struct()
    cfg.lbfgs_memory = 0
    hnd = ctypes.c_void_p()
    assert lib.nmpc_create(ctypes.byref(cfg), ctypes.byref(hnd)) == -4          # NMPC_ERR_UNSUPPORTED
    cfg.lbfgs_memory = 1
    with nm.Handle(cfg) as h:
        r = h.solve(oc.mem_case("free")[1][:4])
    assert set(np.unique(r["status"])) <= {0, 1} and np.isfinite(r["U"]).all()
