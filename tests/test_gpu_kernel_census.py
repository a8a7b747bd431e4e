"""One test per row of tests/kernel_census.py: the solver, evaluation and trace kernels that no declared suite names, each reached
on purpose and held to the oracle.

The declared suites stream the obstacle table from global memory at one lane per horizon step only (N = 40); the GLB kernels at
two and three lanes per step, the cooperative kernels' evaluation entry, several general and tail members of the register-table
pairs, the fp64 register-table solve and every trace kernel were reached by the fixed-seed fuzz runs at most -- four fp32 solve
kernels by nothing at all (profiles/kernel_census_fuzz.txt). The rows use the smallest dimensions at which each path exists, on
the global side of the boundary that nmpc_layout draws (N = 21 and 32, Nother = Nstcobs = 10), plus evaluation rows one
obstacle row below it, where the table is still in LDS.

Every row first asserts that it reached its kernel, by the fields the naming rule keys on (nmpc_last_launch_info: family and
pair member; nmpc_layout: global table, register slots; 64 / N: lanes per step; for solves info[7]: wavefronts -- an evaluation
returns no info, and both wave counts of the cooperative evaluation run the same W = 4 instantiation), then compares values:
  * eval rows (B = 3, a quarter to a half of the provisioned rows on the robot's path): psi, grad psi, ||F2||^2 against the
    fp64 oracle -- fp64 1e-11 / 1e-10, fp32 5e-5 / 5e-4 (psi relative, grad scaled by max(1, |g|max): test_gpu_dims_sweep.py),
    ||F2||^2 to 10x the psi bar; a gradient beyond its bar is a kink, not an error, if the oracle's own gradient moves as much
    under a 1e-6 perturbation of u (fuzz_eval.run).
  * fp64 solve rows (8 instances per family): 1 x 3 iterations at a Lipschitz step of 1e-4 against oracle.solve_batch -- equal
    inner-iteration counts, du median < 1e-7, max < 50x that (test_gpu_dims_sweep.py).
  * fp32 solve rows: 1 x 1 and 1 x 3 paths against the fp32 oracle at the step 1e-2 with the "exact paths" bars and helpers of
    test_gpu_fp32_paths.py -- the oracle's counts on every instance but at most one that the twin does not reproduce either,
    du q90 <= max(1e-4, 2 x the twin's), max <= 5e-3 over the instances the twin reproduces to 1e-3.
  * rows of the general member of a pair: both members on the SAME axis-aligned batch (axis_aligned = 1 against -1) agree to
    the row's bars.
  * trace rows: U, status and iters of nmpc_solve_trace_f64 equal, bit for bit, those of nmpc_solve_batch_f64 on the
    one-wavefront kernel; the oracle's 1 x 3 solve and every record's iterate to 1e-7, the records' discrete fields equal to
    the oracle's. One record per completed step of the inner loop: the inner iterations plus one for a solve that ran into
    max_inner_iterations (3 iterations, 4 records here, in the oracle's trace as well). U is the projected gradient step
    from the last record's u (the solver returns u_half), not that u itself: held with the oracle's gradient there.

The oracle's fp32 twin on the batches of the fp32 solve rows (CPU, 40 instances each; q90 of du over the instances with the
oracle's counts, 1 x 1 / 1 x 3; instances the twin does not reproduce):
    batch (N, Ndynobs, pedestrians x hypotheses)      1 x 1      1 x 3      not reproduced   rows
    21, 193, 3 x 20, axis-aligned                     1.6e-5     1.4e-5     0 / 0            coop4-glb-l3-compressed, members of coop2-glb-l3-general
    21, 193, 3 x 20, every other instance turned      2.2e-5     2.1e-5     0 / 0            tp-glb-l3, lat4-glb-l3, coop2-glb-l3-general
    32, 127, 3 x 15, axis-aligned                     1.8e-5     2.1e-5     0 / 0            coop4-glb-l2-compressed, members of coop2-glb-l2-general
    32, 127, 3 x 15, turned                           1.8e-5     2.1e-5     0 / 0            tp-glb-l2, lat4-glb-l2, coop2-glb-l2-general
    20, 42, 3 x 5, axis-aligned                       1.8e-5     6.5e-6     0 / 0            members of lat4-reg14-flat-general
    20, 42, 3 x 5, turned                             1.8e-5     1.1e-5     0 / 0            lat4-reg14-flat-general
    20, 12, 4 x 1, axis-aligned                       1.9e-5     1.0e-5     0 / 0            lat4-reg4-tail-axis, members of the reg4 general rows
    20, 12, 4 x 1, turned                             1.5e-5     6.7e-6     0 / 0            lat4-reg4-flat-general, lat4-reg4-tail-general
    20, 18, 3 x 2, axis-aligned                       1.0e-5     9.2e-6     0 / 0            members of lat4-reg6-tail-general
    20, 18, 3 x 2, turned                             1.5e-5     1.1e-5     0 / 0            lat4-reg6-tail-general
(no batch needed another seed: the twin reproduces every instance)

Measured on an MI355X:
  * the module: 62 rows in 2.5 s of pytest time, 0.6 s of it in the tests themselves (the rest is collection and imports).
  * eval rows, worst relative error over the class (psi / grad / ||F2||^2), no instance on a kink:
      fp64 5.1e-15 / 1.6e-14 / 1.6e-14 (bars 1e-11 / 1e-10 / 1e-10); fp32 2.3e-7 / 2.3e-6 / 3.4e-6 (bars 5e-5 / 5e-4 / 5e-4).
  * fp64 solve rows: the oracle's inner-iteration counts everywhere; du median at most 1.6e-12, max 2.4e-10.
  * fp32 solve rows: the oracle's counts on all 40 instances of every row and path; du q90 9.3e-6 .. 5.0e-5 (the twin's
    6.5e-6 .. 2.2e-5), max 8.6e-4.
  * pair members on the same axis-aligned batch: identical bits in every row (psi, grad, U, counts) except the fp32
    one-lane-per-step global-table evaluation, whose gradients differ by 1.1e-7 of their scale. That the two runs are different
    kernels is what nmpc_last_launch_info says and what a mutant of the compressed member alone shows (below).
  * trace rows: 4 records for 3 inner iterations; U within 5.8e-12 of the oracle's, within 6.7e-16 of the half step from the
    last record.
  * two wrong-number mutants, built apart and loaded through NMPC_HIP_LIBRARY, not kept: (A) the second plane of the cooperative
    exchange area stored one Quad early for GLB kernels with more than one lane per step fails the 16 cooperative global-table
    rows at two and three lanes per step (evaluation and solve, both members, both precisions) and nothing else; (B) the weight
    of the compressed table's t = 0 rows taken as 1 at three lanes per step fails the 8 cooperative global-table rows at three
    lanes per step (the general-member rows through their member comparison). Both pass test_gpu_dims_sweep.py,
    test_gpu_fp32_paths.py, test_gpu_parity.py, test_gpu_coop.py, test_gpu_handle_history.py, test_gpu_offnominal.py (289 tests)
    and the evaluation and solve tests of test_gpu_read_bounds.py (40). The fixed-seed fuzz runs catch both today -- A in 7 of
    its 8 evaluation and solve runs, B in the 3 evaluation and 2 of the 3 fp64 solve runs, not in the fp32 solve runs, which
    never reach a three-lane global-table kernel -- by the draws of their seeds, not by a declared case.
"""
import time

import numpy as np
import pytest

import dyobav_mpcnwta_warehouse_amd as nm
import kernel_census as kc
import oracle
import test_gpu_fp32_paths as paths
from accuracy_protocol import HOST_THREADS

pytestmark = pytest.mark.gpu

# the file's order: evaluations (the LDS side of the boundary last among them), solves, traces
ROWS = [r for r in kc.CENSUS if r.entry == "eval"] + list(kc.BOUNDARY) + [r for r in kc.CENSUS if r.entry == "solve"] + \
       [r for r in kc.CENSUS if r.entry == "trace"]
FAMILY = {kc.THROUGHPUT: "throughput", kc.EVAL: "throughput", kc.LATENCY_FLAT: "latency", kc.LATENCY_TAIL: "latency", kc.COOP: "cooperative",
          kc.COOP_ONCHIP: "cooperative", kc.EVAL_COOP: "cooperative", kc.EVAL_COOP_ONCHIP: "cooperative"}
SHORT = dict(max_outer_iterations=1, max_inner_iterations=3, lip_eps_f64=1e-4, lip_delta_f64=1e-4)
SHORT_ORACLE = dict(max_outer=1, max_inner=3, lip_delta=1e-4, lip_eps=1e-4)


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.time()
    yield
    print(f"\n[kernel census] {time.time() - t0:.1f} s")


def _cfg(r, **ov):
    cfg = nm.default_config_struct()
    cfg.N_hor, cfg.Nother, cfg.Nstcobs, cfg.Ndynobs = r.dims
    cfg.lip_eps_f32 = cfg.lip_delta_f32 = paths.LIP
    for k, v in {**r.options, **ov}.items():
        assert hasattr(cfg, k), k
        setattr(cfg, k, v)
    return cfg


def _assert_layout(r, cfg):
    """The fields of the naming rule that the configuration fixes: table placement, register slots, lanes per step."""
    v, elem, _ = kc.universe()[r.kernel]
    li = nm.layout_info(cfg)
    assert min(3, 64 // cfg.N_hor) == v.lps, (r.id, cfg.N_hor)
    if v.rs != 12:          # (the on-chip cooperative kernels have a layout of their own)
        assert bool(li.global_table_f32 if elem == 4 else li.global_table_f64) == v.glb, r.id
        if elem == 4:
            assert li.reg_slots_f32 == v.rs, (r.id, li.reg_slots_f32)
    if v.glb:               # the first Ndynobs on the global side: one row fewer and the table is in LDS
        below = _cfg(r)
        below.Ndynobs -= 1
        lb = nm.layout_info(below)
        assert not (lb.global_table_f32 if elem == 4 else lb.global_table_f64), r.id
    return v


def _assert_reached(r, cfg, li, info=None, axis=None):
    v, elem, member = kc.universe()[r.kernel]
    want_axis = -1 if not v.pair else (1 if member == 1 else 0) if axis is None else axis
    assert li["family"] == FAMILY[v.family] and li["axis_aligned"] == want_axis, (r.id, li)
    if info is not None:
        w = {"throughput": 0, "latency": cfg.latency_waves, "cooperative": -8 if v.rs == 12 else -min(cfg.coop_waves, 4)}[FAMILY[v.family]]
        assert (info[:, 7] == w).all(), (r.id, np.unique(info[:, 7]))


# ---- evaluations ----------------------------------------------------------------------------------------------------------------------
_WANT = {}


def _want(dims, n_rows, rotated, dtype):
    """psi, grad psi and ||F2||^2 of the oracle at the inputs as the kernel gets them (rounded to `dtype`); computed once."""
    key = (dims, n_rows, rotated, np.dtype(dtype).name)
    if key not in _WANT:
        lay, P, U, Y, C = kc.eval_problem(dims, n_rows, rotated)
        pr = oracle.Problem(*dims)
        rd = lambda a: np.asarray(a).astype(dtype).astype(np.float64)
        out = []
        for i in range(P.shape[0]):
            u, y, c, p = rd(U[i]), rd(Y[i]), float(rd(C[i])), rd(P[i])
            v, g = oracle.psi(pr, u, c, y, p)
            out.append((v, g, float(np.sum(np.asarray(oracle.eval_problem(pr, u, p)[2]) ** 2)), (u, y, c, p)))
        _WANT[key] = (pr, out)
    return _WANT[key]


def _tol(dtype):
    return (1e-11, 1e-10) if np.dtype(dtype) == np.float64 else (5e-5, 5e-4)


def _eval(r, P, U, Y, C, dtype, **ov):
    cfg = _cfg(r, **ov)
    with nm.Handle(cfg) as h:
        out = h.eval(P, U, Y, C, dtype=dtype)
        return cfg, out, h.last_launch_info()


def _run_eval_row(r):
    dtype = np.float64 if r.elem == 8 else np.float32
    tp, tg = _tol(dtype)
    _assert_layout(r, _cfg(r))
    lay, P, U, Y, C = kc.eval_problem(r.dims, r.obstacles, r.rotated)
    cfg, got, li = _eval(r, P, U, Y, C, dtype)
    _assert_reached(r, cfg, li)
    pr, want = _want(r.dims, r.obstacles, r.rotated, dtype)
    worst, kinks = [0.0, 0.0, 0.0], 0
    for i, (v, g, f2, (u, y, c, p)) in enumerate(want):
        ep, ef = abs(got["psi"][i] - v) / abs(v), abs(got["f2sq"][i] - f2) / max(1.0, abs(f2))
        eg = np.abs(got["grad"][i] - g).max() / max(1.0, np.abs(g).max())
        assert f2 > 0 and ep <= tp and ef <= 10 * tp, (r.id, i, ep, ef)       # (psi and ||F2||^2 have no kink: held on every instance)
        worst[0], worst[2] = max(worst[0], ep), max(worst[2], ef)
        if eg > tg:
            jump = max(np.abs(oracle.psi(pr, u * (1 + s), c, y, p)[1] - g).max() for s in (1e-6, -1e-6))
            # a step ON a hard ellipse's boundary: the gradient jumps there
            assert jump / max(1.0, np.abs(g).max()) > 0.3 * eg, (r.id, i, eg, jump)
            kinks += 1
            continue
        worst[1] = max(worst[1], eg)
    assert kinks <= 1, (r.id, kinks)                                         # at most one of the three instances on a kink
    line = f"psi {worst[0]:.1e} grad {worst[1]:.1e} f2sq {worst[2]:.1e} kinks {kinks}"
    v, _, member = kc.universe()[r.kernel]
    if v.pair and member == 2:
        # both members on the same axis-aligned batch
        _, Pa, Ua, Ya, Ca = kc.eval_problem(r.dims, r.obstacles, False)
        res = {}
        for axis in (1, -1):
            cfg, res[axis], li = _eval(r, Pa, Ua, Ya, Ca, dtype, axis_aligned=axis)
            _assert_reached(r, cfg, li, axis=max(axis, 0))
        dp = np.abs(res[1]["psi"] - res[-1]["psi"]) / np.abs(res[-1]["psi"])
        dg = np.abs(res[1]["grad"] - res[-1]["grad"]).max(axis=1) / np.maximum(1.0, np.abs(res[-1]["grad"]).max(axis=1))
        assert np.isfinite(res[1]["grad"]).all() and (dp <= tp).all() and (dg <= tg).all(), (r.id, dp, dg)
        line += f"; members psi {dp.max():.1e} grad {dg.max():.1e}"
    print(f"[census] {r.id}: {line}")


# ---- solves -----------------------------------------------------------------------------------------------------------------------------
_ORACLE64 = {}


def _oracle64(dims, peds, rotated):
    key = (dims, peds, rotated)
    if key not in _ORACLE64:
        P = kc.solve_batch(dims, peds, rotated).astype(np.float64)
        _ORACLE64[key] = oracle.solve_batch(oracle.Problem(*dims), oracle.Options(**SHORT_ORACLE), P, nthreads=HOST_THREADS)
    return _ORACLE64[key]


def _solve(r, P, dtype, axis=None, **ov):
    cfg = _cfg(r, **ov)
    with nm.Handle(cfg) as h:
        out = h.solve(P, dtype=dtype)
        li = h.last_launch_info()
    _assert_reached(r, cfg, li, out["info"], axis=axis)
    assert np.isfinite(out["U"]).all(), r.id
    return out


def _hold64(r, got, U_ref, inner_ref, what):
    du = np.abs(got["U"] - U_ref).max(axis=1)
    print(f"[census] {r.id} {what}: du median {np.median(du):.1e} max {du.max():.1e}")
    assert np.array_equal(got["iters"][:, 1], inner_ref), (r.id, what)
    assert np.median(du) < 1e-7 and du.max() < 50 * 1e-7, (r.id, what, np.median(du), du.max())


def _hold32(r, got, ref, twin, what):
    """The "exact paths" bars of test_gpu_fp32_paths.py: `got` (a kernel's result) against `ref` = (U, record) with `twin` as the floor."""
    (Uo, ro), (Ut, rt) = ref, twin
    hip = paths._as_record(got)
    same, tw = paths._same_counts(hip, ro), paths._same_counts(rt, ro)
    du, du_t = paths._du(got["U"], Uo), paths._du(Ut, Uo)
    floor = ~tw | (du_t > 1e-3)
    near = same & ~floor
    q90, q90_t = np.quantile(du[same], 0.9), np.quantile(du_t[tw], 0.9)
    print(f"[census] {r.id} {what}: same {same.sum()}/{same.size} (twin {tw.sum()}, floor {floor.sum()}) du q90 {q90:.1e} max {du[near].max():.1e}; twin q90 {q90_t:.1e}")
    assert floor.sum() <= 1, (r.id, what, "the twin alone leaves more than one instance out")
    bad = np.flatnonzero(~same)
    assert bad.size <= 1 and floor[bad].all(), (r.id, what, {k: (hip[k][bad[:4]], ro[k][bad[:4]]) for k, _ in paths.COUNTS})
    assert q90 <= max(1e-4, 2 * q90_t), (r.id, what, q90, q90_t)
    assert du[near].max() <= 5e-3, (r.id, what, du[near].max())


def _run_solve_row(r):
    N, _, _, Ndyn = r.dims
    v = _assert_layout(r, _cfg(r))
    _, _, member = kc.universe()[r.kernel]
    pair = v.pair and member == 2
    P = kc.solve_batch(r.dims, r.obstacles, r.rotated)
    assert P.shape[0] == 5 * kc.PER_FAMILY and kc._rotated(P, nm.scenarios.ParamLayout(*r.dims)) == r.rotated
    if r.elem == 8:
        Uo, ro = _oracle64(r.dims, r.obstacles, r.rotated)
        _hold64(r, _solve(r, P.astype(np.float64), np.float64, **SHORT), Uo, ro["inner_iters"], "1x3")
        if pair:
            Pa = kc.solve_batch(r.dims, r.obstacles, False).astype(np.float64)
            a, g = (_solve(r, Pa, np.float64, axis=max(axis, 0), axis_aligned=axis, **SHORT) for axis in (1, -1))
            _hold64(r, a, g["U"], g["iters"][:, 1], "members 1x3")
        return
    for outer, inner in paths.EXACT_PATHS:
        it = dict(max_outer_iterations=outer, max_inner_iterations=inner)
        key = ("census", r.obstacles, kc.PER_FAMILY, r.rotated)
        ref, twin = (paths._oracle(N, Ndyn, P, key, t, max_outer=outer, max_inner=inner) for t in (False, True))
        _hold32(r, _solve(r, P, np.float32, **it), ref, twin, f"{outer}x{inner}")
    if pair:
        outer, inner = paths.EXACT_PATHS[-1]
        Pa = kc.solve_batch(r.dims, r.obstacles, False)
        a, g = (_solve(r, Pa, np.float32, axis=max(axis, 0), axis_aligned=axis, max_outer_iterations=outer, max_inner_iterations=inner) for axis in (1, -1))
        key = ("census", r.obstacles, kc.PER_FAMILY, False)
        (Uo, ro), (Ut, rt) = (paths._oracle(N, Ndyn, Pa, key, t, max_outer=outer, max_inner=inner) for t in (False, True))
        # the members against each other, with the oracle against its twin on this batch as the floor
        du_t = paths._du(Ut, Uo)
        tw = paths._same_counts(rt, ro)
        floor = ~tw | (du_t > 1e-3)
        du, same = paths._du(a["U"], g["U"]), paths._same_counts(paths._as_record(a), paths._as_record(g))
        near = same & ~floor
        print(f"[census] {r.id} members {outer}x{inner}: same {same.sum()}/{same.size} du q90 {np.quantile(du[same], 0.9):.1e} max {du[near].max():.1e}; "
              f"twin q90 {np.quantile(du_t[tw], 0.9):.1e}")
        bad = np.flatnonzero(~same)
        assert floor.sum() <= 1 and bad.size <= 1 and floor[bad].all(), (r.id, "members", bad)
        assert np.quantile(du[same], 0.9) <= max(1e-4, 2 * np.quantile(du_t[tw], 0.9)) and du[near].max() <= 5e-3, (r.id, "members")


# ---- traces ---------------------------------------------------------------------------------------------------------------------------------
def _run_trace_row(r):
    cfg = _cfg(r, reg_table=-1, **SHORT)
    v = _assert_layout(r, cfg)
    assert (cfg.latency_waves, cfg.coop_waves, cfg.reg_table) == (1, 1, -1)
    i = 2 * kc.PER_FAMILY                     # the first instance of the "oncoming" family: pedestrians on the path
    p = kc.solve_batch(r.dims, r.obstacles, r.rotated)[i].astype(np.float64)
    with nm.Handle(cfg) as h:
        t = h.solve_trace(p)
    with nm.Handle(cfg) as h:
        s = h.solve(p[None])
        li = h.last_launch_info()
    assert li["family"] == "throughput" and li["axis_aligned"] == -1 and (s["info"][:, 7] == 0).all(), (r.id, li)
    assert np.array_equal(t["U"], s["U"][0]) and t["status"] == s["status"][0] and np.array_equal(t["iters"], s["iters"][0]), r.id
    # U is not the last record's u itself: the inner solve ends with u <- u_half (the epilogue of OpEn's PANOCOptimizer::solve,
    # which the oracle's trace shows too), the projected gradient step from the last iterate with that record's gamma and
    # penalty. Held here with the oracle's gradient at the kernel's own last iterate, to the evaluation bar of the fp64 rows.
    pr = oracle.Problem(*r.dims)
    last, gamma, c = t["Ut"][-1], t["head"][-1, 6], t["head"][-1, 14]
    g = oracle.psi(pr, last, c, np.zeros(2 * cfg.N_hor), p)[1]
    half = last - gamma * g
    half[0::2], half[1::2] = np.clip(half[0::2], cfg.lin_vel_min, cfg.lin_vel_max), np.clip(half[1::2], -cfg.ang_vel_max, cfg.ang_vel_max)
    d_half = np.abs(half - t["U"]).max()
    assert d_half <= gamma * 1e-10 * max(1.0, np.abs(g).max()) + 4 * np.finfo(float).eps * np.abs(half).max(), (r.id, d_half, gamma)
    assert not np.array_equal(last, t["U"]), r.id                     # (the step is not empty on these instances)
    # One record per completed step of the inner loop: the inner iterations, plus one for an inner solve that ran into
    # max_inner_iterations (its last step is taken but not counted -- the identity of tests/test_solver_count_identities_cpu.py,
    # which the oracle's trace obeys too). A 1 x 3 solve that is cut off has 3 inner iterations and 4 records.
    steps = np.bincount(t["head"][:, 0].astype(int), minlength=2)
    capped = int((steps == cfg.max_inner_iterations + 1).sum())
    assert t["head"].shape[0] == t["iters"][1] + capped and np.array_equal(t["head"][:, 1], np.arange(t["head"].shape[0])), (r.id, t["head"][:, :2], t["iters"])
    _, _, res, ho, Uto = oracle.solve_trace(pr, oracle.Options(**SHORT_ORACLE), p)
    assert len(ho) == t["head"].shape[0] and np.array_equal(t["head"][:, :5], ho[:, :5]), (r.id, t["head"][:, :5], ho[:, :5])
    Uo, ro = _oracle64(r.dims, r.obstacles, r.rotated)
    du = np.abs(t["U"] - Uo[i]).max()
    print(f"[census] {r.id}: du {du:.1e}, half step {d_half:.1e}, {t['head'].shape[0]} records for {t['iters'][1]} inner iterations")
    assert t["iters"][1] == ro["inner_iters"][i] == res["inner_iters"] and du < 1e-7 and np.abs(t["Ut"] - Uto).max() < 1e-7, (r.id, du)
    assert v.family == kc.TRACE


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_census_row(row):
    {"eval": _run_eval_row, "solve": _run_solve_row, "trace": _run_trace_row}[row.entry](row)
