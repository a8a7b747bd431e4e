"""A solve does not depend on what its handle ran before. nmpc_handle_s (csrc/nmpc_capi.hip) carries bucket counters, the
hand-off's counters, the axis flag and its epoch, grow-only buffers shared by float and double solves, staging buffers, a
dispatch order, the polish's selection and the launch record from call to call ("The handle's state between
calls"). The product keeps one handle for a whole run -- the batch shrinks across the thresholds of plan_solve, fp32 solves,
the fp64 polish, evaluations and the predictor kernels alternate -- while every other device test asks one question of a
brand-new handle. Here a call on a handle with a history must equal, bit for bit, the same call on a handle just created with
the same configuration: U, y, cost, status, iters, info[:, :6] with NaNs equal and the timing-independent fields of
nmpc_last_launch_info (tests/handle_history.py: compare). The reference is always the fresh handle, and every reference is
first shown to reproduce on a second fresh handle.

Every call here is a legal call. Measured on an MI355X: see HISTORY.md ("One handle through a history of calls")."""
import numpy as np
import pytest
import torch

import dyobav_mpcnwta_warehouse_amd as nm
import handle_history as hh
from plan_cases import LAY, PLAN_IDS, n_simd, plan_batch, plan_cfg, plans

pytestmark = pytest.mark.gpu

SMALLEST, TAIL, LARGEST = PLAN_IDS.index("fp64-pilot"), PLAN_IDS.index("throughput-evaluation-order-tail"), PLAN_IDS.index("throughput-pilot-tail")


def fresh(cfg, fn, what, compare=hh.compare):
    """fn(handle) -> (result arrays, launch info or None) on a fresh handle of cfg. The precondition of every comparison: a
    second fresh handle returns the same bits."""
    with nm.Handle(cfg) as h:
        a = fn(h)
    with nm.Handle(cfg) as h:
        b = fn(h)
    compare(b, a, f"two fresh handles: {what}")
    return a


class _Lazy(dict):
    def __init__(self, make):
        super().__init__()
        self.make = make

    def __missing__(self, key):
        self[key] = self.make(key)
        return self[key]


# the tour's ten batches and their fresh-handle references: made once, on first use, shared by the tests, never written to
BATCHES = _Lazy(lambda v: hh.tour_batch(*v))
REFS = _Lazy(lambda v: fresh(plan_cfg(), lambda h: hh.call(h, BATCHES[v]), f"{PLAN_IDS[v[0]]}/{v[1]}"))


def _want():
    return {i: w for i, (_, _, _, w, _) in enumerate(plans())}


def _equal(got, want, what):
    """Every array of two result dicts (evaluations, traces) bit for bit, NaNs equal."""
    assert set(got) == set(want)
    for k in want:
        d = hh.differing(got[k], want[k])
        assert d == 0, f"{what}: {k} differs from the fresh handle's in {d} of {len(np.atleast_1d(want[k]))} rows"


def _equal_with_info(got, want, what):
    _equal(got[0], want[0], what)
    assert got[1] == want[1], (what, got[1], want[1])


# ---- a. the plan tour, host arrays ------------------------------------------------------------------------------------------
def test_plan_tour_on_one_handle_equals_fresh_handles():
    """All 25 ordered pairs of the five plans on ONE handle, cold starts from host arrays (Handle.solve passes a zeroed y without
    y_is_input: stale multipliers in the staging buffer dy would show), batches a / b alternating per plan."""
    visits = hh.tour(5)
    assert {(a[0], b[0]) for a, b in hh.pairs(visits)} == {(i, j) for i in range(5) for j in range(5)}
    for v in sorted(set(visits)):                                   # the references first: the handle under test runs back to back
        assert REFS[v][1]["axis_aligned"] == (2 if v[0] != PLAN_IDS.index("fp64-pilot") else -1), (v, REFS[v][1])
    print("SIMDs:", n_simd(), "batch sizes (a, b) per plan:", hh.tour_sizes())
    rotated = BATCHES[(TAIL, "b")]
    assert (rotated[::7, LAY.od + (3 * (LAY.N + 1)) * 6 + 4] == np.float32(0.4)).all() and (BATCHES[(TAIL, "a")][:, LAY.od + 4::6][:, :15 * 21] == 0).all()
    with nm.Handle(plan_cfg()) as h:
        hh.run_tour(h, visits, REFS, BATCHES, want=_want(), fresh=lambda: nm.Handle(plan_cfg()), names=PLAN_IDS)


# ---- b. the same, the way the closed loop calls ------------------------------------------------------------------------------
FP32_PLANS = [i for i, (_, dtype, _, _, _) in enumerate(plans(1024)) if dtype == np.float32]


@pytest.mark.parametrize("optional", [True, False], ids=["every-array", "status-info-y-left-out"])
def test_fp32_plan_tour_back_to_back_on_device_tensors(optional):
    """Every pair among the fp32 plans (latency, two-wavefront, throughput with tail, throughput with pilot and tail) through
    solve_raw with device tensors, sync = False, on torch's current stream, no host synchronisation between the calls. The
    plans come in ascending batch size first, so that the grow-only buffers are re-reserved while earlier work is queued. The
    outputs are ONE set of tensors, poisoned before each call: status = -1 (the in-progress marker that the ranking trusts),
    NaN in U, cost, info and y (no y_is_input: a cold start that read y would project the NaNs on a bound of the multipliers' box
    and differ in every instance), 0x7fffffff in iters. Results are
    copied aside on the stream and compared after one synchronise. Once more with status, info and y left out: the handle's
    own dstatus stands in, holding the previous call's statuses."""
    assert FP32_PLANS == [0, 1, 2, 3]
    sizes = [hh.tour_sizes()[i][0] for i in FP32_PLANS]
    assert sizes == sorted(sizes)
    visits = hh.with_batches(FP32_PLANS + [p for p, _ in hh.tour(len(FP32_PLANS))])
    assert {(a[0], b[0]) for a, b in hh.pairs(visits)} == {(i, j) for i in FP32_PLANS for j in FP32_PLANS}
    for v in sorted(set(visits)):
        REFS[v]
    n, stream = 2 * LAY.N, torch.cuda.Stream()
    kept = []
    with torch.cuda.stream(stream), nm.Handle(plan_cfg()) as h:
        dev = {v: torch.from_numpy(BATCHES[v]).cuda() for v in sorted(set(visits))}
        Bmax = max(len(p) for p in dev.values())
        f32 = dict(dtype=torch.float32, device="cuda")
        out = dict(U=torch.empty((Bmax, n), **f32), cost=torch.empty(Bmax, **f32), y=torch.empty((Bmax, n), **f32), info=torch.empty((Bmax, 8), **f32),
                   status=torch.empty(Bmax, dtype=torch.int32, device="cuda"), iters=torch.empty((Bmax, 2), dtype=torch.int32, device="cuda"))
        passed = [k for k in out if optional or k not in ("status", "info", "y")]
        stream.synchronize()
        h.set_stream(stream.cuda_stream)
        for v in visits:
            B = len(dev[v])
            for k, t in out.items():
                t.fill_(-1 if k == "status" else 0x7fffffff if k == "iters" else float("nan"))
            a = {k: (out[k] if k in passed else None) for k in out}
            h.solve_raw(np.float32, dev[v], B, a["U"], a["cost"], a["status"], a["iters"], None, a["y"], False, None, a["info"], sync=False)
            kept.append({k: out[k][:B].clone() for k in passed})
        stream.synchronize()
        host = [{k: t.cpu().numpy() for k, t in r.items()} for r in kept]
    prev = None
    for pos, (v, r) in enumerate(zip(visits, host)):
        what = f"visit {pos} of {len(visits)}: {PLAN_IDS[v[0]]}/{v[1]} after {prev and PLAN_IDS[prev[0]] + '/' + prev[1]}"
        hh.compare((r, None), ({k: REFS[v][0][k] for k in passed}, None), what)
        prev = v


# ---- c. a caller's dispatch order does not outlive its use ---------------------------------------------------------------------
def test_dispatch_order_is_applied_ignored_applied_again_and_cleared():
    P, other = BATCHES[(TAIL, "a")], BATCHES[(0, "b")]
    B = len(P)
    order = np.random.default_rng(5).permutation(B).astype(np.int32)
    park = plans()[TAIL][3]["tail_handed_off"]

    def ordered(h):
        h.set_dispatch_order(order)
        return hh.call(h, P)
    ref_ordered = fresh(plan_cfg(), ordered, "under the caller's order")
    # one throughput launch in the caller's order from scratch (dyn_init_kernel sets the hand-off's counters) + the tail launch
    assert ref_ordered[1]["order_source"] == 1 and ref_ordered[1]["tail_handed_off"] == park > 0 and ref_ordered[1]["staged_outer_iterations"] == 0
    hh.compare((ref_ordered[0], None), (REFS[(TAIL, "a")][0], None), "the caller's order changes no value")
    with nm.Handle(plan_cfg()) as h:
        hh.compare(ordered(h), ref_ordered, "1: the order applied")
        got = hh.call(h, other)
        assert got[1]["order_source"] != 1, got[1]
        hh.compare(got, REFS[(0, "b")], "2: another size, the order ignored")
        hh.compare(hh.call(h, P), ref_ordered, "3: the first size again, the order applied again")
        h.set_dispatch_order(None)
        got = hh.call(h, P)
        assert got[1]["order_source"] == 2, got[1]
        hh.compare(got, REFS[(TAIL, "a")], "4: the order cleared, the plan of a fresh handle")


# ---- d. both element types through one workspace ---------------------------------------------------------------------------------
def _trace(h, p):
    r = h.solve_trace(p)
    return {k: np.atleast_1d(r[k]) for k in ("U", "y", "status", "iters", "head", "Ut")} | {"info": r["info"][:6]}


@pytest.mark.parametrize("kernels", ["automatic", "one-wavefront"])
def test_float_and_double_solves_share_one_workspace(kernels):
    """N = 40 with 160 obstacle rows (tests/test_gpu_coop.py): the fp64 layout streams the obstacle table through the
    workspace dws -- B * ws_stride doubles, of which nmpc_solve_trace_f64 reserves one instance's worth in the same buffer --
    while fp32 runs the on-chip cooperative kernel (info[:, 7] = -8 / -4). With latency_waves = coop_waves = 1 and reg_table = -1
    the one-wavefront global-table kernels run in both types, and float and double tables follow each other in dws. The second
    fp64 batch is smaller, holds other instances and a rotated ellipse: the general table (9 values per entry) overwrites the
    compressed one (5 per entry) and the other way round."""
    lay = nm.scenarios.ParamLayout(N=40, Ndyn=160)
    P = nm.scenarios.make_batch(9, lay, seed=61, n_ped=8, n_hyp=20, ped_mode="oncoming")
    P6, P3 = P[:6].copy(), hh.rotate_every_seventh(P[6:].copy(), lay)
    cfg = nm.default_config_struct()
    cfg.N_hor, cfg.Ndynobs = 40, 160
    cfg.max_outer_iterations, cfg.max_inner_iterations = 2, 8
    if kernels == "one-wavefront":
        cfg.latency_waves, cfg.coop_waves, cfg.reg_table = 1, 1, -1
    info = nm.layout_info(cfg)
    assert info.global_table_f64 and info.ws_elems_f64 > 0
    steps = [("f64 B = 6", lambda h: hh.call(h, P6)), ("f32 B = 6", lambda h: hh.call(h, P6.astype(np.float32))),
             ("f64 B = 3, other instances, rotated", lambda h: hh.call(h, P3)), ("trace", lambda h: (_trace(h, P3[1]), None)),
             ("f64 B = 6 again", lambda h: hh.call(h, P6))]
    refs = [fresh(cfg, fn, name, _equal_with_info if name == "trace" else hh.compare) for name, fn in steps[:4]]
    refs.append(refs[0])
    if kernels == "automatic":
        assert (refs[0][0]["info"][:, 7] == -4).all() and (refs[1][0]["info"][:, 7] == -8).all() and refs[0][1]["family"] == "cooperative"
        assert refs[0][1]["axis_aligned"] == 2 and refs[2][1]["axis_aligned"] == 2
    else:
        assert (refs[0][0]["info"][:, 7] >= 0).all() and refs[0][1]["family"] == "throughput" and refs[1][1]["family"] == "throughput"
    assert not np.array_equal(refs[0][0]["U"][:3], refs[2][0]["U"])             # (other instances)
    with nm.Handle(cfg) as h:
        for (name, fn), ref in zip(steps, refs):
            got = fn(h)
            if name == "trace":
                _equal(got[0], ref[0], name)
            else:
                hh.compare(got, ref, name)


def test_staged_cooperative_plan_between_other_solves():
    """The resumable solve of the cooperative kernels (kCoopStageFills fills; fp64 on the tour's dimensions with coop_waves = 4:
    from B = 2 S on, tests/test_handle_history_cpu.py) parks every instance in dresume after one outer iteration and ranks
    them: behind an fp32 solve that left float states there, ahead of a smaller unstaged one, and once more."""
    S = n_simd()
    cfg = plan_cfg(coop_waves=4)
    staged = plan_batch(2 * S, np.float64, seed=520)
    unstaged = hh.rotate_every_seventh(plan_batch(2 * S - hh.ODD, np.float64, seed=522), LAY)
    f32 = BATCHES[(1, "a")]                                         # (2 S floats: the two-wavefront plan, order from one evaluation)
    steps = [("f32", f32), ("staged", staged), ("unstaged", unstaged), ("staged again", staged)]
    refs = {name: fresh(cfg, lambda h, P=P: hh.call(h, P), name) for name, P in steps[:3]}
    refs["staged again"] = refs["staged"]
    li = refs["staged"][1]
    assert li["family"] == "cooperative" and li["staged_outer_iterations"] == 1 and li["order_source"] == 3, li
    assert refs["unstaged"][1]["family"] == "cooperative" and refs["unstaged"][1]["staged_outer_iterations"] == 0
    assert (refs["staged"][0]["info"][:, 7] == -4).all()
    with nm.Handle(cfg) as h:
        for name, P in steps:
            hh.compare(hh.call(h, P), refs[name], name)


# ---- e. the polish -----------------------------------------------------------------------------------------------------------
def test_polish_selection_of_the_previous_call_is_not_reused():
    """polish = 1: psel, the compact fp64 copies pP .. pinfo and host_sel / host_status hold the previous call's selection."""
    cfg = plan_cfg(polish=1)
    big = plan_batch(384, np.float32, seed=540)
    small = hh.rotate_every_seventh(plan_batch(384 - hh.ODD - 128, np.float32, seed=542), LAY)
    refs = {"big": fresh(cfg, lambda h: hh.call(h, big), "big"), "small": fresh(cfg, lambda h: hh.call(h, small), "small")}
    nb, ns = refs["big"][1]["polish_selected"], refs["small"][1]["polish_selected"]
    assert 0 < ns < nb < 384 and (refs["big"][0]["info"][:, 6] >= 1).sum() == nb, (nb, ns)     # (info[:, 6]: the polish's outcome per instance)
    with nm.Handle(cfg) as h:
        for name, P in (("big", big), ("small", small), ("big", big)):
            hh.compare(hh.call(h, P), refs[name], f"polish, {name}")


# ---- f. other entry points in between --------------------------------------------------------------------------------------------
def _eval_inputs(dtype, B=64):
    P = BATCHES[(0, "b")][:B]                                       # (rotated ellipses in every seventh instance)
    rng = np.random.default_rng(9)
    U = np.stack([rng.uniform(0.2, 1.2, (B, LAY.N)), rng.uniform(-0.3, 0.3, (B, LAY.N))], axis=2).reshape(B, 2 * LAY.N)
    return P.astype(dtype), U.astype(dtype), rng.normal(size=(B, 2 * LAY.N)).astype(dtype), rng.uniform(1, 100, B).astype(dtype)


def test_other_entry_points_between_two_solves_change_nothing():
    import mmp_block_reference as br
    import test_gpu_mmp_block as tmb
    v = (SMALLEST, "a")
    P = BATCHES[v]
    ev32 = fresh(plan_cfg(), lambda h: (h.eval(*_eval_inputs(np.float32)), h.last_launch_info()), "eval f32", _equal_with_info)
    ev64 = fresh(plan_cfg(), lambda h: (h.eval(*_eval_inputs(np.float64)), h.last_launch_info()), "eval f64", _equal_with_info)
    x, spec, want, bound = br.case("random", *br.PLANES[0], *br.CHANNELS[0])
    ts = torch.cuda.current_stream()
    with nm.Handle(plan_cfg()) as h:
        hh.compare(hh.call(h, P), REFS[v], "first solve")
        for dtype, ref in ((np.float32, ev32), (np.float64, ev64)):
            _equal(h.eval(*_eval_inputs(dtype)), ref[0], f"eval {np.dtype(dtype)} behind a solve")
            assert h.last_launch_info() == ref[1]
        U = np.full((4, 2 * LAY.N), 7.0, np.float32)
        h.solve_raw(np.float32, P.astype(np.float32), 0, U)         # B = 0: nothing is launched, nothing is written
        assert (U == 7.0).all()
        for refused in (dict(P=P.astype(np.float32), B=-1), dict(P=None, B=4)):
            with pytest.raises(nm.NmpcError):
                h.solve_raw(np.float32, refused["P"], refused["B"], U)
        assert (U == 7.0).all()
        h.selftest()
        for mode in (2, 1, 0):
            h.set_pointer_mode(mode)
        h.set_stream(ts.cuda_stream)
        got = tmb._run(h, x[:1], spec)                              # one predictor launch: it shares only the stream
        assert (np.abs(got - want[:1]) <= bound[:1]).all()
        h.set_stream(None)
        ts.synchronize()
        h.set_stream(ts.cuda_stream)
        h.set_stream(None)
        hh.compare(hh.call(h, P), REFS[v], "second solve, behind eval, B = 0, refused calls, selftest, pointer modes, streams, mmp_block")


def test_eval_and_trace_behind_the_largest_solve_equal_a_fresh_handle():
    v = (LARGEST, "a")
    p = BATCHES[(SMALLEST, "b")][0]
    ev32 = fresh(plan_cfg(), lambda h: (h.eval(*_eval_inputs(np.float32)), None), "eval f32", _equal_with_info)
    ev64 = fresh(plan_cfg(), lambda h: (h.eval(*_eval_inputs(np.float64)), None), "eval f64", _equal_with_info)
    tr = fresh(plan_cfg(), lambda h: (_trace(h, p), None), "trace", _equal_with_info)
    assert len(tr[0]["head"]) > 10 and np.isfinite(ev32[0]["psi"]).all() and (ev32[0]["f2sq"] > 0).any()
    with nm.Handle(plan_cfg()) as h:
        hh.compare(hh.call(h, BATCHES[v]), REFS[v], "the largest solve")
        _equal(h.eval(*_eval_inputs(np.float32)), ev32[0], "eval f32 behind the largest solve")
        _equal(h.eval(*_eval_inputs(np.float64)), ev64[0], "eval f64 behind the largest solve")
        _equal(_trace(h, p), tr[0], "trace behind the largest solve")


# ---- g. nmpc_last_launch_info describes the last call only -----------------------------------------------------------------------
def test_launch_info_describes_the_last_call_only():
    cfg = plan_cfg(polish=1)
    tail, small = BATCHES[(TAIL, "a")], BATCHES[(0, "a")][:100]
    ref_tail = fresh(cfg, lambda h: hh.call(h, tail), "tail solve with polish")
    ref_small = fresh(cfg, lambda h: hh.call(h, small), "small solve with polish")
    ref_eval = fresh(cfg, lambda h: (h.eval(*_eval_inputs(np.float32)), h.last_launch_info()), "eval", _equal_with_info)
    lt, ls, le = ref_tail[1], ref_small[1], ref_eval[1]
    assert lt["tail_handed_off"] > 0 and lt["order_source"] == 2 and lt["polish_selected"] > ls["polish_selected"] > 0, (lt, ls)
    assert ls["tail_handed_off"] == 0 and ls["deep_parked"] == 0 and ls["staged_outer_iterations"] == 0 and ls["order_source"] == 0, ls
    assert le == dict(ls, family="throughput", polish_selected=0, axis_aligned=le["axis_aligned"]), le
    with nm.Handle(cfg) as h:
        hh.compare(hh.call(h, tail), ref_tail, "tail solve")
        got = hh.call(h, small)
        hh.compare(got, ref_small, "small solve behind a tail solve")
        assert got[1] == ls, (got[1], ls)                           # (deep_parked included: no hand-off, nothing parked)
        hh.compare(hh.call(h, tail), ref_tail, "tail solve again")
        _equal(h.eval(*_eval_inputs(np.float32)), ref_eval[0], "eval behind a tail solve")
        assert h.last_launch_info() == le, (h.last_launch_info(), le)
