"""The throughput kernels' solver state across the evaluation boundary, against the tail member, bit for bit.

The fp32 one-wavefront kernels keep the solver's per-lane vectors (u, g, u_half, gamma*fpr, direction, gradient step,
previous gradient, the L-BFGS old point) in home slots in LDS: a phase stores what it produces and loads what it reads, and
only the evaluation's own argument crosses the evaluation in registers (csrc/nmpc_device.h, solve_instance, HOME). A slip in
that bookkeeping -- a phase reading a slot that an earlier phase did not bring up to date -- is a wrong VALUE, not a
rounding difference, and it shows only on the path that takes the stale slot.

The witness is the latency family's tail member (``batch_invariant = 1``, four wavefronts, csrc/nmpc_spec.h): its own copy of
the state machine, its vectors in registers, the throughput kernels' evaluation -- it returns their bits. Every case compares
U, y, cost, status, iters and info[:, :6] of the throughput kernel (``latency_waves = 1``) with it bit for bit, after
asserting from the returned counts that the path the case is about was taken.

Count identities (tests/test_solver_count_identities_cpu.py holds them against the oracle's iteration trace). With
``outer``, ``inner`` = iters, ``points`` = info[4], ``grads`` = info[5], ``ncap`` = inner solves that ran into
max_inner_iterations (they complete one step more than they count), per solve:
    rejected line-search candidates = grads - inner - 2 outer - ncap     (>= grads - inner - 3 outer)
    Lipschitz halvings              = (points - grads) - inner - outer - ncap   (>= points - grads - inner - 2 outer)
("Cost-only evaluations exceed inner + outer" alone holds without a single halving once an inner solve runs into its cap;
the bound with 2 outer implies it.)

Every case runs at all four shapes: the axis-aligned and the general 14-slot member, the 6-slot and the 4-slot axis-aligned
member. fp64 and the cooperative kernels park and unpark all vectors as before, and so does the general member of the 6-slot
pair: no case for them here. The LDS- and global-table fp32 kernels took the home slots too; they have no tail member to
witness them and rest on the parity tests of the suite (tests/test_gpu_fp32_paths.py: tp-lds, tp-glb, tp-n22 .. tp-n33).
"""
import numpy as np
import pytest

import dyobav_mpcnwta_warehouse_amd as nm

pytestmark = pytest.mark.gpu

B = 96
# id -> (N, Ndyn, provisioned rows, (n_ped, n_hyp), every other instance's ellipses turned, register slots)
SHAPES = {
    "n20-40rows-axis": (20, 40, 40, (4, 10), False, 14),
    "n20-40rows-turned": (20, 40, 40, (4, 10), True, 14),
    "n20-15rows": (20, 40, 15, (3, 5), False, 6),
    "n12-12rows": (12, 40, 12, (2, 6), False, 4),
}
CAPS = dict(max_inner_iterations=40, max_outer_iterations=3)

_BATCHES = {}


def _batch(shape, family, n=B):
    """Seeded make_batch as in tests/test_gpu_fp32_paths.py: pedestrians with unequal radii, optionally turned."""
    key = (shape, family, n)
    if key not in _BATCHES:
        N, Ndyn, _, (n_ped, n_hyp), rotate, _ = SHAPES[shape]
        lay = nm.scenarios.ParamLayout(N, 10, 10, Ndyn)
        P = nm.scenarios.make_batch(n, lay, seed=70 + N, n_ped=n_ped, n_hyp=n_hyp, ped_mode=family)
        rng = np.random.default_rng(170 + N)
        od = P[:, lay.od:lay.od + 6 * (N + 1) * Ndyn].reshape(n, Ndyn, N + 1, 6)
        act = np.abs(od[..., 2]).sum(axis=2) > 0
        od[..., 3] *= rng.uniform(0.6, 1.6, od[..., 3].shape)
        if rotate:
            ang = np.where(act[..., None], rng.uniform(-1.2, 1.2, od[..., 4].shape), 0.0)
            od[::2, ..., 4] = ang[::2]
        _BATCHES[key] = np.ascontiguousarray(P, dtype=np.float32)
    return _BATCHES[key]


def _cfg(shape, witness, **ov):
    N, Ndyn, hint, _, rotate, slots = SHAPES[shape]
    cfg = nm.default_config_struct()
    cfg.N_hor, cfg.Ndynobs, cfg.max_active_dynobs = N, Ndyn, hint
    cfg.axis_aligned = -1 if rotate else 1
    cfg.coop_waves = 1
    cfg.staged = cfg.tail_latency = -1
    if witness:
        cfg.latency_waves, cfg.batch_invariant = 4, 1
    else:
        cfg.latency_waves = 1
    for k, v in ov.items():
        assert hasattr(cfg, k), k
        setattr(cfg, k, v)
    assert nm.layout_info(cfg).reg_slots_f32 == slots, shape
    return cfg


def _solve(shape, witness, P, warm=None, **ov):
    with nm.Handle(_cfg(shape, witness, **ov)) as h:
        r = h.solve(P, **(warm or {}))
        li = h.last_launch_info()
    # the kernel the side is meant to run, and no other: info[7] = wavefronts per instance where the latency family solved it
    assert li["family"] == ("latency" if witness else "throughput"), (shape, li)
    assert li["axis_aligned"] == (0 if SHAPES[shape][4] else 1), (shape, li)
    if witness:
        assert (r["info"][:, 7] == 4).all(), np.unique(r["info"][:, 7])
    return r, li


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(r, w, what):
    for k in ("U", "y", "cost", "status", "iters"):
        assert np.array_equal(_bits(r[k]), _bits(w[k])), (what, k, int((_bits(r[k]) != _bits(w[k])).sum()))
    assert np.array_equal(_bits(r["info"][:, :6]), _bits(w["info"][:, :6])), (what, "info")


def _counts(r):
    outer, inner = r["iters"][:, 0].astype(int), r["iters"][:, 1].astype(int)
    points, grads = r["info"][:, 4].astype(int), r["info"][:, 5].astype(int)
    return outer, inner, points, grads


def _assert_contract_paths(r, what):
    """Candidates rejected (on most instances more than once per outer iteration) and some Lipschitz halvings."""
    outer, inner, points, grads = _counts(r)
    rejected_lb = grads - inner - 3 * outer
    halvings_lb = (points - grads) - inner - 2 * outer
    print(what, "rejected >=", np.percentile(rejected_lb, (0, 50, 100)), "halvings >=", np.percentile(halvings_lb, (0, 50, 100)))
    assert (rejected_lb > 0).mean() > 0.5, (what, rejected_lb)
    assert (halvings_lb > 0).any(), (what, halvings_lb)
    assert ((points - grads) > inner + outer).any()          # (implied by the one above)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_contract_family_with_rejected_candidates_and_lipschitz_halvings(shape):
    P = _batch(shape, "toward_robot")
    r, _ = _solve(shape, False, P, **CAPS)
    _assert_contract_paths(r, shape)
    w, _ = _solve(shape, True, P, **CAPS)
    _same(r, w, shape)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_passing_family_inner_solves_end_on_the_tolerance(shape):
    """Default caps. An inner solve that ends by its exit test leaves through the step head's u <- u_half epilogue, and each
    starts with the iteration without a line search."""
    P = _batch(shape, "passing")
    r, _ = _solve(shape, False, P)
    outer, inner, points, grads = _counts(r)
    cap = nm.default_config_struct().max_inner_iterations
    on_tolerance = (r["status"] == 0) & (inner < cap)          # (no inner solve of the instance can have run into the cap)
    print(shape, "converged", (r["status"] == 0).mean(), "all inner solves on the tolerance", on_tolerance.mean())
    assert on_tolerance.sum() >= B // 4, (shape, on_tolerance.sum())  # (the fp32 oracle: 36 .. 50 of the 96 per shape)
    assert (grads >= 2 * outer + inner).all() and (outer[on_tolerance] >= 1).all()
    w, _ = _solve(shape, True, P)
    _same(r, w, shape)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_evaluation_budget_cuts_behind_every_kind_of_evaluation(shape):
    """max_evaluations = 30 .. 61: the budget is found exhausted behind a completed step or an outer iteration, whatever kind
    of evaluation used it up, and the exit reads its vectors from their home slots."""
    P = _batch(shape, "toward_robot", 32)
    last_points, last_grads, grad_steps, cost_steps = None, None, 0, 0
    for E in range(30, 62):
        r, _ = _solve(shape, False, P, max_evaluations=E)
        outer, inner, points, grads = _counts(r)
        cut = r["status"] == 2
        assert cut.any() and (points[cut] >= E).all(), (shape, E, r["status"], points)
        if last_points is not None:
            both = cut & last_cut
            grad_steps += int((grads[both] > last_grads[both]).sum())
            cost_steps += int(((points - grads)[both] > (last_points - last_grads)[both]).sum())
        last_points, last_grads, last_cut = points, grads, cut
        w, _ = _solve(shape, True, P, max_evaluations=E)
        _same(r, w, (shape, E))
    # the cut moved past gradient evaluations and past cost-only evaluations as the budget grew
    assert grad_steps > 0 and cost_steps > 0, (grad_steps, cost_steps)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_warm_start(shape):
    P = _batch(shape, "toward_robot")
    first, _ = _solve(shape, False, P, **CAPS)
    warm = dict(u0=first["U"], y0=first["y"], c0=first["info"][:, 3].copy())
    r, _ = _solve(shape, False, P, warm=warm, **CAPS)
    assert not np.array_equal(r["U"], first["U"])               # (the second solve went on from where the first stopped)
    outer, inner, points, grads = _counts(r)
    assert (grads - inner - 3 * outer > 0).any()
    w, _ = _solve(shape, True, P, warm=warm, **CAPS)
    _same(r, w, shape)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_two_stage_plan_with_the_tail_handoff_forced(shape):
    """staged = 1 and tail_latency as in tests/test_gpu_tail.py: the pilot parks at the first outer boundary, the resumed
    launch hands its drain phase to the tail member -- at outer boundaries and inside inner solves (deep parks), where every
    home slot has to be current before the copy to global memory. 19 is the largest threshold B = 96 admits."""
    P = _batch(shape, "toward_robot")
    w, _ = _solve(shape, True, P, **CAPS)
    handed = deep = 0
    for thr in (19, 12, 6):
        r, li = _solve(shape, False, P, staged=1, tail_latency=thr, **CAPS)
        print(shape, thr, li)
        assert li["staged_outer_iterations"] == 1 and li["tail_handed_off"] == thr, li
        _same(r, w, (shape, thr))
        handed += int((r["info"][:, 7] > 0).sum())
        deep += li["deep_parked"]
    assert handed > 0 and deep > 0, (handed, deep)
