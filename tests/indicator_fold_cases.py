"""Constructed batches for tests/test_gpu_indicator_fold.py and tools/record_indicator_fold.py.

The axis-aligned fp32 register-table kernels form their ellipse indicators max(0, 1 - d^T M d) with the clamp output modifier
of the second FMA (csrc/nmpc_device.h, unit_clamp_floor) and select the hard gradient's factor -2 on the penalty factor, not on
the two products. Both are meant to return the bits of the plain form. The fixtures under tests/golden/indicator_fold/ were
recorded with the plain form (the commit before the change) on an MI355X; the batches below are what they were recorded on.

Every batch has 8 instances, N = 20, Ndyn = 42 slots of which the first ``rows`` are occupied (stored row i = slot i, its
sub-lane class is i % 3, its register slot i // 3, its pair of slots i // 6). The ellipses are placed RELATIVE TO THE NOMINAL
ROLLOUT (controls (1.0, 0): 2/3 of lin_vel_max, straight ahead), so that the situations the change touches are there by
construction; ``situations`` recomputes them in float64 from the float32 inputs, and the test fails where one is missing:

  centre     under ZERO controls the robot stays at s0 bit for bit (v = 0: every RK4 increment is an exact 0), and row 1 has a
             snapshot whose centre is s0 in float32: d = 0 exactly, h = 1 -- the clamp's upper end
  outside    a step lane outside the margin-inflated ellipse (h_m < 0)
  between    a step lane between the hard and the inflated ellipse (soft term only)
  classes    a violated hard ellipse in each of the three sub-lane classes
  pairs      pair 0 (rows 0..5) has both slots violated, pair 1 (rows 6..11) exactly one
  dummies    rows behind the last one (none at 42 rows and at 12 rows of the 4-slot kernel: the full tables)
  t0         the last instance has a t = 0 hard violation (the passes run with their t = 0 half), instance 0 has no t = 0
             snapshot in reach of any step at all, and the one before the last has a t = 0 soft term without a hard violation
"""
import hashlib

import numpy as np

import dyobav_mpcnwta_warehouse_amd as nm

B, N, NDYN = 8, 20, 42
TS, V_NOM, VM, SM = 0.2, 1.0, 0.2, 0.2          # nmpc_config defaults: ts, 2/3 lin_vel_max, vehicle and social margin
EPS = 1e-3                                       # an indicator counts as > 0 / < 0 only this far from 0 (fp32 rounds at 1e-7)
# id -> (occupied rows, register slots of the fp32 kernel that takes them)
SHAPES = {"rows19": (19, 14), "rows40": (40, 14), "rows42": (42, 14), "rows12": (12, 4), "rows15": (15, 6)}
CONTROLS = ("zero", "nominal", "random1", "random2")
LAYOUT = nm.scenarios.ParamLayout(N, 10, 10, NDYN)


def nominal_positions(P):
    """[B, N + 1, 2]: the robot under the nominal controls, t = 0 .. N (w = 0: a straight line, exact in real arithmetic)."""
    s0 = P[:, LAYOUT.s0:LAYOUT.s0 + 3].astype(np.float64)
    d = np.stack([np.cos(s0[:, 2]), np.sin(s0[:, 2])], axis=1)
    return s0[:, None, :2] + (np.arange(N + 1) * TS * V_NOM)[None, :, None] * d[:, None, :]


def make_batch(shape, rotate=False):
    """P[8, np] float32 of one shape. ``rotate``: every occupied ellipse turned (the general member of the kernel pair)."""
    rows, _ = SHAPES[shape]
    P = nm.scenarios.make_batch(B, LAYOUT, seed=900 + rows, n_ped=0, n_boxes=2).astype(np.float32)
    pos = nominal_positions(P)                                             # from the float32 s0
    rng = np.random.default_rng(1900 + rows)
    od = np.zeros((B, NDYN, N + 1, 6))
    r = 0.2 + 0.05 * np.arange(N + 1)
    od[:, :rows, :, 2] = r
    od[:, :rows, :, 3] = 1.3 * r
    od[:, :rows, :, 5] = 1.0
    # default: far away, every row somewhere else
    ang = 2.0 * np.pi * np.arange(rows) / rows
    od[:, :rows, :, 0] = pos[:, None, :, 0] + 50.0 * np.cos(ang)[None, :, None]
    od[:, :rows, :, 1] = pos[:, None, :, 1] + 50.0 * np.sin(ang)[None, :, None]
    # rows 12 .. : half of the snapshots at a random place within 1.5 m of the nominal position (seeded)
    for i in range(12, rows):
        near = rng.random((B, N + 1)) < 0.5
        rho, phi = rng.uniform(0.0, 1.5, (B, N + 1)), rng.uniform(-np.pi, np.pi, (B, N + 1))
        od[:, i, :, 0] = np.where(near, pos[..., 0] + rho * np.cos(phi), od[:, i, :, 0])
        od[:, i, :, 1] = np.where(near, pos[..., 1] + rho * np.sin(phi), od[:, i, :, 1])
    s0 = P[:, LAYOUT.s0:LAYOUT.s0 + 2].astype(np.float64)
    for b in range(B):
        def put(i, t, off_x, off_y=0.0):
            od[b, i, t, 0], od[b, i, t, 1] = pos[b, t, 0] + off_x, pos[b, t, 1] + off_y
        ta, tb, tc = 3 + b % 4, 8 + b % 5, 14 + b % 6
        put(0, ta, 0.05)                       # class 0, slot 0 of pair 0: inside the hard ellipse
        put(0, tb, 0.02, -0.03)
        put(4, tb, -0.04, 0.03)                # class 1, slot 1 of pair 0: inside the hard ellipse
        put(8, tc, 0.03, 0.05)                 # class 2, slot 0 of pair 1: inside the hard ellipse
        put(10, ta, r[ta] + 0.1)               # slot 1 of pair 1: between the hard (r) and the inflated (r + 0.2) ellipse, only
        put(2, tb, r[tb] + 0.5)                # outside the inflated ellipse, close by
        od[b, 1, tc, 0], od[b, 1, tc, 1] = s0[b]   # centre = s0: h = 1 under zero controls
    # t = 0 snapshots: one position per group of three rows (the producer writes a pedestrian's current position into all of
    # its hypotheses; the 14-slot kernels merge such rows), 3 m and more from every nominal position ...
    grp = np.arange(rows) // 3
    for b in range(B):
        th = float(P[b, LAYOUT.s0 + 2])
        lat = np.array([-np.sin(th), np.cos(th)])
        for i in range(rows):
            od[b, i, 0, :2] = pos[b, 0] + (3.0 + 0.5 * grp[i]) * lat
        if b >= 1:                              # ... a soft term of group 1 at step 2 (0.45 m: hard 0.2 x 0.26, inflated 0.6 x 0.66)
            od[b, 3:6, 0, :2] = pos[b, 2] + 0.45 * lat
        if b == B - 1:                          # ... and a hard violation of group 0 at step 1
            od[b, 0:3, 0, :2] = pos[b, 1] + 0.05 * lat
    if rotate:
        od[:, :rows, :, 4] = rng.uniform(-1.2, 1.2, (B, rows, N + 1))
    P[:, LAYOUT.od:LAYOUT.od + 6 * (N + 1) * NDYN] = od.reshape(B, -1).astype(np.float32)
    return np.ascontiguousarray(P)


def controls(shape, name):
    """U[8, 2N] float32 (v, w interleaved per step, as Handle.eval takes them)."""
    rows, _ = SHAPES[shape]
    U = np.zeros((B, N, 2))
    if name == "nominal":
        U[..., 0] = V_NOM
    elif name.startswith("random"):
        rng = np.random.default_rng(2900 + rows + int(name[-1]))
        U[..., 0], U[..., 1] = rng.uniform(0.3, 1.4, (B, N)), rng.uniform(-0.3, 0.3, (B, N))
    else:
        assert name == "zero", name
    return np.ascontiguousarray(U.reshape(B, 2 * N), dtype=np.float32)


def multipliers(shape):
    """Y[8, 2N], c[8] float32 of the evaluation-level cases."""
    rng = np.random.default_rng(3900 + SHAPES[shape][0])
    return rng.normal(size=(B, 2 * N)).astype(np.float32), rng.uniform(1.0, 300.0, B).astype(np.float32)


def indicators(P):
    """float64 indicators of the occupied rows on the nominal rollout, before the max(0, .): (hp, hm, hp0, hm0), each
    [B, Ndyn, N] -- row j's own snapshot t = k + 1 and its t = 0 snapshot against the position of step lane k."""
    od = P[:, LAYOUT.od:LAYOUT.od + 6 * (N + 1) * NDYN].astype(np.float64).reshape(B, NDYN, N + 1, 6)
    pos = nominal_positions(P)[:, None, 1:, :]                              # [B, 1, N, 2]

    def ind(e, marg):
        dx, dy = pos[..., 0] - e[..., 0], pos[..., 1] - e[..., 1]
        return 1.0 - (dx / (e[..., 2] + marg + 1e-6)) ** 2 - (dy / (e[..., 3] + marg + 1e-6)) ** 2
    own, first = od[:, :, 1:, :], od[:, :, :1, :]
    return ind(own, 0.0), ind(own, VM), ind(first, 0.0), ind(first, VM + SM)


def situations(shape, P):
    """name -> bool: which of the situations of the module docstring the batch holds (axis-aligned batches)."""
    rows, slots = SHAPES[shape]
    hp, hm, hp0, hm0 = (a[:, :rows] for a in indicators(P))
    od = P[:, LAYOUT.od:LAYOUT.od + 6 * (N + 1) * NDYN].reshape(B, NDYN, N + 1, 6)
    s0 = P[:, LAYOUT.s0:LAYOUT.s0 + 2]
    on_centre = (od[:, :rows, 1:, 0] == s0[:, None, None, 0]) & (od[:, :rows, 1:, 1] == s0[:, None, None, 1])
    viol = (hp > EPS).any(axis=2)                                            # [B, rows]: the row's own snapshots
    clear = (hp < -EPS).all(axis=2) & (hp0 < -EPS).all(axis=2)
    slot_v = lambda m: viol[:, 3 * m:3 * m + 3].any(axis=1)
    slot_c = lambda m: clear[:, 3 * m:3 * m + 3].all(axis=1)
    out = {
        "centre": bool(on_centre.any()),
        "outside": bool((hm < -EPS).any()),
        "between": bool(((hp < -EPS) & (hm > EPS)).any()),
        "classes": all(bool(viol[:, c::3].any()) for c in range(3)),
        "pair_both": bool((slot_v(0) & slot_v(1)).any()),
        "pair_one": bool((slot_v(2) & slot_c(3)).any()),
        "t0_hard": bool((hp0[B - 1] > EPS).any()),
        "t0_soft_only": bool(((hm0[B - 2] > EPS).any() and (hp0[B - 2] < -EPS).all())),
        "t0_none": bool((hm0[0] < -EPS).all()),
        "dummies": rows < 3 * slots,
    }
    return out


def config(shape, plan=None, rotate=False, **ov):
    """nmpc_config of one shape. plan: None (evaluations), 'throughput' (latency_waves = 1), 'tail' (the automatic plan of
    8 instances, the latency family, with its tail member: automatic with 14 slots, batch_invariant = 1 below), 'flat' (the
    same plan with batch_invariant = -1: the latency family's own straight-line passes)."""
    rows, slots = SHAPES[shape]
    cfg = nm.default_config_struct()
    cfg.N_hor, cfg.Ndynobs, cfg.max_active_dynobs = N, NDYN, rows
    cfg.axis_aligned = -1 if rotate else 1      # (the member of the kernel pair is the caller's choice, not the device scan's)
    cfg.coop_waves = 1
    cfg.staged = cfg.tail_latency = -1
    cfg.max_inner_iterations, cfg.max_outer_iterations = 40, 3
    if plan == "throughput":
        cfg.latency_waves = 1
    elif plan == "tail":
        cfg.batch_invariant = 0 if slots == 14 else 1
    elif plan == "flat":
        cfg.batch_invariant = -1
    else:
        assert plan is None, plan
    for k, v in ov.items():
        assert hasattr(cfg, k), k
        setattr(cfg, k, v)
    assert nm.layout_info(cfg).reg_slots_f32 == slots, (shape, nm.layout_info(cfg).reg_slots_f32)
    assert (cfg.ts, cfg.vehicle_margin, cfg.social_margin, cfg.lin_vel_max) == (TS, VM, SM, 1.5 * V_NOM)
    return cfg


PLANS = ("throughput", "tail", "flat")
SOLVE_KEYS = ("U", "cost", "status", "iters", "info")


def run_all(shape, rotate=False):
    """Everything the fixture of one shape holds, computed with the loaded library: name -> array."""
    P = make_batch(shape, rotate)
    Y, Cp = multipliers(shape)
    want_axis = 0 if rotate else 1
    out = {"inputs_sha256": np.frombuffer(hashlib.sha256(P.tobytes() + Y.tobytes() + Cp.tobytes()).digest(), dtype=np.uint8).copy()}
    with nm.Handle(config(shape, rotate=rotate)) as h:
        for name in CONTROLS:
            U = controls(shape, name)
            for grad in (True, False):
                r = h.eval(P, U, Y, Cp, grad=grad, dtype=np.float32)
                assert h.last_launch_info()["axis_aligned"] == want_axis, h.last_launch_info()
                tag = f"eval/{name}/{'grad' if grad else 'cost'}"
                out[tag + "/psi"], out[tag + "/f2sq"] = r["psi"], r["f2sq"]
                if grad:
                    out[tag + "/grad"] = r["grad"]
    for plan in PLANS:
        with nm.Handle(config(shape, plan, rotate)) as h:
            r = h.solve(P, dtype=np.float32)
            li = h.last_launch_info()
        assert li["family"] == ("throughput" if plan == "throughput" else "latency") and li["axis_aligned"] == want_axis, (plan, li)
        for k in SOLVE_KEYS:
            out[f"solve/{plan}/{k}"] = r[k][:, :6] if k == "info" else r[k]
    return out
