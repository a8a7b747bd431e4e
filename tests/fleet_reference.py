"""The fleet stage in plain numpy: what ``fleet_exchange_kernel`` and ``fleet_post_kernel`` (csrc/nmpc_fleet.h, entry points
nmpc_fleet_exchange_* / nmpc_fleet_post_*) compute, stated independently of them -- rollout, selection, layout, epilogue.

A fleet is a group of R consecutive scenarios b = g R + i. Every function takes ``dtype``: all arithmetic is done in it, one
rounding per operation (numpy never contracts), which is the form the kernels' ranking key is written in.

Checked without a GPU by tests/test_fleet_reference_cpu.py: the rollout against the reference project's ``UnicycleModel`` and its
recorded ``pred_states``; the block layout against the fp64 oracle's cost, i.e. against the builder's slicing of c_0 and c.
"""
import numpy as np


def unicycle_step(s, u, ts, dtype=np.float64):
    """``UnicycleModel(ts, rk4=True)`` (basic_motion_model/motion_model.py:141-163) in closed form, the expressions of
    ``loop_post_kernel``: RK4 of x' = v cos(th), y' = v sin(th), th' = w with constant (v, w) samples the cosine at th, th + h w / 2
    (twice) and th + h w, hence (c0 + 4 c1 + c2) / 6."""
    t = np.dtype(dtype).type
    x, y, th = (t(v) for v in s)
    v, w = t(u[0]), t(u[1])
    ts = t(ts)
    hh = t(0.5) * ts * w
    cc = (np.cos(th) + t(4) * np.cos(th + hh) + np.cos(th + t(2) * hh)) / t(6)
    ss = (np.sin(th) + t(4) * np.sin(th + hh) + np.sin(th + t(2) * hh)) / t(6)
    return np.array([x + ts * v * cc, y + ts * v * ss, th + ts * w], dtype=dtype)


def rollout(state, U, ts, dtype=np.float64):
    """What a peer publishes: ``state`` rolled through ALL N controls of ``U`` [2N], unshifted -> [N, 3]: the reference's
    ``pred_states`` (pkg_mpc_tracker/trajectory_tracker.py:369-378)."""
    s = np.asarray(state, dtype=dtype)
    U = np.asarray(U, dtype=dtype).reshape(-1, 2)
    out = np.empty((U.shape[0], 3), dtype=dtype)
    for j in range(U.shape[0]):
        s = unicycle_step(s, U[j], ts, dtype)
        out[j] = s
    return out


def c0_index(s):
    """First element of slot ``s`` of c_0 inside a block [c_0 | c]."""
    return 3 * s


def c_index(s, j, N, Nother):
    """First element of slot ``s``, step ``j`` of c inside a block [c_0 | c]: the builder slices c[kt*ns :: ns*N_hor]."""
    return 3 * Nother + s * 3 * N + 3 * j


def block_len(N, Nother):
    return 3 * (N + 1) * Nother


def rank_peers(robot, R, b, dtype=np.float64, cap=None):
    """The other members of b's group, nearest first by (d2, member index) with d2 = dx * dx + dy * dy in ``dtype``. Returns
    (global indices, their distances sqrt(d2) as float64, margin): ``margin`` = the smallest gap between two consecutive
    distances among the first ``cap + 1`` of the list -- the gaps that decide who is taken and in which slot (``cap`` None: the
    whole list; inf with fewer than two) -- below a rounding-sized margin another order is as good."""
    robot = np.asarray(robot, dtype=dtype)
    g, me = divmod(int(b), R)
    keys = []
    for l in range(R):
        if l == me:
            continue
        m = g * R + l
        dx, dy = robot[m, 0] - robot[b, 0], robot[m, 1] - robot[b, 1]
        keys.append((dx * dx + dy * dy, l, m))
    keys.sort(key=lambda k: (k[0], k[1]))
    d = np.sqrt(np.array([float(k[0]) for k in keys], dtype=np.float64))
    dd = d if cap is None else d[:cap + 1]
    margin = float(np.diff(dd).min()) if len(dd) > 1 and (cap is None or cap > 0) else float("inf")
    return [k[2] for k in keys], d, margin


def exchange(robot, U, alive, R, N, Nother, ts, run=None, dtype=np.float64):
    """``other_c`` [n_run, 3 (N + 1) Nother] for the running robots (``run``: indices, None = all B), plus per running robot the
    peers chosen (nearest first: slot s + 1 holds peers[s]) and the ranking margin. ``robot`` [B, 3], ``U`` [B, 2N] or None (no
    previous solution: everyone at rest), ``alive`` [B] (0: at rest)."""
    robot = np.asarray(robot, dtype=dtype)
    B = robot.shape[0]
    assert R >= 1 and B % R == 0
    rows = np.arange(B) if run is None else np.asarray(run, dtype=np.int64)
    out = np.zeros((len(rows), block_len(N, Nother)), dtype=dtype)
    peers, margins = [], []
    cap = Nother - 1
    published = {}      # (what member m publishes is the same for every robot that takes it)

    def publish(m):
        if m not in published:
            if U is None or not alive[m]:
                published[m] = np.repeat(robot[m][None, :], N, axis=0)
            else:
                published[m] = rollout(robot[m], np.asarray(U, dtype=dtype)[m], ts, dtype)
        return published[m]
    for a, b in enumerate(rows):
        order, _, margin = rank_peers(robot, R, b, dtype, cap=max(cap, 0))
        order = order[:max(cap, 0)]
        for k, m in enumerate(order):
            s = k + 1
            out[a, c0_index(s):c0_index(s) + 3] = robot[m]
            i0 = c_index(s, 0, N, Nother)
            out[a, i0:i0 + 3 * N] = publish(m).reshape(-1)
        peers.append(order)
        margins.append(margin)
    return out, peers, np.array(margins)


def post(robot, R, width, clr_fleet, collision, complete, alive, collision_fleet, run=None, dtype=np.float64):
    """The epilogue for the robots that ran this step (``run``, None = all): new (clr_fleet, collision, complete, alive,
    collision_fleet) and per running robot |d_min - width| (inf without a peer), the margin of the collision decision.
    ``robot`` holds the positions AFTER the step."""
    robot = np.asarray(robot, dtype=dtype)
    B = robot.shape[0]
    assert R >= 1 and B % R == 0
    rows = np.arange(B) if run is None else np.asarray(run, dtype=np.int64)
    clr = np.array(clr_fleet, dtype=dtype)
    col, comp, liv, colf = (np.array(v, dtype=np.uint8) for v in (collision, complete, alive, collision_fleet))
    w = np.dtype(dtype).type(width)
    margins = []
    for b in rows:
        g = int(b) // R
        d = [np.hypot(robot[b, 0] - robot[m, 0], robot[b, 1] - robot[m, 1]) for m in range(g * R, g * R + R) if m != b]
        dmin = np.dtype(dtype).type(min(d)) if d else np.dtype(dtype).type(np.inf)
        clr[b] = min(clr[b], dmin)
        if dmin <= w:
            col[b], comp[b], liv[b], colf[b] = 1, 0, 0, 1
        margins.append(abs(float(dmin) - float(w)))
    return dict(clr_fleet=clr, collision=col, complete=comp, alive=liv, collision_fleet=colf), np.array(margins)


def fleet_cost(own_state, U, block, N, Nother, ts, width):
    """The two fleet sums of the cost (solver_build/mpc_builder.py:85-97 with mpc_cost.cost_fleet_collision, mpc_cost.py:65-76),
    float64: per step kt, with p = the own position after kt + 1 controls,
    1000 sum over c_0 slots 1 .. Nother - 1 of max(0, width^2 - |p - c_0[s]|^2) + 10 sum over ALL slots of c at step kt of the same
    hinge -- the zero slots at the origin included."""
    block = np.asarray(block, dtype=np.float64)
    pred = rollout(own_state, U, ts)
    total = 0.0
    for kt in range(N):
        p = pred[kt, :2]
        for s in range(1, Nother):
            q = block[c0_index(s):c0_index(s) + 2]
            total += 1000.0 * max(0.0, width ** 2 - float(((p - q) ** 2).sum()))
        for s in range(Nother):
            i = c_index(s, kt, N, Nother)
            q = block[i:i + 2]
            total += 10.0 * max(0.0, width ** 2 - float(((p - q) ** 2).sum()))
    return total
