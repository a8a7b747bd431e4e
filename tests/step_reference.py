"""A plain reference of ONE closed-loop time step (row f3), one scenario at a time, in numpy.

Written from the lines of the reference project that ``csrc/nmpc_step.h`` cites -- not from ``evaluate.py``'s torch
expressions, and without importing them:

  pre   main_base.py:238-264, 293-302        run_cv_prediction and the obstacle rows [mu_x, mu_y, std_x, std_y, 0, 1]
        interfaces/cvmp_interface.py:24-57   constant-velocity prediction from the latest <= 5 positions
        trajectory_tracker.py:242-270        get_ref_states (called with action_steps = N_hor, :186-188; the horizon is
                                             N_hor here -- the reference's default 20 equals N_hor in its yaml files)
        trajectory_tracker.py:304-310        speed reference (``max``, as written there)
  post  main_base.py:320-324                 no-backward clip, robot step, pedestrian steps
        basic_agent.py:52-82                 MovingAgent.get_next_goal / get_action / one_step / run_step
        motion_model.py:130-163              omnidirectional model, unicycle model with its four RK4 stages written out
        main_pre.py:20-53                    check_collision, clearances, deviation
        main_base.py:326-335, 366-371        collision / completion flags, trajectory_tracker.py:191-199

The state is a dict of arrays that mirrors ``nmpc_loop_args`` (include/nmpc_hip.h), leading dimension B:
``robot [B,3] last_u [B,2] humans [B,H,2] hist [B,H,5,2] hcount [B,H] hidx [B,H] hpath [B,H,W,2] ref_traj [B,Lmax,3]
ref_len [B] idx_ref [B] goal [B,2] polys [M,4,2] alive collision complete [B] steps [B] clr_dyn clr_stc dev_sum dev_max
n_traj [B] traj [B,max_steps+1,3] acts [B,max_steps,2] U y [B,2N]``.

The reference keeps a pedestrian's ``past_traj`` as a growing list; the C ABI keeps its last five entries in ``hist``
(newest last) and their number in ``hcount``: appending a position shifts the five slots by one. ``hist[..., 4]`` is the
pedestrian's current position whenever ``hcount`` >= 1 (``past_traj[-1] is state``, basic_agent.py:72-74), and the
prediction starts from it (cvmp_interface.py:55). Two things the reference does not define are extensions of this
project, restated from include/nmpc_hip.h: the hypothesis fan (``n_hyp`` > 1), and what happens to the pedestrians of a
scenario that is over but still part of a launch (they keep walking; labelled as a regression value in the tests).

Every DECISION comes back with its margin in the arithmetic's own type, so that a comparison in a lower precision
knows which decisions rounding could flip:
  pre   ``argmin`` gap between the two smallest distances of the window, ``near`` |dist_to_goal - base_speed N ts|
  post  ``wp`` [B,H] |d - vmax ts|, ``col_dyn`` min_h |dist_h - human_size|, ``col_stc`` min over polygon edges of
        |cross| / edge length, ``done_x`` / ``done_y`` |0.5 - |x - gx|| (and y), ``done_v`` |0.4 - |v||, ``back`` |v|.
``force`` overrides decisions per scenario (``{b: {"idx": int, "near": bool, "wp": {h: bool}, "col": bool, "done":
bool}}``): the continuous outputs that FOLLOW from a given decision.

``dtype = np.float32`` evaluates the same lines with every array and scalar in float32: the reference's own rounding
in that type, the yardstick of the fp32 kernels.
"""
import numpy as np

REAL_KEYS = ("robot", "last_u", "humans", "hist", "hpath", "ref_traj", "goal", "polys", "clr_dyn", "clr_stc", "dev_sum",
             "dev_max", "n_traj", "traj", "acts", "U", "y")
INT_KEYS = ("hcount", "hidx", "ref_len", "idx_ref", "steps")
FLAG_KEYS = ("alive", "collision", "complete")
PRE_MARGINS = ("argmin", "near")
POST_MARGINS = ("wp", "col_dyn", "col_stc", "done_x", "done_y", "done_v", "back")


def cast_state(s, dtype):
    """The state with its real arrays in ``dtype`` (copies); counters int64, flags uint8."""
    out = {}
    for k, v in s.items():
        if v is None:
            out[k] = None
        elif k in REAL_KEYS or k == "stagger":
            out[k] = np.array(v, dtype=dtype)
        elif k in INT_KEYS:
            out[k] = np.array(v, dtype=np.int64)
        else:
            out[k] = np.array(v, dtype=np.uint8)
    return out


# ---- pieces --------------------------------------------------------------------------------------------------------
def past_points(hist_bh, hcount_bh):
    """The reference's ``past_traj[-5:]`` from the five-slot window."""
    n = int(min(max(int(hcount_bh), 0), 5))
    return [hist_bh[5 - n + i] for i in range(n)]


def cv_velocity(past, T):
    """cvmp_interface.py:41-51: mean of the differences of the latest <= 5 points, 0 with fewer than two."""
    past = past[-5:] if len(past) > 5 else past
    if len(past) > 1:
        vx = np.mean(np.array([past[i + 1][0] - past[i][0] for i in range(len(past) - 1)], dtype=T))
        vy = np.mean(np.array([past[i + 1][1] - past[i][1] for i in range(len(past) - 1)], dtype=T))
        return T(vx), T(vy)
    return T(0), T(0)


def unicycle_rk4(state, action, ts, T):
    """motion_model.py:141-163 with rk4=True, stage by stage."""
    def d_state_f(st):
        return ts * np.array([action[0] * np.cos(st[2]), action[0] * np.sin(st[2]), action[1]], dtype=T)
    k1 = d_state_f(state)
    k2 = d_state_f(state + T(0.5) * k1)
    k3 = d_state_f(state + T(0.5) * k2)
    k4 = d_state_f(state + k3)
    return state + T(1 / 6) * (k1 + T(2) * k2 + T(2) * k3 + k4)


def polygon_clearance(polys, px, py, T):
    """(distance to the closest polygon with 0 inside, strictly inside any, min |cross| / edge length): what shapely's
    ``Polygon.distance(Point)`` / ``Polygon.contains(Point)`` give for convex quadrilaterals (main_pre.py:26, 42)."""
    inf = T(np.inf)
    if polys.shape[0] == 0:
        return inf, False, inf
    a, bq = polys, np.roll(polys, -1, axis=1)
    abx, aby = bq[..., 0] - a[..., 0], bq[..., 1] - a[..., 1]
    t = ((px - a[..., 0]) * abx + (py - a[..., 1]) * aby) / (abx * abx + aby * aby)
    t = np.clip(t, T(0), T(1))
    ex, ey = a[..., 0] + t * abx - px, a[..., 1] + t * aby - py
    d = np.sqrt(ex * ex + ey * ey).min(axis=1)                          # [M] distance to the boundary
    cross = abx * (py - a[..., 1]) - aby * (px - a[..., 0])             # [M,4] side of every edge
    inside = (cross > 0).all(axis=1) | (cross < 0).all(axis=1)          # interior only: a boundary point is outside
    margin = (np.abs(cross) / np.hypot(abx, aby)).min()
    return T(np.where(inside, T(0), d).min()), bool(inside.any()), T(margin)


# ---- before the solve ----------------------------------------------------------------------------------------------
def pre(s, N, ts, base_speed, lin_vel_max, human_size, n_hyp=1, hyp_fan=0.0, hyp_r0=0.0, hyp_grow=0.0, run=None,
        gather_y=False, dtype=np.float64, force=None):
    """-> (out, margins): ``dyn_c refs_c speed_c state_c last_u_c`` with leading dimension len(run), ``y_c`` (None
    unless ``gather_y`` with a ``run`` list) and the full ``idx_ref``."""
    T = np.dtype(dtype).type
    c = cast_state(s, T)
    B, H = c["humans"].shape[:2]
    rows = list(range(B)) if run is None else [int(b) for b in run]
    nh = int(n_hyp) if n_hyp > 1 else 1
    ts, base_speed, lin_vel_max, human_size = T(ts), T(base_speed), T(lin_vel_max), T(human_size)
    hyp_fan, hyp_r0, hyp_grow = T(hyp_fan), T(hyp_r0), T(hyp_grow)
    out = dict(dyn_c=np.zeros((len(rows), H * nh, N + 1, 6), T), refs_c=np.zeros((len(rows), N, 3), T),
               speed_c=np.zeros(len(rows), T), state_c=np.zeros((len(rows), 3), T), last_u_c=np.zeros((len(rows), 2), T),
               y_c=None, idx_ref=c["idx_ref"].copy())
    mar = {k: np.full(B, np.inf) for k in PRE_MARGINS}
    offs = np.arange(1, N + 1).astype(T)
    for a, b in enumerate(rows):
        f = (force or {}).get(b, {})
        # main_base.py:238-264 + cvmp_interface.py:24-57, rows as main_base.py:293-302
        for h in range(H):
            cur = c["humans"][b, h]
            past = past_points(c["hist"][b, h], c["hcount"][b, h])
            vx, vy = cv_velocity(past, T)
            last = past[-1] if past else cur
            if nh == 1:
                r = out["dyn_c"][a, h]
                r[0] = [cur[0], cur[1], human_size, human_size, 0, 1]
                r[1:, 0] = last[0] + vx * offs
                r[1:, 1] = last[1] + vy * offs
                r[1:, 2:4] = T(1.0)
                r[1:, 4], r[1:, 5] = T(0), T(1)
            else:       # include/nmpc_hip.h, nmpc_loop_args::n_hyp
                t = np.arange(N + 1).astype(T)
                for j in range(nh):
                    ang = (T(j) - T(nh - 1) / T(2)) * hyp_fan
                    ca, sa = np.cos(ang), np.sin(ang)
                    wx, wy = ca * vx - sa * vy, sa * vx + ca * vy
                    r = out["dyn_c"][a, h * nh + j]
                    r[:, 0] = cur[0] + wx * t
                    r[:, 1] = cur[1] + wy * t
                    r[:, 2] = r[:, 3] = hyp_r0 + hyp_grow * t
                    r[:, 4], r[:, 5] = T(0), T(1)
        # trajectory_tracker.py:242-270
        state = c["robot"][b]
        idx0, L = int(c["idx_ref"][b]), int(c["ref_len"][b])
        traj = c["ref_traj"][b, :L]
        lb, ub = max(0, idx0 - N), min(L, idx0 + 5 * N)
        dist = np.hypot(state[0] - traj[lb:ub, 0], state[1] - traj[lb:ub, 1]).tolist()
        idx = dist.index(min(dist)) + lb
        if len(dist) > 1:
            two = np.partition(np.array(dist), 1)[:2]
            mar["argmin"][b] = float(two[1]) - float(two[0])
        if "idx" in f:
            idx = int(f["idx"])
        if idx + N >= L:
            sel = list(range(idx, L)) + [L - 1] * (N - (L - idx))
        else:
            sel = list(range(idx, idx + N))
        out["refs_c"][a] = traj[sel]
        out["idx_ref"][b] = idx
        # trajectory_tracker.py:304-310
        dg = np.hypot(state[0] - c["goal"][b, 0], state[1] - c["goal"][b, 1])
        thr = base_speed * T(N) * ts
        mar["near"][b] = abs(float(dg) - float(thr))
        far = bool(f["near"] is False) if "near" in f else bool(dg >= thr)
        if far:
            out["speed_c"][a] = base_speed
        else:
            out["speed_c"][a] = max(dg / T(N) / ts, lin_vel_max)
        out["state_c"][a] = state
        out["last_u_c"][a] = c["last_u"][b]
    if gather_y and run is not None:
        out["y_c"] = c["y"][rows].copy()
    return out, mar


# ---- after the solve -----------------------------------------------------------------------------------------------
def post(s, U_c, y_c, ts, human_size, human_vmax, step, run=None, stagger=None, dtype=np.float64, force=None):
    """-> (out, margins): every array ``nmpc_loop_post`` writes, full size (copies of the state's arrays, updated for the
    scenarios of ``run``; ``U`` / ``y`` are scattered only under a ``run`` list)."""
    T = np.dtype(dtype).type
    c = cast_state(s, T)
    U_c, y_c = np.asarray(U_c, dtype=T), np.asarray(y_c, dtype=T)
    stagger = None if stagger is None else np.asarray(stagger, dtype=T)
    B, H, W = c["hpath"].shape[:3]
    rows = list(range(B)) if run is None else [int(b) for b in run]
    ts, human_size, vmax = T(ts), T(human_size), T(human_vmax)
    out = {k: c[k] for k in ("robot", "last_u", "humans", "hist", "hcount", "hidx", "alive", "collision", "complete", "steps",
                             "clr_dyn", "clr_stc", "dev_sum", "dev_max", "n_traj", "traj", "acts", "U", "y")}
    mar = {k: np.full((B, H) if k == "wp" else B, np.inf) for k in POST_MARGINS}
    for a, b in enumerate(rows):
        f = (force or {}).get(b, {})
        alive = bool(c["alive"][b])
        if run is not None:
            out["U"][b], out["y"][b] = U_c[a], y_c[a]
        raw = [U_c[a, 0], U_c[a, 1]]
        action = list(raw)
        mar["back"][b] = abs(float(raw[0]))
        if action[0] < 0:                                   # main_base.py:320-321
            action = [T(0) for _ in action]
        state = c["robot"][b].copy()
        if alive:
            state = unicycle_rk4(state, action, ts, T)      # main_base.py:322
        # main_base.py:323-324 -> basic_agent.py:76-82 per pedestrian
        for h in range(H):
            pos = out["humans"][b, h].copy()
            hi = int(out["hidx"][b, h])
            path = c["hpath"][b, h]
            if hi < W:                                      # get_next_goal: coming_path not empty
                d = np.hypot(path[hi, 0] - pos[0], path[hi, 1] - pos[1])
                mar["wp"][b, h] = abs(float(d) - float(vmax * ts))
                reached = bool(d < vmax * ts)
                if h in f.get("wp", {}):
                    reached = bool(f["wp"][h])
                if reached:
                    hi += 1
            if hi < W:                                      # run_step: there is a next node
                node = path[hi]
                d = np.hypot(node[0] - pos[0], node[1] - pos[1])
                if d == 0:
                    raise ValueError("pedestrian exactly on its next way-point: get_action divides by zero")
                st = T(0) if stagger is None else stagger[b, h]
                act = np.array([(node[0] - pos[0]) / d * vmax + st, (node[1] - pos[1]) / d * vmax + st], dtype=T)
                pos = pos + ts * act                        # omnidirectional model
                out["humans"][b, h] = pos
                out["hist"][b, h, :4] = out["hist"][b, h, 1:].copy()      # past_traj.append(state), five slots kept
                out["hist"][b, h, 4] = pos
                out["hcount"][b, h] += 1
            out["hidx"][b, h] = hi
        out["traj"][b, step + 1] = state
        if not alive:
            continue
        out["robot"][b] = state
        out["last_u"][b] = raw
        out["acts"][b, step] = raw
        out["steps"][b] += 1
        hum = out["humans"][b]
        dx, dy = state[0] - hum[:, 0], state[1] - hum[:, 1]
        out["clr_dyn"][b] = min(out["clr_dyn"][b], np.sqrt(dx * dx + dy * dy).min())      # main_pre.py:45-47
        dstc, inside, mstc = polygon_clearance(c["polys"], state[0], state[1], T)
        out["clr_stc"][b] = min(out["clr_stc"][b], dstc)                                    # main_pre.py:39-43
        L = int(c["ref_len"][b])
        dref = np.hypot(c["ref_traj"][b, :L, 0] - state[0], c["ref_traj"][b, :L, 1] - state[1]).min()   # main_pre.py:49-53
        out["dev_sum"][b] += dref
        out["dev_max"][b] = max(out["dev_max"][b], dref)
        out["n_traj"][b] += T(1)
        # main_pre.py:20-32, main_base.py:330-335, trajectory_tracker.py:191-192
        dh = np.hypot(dx, dy)
        mar["col_dyn"][b] = float(np.abs(dh - human_size).min())
        mar["col_stc"][b] = float(mstc)
        col = bool(inside or (dh <= human_size).any())
        if "col" in f:
            col = bool(f["col"])
        gx, gy = c["goal"][b]
        mar["done_x"][b] = abs(0.5 - abs(float(state[0]) - float(gx)))
        mar["done_y"][b] = abs(0.5 - abs(float(state[1]) - float(gy)))
        mar["done_v"][b] = abs(0.4 - abs(float(action[0])))
        if col:
            done = False
        else:
            done = bool(abs(state[0] - gx) <= T(0.5) and abs(state[1] - gy) <= T(0.5) and abs(action[0]) < T(0.4))
            if "done" in f:
                done = bool(f["done"])
        if col:
            out["collision"][b] = 1
        if done:
            out["complete"][b] = 1
        if col or done:                                     # main_base.py:360-367: the run ends
            out["alive"][b] = 0
    return out, mar
