"""A plain numpy restatement of ONE dynamic-window (DWA) tracker step, one scenario at a time.

Written from the description of the stage (include/nmpc_hip.h, ``nmpc_dwa_args``), not from the reference's text and not
from the kernel:

  base speed   0.8 lin_vel_max; if hypot(state - goal) < base N ts: min(2 dist / N / ts, lin_vel_max)
  window       [max(vmin, v - a ts), min(vmax, v + a ts)] around the previous chosen control, likewise w with +-ang_vel_max
  grid         np.arange's rule: n = ceil((stop - start) / step), value_i = start + i ((start + step) - start); v-major
  rollout      N + 1 points, the unicycle RK4 step (four stages) with the constant candidate control
  cost         q_speed |v - base| + q_goal_dir |wrap(atan2(goal - p_N) - theta_N)| + q_ref_deviation min over the path's
               segments of the distance of p_N + static + dynamic; segment distance = hypot(max(s, t, 0), c) with the
               normalised tangent; no inside test
  static       d = min over points x edges: d < 0.05 -> inf, d > 0.5 -> 0, else q_stc / d; no rectangles -> 0
  dynamic      mode 1: d = min over points x current positions: d > 0.5 -> 0, then d < 0.2 -> inf, else q_dyn / d
               mode 2: mode 1 on offset 0 plus d_i = sqrt(i + 1) min_h |p_i - mu[h][i + 1]|, i = 0 .. N-1:
               any d_i < 0.2 -> inf, min d_i > 0.5 -> 0, else q_dyn / min d_i  (EUCLIDEAN: the reference's function of that
               name broadcasts a 1-D point along the wrong axis and raises for three or more pedestrians)
  selection    first strict minimum in candidate order, NaN / inf never win; none -> (0, 0), inf, -1; |v| < stuck_threshold
               -> w = -ang_vel_max

``dtype = np.float32`` is the float32 twin: window and grid stay in double (the candidates are cast afterwards), every
other operation is rounded to float32 on its own. All arithmetic is on arrays over the candidates, so that numpy keeps
the element type whatever its scalar promotion rules are.
"""
import math
from types import SimpleNamespace

import numpy as np

DEFAULTS = dict(ts=0.2, N_hor=20, vel_resolution=0.1, ang_resolution=0.1, stuck_threshold=0.001, q_goal_dir=0.05,
                q_ref_deviation=0.1, q_speed=1.0, q_stc_obstacle=2.0, q_dyn_obstacle=2.0, lin_vel_min=-0.5, lin_vel_max=1.5,
                lin_acc_max=1.0, ang_vel_max=0.5, ang_acc_max=3.0)
THRESHOLDS = {"d_stc": (0.05, 0.5), "d_cur": (0.2, 0.5), "d_steps": (0.2, 0.5)}


def config(**kw):
    d = dict(DEFAULTS)
    d.update(kw)
    return SimpleNamespace(**d)


def arange_rule(start, stop, step):
    """(n, values) of np.arange(start, stop, step) for doubles, every operation rounded on its own."""
    start, stop, step = float(start), float(stop), float(step)
    n = max(int(math.ceil((stop - start) / step)), 0)
    delta = (start + step) - start
    return n, np.array([start + i * delta for i in range(n)], dtype=np.float64)


def window(last_u, cfg):
    v, w, ts = float(last_u[0]), float(last_u[1]), float(cfg.ts)
    return (max(float(cfg.lin_vel_min), v - float(cfg.lin_acc_max) * ts), min(float(cfg.lin_vel_max), v + float(cfg.lin_acc_max) * ts),
            max(-float(cfg.ang_vel_max), w - float(cfg.ang_acc_max) * ts), min(float(cfg.ang_vel_max), w + float(cfg.ang_acc_max) * ts))


def candidates(last_u, cfg):
    """(nv, nw, cand [nv nw, 2] float64), v-major."""
    v0, v1, w0, w1 = window(last_u, cfg)
    nv, V = arange_rule(v0, v1, cfg.vel_resolution)
    nw, W = arange_rule(w0, w1, cfg.ang_resolution)
    cand = np.stack([np.repeat(V, nw), np.tile(W, nv)], axis=1) if nv * nw else np.zeros((0, 2))
    return nv, nw, cand


def rk4(S, U, ts, T):
    """S [n,3], U [n,2] -> [n,3]: the four stages written out."""
    ts = T(ts)

    def f(st):
        return np.stack([ts * (U[:, 0] * np.cos(st[:, 2])), ts * (U[:, 0] * np.sin(st[:, 2])), ts * U[:, 1]], axis=1).astype(T)
    k1 = f(S)
    k2 = f(S + T(0.5) * k1)
    k3 = f(S + T(0.5) * k2)
    k4 = f(S + k3)
    return (S + T(1 / 6) * (k1 + T(2) * k2 + T(2) * k3 + k4)).astype(T)


def rollout(state, cand, N, ts, T):
    """[n, N+1, 3]"""
    S = np.repeat(np.asarray(state, dtype=T)[None], cand.shape[0], axis=0)
    out = [S]
    for _ in range(N):
        S = rk4(S, cand, ts, T)
        out.append(S)
    return np.stack(out, axis=1)


def seg_dists(P, A, Bp, T):
    """P [..., 2] points, A / Bp [m, 2] segment ends -> [..., m]."""
    d = Bp - A
    d = (d / np.hypot(d[:, 0], d[:, 1])[:, None]).astype(T)
    px, py = P[..., 0, None], P[..., 1, None]
    s = (A[:, 0] - px) * d[:, 0] + (A[:, 1] - py) * d[:, 1]
    t = (px - Bp[:, 0]) * d[:, 0] + (py - Bp[:, 1]) * d[:, 1]
    h = np.maximum(np.maximum(s, t), T(0))
    c = (px - A[:, 0]) * d[:, 1] - (py - A[:, 1]) * d[:, 0]
    return np.hypot(h, c).astype(T)


def steps_distance(traj, mu, T):
    """traj [n, N+1, >=2], mu [N, H, 2] (offset i + 1 for point i) -> [n]: min_i sqrt(i + 1) min_h |p_i - mu[i][h]|."""
    N = mu.shape[0]
    e = traj[:, :N, None, :2] - mu[None]
    di = np.sqrt((e * e).sum(axis=-1)).min(axis=2) * np.sqrt(np.arange(1, N + 1).astype(T))[None]
    return di.min(axis=1).astype(T)


def run_step(state, goal, last_u, path, polys, dyn, dyn_mode, cfg, dtype=np.float64):
    """One tracker step. ``path`` [P,2] nodes, ``polys`` [M,4,2], ``dyn`` [H, N+1, >=2] (offset 0 = current positions; only
    offset 0 is read in mode 1), ``last_u`` the previous chosen control. Returns a dict: ``nv nw cand cost d_stc d_cur d_steps
    c_stc c_cur c_steps base choice u min_cost traj`` (arrays over the candidates; distances are inf where a term is off)."""
    T = np.dtype(dtype).type
    N, ts = int(cfg.N_hor), cfg.ts
    state = np.asarray(state, dtype=T)
    goal = np.asarray(goal, dtype=T)
    base = T(T(cfg.lin_vel_max) * T(0.8)) if T is np.float32 else T(cfg.lin_vel_max * 0.8)
    dist = np.hypot(state[:1] - goal[:1], state[1:2] - goal[1:2]).astype(T)[0]
    if dist < T(T(base * T(N)) * T(ts)):
        base = min(T(T(T(T(2) * dist) / T(N)) / T(ts)), T(cfg.lin_vel_max))
    nv, nw, cand64 = candidates(last_u, cfg)
    cand = cand64.astype(T)
    n = cand.shape[0]
    inf = T(np.inf)
    out = dict(nv=nv, nw=nw, cand=cand, base=base)
    if n == 0:
        z = np.zeros(0, T)
        out.update(cost=z, d_stc=z, d_cur=z, d_steps=z, c_stc=z, c_cur=z, c_steps=z, choice=-1, u=np.zeros(2, T), min_cost=inf,
                   traj=np.zeros((0, N + 1, 3), T))
        return out
    traj = rollout(state, cand, N, ts, T)
    end = traj[:, -1]
    c_speed = np.abs(cand[:, 0] - base) * T(cfg.q_speed)
    ang = np.arctan2(goal[1] - end[:, 1], goal[0] - end[:, 0]) - end[:, 2]
    c_goal = np.abs(np.arctan2(np.sin(ang), np.cos(ang))) * T(cfg.q_goal_dir)
    path = np.asarray(path, dtype=T)[:, :2]
    c_ref = seg_dists(end[:, :2], path[:-1], path[1:], T).min(axis=-1) * T(cfg.q_ref_deviation)
    polys = np.asarray(polys, dtype=T).reshape(-1, 4, 2)
    d_stc = np.full(n, inf, T)
    c_stc = np.zeros(n, T)
    if polys.shape[0]:
        A = polys.reshape(-1, 2)
        Bp = np.roll(polys, -1, axis=1).reshape(-1, 2)
        d_stc = seg_dists(traj[:, :, :2], A, Bp, T).min(axis=(1, 2))
        with np.errstate(divide="ignore"):
            c_stc = np.where(d_stc < T(0.05), inf, np.where(d_stc > T(0.5), T(0), T(1) / d_stc * T(cfg.q_stc_obstacle))).astype(T)
    d_cur, d_steps = np.full(n, inf, T), np.full(n, inf, T)
    c_cur, c_steps = np.zeros(n, T), np.zeros(n, T)
    if dyn_mode >= 1:
        dyn = np.asarray(dyn, dtype=T)
        e = traj[:, :, None, :2] - dyn[None, None, :, 0, :2]                 # [n, N+1, H, 2]
        d_cur = np.sqrt((e * e).sum(axis=-1)).min(axis=(1, 2)).astype(T)
        with np.errstate(divide="ignore"):
            c_cur = np.where(d_cur > T(0.5), T(0), np.where(d_cur < T(0.2), inf, T(1) / d_cur * T(cfg.q_dyn_obstacle))).astype(T)
    if dyn_mode == 2:
        mu = np.transpose(dyn[:, 1:N + 1, :2], (1, 0, 2))                    # [N, H, 2]: offset i + 1 for point i
        d_steps = steps_distance(traj, mu, T)
        with np.errstate(divide="ignore"):
            c_steps = np.where(d_steps < T(0.2), inf, np.where(d_steps > T(0.5), T(0), T(1) / d_steps * T(cfg.q_dyn_obstacle))).astype(T)
    cost = (c_speed + c_goal + c_ref + c_stc + (c_steps + c_cur)).astype(T)
    choice, best = -1, inf
    for i in range(n):
        if cost[i] < best:
            best, choice = cost[i], i
    u = np.zeros(2, T)
    if choice >= 0:
        u = cand[choice].copy()
        if abs(u[0]) < T(cfg.stuck_threshold):
            u[1] = T(-cfg.ang_vel_max)
    out.update(cost=cost, d_stc=d_stc, d_cur=d_cur, d_steps=d_steps, c_stc=c_stc, c_cur=c_cur, c_steps=c_steps, choice=choice, u=u,
               min_cost=best, traj=traj)
    return out


def near_threshold(r, tol_abs):
    """[n] bool: a deciding distance of the candidate lies within ``tol_abs`` of one of its thresholds."""
    near = np.zeros(len(r["cost"]), bool)
    for k, thr in THRESHOLDS.items():
        d = np.asarray(r[k], dtype=np.float64)
        for t in thr:
            near |= np.isfinite(d) & (np.abs(d - t) <= tol_abs)
    return near
