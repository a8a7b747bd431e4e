"""A plain numpy restatement of ONE dynamic-window tracker step over PER-OFFSET LISTS, one scenario at a time.

Written from the description of the entry (include/nmpc_hip.h, ``nmpc_dwa_lists_args``), around the functions of
tests/dwa_reference.py, which stay as they are:

  everything but the dynamic term   ``dwa_reference.run_step`` with ``dyn_mode = 0``: window, grid, rollout, speed + goal direction +
                                    path deviation + static; its ``cost`` is that partial sum (adding the absent dynamic term's
                                    0 changes no bit of a non-negative sum)
  rows                              ``dyn`` [R, N+1, >= 2] with ``count`` [N+1]: row r of offset t exists when r < count[t], counts
                                    clamped to 0 .. R; nothing else of ``dyn`` is looked at
  offset 0                          the term of mode 1 over the count[0] current positions: d = min over points x positions,
                                    d > 0.5 -> 0, then d < 0.2 -> inf, else q_dyn / d; no position -> 0
  offsets 1 .. N                    point i with offset i + 1: d_i = sqrt(i + 1) min over the count[i + 1] means; an empty offset
                                    gives no d_i; any d_i < 0.2 -> inf, min d_i > 0.5 -> 0, else q_dyn / min d_i; all empty -> 0
  cost, selection                   partial sum + (per-step term + offset-0 term); first strict minimum, as in mode 2

With every count equal to H this is ``dwa_reference.run_step(..., dyn_mode=2)`` bit for bit (tests/test_dwa_lists_cpu.py)."""
import numpy as np

import dwa_reference as dr


def clamp_counts(count, R):
    return np.clip(np.asarray(count, dtype=np.int64), 0, int(R))


def run_step(state, goal, last_u, path, polys, dyn, count, cfg, dtype=np.float64):
    """One tracker step. ``dyn`` [R, N+1, >=2], ``count`` [N+1] ints (clamped to 0 .. R). Returns the dict of
    ``dwa_reference.run_step`` (``d_cur`` / ``d_steps`` are inf where a term has no rows)."""
    T = np.dtype(dtype).type
    N = int(cfg.N_hor)
    dyn = np.asarray(dyn, dtype=T)
    cnt = clamp_counts(count, dyn.shape[0])
    assert cnt.shape == (N + 1,) and dyn.shape[1] >= N + 1
    out = dr.run_step(state, goal, last_u, path, polys, None, 0, cfg, dtype)
    n = out["cand"].shape[0]
    if n == 0:
        return out
    inf = T(np.inf)
    traj = out["traj"]
    d_cur, d_steps = np.full(n, inf, T), np.full(n, inf, T)
    c_cur, c_steps = np.zeros(n, T), np.zeros(n, T)
    if cnt[0] > 0:
        e = traj[:, :, None, :2] - dyn[None, None, :cnt[0], 0, :2]           # [n, N+1, count[0], 2]
        d_cur = np.sqrt((e * e).sum(axis=-1)).min(axis=(1, 2)).astype(T)
        with np.errstate(divide="ignore"):
            c_cur = np.where(d_cur > T(0.5), T(0), np.where(d_cur < T(0.2), inf, T(1) / d_cur * T(cfg.q_dyn_obstacle))).astype(T)
    for i in range(N):
        c = cnt[i + 1]
        if c == 0:
            continue
        e = traj[:, i, None, :2] - dyn[None, :c, i + 1, :2]                  # [n, count[i + 1], 2]
        di = (np.sqrt((e * e).sum(axis=-1)).min(axis=1) * np.sqrt(np.array([i + 1]).astype(T))).astype(T)
        d_steps = np.minimum(d_steps, di)
    if (cnt[1:] > 0).any():                                                  # (no cluster at any offset: the term is 0)
        with np.errstate(divide="ignore"):
            c_steps = np.where(d_steps < T(0.2), inf, np.where(d_steps > T(0.5), T(0), T(1) / d_steps * T(cfg.q_dyn_obstacle))).astype(T)
    cost = (out["cost"] + (c_steps + c_cur)).astype(T)
    choice, best = -1, inf
    for i in range(n):
        if cost[i] < best:
            best, choice = cost[i], i
    u = np.zeros(2, T)
    if choice >= 0:
        u = out["cand"][choice].copy()
        if abs(u[0]) < T(cfg.stuck_threshold):
            u[1] = T(-cfg.ang_vel_max)
    out.update(cost=cost, d_cur=d_cur, d_steps=d_steps, c_cur=c_cur, c_steps=c_steps, choice=choice, u=u, min_cost=best)
    return out


def lists_from(obstacles, R, N=20, fill=np.nan):
    """A list of N + 1 lists of (x, y) -> (``dyn`` [R, N+1, 2] with ``fill`` in the rows that do not exist, ``count`` [N+1]):
    entries beyond R are dropped."""
    dyn = np.full((R, N + 1, 2), fill, dtype=np.float64)
    count = np.zeros(N + 1, dtype=np.int32)
    for t, pts in enumerate(obstacles[:N + 1]):
        pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)[:R]
        count[t] = len(pts)
        dyn[:len(pts), t] = pts
    return dyn, count
