"""``DwaInterface``: the dynamic-window baseline tracker behind the reference's interface.

Mirror of the reference class ``interfaces/dwa_interface.py:20-66`` (``update_global_path``, ``set_current_state``,
``update_map``, ``run_step(mode, dyn_obstacle_list)``), so that ``MainBase.run_one_step`` (main_base.py:303-321) can drive it.
The tracker step itself (``pkg_dwa_tracker.TrajectoryTracker.run_step``, trajectory_tracker.py:304-355) runs on the device
through ``nmpc_dwa_step_f64`` with one scenario -- there is no host implementation of it in this package. As in the
reference the previous chosen control belongs to the object and opens the next step's window.

``run_step`` returns ``(action, pred_states, cost)``; the reference's three plot lists (all / feasible trajectories and
their costs) are not produced. ``dyn_obstacle_list``: ``None``, a list of positions (ndim 2: the pedestrians' current
positions) or a list of such lists per time offset 0 .. N_hor (ndim 3: offset 0 = the current positions). With a 3-D list
the per-step term uses Euclidean distances (the reference's own function raises for three or more pedestrians; see
include/nmpc_hip.h, ``nmpc_dwa_args``). A list of lists of UNEQUAL length -- the cluster means of the multi-hypothesis predictor,
as ``MainBase.run_wta_prediction`` returns them -- goes through ``nmpc_dwa_step_lists_f64`` (``nmpc_dwa_lists_args``: the reference
itself raises on such a list); a rectangular one stays on dyn_mode 2.

For whole batches of scenarios use ``evaluate.BatchEvaluator(tracker="dwa")``.
"""
from __future__ import annotations

import os
from typing import List, Optional

import numpy as np

from . import _capi
from .configs import DwaConfiguration

ROOT_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEED_SCALE = {"aligning": 0.1, "safe": 0.2, "work": 0.8, "super": 1.0}     # trajectory_tracker.py:206-223


class DwaInterface:
    def __init__(self, config_file_name: Optional[str], current_state: np.ndarray, geo_map=None, verbose: bool = True,
                 static_obstacles=None):
        """``config_file_name``: a yaml with the keys of the reference's ``dwa_test.yaml`` (absolute, or relative to
        ``config/``), or ``None`` for those values. ``geo_map``: anything with ``processed_obstacle_list`` (rectangles as
        four corner points), or pass ``static_obstacles`` [M,4,2] directly."""
        self._prt_name = "DWAInterface"
        if config_file_name is None:
            self.config_dwa = DwaConfiguration()
        else:
            path = config_file_name if os.path.isabs(config_file_name) else os.path.join(ROOT_DIR, "config", config_file_name)
            self.config_dwa = DwaConfiguration.from_yaml(path)
        self.config_robot = self.config_dwa
        self.state = np.asarray(current_state, dtype=np.float64)
        self.geo_map = geo_map
        self._static = static_obstacles
        self.prepared = False
        self.past_actions: List[np.ndarray] = []
        self._h = None

    def set_current_state(self, current_state: np.ndarray):
        self.state = np.asarray(current_state, dtype=np.float64)

    def update_map(self, geo_map):
        self.geo_map = geo_map

    def update_global_path(self, new_global_path: List[tuple]):
        self.ref_path = [tuple(p) for p in new_global_path]
        if len(self.ref_path) < 2:
            raise ValueError("the global path needs at least two nodes")
        self.final_goal = np.array(self.ref_path[-1], dtype=np.float64)[:2]
        self.base_speed = self.config_dwa.lin_vel_max * SPEED_SCALE["work"]
        self.past_actions = []
        self.prepared = True

    def _polygons(self) -> np.ndarray:
        obs = self._static if self._static is not None else getattr(self.geo_map, "processed_obstacle_list", None)
        if obs is None or len(obs) == 0:
            return np.zeros((0, 4, 2))
        return np.ascontiguousarray(np.array(obs, dtype=np.float64).reshape(-1, 4, 2))

    def run_step(self, mode: str = "work", dyn_obstacle_list=None, map_updated=None):
        """-> ``(action [2], pred_states [N_hor + 1, 3], cost)``."""
        if not self.prepared:
            raise ValueError("DwaInterface is not prepared. Call update_global_path() first.")
        if mode not in SPEED_SCALE:
            raise ModuleNotFoundError(f"There is no mode called {mode}.")
        import torch
        c = self.config_dwa
        N = int(c.N_hor)
        if self._h is None:
            cfg = _capi.default_config_struct()
            cfg.N_hor, cfg.ts = N, float(c.ts)
            self._h = _capi.Handle(cfg)
        dev = lambda x, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(x), dtype=dt, device="cuda")
        dyn_mode, H = 0, 0
        rows = count = None
        ragged = _offset_lists(dyn_obstacle_list)
        if ragged is not None:          # unequal numbers of entries per offset: the lists entry (R = the longest list)
            if len(ragged) < N + 1:
                raise ValueError(f"dyn_obstacle_list has {len(ragged)} time offsets, N_hor + 1 = {N + 1} are needed")
            ragged = ragged[:N + 1]
            dyn_mode, H = 2, max(len(q) for q in ragged)
            rows, count = np.zeros((1, H, N + 1, 6)), np.zeros((1, N + 1), dtype=np.int32)
            for t, q in enumerate(ragged):
                count[0, t] = len(q)
                rows[0, :len(q), t, :2] = q[:, :2]
        elif dyn_obstacle_list is not None:
            d = np.array(dyn_obstacle_list, dtype=np.float64)
            if d.ndim == 2:
                dyn_mode, H = 1, d.shape[0]
                rows = np.zeros((1, H, N + 1, 6))
                rows[0, :, 0, :2] = d[:, :2]
            elif d.ndim == 3:
                if d.shape[0] < N + 1:
                    raise ValueError(f"dyn_obstacle_list has {d.shape[0]} time offsets, N_hor + 1 = {N + 1} are needed")
                dyn_mode, H = 2, d.shape[1]
                rows = np.zeros((1, H, N + 1, 6))
                rows[0, :, :, :2] = np.transpose(d[:N + 1, :, :2], (1, 0, 2))
            else:
                raise ValueError("Dynamic obstacles should be a list of tuples or a list of list of tuples.")
        polys = self._polygons()
        path = np.array([p[:2] for p in self.ref_path], dtype=np.float64)
        last_u = self.past_actions[-1] if self.past_actions else np.zeros(2)
        a = (_capi.NmpcDwaArgs() if count is None else _capi.NmpcDwaListsArgs()).set_config(c, SPEED_SCALE[mode])
        cap = 1
        for rng, acc, res in ((c.lin_vel_max - c.lin_vel_min, c.lin_acc_max, c.vel_resolution), (2.0 * c.ang_vel_max, c.ang_acc_max, c.ang_resolution)):
            w = min(rng, 2.0 * acc * float(c.ts))
            cap *= int(w / res * (1.0 + 1e-9)) + 1 if w > 0 else 1
        t = dict(state_c=dev(self.state.reshape(1, 3)), last_u_c=dev(np.asarray(last_u, dtype=np.float64).reshape(1, 2)),
                 goal=dev(self.final_goal.reshape(1, 2)), path=dev(path.reshape(1, -1, 2)), path_len=dev([path.shape[0]], torch.long),
                 U_c=torch.zeros(1, 2 * N, dtype=torch.float64, device="cuda"), min_cost=torch.zeros(1, dtype=torch.float64, device="cuda"),
                 choice=torch.zeros(1, dtype=torch.int32, device="cuda"), counts=torch.zeros(1, 2, dtype=torch.int32, device="cuda"),
                 cand_all=torch.zeros(1, cap, 2, dtype=torch.float64, device="cuda"))
        if rows is not None:
            t["dyn_c"] = dev(rows)
        if polys.shape[0]:
            t["polys"] = dev(polys)
        if count is not None:
            t["dyn_count"] = dev(count, torch.int32)
            a.R = H
        a.B, a.n_run, a.H, a.M, a.Pmax, a.cap, a.dyn_mode = 1, 1, H, int(polys.shape[0]), int(path.shape[0]), cap, dyn_mode
        for k, v in t.items():
            setattr(a, k, v.data_ptr())
        self._h.set_stream(torch.cuda.current_stream().cuda_stream)
        (self._h.dwa_step if count is None else self._h.dwa_step_lists)(np.float64, a)
        action = t["U_c"][0, :2].cpu().numpy()
        cost = float(t["min_cost"].cpu()[0])
        choice = int(t["choice"].cpu()[0])
        self.base_speed = c.lin_vel_max * SPEED_SCALE[mode]
        # the predicted trajectory of the chosen candidate (as found on the grid, before the stuck rule), for the caller's plots
        u = t["cand_all"][0, choice].cpu().numpy() if choice >= 0 else np.zeros(2)
        pred = self.state.reshape(1, -1) if choice < 0 else _rollout(self.state, u, N, float(c.ts))
        self.pred_states = pred
        self.past_actions.append(action.copy())
        return action, pred, cost

    def close(self):
        if self._h is not None:
            self._h.close()
            self._h = None


def _offset_lists(obstacles):
    """The per-offset arrays [n_t, >= 2] of a list of lists of positions whose lengths differ (what ``run_wta_prediction`` returns:
    offset 0 = the current positions, then the cluster means of every offset), or ``None`` for anything else -- ``None``, a list of
    positions, a rectangular list of lists: those keep their path."""
    if obstacles is None or len(obstacles) == 0:
        return None
    out = []
    for q in obstacles:
        try:
            q = np.asarray(q, dtype=np.float64)
        except (TypeError, ValueError):
            return None
        if q.size == 0:
            q = np.zeros((0, 2))
        if q.ndim != 2 or q.shape[1] < 2:
            return None
        out.append(q)
    return out if len({len(q) for q in out}) > 1 else None


def _rollout(state, u, N, ts):
    """The N + 1 states of the unicycle RK4 step applied N times with the constant control ``u`` (host side, output only)."""
    x, y, th = (float(v) for v in state[:3])
    out = [(x, y, th)]
    hh = 0.5 * ts * u[1]
    for _ in range(N):
        cc = (np.cos(th) + 4 * np.cos(th + hh) + np.cos(th + 2 * hh)) / 6
        ss = (np.sin(th) + 4 * np.sin(th + hh) + np.sin(th + 2 * hh)) / 6
        x, y, th = x + ts * u[0] * cc, y + ts * u[0] * ss, th + ts * u[1]
        out.append((x, y, th))
    return np.array(out)
