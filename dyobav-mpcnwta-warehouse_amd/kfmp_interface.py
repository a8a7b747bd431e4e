"""``KfmpInterface``: the Kalman-filter motion predictor behind the reference's interface.

Mirror of the reference class ``interfaces/kfmp_interface.py:14-56`` (same constructor arguments, the same
``get_motion_prediction`` signature and return value), so that ``MainBase.run_kf_prediction`` (main_base.py:210-236) can
drive it unchanged. The filter itself (``zfilter.KalmanFilter.inference``, zfilter.py:45-78) runs on the device through
``nmpc_kf_predict_f64`` with one scenario, one pedestrian and the given trajectory as the stored one -- there is no host
implementation of it in this package. As in the reference the covariance belongs to the object and is never reset: it
runs on from call to call.

For whole batches of scenarios use ``evaluate.BatchEvaluator(predictor="kfmp")``, which keeps the trajectories on the
device; this class uploads its argument at every call.
"""
from __future__ import annotations

import os
from typing import List, Optional, Tuple

import numpy as np

from . import _capi
from .configs import CircularRobotSpecification, MpcConfiguration
from .solver import make_config

ROOT_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HUMAN_SIZE = 0.2


def model_CV(ts: float = 1.0) -> List[np.ndarray]:
    """``zfilter.model_CV``: [A, B, C, D] of the constant-velocity model."""
    A = np.array([[1, 0, ts, 0], [0, 1, 0, ts], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=float)
    C = np.array([[1, 0, 0, 0], [0, 1, 0, 0]], dtype=float)
    return [A, np.zeros((4, 1)), C, np.zeros((2, 1))]


class KfmpInterface:
    def __init__(self, config_file_name: str, Q=np.eye(4), R=np.eye(2), state_space: Optional[List[np.ndarray]] = None):
        self._prt_name = "KFMPInterface"
        path = config_file_name if os.path.isabs(config_file_name) else os.path.join(ROOT_DIR, "config", config_file_name)
        self.config = MpcConfiguration.from_yaml(path)
        self._robot = CircularRobotSpecification.from_yaml(path)
        self.state_space = model_CV(self.config.ts) if state_space is None else state_space
        self.Q, self.R = np.asarray(Q, dtype=np.float64), np.asarray(R, dtype=np.float64)
        self._h = None        # device handle and the carried covariance (P0 = eye(4)), created on first use
        self._P = None

    def get_motion_prediction(self, input_traj: List[tuple], ref_image=None, pred_offset=None, rescale: float = 1.0,
                              batch_size=None) -> Tuple[List[list], List[list]]:
        """``input_traj``: the past positions (x, y), oldest first. Returns ``(positions, uncertainty)``: the ``N_hor``
        predicted positions and, for each, ``[P[0,0], P[1,1]]`` of the covariance after the filter pass (the same pair
        for every offset). ``ref_image``, ``pred_offset``, ``batch_size``: placeholders, as in the reference."""
        if input_traj is None:
            return None
        import torch
        traj = np.array([[x * rescale for x in y] for y in input_traj], dtype=np.float64).reshape(-1, 2)
        if traj.shape[0] < 1:
            raise ValueError("input_traj is empty")
        if self._h is None:
            self._h = _capi.Handle(make_config(self.config, self._robot))
            self._P = torch.eye(4, dtype=torch.float64, device="cuda").reshape(1, 4, 4).contiguous()
        N, L = int(self.config.N_hor), int(traj.shape[0])
        kf_traj = torch.from_numpy(np.ascontiguousarray(traj.reshape(1, 1, L, 2))).cuda()
        humans = kf_traj[:, :, L - 1].contiguous()
        count = torch.full((1, 1), L, dtype=torch.long, device="cuda")       # hcount = kf_len: nothing is appended
        kf_len = count.clone()
        rows = torch.empty(1, 1, N + 1, 6, dtype=torch.float64, device="cuda")
        a = _capi.NmpcKfArgs().set_matrices(self.state_space[0], self.state_space[2], self.Q, self.R)
        a.B, a.n_run, a.H, a.cap, a.human_size = 1, 1, 1, L, HUMAN_SIZE
        a.humans, a.hcount, a.kf_traj, a.kf_len = humans.data_ptr(), count.data_ptr(), kf_traj.data_ptr(), kf_len.data_ptr()
        a.kf_P, a.dyn_c = self._P.data_ptr(), rows.data_ptr()
        self._h.set_stream(torch.cuda.current_stream().cuda_stream)
        self._h.kf_predict(np.float64, a)
        out = rows[0, 0, 1:].cpu().numpy()
        positions = out[:, :2].tolist()
        uncertainty = [[float(out[0, 2]), float(out[0, 3])]] * len(positions)
        return positions, uncertainty

    def close(self):
        if self._h is not None:
            self._h.close()
            self._h = None
