"""A plain numpy reference of the Kalman-filter predictor stage (``nmpc_kf_predict_*``, csrc/nmpc_kf.h), one scenario and
one pedestrian at a time. Written from the formulas of the reference project's lines the kernel cites, without importing
them (tests/test_kf_reference_cpu.py pins it against recordings of the reference's own classes):

  zfilter.py:45-78                     X = A X;  P = A (P A') + Q;  S = R + C (P C');  K = P (C' S^-1);
                                       X += K (Y - C X);  P = P - K (S K')   (input U = 0)
  interfaces/kfmp_interface.py:26-56   initial state [p0, p1 - p0] ([p0, 0] with one point), filter over the whole past
                                       trajectory, N predictions without evolving P, (P00, P11) for every offset
  main_base.py:210-236, 293-302        one filter object for the pedestrians h = 0, 1, ... in order, never reset: the
                                       covariance is carried from pedestrian to pedestrian and from call to call; rows
                                       [x, y, HUMAN_SIZE, HUMAN_SIZE, 0, 1] at offset 0, [mu_x, mu_y, P00, P11, 0, 1] after

and from include/nmpc_hip.h the append rule of the stored trajectories (``hcount > kf_len``: the current position becomes
row ``kf_len``, at most one per call, dropped beyond ``cap`` rows).

The state is a dict mirroring ``nmpc_kf_args``: ``humans [B,H,2] hcount [B,H] kf_traj [B,H,cap,2] kf_len [B,H] kf_P [B,4,4]``.

``dtype = np.float32`` evaluates the same lines with every array and scalar in float32 -- the restatement's own rounding
in that type, the yardstick of the fp32 kernel. Products are written as sums of elementwise products in index order, so
that the float32 figures do not depend on a BLAS.
"""
import numpy as np

REAL_KEYS = ("humans", "kf_traj", "kf_P")
INT_KEYS = ("hcount", "kf_len")


def model_cv(ts):
    """zfilter.model_CV: (A [4,4], C [2,4]) of the constant-velocity model."""
    A = np.array([[1, 0, ts, 0], [0, 1, 0, ts], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float64)
    C = np.array([[1, 0, 0, 0], [0, 1, 0, 0]], dtype=np.float64)
    return A, C


def default_matrices(ts):
    """What main_base.py:165 and KfmpInterface set up: (A, C, Q, R, P0)."""
    A, C = model_cv(ts)
    return A, C, np.eye(4), np.eye(2), np.eye(4)


def mm(a, b):
    """a @ b as a sum over k in index order, every operation in the arrays' own type."""
    s = a[:, 0:1] * b[0:1, :]
    for k in range(1, a.shape[1]):
        s = s + a[:, k:k + 1] * b[k:k + 1, :]
    return s


def one_step(X, P, Y, A, C, Q, R):
    """KalmanFilter.one_step with U = 0: ``X`` [4,1], ``P`` [4,4], measurement ``Y`` [2,1] -> (X, P)."""
    X = mm(A, X)
    P = mm(A, mm(P, A.T)) + Q
    S = R + mm(C, mm(P, C.T))
    det = S[0, 0] * S[1, 1] - S[0, 1] * S[1, 0]
    Si = np.array([[S[1, 1] / det, -S[0, 1] / det], [-S[1, 0] / det, S[0, 0] / det]], dtype=S.dtype)
    K = mm(P, mm(C.T, Si))
    X = X + mm(K, Y - mm(C, X))
    P = P - mm(K, mm(S, K.T))
    return X, P


def filter_traj(traj, P, A, C, Q, R, N, dtype=np.float64):
    """KfmpInterface.get_motion_prediction for one trajectory ``traj`` [L,2] (L >= 1) with the carried covariance ``P``:
    -> (positions [N,2], P after the L - 1 one-steps)."""
    T = np.dtype(dtype).type
    traj = np.asarray(traj, dtype=T)
    A, C, Q, R, P = (np.asarray(m, dtype=T) for m in (A, C, Q, R, P))
    L = traj.shape[0]
    X = np.zeros((4, 1), T)
    X[0, 0], X[1, 0] = traj[0]
    if L > 1:
        X[2, 0], X[3, 0] = traj[1, 0] - traj[0, 0], traj[1, 1] - traj[0, 1]
    for i in range(L - 1):
        X, P = one_step(X, P, traj[i + 1].reshape(2, 1), A, C, Q, R)
    pos = np.zeros((N, 2), T)
    for t in range(N):
        X = mm(A, X)
        pos[t] = X[:2, 0]
    return pos, P


def chain_values(n, ts=0.2):
    """P[0,0] of the default chain (P0 = Q = I, R = I, model_CV(ts)) after 0 .. n one-steps: data-independent."""
    A, C, Q, R, P = default_matrices(ts)
    out = [float(P[0, 0])]
    for _ in range(n):
        _, P = one_step(np.zeros((4, 1)), P, np.zeros((2, 1)), A, C, Q, R)
        out.append(float(P[0, 0]))
    return out


def predict(s, N, human_size, A, C, Q, R, run=None, dtype=np.float64):
    """One ``nmpc_kf_predict`` call on the state ``s`` -> dict(dyn_c [n_run,H,N+1,6], kf_traj, kf_len, kf_P): the compact
    rows of the running scenarios and full-size copies of the three arrays the call updates."""
    T = np.dtype(dtype).type
    humans = np.array(s["humans"], dtype=T)
    hcount = np.array(s["hcount"], dtype=np.int64)
    out = dict(kf_traj=np.array(s["kf_traj"], dtype=T), kf_len=np.array(s["kf_len"], dtype=np.int64), kf_P=np.array(s["kf_P"], dtype=T))
    B, H = humans.shape[:2]
    cap = out["kf_traj"].shape[2]
    rows = list(range(B)) if run is None else [int(b) for b in run]
    out["dyn_c"] = np.zeros((len(rows), H, N + 1, 6), T)
    for a, b in enumerate(rows):
        P = out["kf_P"][b]
        for h in range(H):
            L = int(out["kf_len"][b, h])
            if hcount[b, h] > L and L < cap:          # past_traj grew: one new position per call, nothing beyond cap rows
                out["kf_traj"][b, h, L] = humans[b, h]
                L += 1
                out["kf_len"][b, h] = L
            traj = out["kf_traj"][b, h, :L] if L > 0 else humans[b, h][None]
            pos, P = filter_traj(traj, P, A, C, Q, R, N, T)
            r = out["dyn_c"][a, h]
            r[0] = [humans[b, h, 0], humans[b, h, 1], T(human_size), T(human_size), 0, 1]
            r[1:, :2] = pos
            r[1:, 2], r[1:, 3] = P[0, 0], P[1, 1]
            r[1:, 4], r[1:, 5] = T(0), T(1)
        out["kf_P"][b] = P
    return out
