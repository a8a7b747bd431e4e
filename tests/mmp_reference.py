"""numpy restatement (test infrastructure) of the multi-hypothesis predictor stage of the closed loop -- what the reference
does on the host per pedestrian and time step in front of and behind its network:

* ``ct2real(x, forward=False)``           basic_map/map_tf.py:115-121 (main_base.py:190, 193)
* ``x * rescale``                         interfaces/mmp_interface.py:36
* ``pre_load.traj_to_input``              pkg_motion_prediction/pre_load.py:119-136, ``utils_np.np_gaudist_map`` utils_np.py:76-91
* one copy per time offset, ``.float()``  interfaces/mmp_interface.py:45-49
* snap, ``/ rescale``, ``cvt_coords``     tests/snap_reference.py
* DBSCAN, Gaussian fit, obstacle rows     oracle/hypotheses.py

Pinned against recordings of the reference's own functions (tests/golden/make_mmp_golden.py) by
tests/test_mmp_reference_cpu.py.

THE TEST NETWORK (``network_numpy`` / ``network_torch``) stands in for the trained CNN, whose weights are not available:
it reads the arg-max pixel a3, a4 of channels 3 and 4 (the two newest positions) and the offset t of channel 6 and returns
``a4 + t (a4 - a3) + t fan[k]``. Pixels and offsets are small integers and ``fan`` holds multiples of 1/8, so every value
and every intermediate is exact in float32: numpy on the host and torch on the device agree bit for bit, whatever the order
of operations, and the discrete choices of snap and DBSCAN behind it cannot flip. It is only defined where the arg-max is
unique (``unique_argmax``): not at half-integer centres."""
from __future__ import annotations

import numpy as np

import snap_reference as sr
from oracle import hypotheses as oh

SIGMA = 20.0
OBSV_LEN = 5


def fan(K, seed=0):
    """[K, 2] float32 multiples of 1/8 pixel: three modes 3/4 .. 9/8 pixel per offset apart plus a spread of up to 3/8, so
    that the hypotheses of a pedestrian are one cluster at small offsets and several at large ones (1 m = 10 pixels)."""
    rng = np.random.default_rng(1000 + seed)
    modes = np.array([[0, 0], [6, 7], [-9, 5]])
    f = modes[np.arange(K) % 3] + rng.integers(-3, 4, (K, 2))
    return (f / 8.0).astype(np.float32)


def to_pixels(traj, tf, rescale=1.0):
    """World positions [n, 2] -> the centres in network pixels (float64)."""
    p = np.asarray(traj, dtype=np.float64).reshape(-1, 2)
    x, y = (p[:, 0] - tf.offsetx_after) / tf.scale, (p[:, 1] - tf.offsety_after) / tf.scale
    if tf.x_reverse:
        x = tf.x_max_before - x
    if tf.y_reverse:
        y = tf.y_max_before - y
    return np.stack([x * rescale, y * rescale], axis=1)


def entries(n_traj):
    """Indices into the past trajectory (length ``n_traj``) that channels 0 .. 4 show: the last five, the newest repeated at
    the end."""
    n = min(n_traj, OBSV_LEN)
    return [n_traj - n + min(c, n - 1) for c in range(OBSV_LEN)]


def gauss_plane(cx, cy, Hm, Wm, sigma=SIGMA):
    """np_gaudist_map with sigmas = [sigma, sigma], rho = 0: float64 [Hm, Wm]."""
    x, y = np.meshgrid(np.arange(Wm), np.arange(Hm))
    s2 = sigma * sigma
    z = 1.0 / (2.0 * np.pi * sigma * sigma) * np.exp(-0.5 * ((x - cx) ** 2 / s2 + (y - cy) ** 2 / s2))
    return z / z.max()


def input_planes(centres, ref_image, sigma=SIGMA):
    """centres [n, 2] in pixels, the pedestrian's WHOLE past trajectory -> the six distinct planes [6, Hm, Wm] float32."""
    centres = np.asarray(centres, dtype=np.float64).reshape(-1, 2)
    ref = np.asarray(ref_image)
    Hm, Wm = ref.shape
    planes = [gauss_plane(*centres[e], Hm, Wm, sigma) for e in entries(len(centres))]
    return np.stack(planes + [ref.astype(np.float64)]).astype(np.float32)


def input_stack(planes, n_off):
    """[6, Hm, Wm] -> [n_off, 7, Hm, Wm] float32, channel 6 = 1 .. n_off."""
    out = np.empty((n_off, 7) + planes.shape[1:], dtype=np.float32)
    out[:, :6] = planes[None]
    out[:, 6] = np.arange(1, n_off + 1, dtype=np.float32)[:, None, None]
    return out


def unique_argmax(plane):
    return int((plane == plane.max()).sum()) == 1


def argmax_xy(plane):
    """(x, y) of the unique maximum of one float32 plane, as float32."""
    assert unique_argmax(plane), "tied maxima: the test network is not defined"
    i = int(np.asarray(plane).reshape(-1).argmax())
    return np.array([i % plane.shape[1], i // plane.shape[1]], dtype=np.float32)


def hypotheses(a3, a4, t, fan_):
    """a4 + t (a4 - a3) + t fan in float32: a3, a4 [2], t [M] -> [M, K, 2]."""
    t = np.asarray(t, dtype=np.float32)[:, None, None]
    return (a4[None, None, :] + t * (a4 - a3)[None, None, :] + t * np.asarray(fan_, dtype=np.float32)[None]).astype(np.float32)


def network_numpy(stack, fan_):
    """stack [M, 7, Hm, Wm] float32 -> [M, K, 2] float32."""
    stack = np.asarray(stack, dtype=np.float32)
    return np.concatenate([hypotheses(argmax_xy(s[3]), argmax_xy(s[4]), s[6, :1, 0], fan_) for s in stack])


def network_torch(fan_):
    """The same function as a callable on device tensors."""
    import torch

    def net(x):
        M, _, Hm, Wm = x.shape
        f = torch.as_tensor(np.asarray(fan_, dtype=np.float32), device=x.device)
        i3, i4 = x[:, 3].reshape(M, -1).argmax(dim=1), x[:, 4].reshape(M, -1).argmax(dim=1)
        a3 = torch.stack([i3 % Wm, i3 // Wm], dim=1).to(torch.float32)
        a4 = torch.stack([i4 % Wm, i4 // Wm], dim=1).to(torch.float32)
        t = x[:, 6, 0, 0][:, None, None]
        return a4[:, None, :] + t * (a4 - a3)[:, None, :] + t * f[None]
    return net


def no_near_tie(world, eps=1.0, tol=1e-6):
    """No pair of points of any offset within ``tol`` of ``eps``: world [N, P, 2]."""
    d = np.linalg.norm(world[:, :, None, :] - world[:, None, :, :], axis=-1)
    return not bool((np.abs(d - eps) <= tol).any())


def predict(trajs, ref_image, tf, rescale, n_off, fan_):
    """The network's answer for the pedestrians of one scenario: ``trajs`` = a list of world trajectories -> raw
    [n_off, H * K, 2] float64 in network pixels, the pedestrians' segments side by side."""
    segs = []
    for traj in trajs:
        planes = input_planes(to_pixels(traj, tf, rescale), ref_image)
        # (network_numpy on input_stack(planes, n_off), without building the n_off copies)
        segs.append(hypotheses(argmax_xy(planes[3]), argmax_xy(planes[4]), np.arange(1, n_off + 1), fan_))
    return np.concatenate(segs, axis=1).astype(np.float64)


def stage(trajs, cur, ref_image, occupied, edge, tf, rescale, n_off, fan_, Ndyn, human_size=0.2):
    """The whole predictor stage for one scenario -> (dyn [Ndyn, n_off + 1, 6], n_obs, n_outside, world [n_off, H * K, 2])."""
    H, K = len(trajs), len(fan_)
    raw = predict(trajs, ref_image, tf, rescale, n_off, fan_)
    world, _, n_out = sr.snap(raw, H, K, occupied, edge, tf, rescale)
    assert no_near_tie(world), "a pair of hypotheses lies within 1e-6 of eps: the clustering is not stable"
    dyn, n_obs = oh.hypotheses_to_obstacles(np.asarray(cur, dtype=np.float64), world, human_size=human_size, eps=1.0, enlarge=2.0,
                                            extra_margin=0.0, Ndyn=Ndyn)
    return dyn, n_obs, int(np.sum(n_out)), world


def interface(traj_px, ref_image, occupied, edge, pred_offset, rescale, fan_):
    """MmpInterface.get_motion_prediction with the test network: ``traj_px`` in map pixels before ``rescale`` -> a list of
    ``pred_offset`` arrays [K, 2]."""
    ident = type("T", (), dict(scale=1.0, offsetx_after=0.0, offsety_after=0.0, x_reverse=False, y_reverse=False,
                               x_max_before=0.0, y_max_before=0.0))
    raw = predict([traj_px], ref_image, ident, rescale, pred_offset, fan_)
    world, _, n_out = sr.snap(raw, 1, len(fan_), occupied, edge, ident, rescale)
    assert not np.sum(n_out)
    return list(world)


def ulp_distance_f32(got, want):
    """Element-wise distance in float32 steps between two float32 arrays of non-negative finite values (subnormal steps
    counted like any other: consecutive floats are consecutive integers)."""
    g = np.ascontiguousarray(got, dtype=np.float32).view(np.int32).astype(np.int64)
    w = np.ascontiguousarray(want, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.abs(g - w)
