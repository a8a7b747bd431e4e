"""Inputs of the multi-hypothesis predictor tests, shared by the fixture generator (tests/golden/make_mmp_golden.py), the CPU
test of the restatement and the GPU tests of the kernel, so that what is recorded from the reference is what the kernel is
run on. numpy only; nothing here is drawn at random.

Small maps: nine pedestrians (3 scenarios x 3) whose NEWEST centre, in network pixels, is of one of the kinds below and
whose past trajectory has 1, 2, 4, 5 or 9 entries. The world trajectories are made from the pixel centres through the
case's transform and rescale, whose constants are powers of two and dyadic offsets: the way back is exact, so "on a pixel"
and "half-integer" mean exactly that on the device as in the reference."""
from __future__ import annotations

import os
from types import SimpleNamespace

import numpy as np


def _tf(**kw):
    d = dict(scale=1.0, offsetx_after=0.0, offsety_after=0.0, x_reverse=False, y_reverse=False, x_max_before=0.0, y_max_before=0.0)
    d.update(kw)
    return SimpleNamespace(**d)


TRANSFORMS = {
    "plain": _tf(scale=0.5, offsetx_after=-2.0, offsety_after=-3.0),
    "reversed": _tf(scale=0.25, offsetx_after=1.5, offsety_after=-0.75, x_reverse=True, y_reverse=True, x_max_before=31.0, y_max_before=24.0),
    "warehouse": _tf(scale=0.1, offsetx_after=-15.0, offsety_after=-15.0, y_reverse=True, y_max_before=293.0),   # main_base.py:101-103
}

# (past-trajectory length, newest centre in pixels, step per entry in pixels, kind)
PEDESTRIANS = (
    (1, (10.0, 7.0), (0.0, 0.0), "on a pixel"),
    (2, (12.3125, 9.625), (1.25, 0.5), "between pixels"),
    (4, (8.5, 11.5), (1.0, 0.5), "half-integer: tied maxima"),
    (5, (-3.25, 5.0), (0.75, 0.25), "left of the map"),
    (9, (15.0, 26.5), (0.5, 1.0), "below the map"),
    (5, (20.0, 14.0), (2.0, 1.0), "on a pixel"),
    (9, (25.4375, 3.1875), (-0.625, 0.375), "between pixels"),
    (2, (20.5, 3.0), (1.0, 0.0), "half-integer in x"),
    (4, (-1.5, 30.25), (0.25, -1.0), "left of and below the map"),
)
B_SMALL, H_SMALL = 3, 3
ITEMS_5 = (0, 2, 4, 7, 8)          # a non-contiguous item list out of the 3 x 3 pedestrians

SMALL_CASES = (
    dict(name="syn_plain_r1_n3", map="synthetic", tf="plain", rescale=1.0, n_off=3),
    dict(name="crop_reversed_r2_n1", map="crop", tf="reversed", rescale=2.0, n_off=1),
    dict(name="crop_plain_r1_n20", map="crop", tf="plain", rescale=1.0, n_off=20),
    dict(name="syn_reversed_r2_n3", map="synthetic", tf="reversed", rescale=2.0, n_off=3),
)

# MmpInterface.get_motion_prediction with the test network: trajectories in map pixels before rescale, chosen so that
# every hypothesis stays on the map and some of them fall into occupied cells
INTERFACE_CASES = (
    dict(name="syn_r1", map="synthetic", K=5, seed=0, rescale=1.0, pred_offset=5, batch_size=5,
         traj=[(10.25 + 0.75 * i, 8.125 + 0.25 * i) for i in range(7)]),
    dict(name="syn_r2", map="synthetic", K=20, seed=1, rescale=2.0, pred_offset=3, batch_size=2,
         traj=[(6.125 + 0.5 * i, 4.375 - 0.125 * i) for i in range(3)]),
)


def forward(tf, px, rescale):
    """Pixel centres (after rescale) -> world, the inverse of what the stage applies."""
    x, y = np.asarray(px, dtype=np.float64).reshape(-1, 2).T / rescale
    if tf.x_reverse:
        x = tf.x_max_before - x
    if tf.y_reverse:
        y = tf.y_max_before - y
    return np.stack([tf.scale * x + tf.offsetx_after, tf.scale * y + tf.offsety_after], axis=1)


def small_trajectories(tf, rescale):
    """The nine pedestrians' whole past trajectories in world coordinates, oldest first."""
    out = []
    for n, end, step, _ in PEDESTRIANS:
        px = np.array(end)[None, :] - np.arange(n - 1, -1, -1)[:, None] * np.array(step)[None, :]
        out.append(forward(tf, px, rescale))
    return out


def hist_arrays(trajs):
    """(hist [n, 5, 2], hcount [n]) as the evaluator keeps them: the last <= 5 positions, newest last, the oldest kept one
    repeated in front."""
    hist = np.stack([np.concatenate([np.repeat(t[-5:][:1], 5 - len(t[-5:]), axis=0), t[-5:]]) for t in trajs])
    return hist, np.array([len(t) for t in trajs], dtype=np.int64)


def warehouse_trajectory():
    """Five positions that end near pixel (1.6, 2.3): the top-left corner of the warehouse map."""
    px = np.array([1.6, 2.3])[None, :] + np.arange(4, -1, -1)[:, None] * np.array([1.7, 2.9])[None, :]
    return forward(TRANSFORMS["warehouse"], px, 1.0)


def warehouse_sample(n_pixels):
    """Flat pixel indices of the recorded sample: the first two rows and every 13th pixel."""
    return np.union1d(np.arange(660), np.arange(0, n_pixels, 13))


def load_maps(golden_dir):
    """name -> the grey label image (float32, 255 = free): the synthetic 24 x 31 map of the snap fixtures, its first 23 rows
    (an odd number of pixels per plane) and the warehouse map."""
    z = np.load(os.path.join(golden_dir, "snap_map.npz"))
    H, W = (int(v) for v in z["shape"])
    occupied = np.unpackbits(z["occupied_bits"])[:H * W].reshape(H, W).astype(bool)
    syn = 255.0 - z["synthetic_occupancy"].astype(np.float32)
    return {"synthetic": syn, "crop": np.ascontiguousarray(syn[:23]), "warehouse": np.where(occupied, 0.0, 255.0).astype(np.float32)}
