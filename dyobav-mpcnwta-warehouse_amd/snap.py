"""Host-side companions of the device snap stage (``Handle.set_map`` / ``Handle.snap_hypotheses``, ``csrc/nmpc_snap.h``).

* :class:`WorldTransform` -- the arguments of the reference's ``ScaleOffsetReverseTransform``
  (``basic_map/map_tf.py:82-99``); the device applies its ``cvt_coords`` (``:124-151``).
* :func:`edge_map` -- the edge mask the reference derives inside ``get_closest_edge_point``
  (``pkg_motion_prediction/utils/utils_np.py:132-133``), needed once per map.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np


@dataclass(frozen=True)
class WorldTransform:
    """``ScaleOffsetReverseTransform(scale, offsetx_after, offsety_after, x_reverse, y_reverse, x_max_before,
    y_max_before)``: ``x -> scale * (x_max_before - x if x_reverse else x) + offsetx_after``, likewise for y. The reversal
    flags are taken by truth value, as the reference takes them: ``main_base.py:103`` passes ``~False`` (= -1), which
    switches ``y_reverse`` ON."""
    scale: float = 1.0
    offsetx_after: float = 0.0
    offsety_after: float = 0.0
    x_reverse: bool = False
    y_reverse: bool = False
    x_max_before: float = 0.0
    y_max_before: float = 0.0

    def cvt_coords(self, x, y):
        """numpy counterpart of the device arithmetic (float64, multiply and add rounded separately)."""
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        if self.x_reverse:
            x = self.x_max_before - x
        if self.y_reverse:
            y = self.y_max_before - y
        return np.stack([self.scale * x + self.offsetx_after, self.scale * y + self.offsety_after], axis=-1)


def edge_map(occupied) -> np.ndarray:
    """``roberts(dilation(occ, ones((3, 3)))) > 0`` in plain numpy, for users without skimage: grey dilation (3 x 3
    maximum), then Roberts' two 2 x 2 diagonal differences ``a[r+1, c+1] - a[r, c]`` and ``a[r+1, c] - a[r, c+1]``, both
    with the reflecting border (an index past the last row / column repeats it) that skimage's functions get from
    scipy.ndimage; a pixel is an edge where either difference is not zero. ``occupied`` may have several grey levels.
    Returns a bool array of the same shape. (A restatement: it is not pinned against skimage itself.)"""
    a = np.asarray(occupied)
    if a.ndim != 2:
        raise ValueError(f"occupied must be [H, W], got {a.shape}")
    a = a.astype(np.float64)
    p = np.pad(a, 1, mode="edge")       # reflect = repeat the border pixel; harmless under a maximum
    H, W = a.shape
    d = a.copy()
    for dr in range(3):
        for dc in range(3):
            d = np.maximum(d, p[dr:dr + H, dc:dc + W])
    q = np.pad(d, ((0, 1), (0, 1)), mode="edge")
    pos = q[1:, 1:] - q[:-1, :-1]
    neg = q[1:, :-1] - q[:-1, 1:]
    return (pos != 0) | (neg != 0)
