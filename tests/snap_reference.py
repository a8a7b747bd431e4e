"""numpy restatement (test infrastructure) of the snap stage in front of row f2 -- what the reference does on the host
between the predictor's output and fit_DBSCAN, per pedestrian and time offset:

* ``get_closest_edge_point``   /root/reference/src/pkg_motion_prediction/utils/utils_np.py:102-140
* ``... / rescale``            interfaces/mmp_interface.py:60
* ``ct2real.cvt_coords``       main_base.py:196, basic_map/map_tf.py:124-151

as five rules on a SEGMENT (the K hypotheses of one pedestrian at one time offset, pixel coordinates ``(x, y)``):

1. point i is *in* when ``occupied[int(y_i), int(x_i)]`` (truncation toward zero);
2. ``m`` = max over the segment's in-points ``(xc, yc)`` and all pixels ``(c, r)`` of ``d = (c - xc)**2 + (r - yc)**2``
   (float64, every operation rounded on its own; attained at a corner pixel);
3. an in-point moves to the first edge pixel in row-major order with minimal ``q = d / m`` among those with ``q != 0``,
   as ``(col, row)``; pixel (0, 0) when there is no candidate;
4. the moved points come first in their original order, then the untouched ones in theirs;
5. every point: ``x / rescale``, optional ``x_max - x`` / ``y_max - y``, ``scale * x + offset`` (multiply, add).

Pinned against recordings of the reference's own functions by ``tests/test_snap_cpu.py``. A point whose cell lies outside
the map is left untouched and counted (the reference wraps or raises there; the device contract says untouched)."""
from __future__ import annotations

import numpy as np


def edge_list(edge):
    """(cols, rows) of the set pixels in row-major order, float64."""
    r, c = np.nonzero(np.asarray(edge))
    return c.astype(np.float64), r.astype(np.float64)


def snap(raw, n_ped, n_hyp, occupied, edge, transform, rescale=1.0, chunk=1024):
    """raw ``[..., n_ped * n_hyp, 2]`` -> ``(world [..., n_ped * n_hyp, 2] float64, n_snapped [..., n_ped], n_outside [...])``.
    ``transform``: an object with scale, offsetx_after, offsety_after, x_reverse, y_reverse, x_max_before, y_max_before."""
    raw = np.asarray(raw, dtype=np.float64)
    occupied = np.asarray(occupied) != 0
    H, W = occupied.shape
    lead = raw.shape[:-2]
    assert raw.shape[-2] == n_ped * n_hyp and raw.shape[-1] == 2
    pts = raw.reshape(-1, n_hyp, 2)                        # one row per segment
    x, y = pts[..., 0], pts[..., 1]
    with np.errstate(invalid="ignore"):
        onmap = (x > -1.0) & (x < W) & (y > -1.0) & (y < H)
    ci = np.where(onmap, x, 0.0).astype(np.int64)          # astype(int) truncates toward zero, as the reference's does
    ri = np.where(onmap, y, 0.0).astype(np.int64)
    inside = onmap & occupied[ri, ci]                      # rule 1
    # rule 2: d at the four corner pixels, the largest over the segment's in-points
    dc = np.stack([(cx - x) ** 2 + (cy - y) ** 2 for cx in (0.0, float(W - 1)) for cy in (0.0, float(H - 1))]).max(axis=0)
    m = np.where(inside, dc, 0.0).max(axis=1)              # [segments]
    # rule 3
    ec, er = edge_list(edge)
    moved = pts.copy()
    s_idx, i_idx = np.nonzero(inside)
    for k0 in range(0, len(s_idx), chunk):
        s, i = s_idx[k0:k0 + chunk], i_idx[k0:k0 + chunk]
        xc, yc = x[s, i][:, None], y[s, i][:, None]
        if ec.size:
            d = (ec[None, :] - xc) ** 2 + (er[None, :] - yc) ** 2
            with np.errstate(invalid="ignore", divide="ignore"):
                q = d / m[s][:, None]
            q[q == 0] = np.inf
            k = np.argmin(q, axis=1)                       # first minimum in list (= row-major) order
            none = ~np.isfinite(q[np.arange(len(s)), k])
            moved[s, i, 0] = np.where(none, 0.0, ec[k])
            moved[s, i, 1] = np.where(none, 0.0, er[k])
        else:
            moved[s, i] = 0.0
    # rule 4: stable partition, moved points first
    order = np.argsort(~inside, axis=1, kind="stable")
    moved = np.take_along_axis(moved, order[..., None], axis=1)
    # rule 5
    wx, wy = moved[..., 0] / rescale, moved[..., 1] / rescale
    if transform.x_reverse:
        wx = transform.x_max_before - wx
    if transform.y_reverse:
        wy = transform.y_max_before - wy
    wx = transform.scale * wx + transform.offsetx_after
    wy = transform.scale * wy + transform.offsety_after
    world = np.stack([wx, wy], axis=-1).reshape(raw.shape)
    n_snapped = inside.sum(axis=1).reshape(lead + (n_ped,)).astype(np.int32)
    n_outside = (~onmap).reshape(lead + (-1,)).sum(axis=-1)
    return world, n_snapped, n_outside
