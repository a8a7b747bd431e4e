#!/usr/bin/env python3
"""Generate the fixtures of the snap stage (predictor hypotheses in pixels -> world points) by RUNNING THE REFERENCE'S OWN
``utils_np.get_closest_edge_point`` and ``ScaleOffsetReverseTransform``. Runs only in the authoring container (needs
/root/reference); what it writes is data.

  snap_map.npz     the reference's warehouse map (data/warehouse_sim_original/label.png): occupied mask
                   (255 - label > 0) and edge mask, bit-packed; a small synthetic map with several grey levels (its
                   edge cells overlap occupied cells) as uint8 occupancy + edge mask; the transform constants read from
                   config/global_setting_warehouse.yaml.
  snap_cases.json  segments (float64 pixel points, all representable in float32) with the reference's output after snap, / rescale and cvt_coords.

skimage is not installed here, so ``skimage.morphology.dilation`` and ``skimage.filters.roberts`` are stand-ins (module
objects put into sys.modules the way ``_map_standins.install`` does it) that call what the two skimage functions call
themselves: ``scipy.ndimage.grey_dilation(image, footprint=...)`` and ``scipy.ndimage.convolve`` with Roberts' two 2 x 2
kernels, both with scipy's default reflecting border. THE EDGE MASK IS THEREFORE THE STAND-IN'S, not pinned against the
real library (old skimage releases additionally zero the border of a filter result; with the reflecting border this map
has no edge pixel on its border rows / columns anyway).

Usage:  python tests/golden/make_snap_golden.py
"""
from __future__ import annotations

import contextlib
import io
import json
import os
import sys

import numpy as np
import yaml
from PIL import Image
from scipy import ndimage as ndi

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REF, "src"))

import _map_standins  # noqa: E402


def dilation(image, footprint=None):
    return ndi.grey_dilation(image, footprint=np.asarray(footprint) != 0)


def roberts(image):
    image = np.asarray(image, dtype=float)
    pd = ndi.convolve(image, np.array([[1.0, 0.0], [0.0, -1.0]]))
    nd = ndi.convolve(image, np.array([[0.0, 1.0], [-1.0, 0.0]]))
    return np.sqrt(pd ** 2 + nd ** 2) / np.sqrt(2)


_map_standins.install()
import skimage  # noqa: E402  (the stand-in package, unless the real one is there)

REAL_SKIMAGE = hasattr(skimage, "__version__")
if not REAL_SKIMAGE:
    skimage.morphology.dilation = dilation
    skimage.filters.roberts = roberts

with contextlib.redirect_stdout(io.StringIO()):
    from basic_map.map_tf import ScaleOffsetReverseTransform  # noqa: E402
    from pkg_motion_prediction.utils import utils_np  # noqa: E402
    from skimage import filters, morphology  # noqa: E402

import snap_reference as sr  # noqa: E402


def togray(image):                       # pkg_motion_prediction/data_handle/dataset.py:116-124, on the loaded array
    if image.ndim == 2:
        return image
    if image.shape[2] == 1:
        return image[:, :, 0]
    image = image[:, :, :3]
    return image[:, :, 0] / 3 + image[:, :, 1] / 3 + image[:, :, 2] / 3


def reference_edge(occupancy):
    """The edge mask exactly as get_closest_edge_point derives it (utils_np.py:126, 132-133)."""
    occ = occupancy.astype(np.float64)
    occ = occ / np.amax(occ, axis=(0, 1), keepdims=True) if occ.max() > 0 else occ
    return filters.roberts(morphology.dilation(occ, np.ones((3, 3)))) > 0


def run_reference(points, occupancy, ct, rescale):
    """mmp_interface.py:60 + main_base.py:196 for one segment, float64 input."""
    with np.errstate(invalid="ignore", divide="ignore"):
        h = utils_np.get_closest_edge_point(points.copy(), occupancy.astype(np.float64).copy()) / rescale
    return ct.cvt_coords(h[:, 0], h[:, 1])


def main(out_dir=HERE):
    cfg = yaml.safe_load(open(os.path.join(REF, "config", "global_setting_warehouse.yaml")))
    label = togray(np.array(Image.open(os.path.join(REF, "data", cfg["map_dir"], "label.png"))))
    occupancy = 255 - label.astype(np.float64)             # mmp_interface.py:60
    occupied = occupancy > 0
    edge = reference_edge(occupancy)
    H, W = occupied.shape
    assert (H, W) == (cfg["sim_height"], cfg["sim_width"])
    # main_base.py:101-103 (y_reverse = ~False = -1: truthy)
    tf_args = dict(scale=cfg["scale2real"], offsetx_after=cfg["corner_coords"][0], offsety_after=cfg["corner_coords"][1],
                   x_reverse=False, y_reverse=~cfg["image_axis"], x_max_before=0, y_max_before=cfg["sim_height"])
    tf_rec = {k: (bool(v) if k.endswith("reverse") else float(v)) for k, v in tf_args.items()}
    tf_flip = dict(tf_rec, x_reverse=True, x_max_before=float(W))
    # synthetic map, several grey levels: level boundaries inside the occupied area are edges on occupied cells
    syn = np.zeros((24, 31))
    syn[3:12, 4:15] = 100
    syn[6:10, 7:12] = 255
    syn[14:21, 18:28] = 200
    syn[16:19, 2:9] = 40
    syn_edge = reference_edge(syn)
    assert ((syn > 0) & syn_edge).sum() > 20
    full = np.full((12, 17), 255.0)                        # everything occupied: no edge pixel at all
    assert not reference_edge(full).any()
    maps = {"warehouse": (occupancy, occupied, edge), "synthetic": (syn, syn > 0, syn_edge),
            "full": (full, full > 0, reference_edge(full))}

    rng = np.random.default_rng(20240607)

    def draw(name, K, kind, integer):
        occ = maps[name][1]
        h, w = occ.shape
        rr, cc = np.nonzero(occ)
        fr, fc = np.nonzero(~occ)
        n_in = {"all": K, "none": 0, "mixed": int(rng.integers(1, K)) if K > 1 else int(rng.integers(0, 2))}[kind]
        if fr.size == 0:
            n_in = K
        flags = rng.permutation(np.r_[np.ones(n_in, bool), np.zeros(K - n_in, bool)])
        pts = np.empty((K, 2))
        for i, f in enumerate(flags):
            j = rng.integers(len(rr) if f else len(fr))
            r, c = (rr[j], cc[j]) if f else (fr[j], fc[j])
            frac = (0.0, 0.0) if integer else rng.uniform(0, 1, 2)
            pts[i] = (c + frac[0], r + frac[1])
        # float32-representable, so that the fp32 entry point sees the same numbers as the reference did
        return pts.astype(np.float32).astype(np.float64)

    plan = []
    for K in (1, 10, 20):
        for kind in ("all", "none", "mixed"):
            for integer in (False, True):
                plan.append(("warehouse", K, kind, integer, 1.0, "world"))
    plan += [("warehouse", 10, "mixed", False, 2.0, "world"), ("warehouse", 10, "mixed", True, 2.0, "world"),
             ("warehouse", 20, "all", False, 2.0, "world"), ("warehouse", 1, "all", True, 2.0, "world"),
             ("warehouse", 10, "mixed", False, 1.0, "flip"), ("warehouse", 20, "mixed", True, 2.0, "flip")]
    plan += [("warehouse", 10, "mixed", i % 3 == 0, 1.0, "world") for i in range(21)]
    for K in (1, 10, 20):
        for integer in (False, True, True):
            plan.append(("synthetic", K, "mixed" if K > 1 else "all", integer, 1.0, "world"))
    plan += [("synthetic", 10, "all", True, 2.0, "flip"), ("synthetic", 20, "all", True, 1.0, "world"),
             ("synthetic", 10, "none", False, 1.0, "world")]
    plan += [("full", 10, "all", False, 1.0, "world"), ("full", 1, "all", True, 2.0, "world"), ("full", 20, "all", True, 1.0, "flip")]

    cases, q0 = [], 0
    for name, K, kind, integer, rescale, tfn in plan:
        occn, occd, edg = maps[name]
        tfd = tf_rec if tfn == "world" else tf_flip
        ct = ScaleOffsetReverseTransform(**(tf_args if tfn == "world" else tfd))
        pts = draw(name, K, kind, integer)
        want = run_reference(pts, occn, ct, rescale)
        ins = occd[pts[:, 1].astype(int), pts[:, 0].astype(int)]
        if integer:
            q0 += int((ins & edg[pts[:, 1].astype(int), pts[:, 0].astype(int)]).sum())
        # the restatement must agree before anything is recorded
        got, n_sn, n_out = sr.snap(pts, 1, K, occd, edg, type("T", (), tfd), rescale)
        assert np.array_equal(got, want) and int(n_sn[0]) == int(ins.sum()) and n_out == 0, (name, K, kind, integer)
        cases.append({"map": name, "n_hyp": K, "kind": kind, "integer": bool(integer), "rescale": rescale, "transform": tfd,
                      "points": pts.tolist(), "n_snapped": int(ins.sum()), "world": np.asarray(want, dtype=np.float64).tolist()})
    assert q0 > 0, "no in-point sits on an edge pixel: the q == 0 rule is not exercised"

    np.savez_compressed(
        os.path.join(out_dir, "snap_map.npz"), shape=np.array([H, W]), occupied_bits=np.packbits(occupied),
        edge_bits=np.packbits(edge), synthetic_occupancy=syn.astype(np.uint8), synthetic_edge=syn_edge,
        full_shape=np.array(full.shape),
        note=np.array("edge masks: stand-ins for skimage.morphology.dilation / skimage.filters.roberts built on "
                      "scipy.ndimage (grey_dilation, convolve; reflecting border) -- NOT pinned against skimage itself"
                      if not REAL_SKIMAGE else "edge masks from skimage " + skimage.__version__))
    with open(os.path.join(out_dir, "snap_cases.json"), "w") as f:
        json.dump({"source": "utils_np.get_closest_edge_point + / rescale + ScaleOffsetReverseTransform.cvt_coords, float64 input",
                   "cases": cases}, f)
    print(f"{len(cases)} segments; warehouse {H} x {W}: {int(edge.sum())} edge pixels, {occupied.mean() * 100:.1f} % occupied, "
          f"{int((edge & occupied).sum())} edge pixels occupied, border edge pixels "
          f"{int(edge[0].sum() + edge[-1].sum() + edge[:, 0].sum() + edge[:, -1].sum())}; in-points on an edge pixel: {q0}")


if __name__ == "__main__":
    main()
