"""CPU tests of the snap stage (predictor hypotheses in pixels -> world points in front of row f2): the numpy restatement
``tests/snap_reference.py`` against the recordings of the reference's own ``get_closest_edge_point`` / ``cvt_coords``
(``tests/golden/make_snap_golden.py``), the package's ``edge_map`` against the recorded edge masks, and the new part of the
C ABI (struct layout vs the C compiler, exported symbols)."""
import ctypes
import json
import os
import subprocess
import tempfile
from types import SimpleNamespace

import numpy as np

import dyobav_mpcnwta_warehouse_amd as nm
import snap_reference as sr
from dyobav_mpcnwta_warehouse_amd import snap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_maps(golden_dir):
    """name -> (grey occupancy or occupied mask, occupied mask, recorded edge mask)"""
    z = np.load(os.path.join(golden_dir, "snap_map.npz"))
    H, W = (int(v) for v in z["shape"])
    occupied = np.unpackbits(z["occupied_bits"])[:H * W].reshape(H, W).astype(bool)
    edge = np.unpackbits(z["edge_bits"])[:H * W].reshape(H, W).astype(bool)
    syn = z["synthetic_occupancy"]
    full = np.full(tuple(int(v) for v in z["full_shape"]), 255, dtype=np.uint8)
    return {"warehouse": (occupied, occupied, edge), "synthetic": (syn, syn > 0, z["synthetic_edge"].astype(bool)),
            "full": (full, full > 0, np.zeros(full.shape, bool))}, str(z["note"])


def load_cases(golden_dir):
    return json.load(open(os.path.join(golden_dir, "snap_cases.json")))["cases"]


def test_fixture_covers_what_it_should(golden_dir):
    maps, note = load_maps(golden_dir)
    cases = load_cases(golden_dir)
    assert "NOT pinned against skimage" in note or "from skimage" in note
    occupied, _, edge = maps["warehouse"]
    assert occupied.shape == (293, 330) and int(edge.sum()) == 3576 and not (edge & occupied).any()
    assert {c["kind"] for c in cases} == {"all", "none", "mixed"}
    assert {c["n_hyp"] for c in cases} == {1, 10, 20} and {c["rescale"] for c in cases} == {1.0, 2.0}
    assert {c["map"] for c in cases} == {"warehouse", "synthetic", "full"} and any(c["integer"] for c in cases)
    # the q == 0 rule: an in-point exactly on an edge pixel of the synthetic map
    _, occ, edg = maps["synthetic"]
    hit = 0
    for c in cases:
        if c["map"] == "synthetic" and c["integer"]:
            p = np.array(c["points"]).astype(int)
            hit += int((occ[p[:, 1], p[:, 0]] & edg[p[:, 1], p[:, 0]]).sum())
    assert hit > 0


def test_restatement_equals_every_recording(golden_dir):
    maps, _ = load_maps(golden_dir)
    for c in load_cases(golden_dir):
        _, occupied, edge = maps[c["map"]]
        got, n_snapped, n_outside = sr.snap(np.array(c["points"]), 1, c["n_hyp"], occupied, edge,
                                            SimpleNamespace(**c["transform"]), c["rescale"])
        assert got.dtype == np.float64 and np.array_equal(got, np.array(c["world"])), c
        assert int(n_snapped[0]) == c["n_snapped"] and int(n_outside) == 0


def test_restatement_leaves_points_off_the_map_in_place_and_counts_them(golden_dir):
    maps, _ = load_maps(golden_dir)
    _, occupied, edge = maps["warehouse"]
    tf = snap.WorldTransform(0.1, -15.0, -15.0, False, True, 0.0, 293.0)
    rr, cc = np.nonzero(occupied)
    fr, fc = np.nonzero(~occupied)
    pts = np.array([[cc[5] + 0.5, rr[5] + 0.5], [-3.0, 10.0], [330.0, 5.0], [12.0, float("nan")], [fc[7] + 0.25, fr[7] + 0.75]])
    got, n_snapped, n_outside = sr.snap(pts, 1, 5, occupied, edge, tf)
    assert int(n_snapped[0]) == 1 and int(n_outside) == 3
    assert np.array_equal(got[1:], tf.cvt_coords(pts[1:, 0], pts[1:, 1]), equal_nan=True)   # order kept, only transformed


def test_edge_map_equals_the_recorded_masks(golden_dir):
    maps, _ = load_maps(golden_dir)
    for name, (grey, _, edge) in maps.items():
        got = snap.edge_map(grey)
        assert got.dtype == bool and np.array_equal(got, edge), name
    # binary input in any dtype, and a scaled copy: the edges are where neighbouring dilated values differ
    occupied = maps["warehouse"][1]
    assert np.array_equal(snap.edge_map(occupied.astype(np.uint8) * 255), maps["warehouse"][2])


def test_world_transform_is_the_reference_constructor():
    tf = snap.WorldTransform(scale=0.1, offsetx_after=-15, offsety_after=-15, y_reverse=~False, y_max_before=293)
    assert bool(tf.y_reverse) and not tf.x_reverse
    assert np.array_equal(tf.cvt_coords([10.0], [20.0]), [[0.1 * 10.0 + -15, 0.1 * (293 - 20.0) + -15]])


def test_snap_args_layout_matches_the_c_compiler():
    from dyobav_mpcnwta_warehouse_amd._capi import NmpcSnapArgs
    fields = ("n_ped", "n_hyp", "x_reverse", "y_reverse", "rescale", "scale", "offset_x", "offset_y", "x_max", "y_max",
              "n_snapped", "n_outside")
    assert [f[0] for f in NmpcSnapArgs._fields_] == list(fields)
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "sz.c")
        body = "".join(f'printf(" %zu", offsetof(nmpc_snap_args, {f}));' for f in fields)
        open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "nmpc_hip.h"\nint main(void){printf("%zu", sizeof(nmpc_snap_args));'
                             + body + 'printf(" %d", NMPC_ABI_VERSION);return 0;}\n')
        exe = os.path.join(td, "sz")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert ctypes.sizeof(NmpcSnapArgs) == out[0] == 4 * 4 + 6 * 8 + 2 * 8
    assert [getattr(NmpcSnapArgs, f).offset for f in fields] == out[1:-1]
    assert out[-1] == 5          # functions were added, no struct changed: the ABI version stays


def test_library_exports_the_snap_entry_points():
    lib = nm.load_library()
    for name in ("nmpc_set_map", "nmpc_snap_hypotheses_f32", "nmpc_snap_hypotheses_f64"):
        assert name in nm.EXPORTED_SYMBOLS and hasattr(lib, name), name
    # argument checks that need no device
    a = nm._capi.NmpcSnapArgs()
    assert lib.nmpc_set_map(None, None, None, 0, 0) == -1
    assert lib.nmpc_snap_hypotheses_f64(None, None, ctypes.byref(a), 1, None) == -1
