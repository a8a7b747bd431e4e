"""CPU tests of the multi-hypothesis predictor stage: the numpy restatement (tests/mmp_reference.py) against the recordings
of the reference's own ``traj_to_input`` / ``MmpInterface.get_motion_prediction`` (tests/golden/mmp_cases.npz), the
properties of the shared test network and inputs, the C struct layout, and the argument checks that need no device."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import dyobav_mpcnwta_warehouse_amd as nm
import mmp_cases as mc
import mmp_reference as mr
from dyobav_mpcnwta_warehouse_amd import snap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def recordings(golden_dir):
    return np.load(os.path.join(golden_dir, "mmp_cases.npz")), mc.load_maps(golden_dir)


def test_restatement_equals_the_recorded_stacks(recordings):
    rec, maps = recordings
    kinds = set()
    for case in mc.SMALL_CASES:
        ref, tf = maps[case["map"]], mc.TRANSFORMS[case["tf"]]
        want = rec["stack_" + case["name"]]
        trajs = mc.small_trajectories(tf, case["rescale"])
        assert want.shape == (len(trajs), case["n_off"], 7) + ref.shape and want.dtype == np.float32
        for k, t in enumerate(trajs):
            px = mr.to_pixels(t, tf, case["rescale"])
            # the inputs are what their names say, exactly: the transform's way back loses nothing
            n, end, step, kind = mc.PEDESTRIANS[k]
            assert len(px) == n and np.array_equal(px[-1], end), (case["name"], k, px[-1])
            kinds.add(kind)
            got = mr.input_stack(mr.input_planes(px, ref), case["n_off"])
            assert np.array_equal(got, want[k]), (case["name"], k)
            # the trailing-repeat rule seen in the recording itself: channels n - 1 .. 4 are one plane, the ones before differ
            for c in range(min(n, 5) - 1, 4):
                assert np.array_equal(want[k, 0, c], want[k, 0, 4])
            if n > 1 and step != (0.0, 0.0):
                assert not np.array_equal(want[k, 0, 0], want[k, 0, 4])
            assert np.array_equal(want[k, :, 5], np.broadcast_to(ref, (case["n_off"],) + ref.shape))
            assert all((want[k, o, 6] == o + 1).all() for o in range(case["n_off"]))
    assert {p[0] for p in mc.PEDESTRIANS} == {1, 2, 4, 5, 9} and len(kinds) >= 6
    assert {c["n_off"] for c in mc.SMALL_CASES} == {1, 3, 20} and {c["rescale"] for c in mc.SMALL_CASES} == {1.0, 2.0}
    assert maps["crop"].size % 2 == 1 and maps["synthetic"].size % 4 == 0 and maps["warehouse"].size % 4 == 2


def test_maximum_is_at_the_nearest_pixel_and_is_not_the_value_at_the_centre(recordings):
    rec, maps = recordings
    case = mc.SMALL_CASES[0]
    want = rec["stack_" + case["name"]]
    for k, (n, end, _, kind) in enumerate(mc.PEDESTRIANS):
        plane = want[k, 0, 4]
        assert plane.max() == 1.0
        ys, xs = np.nonzero(plane == 1.0)
        Hm, Wm = plane.shape
        cx, cy = min(max(end[0], 0), Wm - 1), min(max(end[1], 0), Hm - 1)
        assert all(abs(x - cx) <= 0.5 and abs(y - cy) <= 0.5 for x, y in zip(xs, ys)), (k, kind)
        assert len(xs) == (2 if end[0] % 1 == 0.5 else 1) * (2 if end[1] % 1 == 0.5 else 1) or "map" in kind, (k, kind, len(xs))


def test_restatement_equals_the_recorded_warehouse_sample(recordings):
    rec, maps = recordings
    ref, tf = maps["warehouse"], mc.TRANSFORMS["warehouse"]
    assert ref.shape == (293, 330)
    planes = mr.input_planes(mr.to_pixels(mc.warehouse_trajectory(), tf, 1.0), ref)
    sample = mc.warehouse_sample(ref.size)
    want = rec["warehouse_sample"]
    assert np.array_equal(planes[:5].reshape(5, -1)[:, sample], want)
    tiny = np.finfo(np.float32).tiny
    assert ((want > 0) & (want < tiny)).sum() > 100 and (want == 0).sum() > 100 and (want == 1).any()


def test_restatement_equals_the_recorded_interface_answers(recordings):
    rec, maps = recordings
    for case in mc.INTERFACE_CASES:
        ref = maps[case["map"]]
        occ = 255.0 - ref
        fan = mr.fan(case["K"], case["seed"])
        got = np.stack(mr.interface(case["traj"], ref, occ > 0, snap.edge_map(occ), case["pred_offset"], case["rescale"], fan))
        want = rec["interface_" + case["name"]]
        assert want.shape == (case["pred_offset"], case["K"], 2) and np.array_equal(got, want), case["name"]


def test_test_network_is_exact_in_float32_and_agrees_between_numpy_and_torch(recordings):
    import torch
    rec, maps = recordings
    for K, seed in ((5, 0), (20, 1), (20, 7)):
        f = mr.fan(K, seed)
        assert f.shape == (K, 2) and f.dtype == np.float32 and np.array_equal(f * 8, np.round(f * 8)) and len({tuple(v) for v in f}) > K // 2
    ref = maps["synthetic"]
    trajs = [np.array(c["traj"]) * c["rescale"] for c in mc.INTERFACE_CASES]
    stack = np.concatenate([mr.input_stack(mr.input_planes(t, ref), 20) for t in trajs])
    f = mr.fan(20, 1)
    a = mr.network_numpy(stack, f)
    b = mr.network_torch(f)(torch.from_numpy(stack)).numpy()
    assert a.dtype == b.dtype == np.float32 and np.array_equal(a, b)
    # every value is a multiple of 1/8 far below 2^24 / 8: nothing was rounded
    assert np.array_equal(a.astype(np.float64) * 8, np.round(a.astype(np.float64) * 8)) and np.abs(a).max() < 2 ** 12
    with pytest.raises(AssertionError, match="tied"):
        mr.network_numpy(mr.input_stack(mr.input_planes(np.array([[3.0, 4.0], [8.5, 6.0]]), ref), 1), f)


def test_mmp_args_layout_matches_the_c_compiler():
    from dyobav_mpcnwta_warehouse_amd._capi import NmpcMmpArgs
    fields = ("B", "H", "n_item", "n_off", "Hm", "Wm", "x_reverse", "y_reverse", "items", "hist", "hcount", "scale", "offset_x",
              "offset_y", "x_max", "y_max", "rescale", "sigma", "ref_image", "out")
    assert [f[0] for f in NmpcMmpArgs._fields_] == list(fields)
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "sz.c")
        body = "".join(f'printf(" %zu", offsetof(nmpc_mmp_args, {f}));' for f in fields)
        open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "nmpc_hip.h"\nint main(void){printf("%zu", sizeof(nmpc_mmp_args));'
                             + body + 'printf(" %d", NMPC_ABI_VERSION);return 0;}\n')
        exe = os.path.join(td, "sz")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert ctypes.sizeof(NmpcMmpArgs) == out[0] == 8 * 4 + 3 * 8 + 7 * 8 + 2 * 8
    assert [getattr(NmpcMmpArgs, f).offset for f in fields] == out[1:-1]
    assert out[-1] == 5          # functions were added, no struct changed: the ABI version stays


def test_library_exports_the_entry_points_and_refuses_null():
    lib = nm.load_library()
    for name in ("nmpc_mmp_input_f32", "nmpc_mmp_input_f64"):
        assert name in nm.EXPORTED_SYMBOLS and hasattr(lib, name), name
    a = nm._capi.NmpcMmpArgs()
    assert lib.nmpc_mmp_input_f64(None, ctypes.byref(a)) == -1 and lib.nmpc_mmp_input_f32(None, None) == -1


def test_interface_refuses_bad_arguments_before_it_touches_a_device():
    import torch
    from dyobav_mpcnwta_warehouse_amd.mmp_interface import MmpInterface
    with pytest.raises(TypeError):
        MmpInterface("wta_test.yaml")                     # the reference's argument: a file name is not a network
    itf = MmpInterface(lambda x: x)
    ref = torch.zeros(4, 5)
    assert itf.get_motion_prediction(None, ref, 3) is None
    with pytest.raises(TypeError, match="tensor"):
        itf.get_motion_prediction([(1.0, 2.0)], np.zeros((4, 5)), 3)
    for kw in (dict(input_traj=[], pred_offset=3), dict(input_traj=[(1.0, 2.0)], pred_offset=0),
               dict(input_traj=[(1.0, 2.0)], pred_offset=3, batch_size=0), dict(input_traj=[(1.0, 2.0)], pred_offset=3, rescale=0.0)):
        with pytest.raises(ValueError):
            itf.get_motion_prediction(ref_image=ref, **kw)
    with pytest.raises(ValueError, match="Hm, Wm"):
        itf.get_motion_prediction([(1.0, 2.0)], torch.zeros(2, 4, 5), 3)
    itf.close()


def test_evaluator_refuses_an_incomplete_predictor_before_it_touches_a_device():
    from dyobav_mpcnwta_warehouse_amd.evaluate import BatchEvaluator
    tf = snap.WorldTransform()
    ok = dict(predictor="mmp", network=lambda x: x, ref_image=np.zeros((4, 5)), transform=tf)
    for over in (dict(network=None), dict(ref_image=None), dict(transform=None), dict(tracker="dwa"), dict(fused=False), dict(n_hyp=2),
                 dict(mmp_hyp=0), dict(mmp_chunk=0), dict(rescale=0.0)):
        with pytest.raises(ValueError):
            BatchEvaluator(None, None, None, None, None, None, **dict(ok, **over))
