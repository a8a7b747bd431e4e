#!/usr/bin/env python3
"""Generate the fixtures of the multi-hypothesis predictor stage by RUNNING THE REFERENCE'S OWN
``pre_load.traj_to_input`` and ``MmpInterface.get_motion_prediction`` (with ``ScaleOffsetReverseTransform`` for the way
from the world to the map). Runs only in the authoring container (needs /root/reference); what it writes is data:

  mmp_cases.npz   input stacks as the reference hands them to its network (float32, after ``.float()``) for nine pedestrians
                  on two small maps, in full; the five Gaussian planes of one pedestrian in a corner of the warehouse map at
                  a sample of the pixels; what ``get_motion_prediction`` returns with the test network of
                  tests/mmp_reference.py in place of the trained one.

The ``MmpInterface`` object is made with ``__new__`` (its constructor loads the trained weights, which are not available):
``config.obsv_len = 5`` and a ``network_manager`` whose ``inference`` records its input and answers with the test network.
torchvision and skimage are not installed here; ``torchvision.transforms.Compose`` is a stand-in that calls its members in
turn, the skimage functions are those of ``make_snap_golden.py``. Every recording is compared with the restatement
(tests/mmp_reference.py) before it is written.

Usage:  python tests/golden/make_mmp_golden.py
"""
from __future__ import annotations

import contextlib
import io
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import make_snap_golden as msg  # noqa: E402  (installs the skimage stand-ins, puts the reference's src/ on the path)

try:
    import torchvision  # noqa: F401
except ImportError:
    tv = types.ModuleType("torchvision")
    tv.transforms = types.ModuleType("torchvision.transforms")

    class Compose:
        def __init__(self, transforms):
            self.transforms = transforms

        def __call__(self, x):
            for t in self.transforms:
                x = t(x)
            return x
    tv.transforms.Compose = Compose
    sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tv.transforms

with contextlib.redirect_stdout(io.StringIO()):
    from basic_map.map_tf import ScaleOffsetReverseTransform  # noqa: E402
    from interfaces.mmp_interface import MmpInterface  # noqa: E402
    import pkg_motion_prediction.pre_load as pre_load  # noqa: E402

import mmp_cases as mc  # noqa: E402
import mmp_reference as mr  # noqa: E402


class Recorder:
    """Stand-in for NetworkManager: ``inference`` keeps the batches it is given (as the network sees them: ``.float()``)."""

    def __init__(self, fan):
        self.fan, self.seen = fan, []

    def inference(self, batch):
        x = batch.float()
        self.seen.append(x.numpy().copy())
        if self.fan is None:
            return torch.zeros(x.shape[0], 1, 2)
        return torch.from_numpy(mr.network_numpy(x.numpy(), self.fan))


def reference_interface(fan):
    itf = MmpInterface.__new__(MmpInterface)
    itf.config = types.SimpleNamespace(obsv_len=5)
    itf.network_manager = Recorder(fan)
    return itf


def reference_stack(traj_world, ref_image, tf, rescale, n_off):
    """main_base.py:190-191 for one pedestrian: the batches the network receives, [n_off, 7, Hm, Wm] float32."""
    ct = ScaleOffsetReverseTransform(scale=tf.scale, offsetx_after=tf.offsetx_after, offsety_after=tf.offsety_after,
                                     x_reverse=tf.x_reverse, y_reverse=tf.y_reverse, x_max_before=tf.x_max_before,
                                     y_max_before=tf.y_max_before)
    past = [ct(list(map(float, x)), False) for x in traj_world]
    itf = reference_interface(None)
    with np.errstate(all="ignore"):
        # (batch_size = 5 as main_base.py:191 passes it; the reference's loop needs pred_offset >= batch_size)
        itf.get_motion_prediction(past, torch.from_numpy(ref_image.astype(np.float64)), n_off, rescale, batch_size=5 if n_off >= 5 else 1)
    got = np.concatenate(itf.network_manager.seen)
    assert got.shape == (n_off, 7) + ref_image.shape and got.dtype == np.float32
    # traj_to_input on its own gives the same six planes (its last channel is the placeholder)
    direct = pre_load.traj_to_input([[v * rescale for v in p] for p in past], ref_image=ref_image.astype(np.float64), obsv_len=5)
    assert np.array_equal(np.asarray(direct, dtype=np.float32).transpose(2, 0, 1)[:6], got[0, :6])
    return got


def main(out_dir=HERE):
    maps = mc.load_maps(HERE)
    out = {}
    n_all = 0
    for case in mc.SMALL_CASES:
        ref = maps[case["map"]]
        tf = mc.TRANSFORMS[case["tf"]]
        trajs = mc.small_trajectories(tf, case["rescale"])
        stacks = np.stack([reference_stack(t, ref, tf, case["rescale"], case["n_off"]) for t in trajs])
        for t, s in zip(trajs, stacks):
            want = mr.input_stack(mr.input_planes(mr.to_pixels(t, tf, case["rescale"]), ref), case["n_off"])
            assert np.array_equal(want, s), case
            n_all += s.size
        out["stack_" + case["name"]] = stacks
    # the warehouse map: one pedestrian in a corner, five distinct planes; the restatement is compared on EVERY pixel, a
    # sample of them is recorded
    ref = maps["warehouse"]
    tf = mc.TRANSFORMS["warehouse"]
    traj = mc.warehouse_trajectory()
    s = reference_stack(traj, ref, tf, 1.0, 2)
    want = mr.input_stack(mr.input_planes(mr.to_pixels(traj, tf, 1.0), ref), 2)
    assert np.array_equal(want, s)
    tiny = s[0, :5]
    sub = (tiny > 0) & (tiny < np.finfo(np.float32).tiny)
    assert sub.sum() > 1000 and (tiny == 0).sum() > 1000, "the far pixels should run through the subnormals to zero"
    assert np.array_equal(s[0, 5], ref) and (s[1, 6] == 2).all()
    out["warehouse_sample"] = s[0, :5].reshape(5, -1)[:, mc.warehouse_sample(ref.size)]
    # the interface with the test network
    for case in mc.INTERFACE_CASES:
        ref = maps[case["map"]]
        fan = mr.fan(case["K"], case["seed"])
        itf = reference_interface(fan)
        with np.errstate(all="ignore"):
            got = itf.get_motion_prediction([tuple(p) for p in case["traj"]], torch.from_numpy(ref.astype(np.float64)),
                                            case["pred_offset"], case["rescale"], batch_size=case["batch_size"])
        got = np.stack([np.asarray(g, dtype=np.float64) for g in got])
        seen = np.concatenate(itf.network_manager.seen)
        assert all(mr.unique_argmax(seen[m, c]) for m in range(len(seen)) for c in (3, 4))
        occ = 255.0 - ref
        want = np.stack(mr.interface(case["traj"], ref, occ > 0, msg.reference_edge(occ), case["pred_offset"], case["rescale"], fan))
        assert np.array_equal(want, got), case
        moved = int((np.abs(got * case["rescale"] - np.round(got * case["rescale"])) == 0).all(axis=2).sum())
        assert 0 < moved < got.shape[0] * got.shape[1], "the case should have snapped and free hypotheses"
        out["interface_" + case["name"]] = got
    np.savez_compressed(os.path.join(out_dir, "mmp_cases.npz"), **out)
    size = os.path.getsize(os.path.join(out_dir, "mmp_cases.npz"))
    print(f"{len(out)} recordings, {n_all} stack elements equal to the restatement, {size / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
