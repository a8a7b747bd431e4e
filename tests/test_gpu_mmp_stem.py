"""GPU tests of the fused first layer of the multi-hypothesis predictor's network (nmpc_mmp_stem_*, csrc/nmpc_mmp_stem.h)
through the C ABI, against the float64 restatement of tests/mmp_stem_reference.py.

Bound, derived (not tuned): ``|out - ref| <= 352 * 2^-24 * max over the pool window of (|scale_c| S + |shift_c|)`` with
``S = conv2d(|x|, |w|)`` in double, channel 6 included. It covers the 343 products and additions of one output in any order,
with or without fma (gamma_343), at most two extra roundings per term (an input plane one float step away from numpy's,
tests/test_gpu_mmp_input.py, and a folded weight), the offset multiply, the affine and the slope: first order in 2^-24 with
slack; ``max`` and ``leaky`` are 1-Lipschitz. Two controls keep the yardstick honest: torch's own float32 modules on the CPU
meet the same bound on the same inputs, and the restatement with padding 2 (a wrong border rule) violates it. The worst ratio
of error to bound is printed."""
import ctypes

import numpy as np
import pytest
import torch

import dyobav_mpcnwta_warehouse_amd as nm
import mmp_cases as mc
import mmp_reference as mr
import mmp_stem_reference as sr
import oracle
from conftest import config_for

pytestmark = pytest.mark.gpu

SENTINEL = -777.0
BOUND = 352 * sr.U


@pytest.fixture(scope="module")
def maps(golden_dir):
    m = dict(mc.load_maps(golden_dir))
    rng = np.random.default_rng(38)
    m["wide"] = np.where(rng.random((38, 45)) < 0.25, rng.integers(0, 200, (38, 45)), 255).astype(np.float32)   # several tiles down
    m["long"] = np.where(rng.random((9, 101)) < 0.25, rng.integers(0, 200, (9, 101)), 255).astype(np.float32)   # 26 pooled columns: two tiles across
    return m


@pytest.fixture(scope="module")
def handle():
    with nm.Handle(config_for(oracle.Problem())) as h:
        h.set_stream(torch.cuda.current_stream().cuda_stream)
        yield h


def _args(cls, dt, hist, hcount, B, H, items, n_off, d_ref, tf, rescale, sigma=20.0):
    d_hist = torch.from_numpy(np.ascontiguousarray(hist, dtype=dt)).cuda()
    d_cnt = torch.from_numpy(np.ascontiguousarray(hcount, dtype=np.int64)).cuda()
    d_items = None if items is None else torch.tensor(list(items), dtype=torch.long, device="cuda")
    a = cls().set_transform(tf, rescale, sigma)
    a.B, a.H, a.n_off, a.Hm, a.Wm = B, H, n_off, int(d_ref.shape[0]), int(d_ref.shape[1])
    a.hist, a.hcount, a.ref_image = d_hist.data_ptr(), d_cnt.data_ptr(), d_ref.data_ptr()
    a.items = None if d_items is None else d_items.data_ptr()
    return a, [d_hist, d_cnt, d_items, d_ref]


def _stem_args(dt, hist, hcount, B, H, items, n_off, ref, tf, rescale, spec):
    a, keep = _args(nm._capi.NmpcMmpStemArgs, dt, hist, hcount, B, H, items, n_off, torch.from_numpy(ref).cuda(), tf, rescale)
    dev = [torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda() for v in spec[:3]]
    a.C, a.slope = int(spec.weight.shape[0]), spec.slope
    a.weight, a.bn_scale, a.bn_shift = (d.data_ptr() for d in dev)
    return a, keep + dev


def _run(h, dt, hist, hcount, B, H, items, n_item, n_off, ref, tf, rescale, spec, shift=0):
    """The kernel's output [n_item, n_off, C, Hp, Wp] float32. It lies ``shift`` floats into a buffer with 64 sentinel floats
    in front and behind, which must come back untouched."""
    a, keep = _stem_args(dt, hist, hcount, B, H, items, n_off, ref, tf, rescale, spec)
    shape = (n_item, n_off, a.C) + nm._capi.mmp_stem_shape(*ref.shape)
    n = int(np.prod(shape))
    buf = torch.full((64 + shift + n + 64,), SENTINEL, dtype=torch.float32, device="cuda")
    a.n_item, a.out = n_item, buf.data_ptr() + 4 * (64 + shift)
    h.mmp_stem(dt, a)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:64 + shift] == SENTINEL).all() and (got[64 + shift + n:] == SENTINEL).all(), "written outside the output"
    return got[64 + shift:64 + shift + n].reshape(shape)


def _reference(trajs, ref, tf, rescale, n_off, spec, padding=3):
    """(out, bound) [n_ped, n_off, C, Hp, Wp] float64 for the pedestrians' world trajectories."""
    res = [sr.stage(mr.to_pixels(t, tf, rescale), ref, n_off, spec, padding) for t in trajs]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def _torch_float32(trajs, ref, tf, rescale, n_off, spec):
    """torch's own float32 convolution, affine, LeakyReLU and max-pool on the CPU, on the float32 stack."""
    F = torch.nn.functional
    out = []
    for t in trajs:
        x = torch.from_numpy(mr.input_stack(mr.input_planes(mr.to_pixels(t, tf, rescale), ref), n_off))
        pre = F.conv2d(x, torch.from_numpy(spec.weight), stride=2, padding=3)
        act = F.leaky_relu(pre * torch.from_numpy(spec.scale)[None, :, None, None] + torch.from_numpy(spec.shift)[None, :, None, None], spec.slope)
        out.append(F.max_pool2d(act, 3, 2, 1).numpy())
    return np.stack(out)


# ---- 1. the kernel against the restatement: four maps, nine pedestrians, both transforms, both rescales, n_off, C ----------------
@pytest.mark.parametrize("rescale", [1.0, 2.0], ids=["r1", "r2"])
@pytest.mark.parametrize("tf_name", ["plain", "reversed"])
@pytest.mark.parametrize("map_name", ["synthetic", "crop", "wide", "long"])
def test_kernel_against_the_restatement(handle, maps, map_name, tf_name, rescale):
    ref, tf = maps[map_name], mc.TRANSFORMS[tf_name]
    trajs = mc.small_trajectories(tf, rescale)
    hist, hcount = mc.hist_arrays(trajs)
    B, H = mc.B_SMALL, mc.H_SMALL
    Hp, Wp = nm._capi.mmp_stem_shape(*ref.shape)
    worst = 0.0
    for C in (8, 64):
        spec = sr.random_spec(C, seed=C)
        assert (spec.scale < 0).any() and (spec.scale > 0).any() and (spec.shift != 0).all() and spec.slope == 0.1
        want20, bound20 = _reference(trajs, ref, tf, rescale, 20, spec)      # (offsets 1 .. n_off are the first n_off of 20)
        assert want20.shape == (9, 20, C, Hp, Wp)
        for n_off in (1, 3, 20):
            got = _run(handle, np.float64, hist, hcount, B, H, None, B * H, n_off, ref, tf, rescale, spec)
            assert got.shape == (9, n_off, C, Hp, Wp) and got.dtype == np.float32 and np.isfinite(got).all()
            ratio = np.abs(got - want20[:, :n_off]) / bound20[:, :n_off]
            worst = max(worst, float(ratio.max()))
            assert ratio.max() <= BOUND, (map_name, tf_name, rescale, C, n_off, ratio.max() / sr.U)
        # controls, on the same inputs: a correct fp32 implementation is admitted, a wrong border rule is not
        f32 = _torch_float32(trajs, ref, tf, rescale, 3, spec)
        assert (np.abs(f32 - want20[:, :3]) <= BOUND * bound20[:, :3]).all(), "the bound refuses torch's own float32 stem"
        wrong, _ = _reference(trajs, ref, tf, rescale, 3, spec, padding=2)
        hh, ww = min(Hp, wrong.shape[3]), min(Wp, wrong.shape[4])
        assert not (np.abs(wrong[..., :hh, :ww] - want20[:, :3, :, :hh, :ww]) <= BOUND * bound20[:, :3, :, :hh, :ww]).all(), \
            "the bound admits the restatement with padding 2"
    print(f"{map_name} {ref.shape} {tf_name} rescale {rescale}: worst |out - ref| / bound-unit = {worst / sr.U:.1f} x 2^-24 (allowed 352)")


# ---- 2. the warehouse map once, in full ------------------------------------------------------------------------------------------------
def test_warehouse_map_in_full(handle, maps):
    ref, tf = maps["warehouse"], mc.TRANSFORMS["warehouse"]
    assert ref.shape == (293, 330)
    traj = mc.warehouse_trajectory()
    hist, hcount = mc.hist_arrays([traj])
    spec = sr.random_spec(64, seed=64)
    got = _run(handle, np.float64, hist, hcount, 1, 1, None, 1, 2, ref, tf, 1.0, spec)
    want, bound = _reference([traj], ref, tf, 1.0, 2, spec)
    assert got.shape == want.shape == (1, 2, 64, 74, 83) and np.isfinite(got).all()
    ratio = np.abs(got - want) / bound
    print(f"warehouse: worst |out - ref| / bound-unit = {ratio.max() / sr.U:.1f} x 2^-24 (allowed 352)")
    assert ratio.max() <= BOUND


# ---- 3. the exact case: the delta stem copies the stack, bit for bit --------------------------------------------------------------------
@pytest.mark.parametrize("map_name,tf_name,rescale", [("synthetic", "plain", 1.0), ("crop", "reversed", 2.0), ("wide", "plain", 2.0)])
def test_delta_stem_equals_the_pooled_input_stack(handle, maps, map_name, tf_name, rescale):
    ref, tf = maps[map_name], mc.TRANSFORMS[tf_name]
    hist, hcount = mc.hist_arrays(mc.small_trajectories(tf, rescale))
    n_off, spec = 3, sr.delta_spec(8)
    got = _run(handle, np.float64, hist, hcount, 3, 3, None, 9, n_off, ref, tf, rescale, spec)
    a, keep = _args(nm._capi.NmpcMmpArgs, np.float64, hist, hcount, 3, 3, None, n_off, torch.from_numpy(ref).cuda(), tf, rescale)
    stack = torch.empty((9, n_off, 7) + ref.shape, dtype=torch.float32, device="cuda")
    a.n_item, a.out = 9, stack.data_ptr()
    handle.mmp_input(np.float64, a)
    torch.cuda.synchronize()
    sub = stack.cpu()[..., ::2, ::2].reshape((9 * n_off, 7) + tuple(stack[..., ::2, ::2].shape[-2:]))
    sub = torch.cat([sub, torch.zeros_like(sub[:, :1])], dim=1)          # every value >= 0: leaky is the identity
    want = torch.nn.functional.max_pool2d(sub, 3, 2, 1).numpy().reshape(got.shape)
    assert (sub >= 0).all() and np.array_equal(got, want)
    assert np.array_equal(got[:, :, 6], np.broadcast_to(np.arange(1, n_off + 1, dtype=np.float32)[None, :, None, None], got[:, :, 6].shape))


# ---- 4. independence: item list, n_off and the alignment of out do not change a bit ------------------------------------------------------
def test_bits_do_not_depend_on_item_list_offsets_or_alignment(handle, maps):
    ref, tf, rescale = maps["long"], mc.TRANSFORMS["plain"], 1.0
    hist, hcount = mc.hist_arrays(mc.small_trajectories(tf, rescale))
    spec = sr.random_spec(8, seed=3)
    run = lambda items, n_item, n_off, shift=0: _run(handle, np.float64, hist, hcount, 3, 3, items, n_item, n_off, ref, tf, rescale, spec, shift)
    full = run(None, 9, 3)
    assert np.array_equal(run(mc.ITEMS_5, 5, 3), full[list(mc.ITEMS_5)])
    for k in (2, 6):
        assert np.array_equal(run([k], 1, 3)[0], full[k]), k
    assert np.array_equal(run(None, 9, 20)[:, :3], full) and np.array_equal(run(None, 9, 1), full[:, :1])
    for shift in (1, 2, 4):                                # out offset by 4, 8 and 16 bytes
        assert np.array_equal(run(None, 9, 3, shift), full), shift
    # the leading part of hist is not read
    junk = hist.copy()
    for k, n in enumerate(hcount):
        junk[k, :5 - min(n, 5)] = 1e30
    assert np.array_equal(_run(handle, np.float64, junk, hcount, 3, 3, None, 9, 3, ref, tf, rescale, spec), full)


# ---- 5. the two entry points agree on a hist that float holds exactly; a negative slope takes the element-wise path ------------------------
def test_f32_and_f64_entries_agree_and_negative_slope(handle, maps):
    ref, tf, rescale = maps["crop"], mc.TRANSFORMS["reversed"], 2.0
    trajs = mc.small_trajectories(tf, rescale)
    hist, hcount = mc.hist_arrays(trajs)
    assert np.array_equal(hist.astype(np.float32).astype(np.float64), hist)
    spec = sr.random_spec(8, seed=4)
    a = _run(handle, np.float64, hist, hcount, 3, 3, None, 9, 3, ref, tf, rescale, spec)
    b = _run(handle, np.float32, hist, hcount, 3, 3, None, 9, 3, ref, tf, rescale, spec)
    assert np.array_equal(a, b)
    neg = spec._replace(slope=-0.5)                        # leaky is not monotone then: max and leaky do not commute
    got = _run(handle, np.float64, hist, hcount, 3, 3, None, 9, 3, ref, tf, rescale, neg)
    want, bound = _reference(trajs, ref, tf, rescale, 3, neg)
    assert (np.abs(got - want) <= BOUND * bound).all()


# ---- 6. argument errors: refused on the host side, nothing is launched ---------------------------------------------------------------------
def test_errors(handle, maps):
    ref, tf = maps["synthetic"], mc.TRANSFORMS["plain"]
    hist, hcount = mc.hist_arrays(mc.small_trajectories(tf, 1.0))
    spec = sr.random_spec(8, seed=1)
    Hp, Wp = nm._capi.mmp_stem_shape(*ref.shape)
    out = torch.full((9, 3, 8, Hp, Wp), SENTINEL, dtype=torch.float32, device="cuda")

    def make(**over):
        a, keep = _stem_args(np.float64, hist, hcount, 3, 3, None, 3, ref, tf, 1.0, spec)
        a.n_item, a.out = 9, out.data_ptr()
        for k, v in over.items():
            setattr(a, k, v)
        return a, keep
    bad = {"hist = NULL": dict(hist=None), "hcount = NULL": dict(hcount=None), "ref_image = NULL": dict(ref_image=None), "out = NULL": dict(out=None),
           "weight = NULL": dict(weight=None), "bn_scale = NULL": dict(bn_scale=None), "bn_shift = NULL": dict(bn_shift=None),
           "n_item < 0": dict(n_item=-1), "n_item > B H": dict(n_item=10), "n_off = 0": dict(n_off=0), "Hm = 0": dict(Hm=0), "Wm = 0": dict(Wm=0),
           "sigma = 0": dict(sigma=0.0), "sigma < 0": dict(sigma=-20.0), "scale = 0": dict(scale=0.0), "B = 0": dict(B=0), "H = 0": dict(H=0),
           "C = 0": dict(C=0), "C = 4": dict(C=4), "C = 12": dict(C=12), "C < 0": dict(C=-8), "slope = nan": dict(slope=float("nan")),
           "slope = inf": dict(slope=float("inf")), "out misaligned": dict(out=out.data_ptr() + 2)}
    for what, over in bad.items():
        a, keep = make(**over)
        with pytest.raises(nm.NmpcError) as e:
            handle.mmp_stem(np.float64, a)
        assert e.value.code == -1, what
    # more than 2^31 - 1 workgroups: refused as unsupported before anything is looked at on the device
    a, keep = make(B=1 << 15, H=1 << 15, n_item=1 << 30)
    with pytest.raises(nm.NmpcError) as e:
        handle.mmp_stem(np.float64, a)
    assert e.value.code == -4
    lib = nm.load_library()
    a, keep = make()
    assert lib.nmpc_mmp_stem_f64(None, ctypes.byref(a)) == -1 and lib.nmpc_mmp_stem_f64(handle._h, None) == -1
    # a host pointer is refused, not dereferenced
    host = np.zeros(8, dtype=np.float32)
    a, keep = make(weight=host.ctypes.data)
    with pytest.raises(nm.NmpcError):
        handle.mmp_stem(np.float64, a)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), "a refused call wrote to the output"
    a, keep = make(n_item=0)
    handle.mmp_stem(np.float64, a)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    a, keep = make()
    handle.mmp_stem(np.float64, a)
    torch.cuda.synchronize()
    assert bool((out != SENTINEL).all())
