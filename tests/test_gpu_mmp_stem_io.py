"""GPU tests of the fused first layer with its output as binary16 in the octet form (nmpc_mmp_stem_io_*, csrc/nmpc_mmp_stem.h)
through the C ABI. Everything is bit for bit: ``K`` is ``nmpc_mmp_stem_*`` on the same arguments (tests/test_gpu_mmp_stem.py holds it
to the float64 restatement), ``pack`` is ``mmp_stem.pack_activations_f16``, and the claims are ``io(1) == pack(K)`` and
``io(0) == K``. No tolerance appears anywhere in this file.

By hand, not in the suite: the 293 x 330 warehouse map at M = 2 (``warehouse_map_by_hand`` below is the recipe; DESIGN.md
section 7 records the result)."""
import ctypes

import numpy as np
import pytest
import torch

import dyobav_mpcnwta_warehouse_amd as nm
import mmp_cases as mc
import mmp_stem_reference as sr
import test_gpu_mmp_stem as ts
from dyobav_mpcnwta_warehouse_amd import _capi
from dyobav_mpcnwta_warehouse_amd.mmp_stem import F16_MAX, pack_activations_f16, unpack_activations_f16
from guarded_buffers import IntPoison, run_guarded
from test_gpu_mmp_stem import handle, maps  # noqa: F401  (the fixtures)

pytestmark = pytest.mark.gpu

SENTINEL = {np.dtype(np.float32): -777.0, np.dtype(np.int16): -12345}


def _same(a, b):
    """Identical bit patterns; for NaN only the positions must agree."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    fa, fb = (v.view(np.float16) if v.dtype == np.uint16 else v for v in (a, b))
    na, nb = np.isnan(fa), np.isnan(fb)
    return np.array_equal(na, nb) and a[~na].tobytes() == b[~nb].tobytes()


def _io(h, dt, hist, hcount, B, H, items, n_item, n_off, ref, tf, rescale, spec, out_f16, shift=0):
    """The ``_io`` entry. Returns float32 ``[n_item * n_off, C, Hp, Wp]`` or, with ``out_f16``, the uint16 octets ``[n_item * n_off,
    C / 8, Hp, Wp, 8]``. The output lies ``shift`` elements into a buffer with 64 sentinel elements in front and behind, which must
    come back untouched."""
    a, keep = ts._stem_args(dt, hist, hcount, B, H, items, n_off, ref, tf, rescale, spec)
    Hp, Wp = _capi.mmp_stem_shape(*ref.shape)
    n = n_item * n_off * a.C * Hp * Wp
    tdt = torch.int16 if out_f16 else torch.float32
    ndt = np.dtype(np.int16 if out_f16 else np.float32)
    buf = torch.full((64 + shift + n + 64,), SENTINEL[ndt], dtype=tdt, device="cuda")
    a.n_item, a.out = n_item, buf.data_ptr() + ndt.itemsize * (64 + shift)
    h.mmp_stem_io(dt, a, out_f16)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:64 + shift] == SENTINEL[ndt]).all() and (got[64 + shift + n:] == SENTINEL[ndt]).all(), "written outside the output"
    got = got[64 + shift:64 + shift + n]
    return got.view(np.uint16).reshape(n_item * n_off, a.C // 8, Hp, Wp, 8) if out_f16 else got.reshape(n_item * n_off, a.C, Hp, Wp)


def _k(h, dt, hist, hcount, B, H, items, n_item, n_off, ref, tf, rescale, spec):
    """``nmpc_mmp_stem_*`` on the same arguments, rows flattened: float32 ``[n_item * n_off, C, Hp, Wp]``."""
    got = ts._run(h, dt, hist, hcount, B, H, items, n_item, n_off, ref, tf, rescale, spec)
    return got.reshape((n_item * n_off,) + got.shape[2:])


# ---- 1. bit equality: four maps, both transforms, both rescales, C, n_off ------------------------------------------------------------------
@pytest.mark.parametrize("rescale", [1.0, 2.0], ids=["r1", "r2"])
@pytest.mark.parametrize("tf_name", ["plain", "reversed"])
@pytest.mark.parametrize("map_name", ["synthetic", "crop", "wide", "long"])
def test_octets_are_the_packed_float32_output(handle, maps, map_name, tf_name, rescale):
    ref, tf = maps[map_name], mc.TRANSFORMS[tf_name]
    hist, hcount = mc.hist_arrays(mc.small_trajectories(tf, rescale))
    B, H = mc.B_SMALL, mc.H_SMALL
    rounds = False
    for C in (8, 64):
        spec = sr.random_spec(C, seed=C)
        for n_off in (1, 3):
            args = (np.float64, hist, hcount, B, H, None, B * H, n_off, ref, tf, rescale, spec)
            k = _k(handle, *args)
            assert _same(_io(handle, *args, 0), k), (C, n_off, "out_f16 = 0")
            got = _io(handle, *args, 1)
            assert _same(got, pack_activations_f16(k)), (C, n_off, "out_f16 = 1")
            rounds = rounds or not np.array_equal(unpack_activations_f16(got), k)
    assert rounds, "no value of K changed when it was rounded: the case shows nothing"


# ---- 2. both element types of hist, an item list with a gap and a repeat, 1 .. 5 distinct past positions ------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_both_hist_types_item_lists_and_history_lengths(handle, maps, dtype):
    ref, tf, rescale = maps["crop"], mc.TRANSFORMS["reversed"], 2.0
    trajs = mc.small_trajectories(tf, rescale)
    trajs[4] = trajs[4][-3:]                                   # (the nine have 1, 2, 4, 5 and 9 positions: one of three)
    hist, hcount = mc.hist_arrays(trajs)
    assert set(np.minimum(hcount, 5)) == {1, 2, 3, 4, 5} and np.array_equal(hist.astype(np.float32).astype(np.float64), hist)
    spec = sr.random_spec(8, seed=4)
    items = (0, 2, 2, 7, 4)                                    # a gap, a repeat, not ascending
    for its, n in ((None, 9), (items, len(items))):
        args = (dtype, hist, hcount, 3, 3, its, n, 3, ref, tf, rescale, spec)
        k = _k(handle, *args)
        assert _same(_io(handle, *args, 1), pack_activations_f16(k)) and _same(_io(handle, *args, 0), k), its
    full = _io(handle, dtype, hist, hcount, 3, 3, None, 9, 3, ref, tf, rescale, spec, 1).reshape(9, 3, 1, *_capi.mmp_stem_shape(*ref.shape), 8)
    listed = _io(handle, dtype, hist, hcount, 3, 3, items, len(items), 3, ref, tf, rescale, spec, 1).reshape((len(items),) + full.shape[1:])
    assert _same(listed, full[list(items)])
    rows = [full[q].tobytes() for q in range(9)]
    assert len(set(rows)) == 9, "two pedestrians gave the same octets: the item list is not seen"


# ---- 3. a negative slope takes the element-wise branch ----------------------------------------------------------------------------------------
def test_negative_slope(handle, maps):
    ref, tf, rescale = maps["wide"], mc.TRANSFORMS["plain"], 1.0
    hist, hcount = mc.hist_arrays(mc.small_trajectories(tf, rescale))
    neg = sr.random_spec(16, seed=5)._replace(slope=-0.5)
    pos = neg._replace(slope=0.5)
    args = (np.float64, hist, hcount, 3, 3, None, 9, 3, ref, tf, rescale)
    k = _k(handle, *args, neg)
    assert not np.array_equal(k, _k(handle, *args, pos)), "the slope's sign changed nothing"
    assert _same(_io(handle, *args, neg, 1), pack_activations_f16(k)) and _same(_io(handle, *args, neg, 0), k)


# ---- 4. saturation: beyond +-65504 the octets hold +-65504, never an infinity -------------------------------------------------------------------
def test_saturation(handle, maps):
    ref, tf, rescale = maps["synthetic"], mc.TRANSFORMS["plain"], 1.0
    hist, hcount = mc.hist_arrays(mc.small_trajectories(tf, rescale))
    spec = sr.random_spec(8, seed=6)
    spec = spec._replace(scale=(spec.scale * 3e4).astype(np.float32), slope=1.0)      # (slope 1: the negative side is as large)
    args = (np.float64, hist, hcount, 3, 3, None, 9, 3, ref, tf, rescale, spec)
    k = _k(handle, *args)
    assert (k > F16_MAX).any() and (k < -F16_MAX).any() and np.isfinite(k).all(), "the case does not leave the binary16 range"
    got = _io(handle, *args, 1)
    h = got.view(np.float16)
    assert np.isfinite(h).all() and (h == F16_MAX).any() and (h == -F16_MAX).any()
    assert _same(got, pack_activations_f16(k))
    over = np.abs(k) > F16_MAX
    assert np.array_equal(unpack_activations_f16(got)[over], np.sign(k[over]) * np.float32(F16_MAX))


# ---- 5. independence: item list, n_off, neighbours and the placement of out do not change a bit -----------------------------------------------
def test_bits_do_not_depend_on_item_list_offsets_neighbours_or_placement(handle, maps):
    ref, tf, rescale = maps["long"], mc.TRANSFORMS["plain"], 1.0
    hist, hcount = mc.hist_arrays(mc.small_trajectories(tf, rescale))
    spec = sr.random_spec(16, seed=3)
    Hp, Wp = _capi.mmp_stem_shape(*ref.shape)

    def run(items, n_item, n_off, shift=0, hist=hist):
        got = _io(handle, np.float64, hist, hcount, 3, 3, items, n_item, n_off, ref, tf, rescale, spec, 1, shift)
        return got.reshape(n_item, n_off, 2, Hp, Wp, 8)
    full = run(None, 9, 3)
    assert _same(run(mc.ITEMS_5, 5, 3), full[list(mc.ITEMS_5)])
    for k in (2, 6):
        assert _same(run([k], 1, 3)[0], full[k]), k
    assert _same(run(None, 9, 4)[:, :3], full) and _same(run(None, 9, 20)[:, :3], full) and _same(run(None, 9, 1), full[:, :1])
    for shift in (8, 16, 40):                              # out shifted by 16, 32 and 80 bytes
        assert _same(run(None, 9, 3, shift), full), shift
    other = hist.copy()
    other[[0, 1, 3, 5, 7, 8]] += 1.0                       # the neighbours of 2, 4 and 6 move
    moved = run(None, 9, 3, hist=other)
    assert _same(moved[[2, 4, 6]], full[[2, 4, 6]]) and not _same(moved[[0, 1]], full[[0, 1]])


# ---- 6. guarded buffers: nothing outside the arrays the entry reads changes a bit ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_guarded_buffers(handle, dtype):
    Hm, Wm, C, n_off = 37, 41, 16, 2
    tf = mc.TRANSFORMS["plain"]
    peds = ((1, (3.0, 2.0), (0.0, 0.0)), (3, (4.3125, 1.625), (0.25, 0.5)), (7, (1.5, 3.5), (0.5, -0.25)), (4, (5.25, 4.0), (-0.75, 0.25)))
    trajs = [mc.forward(tf, np.array(end)[None, :] - np.arange(n - 1, -1, -1)[:, None] * np.array(step)[None, :], 1.0) for n, end, step in peds]
    hist, hcount = mc.hist_arrays(trajs)
    assert np.array_equal(hist.astype(np.float32).astype(np.float64), hist)
    rng = np.random.default_rng(Hm * 100 + Wm)
    ref = np.where(rng.random((Hm, Wm)) < 0.25, rng.integers(0, 200, (Hm, Wm)), 255).astype(np.float32)
    spec = sr.random_spec(C, 50 + C)
    items = (0, 3)
    inputs = dict(items=np.array(items, dtype=np.int64), hist=np.ascontiguousarray(hist.reshape(2, 2, 5, 2), dtype=dtype), hcount=hcount.reshape(2, 2),
                  ref_image=ref, weight=np.ascontiguousarray(spec.weight, dtype=np.float32), bn_scale=np.ascontiguousarray(spec.scale, dtype=np.float32),
                  bn_shift=np.ascontiguousarray(spec.shift, dtype=np.float32))
    assert set(inputs) == {n for n, t in _capi.NmpcMmpStemArgs._fields_ if t is ctypes.c_void_p} - {"out"}
    Hp, Wp = _capi.mmp_stem_shape(Hm, Wm)
    n = len(items) * n_off * C * Hp * Wp

    def call(t):
        out = torch.full((n,), SENTINEL[np.dtype(np.int16)], dtype=torch.int16, device="cuda")
        a = _capi.NmpcMmpStemArgs().set_transform(tf, 1.0, 20.0)
        a.B, a.H, a.n_item, a.n_off, a.Hm, a.Wm = 2, 2, len(items), n_off, Hm, Wm
        for k, v in t.items():
            setattr(a, k, None if v is None else v.data_ptr())
        a.C, a.slope, a.out = C, spec.slope, out.data_ptr()
        handle.mmp_stem_io(dtype, a, 1)
        torch.cuda.synchronize()
        return {"out": out}
    poisons = {"items": IntPoison((1, 2), 0, 3), "hcount": IntPoison((1, 9), 0, 9)}
    got = run_guarded(call, inputs, device="cuda", int_poisons=poisons, odd_pad=list(inputs))["out"]
    k = _k(handle, dtype, hist, hcount, 2, 2, items, len(items), n_off, ref, tf, 1.0, spec)
    assert _same(got.view(np.uint16).reshape(len(items) * n_off, C // 8, Hp, Wp, 8), pack_activations_f16(k))


# ---- 7. refusals: before the device is touched, nothing is launched ------------------------------------------------------------------------------
def test_refusals(handle, maps):
    ref, tf = maps["synthetic"], mc.TRANSFORMS["plain"]
    hist, hcount = mc.hist_arrays(mc.small_trajectories(tf, 1.0))
    spec = sr.random_spec(8, seed=1)
    Hp, Wp = _capi.mmp_stem_shape(*ref.shape)
    POISON = -12345
    out = torch.full((8 + 9 * 3 * 8 * Hp * Wp,), POISON, dtype=torch.int16, device="cuda")
    assert out.data_ptr() % 16 == 0
    lib = nm.load_library()

    def make(**over):
        a, keep = ts._stem_args(np.float64, hist, hcount, 3, 3, None, 3, ref, tf, 1.0, spec)
        a.n_item, a.out = 9, out.data_ptr()
        for k, v in over.items():
            setattr(a, k, v)
        return a, keep

    def refused(a, flag, code, sentence=None, dt=np.float64):
        with pytest.raises(nm.NmpcError) as e:
            handle.mmp_stem_io(dt, a, flag)
        assert e.value.code == code, (e.value.code, str(e.value))
        if sentence is not None:
            assert sentence in str(e.value), str(e.value)
    # the flag
    for flag in (-1, 2, 3, 256):
        for dt in (np.float64, np.float32):
            refused(make()[0], flag, -1, f"nmpc_mmp_stem_io: out_f16 = {flag} (0 or 1)", dt)
    # a binary16 out off its 16 bytes (4, 8 and 12 bytes are float-aligned: the float32 form takes them)
    for off in (4, 8, 12):
        refused(make(out=out.data_ptr() + off)[0], 1, -1, "nmpc_mmp_stem_io: a binary16 out is not aligned to 16 bytes")
    refused(make(out=out.data_ptr() + 2)[0], 1, -1, "nmpc_mmp_stem: out is not aligned to float")
    refused(make(out=out.data_ptr() + 2)[0], 0, -1, "nmpc_mmp_stem: out is not aligned to float")
    # NULL handle or args
    a, keep = make()
    for fn in (lib.nmpc_mmp_stem_io_f64, lib.nmpc_mmp_stem_io_f32):
        assert fn(None, ctypes.byref(a), 1) == -1 and "null argument" in lib.nmpc_last_error().decode()
        assert fn(handle._h, None, 1) == -1 and "null argument" in lib.nmpc_last_error().decode()
    # everything nmpc_mmp_stem_* refuses, in its words, under both flags
    bad = {"hist = NULL": dict(hist=None), "hcount = NULL": dict(hcount=None), "ref_image = NULL": dict(ref_image=None), "out = NULL": dict(out=None),
           "weight = NULL": dict(weight=None), "bn_scale = NULL": dict(bn_scale=None), "bn_shift = NULL": dict(bn_shift=None),
           "n_item < 0": dict(n_item=-1), "n_item > B H": dict(n_item=10), "n_off = 0": dict(n_off=0), "Hm = 0": dict(Hm=0), "Wm = 0": dict(Wm=0),
           "sigma = 0": dict(sigma=0.0), "sigma < 0": dict(sigma=-20.0), "scale = 0": dict(scale=0.0), "B = 0": dict(B=0), "H = 0": dict(H=0),
           "C = 0": dict(C=0), "C = 4": dict(C=4), "C = 12": dict(C=12), "C < 0": dict(C=-8), "slope = nan": dict(slope=float("nan")),
           "slope = inf": dict(slope=float("inf"))}
    for what, over in bad.items():
        a, keep = make(**over)
        with pytest.raises(nm.NmpcError) as e0:
            handle.mmp_stem(np.float64, a)
        for flag in (0, 1):
            refused(a, flag, -1, str(e0.value).split(": ", 1)[-1])
    a, keep = make(B=1 << 15, H=1 << 15, n_item=1 << 30)
    refused(a, 1, -4, "workgroups")
    host = np.zeros(8, dtype=np.float32)
    refused(make(weight=host.ctypes.data)[0], 1, -1, "every array must be a device pointer")
    torch.cuda.synchronize()
    assert bool((out == POISON).all()), "a refused call wrote to the output"
    # n_item = 0 launches nothing and writes nothing
    for flag in (0, 1):
        handle.mmp_stem_io(np.float64, make(n_item=0)[0], flag)
    torch.cuda.synchronize()
    assert bool((out == POISON).all())
    handle.mmp_stem_io(np.float64, make()[0], 1)
    torch.cuda.synchronize()
    n = 9 * 3 * 8 * Hp * Wp
    assert bool((out[n:] == POISON).all()) and not bool((out[:n] == POISON).any())


# ---- by hand, not in the suite: the warehouse map in full at M = 2 -------------------------------------------------------------------------------
def warehouse_map_by_hand():
    """``PYTHONPATH=.:tests python -c "import test_gpu_mmp_stem_io as t; t.warehouse_map_by_hand()"`` from the repository root: 293 x 330, 64 channels, two offsets."""
    import oracle
    from conftest import config_for
    golden = __import__("os").path.join(__import__("os").path.dirname(__import__("os").path.abspath(__file__)), "golden")
    ref, tf = dict(mc.load_maps(golden))["warehouse"], mc.TRANSFORMS["warehouse"]
    hist, hcount = mc.hist_arrays([mc.warehouse_trajectory()])
    spec = sr.random_spec(64, seed=64)
    with nm.Handle(config_for(oracle.Problem())) as h:
        h.set_stream(torch.cuda.current_stream().cuda_stream)
        args = (np.float64, hist, hcount, 1, 1, None, 1, 2, ref, tf, 1.0, spec)
        k = _k(h, *args)
        got = _io(h, *args, 1)
        assert k.shape == (2, 64, 74, 83) and _same(got, pack_activations_f16(k)) and _same(_io(h, *args, 0), k)
        print(f"warehouse 293 x 330, M = 2: {got.size} halves equal pack(K) bit for bit; {int((unpack_activations_f16(got) != k).sum())} of them rounded")
