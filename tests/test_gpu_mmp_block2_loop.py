"""GPU tests of the fused second residual stage inside the closed loop: ``BatchEvaluator(predictor="mmp", network=trunk,
mmp_stem=spec, mmp_blocks=(...), mmp_blocks2=(...))`` and ``MmpInterface(trunk, stem=, blocks=, blocks2=)`` against the unfused
stage with the same trunk, bit for bit; and of ``MmpFrontEnd`` with ``blocks2`` in the manner of tests/test_gpu_mmp_front.py.

As in tests/test_gpu_mmp_block_loop.py the stem is the delta stem at 16 channels and layer1 three doubling blocks; layer2 is four
exact blocks of ``mmp_block2_reference``: the first at stride 2 duplicates the 16 channels to 32 through delta weights in ``w1``
and ``wd`` (out = 2 x[::2, ::2] on non-negative input), then three doublings. The trunk so sees exactly 128 x the pooled stack,
every second row and column, twice over, and nothing in front of it rounds. The unfused comparator is the same trunk behind that
expression in torch -- slice, ``cat``, ``x + x``: no convolution, so no library algorithm can round. The trunk reads the arg-max
of channels 19 (= 16 + 3) and 4 and the offset from channel 22 (= 16 + 6; / 128, exact): both copies are looked at."""
import numpy as np
import pytest
import torch

import dyobav_mpcnwta_warehouse_amd as nm
import mmp_block2_reference as b2
import mmp_block_reference as br
import mmp_cases as mc
import mmp_reference as mr
import mmp_stem_reference as sr
import oracle
from conftest import config_for
from dyobav_mpcnwta_warehouse_amd.evaluate import BatchEvaluator
from dyobav_mpcnwta_warehouse_amd.mmp_front import MmpFrontEnd
from dyobav_mpcnwta_warehouse_amd.mmp_stem import StemSpec
from dyobav_mpcnwta_warehouse_amd.snap import WorldTransform

pytestmark = pytest.mark.gpu

RESCALE, STEPS, B = 0.96, 6, 6
TF = WorldTransform(**vars(mc.TRANSFORMS["warehouse"]))
SPEC = sr.delta_spec(16)
BLOCKS = (br.doubling_block(),) * 3
BLOCKS2 = (b2.duplicate_and_double_block2(16),) + (b2.doubling_block2(),) * 3


def trunk_of(fan_):
    """[M, 32, H2, W2] = 128 x the pooled stack at every second pixel, twice -> [M, K, 2]: 8 (a4 + t (a4 - a3)) + t fan."""
    def trunk(x):
        M, C, H2, W2 = x.shape
        assert C == 32 and x.dtype == torch.float32
        f = torch.as_tensor(np.asarray(fan_, dtype=np.float32), device=x.device)
        i3, i4 = x[:, 19].reshape(M, -1).argmax(dim=1), x[:, 4].reshape(M, -1).argmax(dim=1)
        a3 = 8.0 * torch.stack([i3 % W2, i3 // W2], dim=1).to(torch.float32)
        a4 = 8.0 * torch.stack([i4 % W2, i4 // W2], dim=1).to(torch.float32)
        t = (x[:, 22, 0, 0] * 0.0078125)[:, None, None]
        return a4[:, None, :] + t * (a4 - a3)[:, None, :] + t * f[None]
    return trunk


def unfused(trunk):
    """The same trunk behind the delta stem, the three doubling blocks and the four exact blocks of layer2 written in torch on the
    input stack [M, 7, Hm, Wm]."""
    F = torch.nn.functional

    def network(x):
        assert x.shape[1] == 7
        sub = x[..., ::2, ::2]
        sub = torch.cat([sub] + [torch.zeros_like(sub[:, :1])] * 9, dim=1)
        y = F.max_pool2d(F.leaky_relu(sub, SPEC.slope), 3, 2, 1)
        for _ in range(3):
            y = y + y
        y = y[..., ::2, ::2]
        y = torch.cat([y, y], dim=1)
        for _ in range(4):
            y = y + y
        return trunk(y)
    return network


@pytest.fixture(scope="module")
def world(golden_dir):
    return dict(ref=mc.load_maps(golden_dir)["warehouse"])


def _scenarios(H, dead=None):
    sc = nm.scenarios.make_reference_scenarios(B, n_ped=H)
    sc.pop("scenario_index")
    if dead is not None:
        # scenario `dead` starts in the middle of the largest static rectangle: it collides in its first step and leaves
        polys = sc["map_polygons"]
        e1, e3 = polys[:, 1] - polys[:, 0], polys[:, 3] - polys[:, 0]
        area = np.abs(e1[:, 0] * e3[:, 1] - e1[:, 1] * e3[:, 0])
        sc["robot_starts"] = sc["robot_starts"].copy()
        sc["robot_starts"][dead, :2] = polys[int(area.argmax())].mean(axis=0)
    return sc


def _run(world, H, K, fused, dtype, sc=None, **kw):
    trunk = trunk_of(mr.fan(K, H))
    net = dict(network=trunk, mmp_stem=SPEC, mmp_blocks=BLOCKS, mmp_blocks2=BLOCKS2) if fused else dict(network=unfused(trunk))
    ev = BatchEvaluator(nm.default_config_struct(), dtype=dtype, predictor="mmp", mmp_hyp=K, ref_image=world["ref"], transform=TF,
                        rescale=RESCALE, **net, **kw, **(sc or _scenarios(H)))
    rec = []
    try:
        res = ev.run(max_steps=STEPS, record=rec)
    finally:
        ev.close()
    return ev, res, rec


def _assert_equal_runs(a, b):
    (_, res_a, rec_a), (_, res_b, rec_b) = a, b
    assert len(rec_a) == len(rec_b) == STEPS
    for t in range(STEPS):
        assert np.array_equal(rec_a[t]["alive"], rec_b[t]["alive"]), t
        for key in ("dyn", "n_obs", "n_outside", "P"):
            assert np.array_equal(rec_a[t][key], rec_b[t][key]), (t, key)
    assert np.array_equal(res_a.n_obs, res_b.n_obs) and np.array_equal(res_a.n_outside, res_b.n_outside)
    assert np.array_equal(res_a.trajectory, res_b.trajectory) and np.isfinite(res_a.trajectory).all()


# ---- 1. the closed loop with the fused stem, layer1 and layer2 equals the unfused stage, bit for bit -----------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", [(2, 5), (4, 20)], ids=["P10", "P80"])
def test_fused_loop_equals_the_unfused_loop(world, shape, dtype):
    H, K = shape
    fused, plain = (_run(world, H, K, f, dtype, compact=False) for f in (True, False))
    assert fused[0].mmp_row == (32, 37, 42) and plain[0].mmp_row == (7, 293, 330)
    # (a 16-channel stem's output is too small for the two 32-channel buffers of layer2: they are allocated, and counted)
    assert fused[0].mmp_chunk == (1 << 30) // (fused[0].N * ((16 + 32) * 74 * 83 + 64 * 37 * 42) * 4) and plain[0].mmp_chunk == 19
    _assert_equal_runs(fused, plain)
    assert (fused[1].n_obs[0] >= 1).all() and fused[1].steps.max() == STEPS


# ---- 2. compaction and chunking leave the bits alone ---------------------------------------------------------------------------------------
def test_fused_loop_with_compaction_and_with_a_chunk_of_one(world):
    H, K, dead = 4, 20, 1
    sc = _scenarios(H, dead=dead)
    fused, plain = (_run(world, H, K, f, np.float64, sc=sc, compact=True) for f in (True, False))
    assert fused[1].collision[dead] and fused[1].steps[dead] < STEPS and not fused[2][STEPS - 1]["alive"][dead], "the scenario was meant to leave early"
    _assert_equal_runs(fused, plain)
    one = _run(world, H, K, True, np.float64, sc=sc, compact=True, mmp_chunk=1)
    assert one[0].mmp_chunk == 1
    _assert_equal_runs(one, fused)


# ---- 3. the timing parts; what the evaluator refuses -----------------------------------------------------------------------------------------
def test_parts_and_refusals(world):
    trunk = trunk_of(mr.fan(5, 2))
    sc = _scenarios(2)
    common = dict(dtype=np.float32, predictor="mmp", network=trunk, mmp_hyp=5, ref_image=world["ref"], transform=TF, rescale=RESCALE, **sc)
    ev = BatchEvaluator(nm.default_config_struct(), mmp_stem=SPEC, mmp_blocks=BLOCKS, mmp_blocks2=BLOCKS2, **common)
    ev.time_predictor = ev.time_predictor_parts = True
    try:
        ev.run(max_steps=2)
    finally:
        ev.close()
    assert set(ev.predictor_part_ms) == {"input", "layer1", "layer2", "network", "snap", "f2"} and all(len(v) == 2 for v in ev.predictor_part_ms.values())
    assert ev.mmp_row == (32, 37, 42) and len(ev.mmp_blocks2) == 4 and ev.mmp_blocks2[0].w1.is_cuda
    with pytest.raises(ValueError, match="mmp_blocks2 needs mmp_blocks"):
        BatchEvaluator(nm.default_config_struct(), mmp_stem=SPEC, mmp_blocks2=BLOCKS2, **common)
    with pytest.raises(ValueError, match="mmp_blocks needs mmp_stem"):
        BatchEvaluator(nm.default_config_struct(), mmp_blocks=BLOCKS, mmp_blocks2=BLOCKS2, **common)
    with pytest.raises(ValueError, match="block 0 takes 32 channels"):
        BatchEvaluator(nm.default_config_struct(), mmp_stem=SPEC, mmp_blocks=BLOCKS, mmp_blocks2=BLOCKS2[1:], **common)
    with pytest.raises(ValueError, match="block 1 takes 16 channels"):
        BatchEvaluator(nm.default_config_struct(), mmp_stem=SPEC, mmp_blocks=BLOCKS, mmp_blocks2=BLOCKS2[:1] * 2, **common)
    with pytest.raises(ValueError, match="Block2Spec"):
        BatchEvaluator(nm.default_config_struct(), mmp_stem=SPEC, mmp_blocks=BLOCKS, mmp_blocks2=(BLOCKS2[0]._replace(stride=3),), **common)
    with pytest.raises(ValueError, match="Block2Spec"):
        BatchEvaluator(nm.default_config_struct(), mmp_stem=SPEC, mmp_blocks=BLOCKS, mmp_blocks2=(BLOCKS2[1]._replace(stride=2),), **common)


# ---- 4. the drop-in interface ------------------------------------------------------------------------------------------------------------------
def test_interface_with_blocks2_equals_the_unfused_interface(golden_dir):
    from dyobav_mpcnwta_warehouse_amd.mmp_interface import MmpInterface
    maps = mc.load_maps(golden_dir)
    with pytest.raises(ValueError, match="blocks2 needs blocks"):
        MmpInterface(trunk_of(mr.fan(5, 0)), stem=SPEC, blocks2=BLOCKS2)
    for case in mc.INTERFACE_CASES:
        trunk = trunk_of(mr.fan(case["K"], case["seed"]))
        fused, plain = MmpInterface(trunk, stem=SPEC, blocks=BLOCKS, blocks2=BLOCKS2), MmpInterface(unfused(trunk))
        try:
            ref = torch.from_numpy(maps[case["map"]].astype(np.float64))
            args = ([tuple(p) for p in case["traj"]], ref, case["pred_offset"], case["rescale"])
            for _ in range(2):                             # the second call reuses the handle, the map and the uploaded weights
                got = fused.get_motion_prediction(*args, batch_size=case["batch_size"])
                want = plain.get_motion_prediction(*args, batch_size=case["batch_size"])
                assert len(got) == len(want) == case["pred_offset"] and all(g.shape == (case["K"], 2) and g.dtype == np.float64 for g in got)
                assert np.array_equal(np.stack(got), np.stack(want)), case["name"]
        finally:
            fused.close()
            plain.close()


# ---- 5. MmpFrontEnd with blocks2: the wiring -------------------------------------------------------------------------------------------------
# A 37 x 41 map (the stem gives 10 x 11, layer2 5 x 6), 2 time offsets, 2 scenarios x 3 pedestrians, integer-valued weights. Two
# stems: 8 channels -- 2 x 32 x 5 x 6 floats do not fit its output, the buffers of layer2 are allocated -- and 64 channels, where
# they lie inside it, as for the real network. Layer2: stride 2 with a projection, then three identities.
HM, WM, N_OFF, FB, FH, SIGMA, FRESCALE = 37, 41, 2, 2, 3, 20.0, 2.0
HP, WP, H2, W2 = 10, 11, 5, 6
FTF = mc.TRANSFORMS["reversed"]
LENGTHS = (1, 3, 7, 5, 2, 7)
ITEMS, CHUNK = (4, 1, 5), 2
POINTERS = ("w1", "s1", "b1", "w2", "s2", "b2", "wd", "sd", "bd")


def _integer_stem(C, seed=8):
    rng = np.random.default_rng(seed)
    w = rng.choice([-1.0, 0.0, 0.0, 1.0], (C, 7, 7, 7)).astype(np.float32)
    return StemSpec(w, rng.choice([-2.0, -0.5, 0.5, 1.0], C).astype(np.float32), rng.integers(-3, 4, C).astype(np.float32), 0.125)


def _front_blocks(C):
    return (br.integer_block(C, 1, True), br.integer_block(16, 2, False), br.integer_block(16, 3, False))


FBLOCKS2 = (b2.integer_block2(16, 4, 2, True),) + tuple(b2.integer_block2(32, 5 + i, 1, False) for i in range(3))


@pytest.fixture(scope="module")
def handle():
    with nm.Handle(config_for(oracle.Problem())) as h:
        h.set_stream(torch.cuda.current_stream().cuda_stream)
        yield h


@pytest.fixture(scope="module")
def fworld():
    rng = np.random.default_rng(37)
    ref = np.where(rng.random((HM, WM)) < 0.25, rng.integers(0, 200, (HM, WM)), 255).astype(np.float32)
    trajs = []
    for n, (_, end, step, _) in zip(LENGTHS, mc.PEDESTRIANS):
        px = np.array(end)[None, :] - np.arange(n - 1, -1, -1)[:, None] * np.array(step)[None, :]
        trajs.append(mc.forward(FTF, px, FRESCALE))
    hist, hcount = mc.hist_arrays(trajs)
    hist, hcount = hist.reshape(FB, FH, 5, 2), hcount.reshape(FB, FH)
    return dict(hist=hist, hcount=hcount, d_ref=torch.from_numpy(ref).cuda(), d_hist=torch.from_numpy(hist).cuda(),
                d_hcount=torch.from_numpy(hcount).cuda())


def _front(handle, fworld, C, blocks2=FBLOCKS2, blocks="default"):
    return MmpFrontEnd(handle, dtype=np.float64, device=fworld["d_ref"].device, Hm=HM, Wm=WM, n_off=N_OFF, transform=FTF, rescale=FRESCALE,
                       sigma=SIGMA, ref_image=fworld["d_ref"], stem=_integer_stem(C), blocks=_front_blocks(C) if blocks == "default" else blocks,
                       blocks2=blocks2)


def _direct_layer2(handle, x):
    """The four blocks of FBLOCKS2 through the C ABI on x [M, 16, HP, WP], a buffer of its own per block: no ping-pong here."""
    keep = []
    for b in FBLOCKS2:
        g = nm._capi.NmpcMmpBlock2Args()
        g.M, g.Cin, g.H, g.W = (int(v) for v in x.shape)
        g.stride = b.stride
        out = torch.empty(g.M, 32, *b2.out_plane(g.H, g.W, b.stride), dtype=torch.float32, device="cuda")
        for name in POINTERS:
            if getattr(b, name) is not None:
                keep.append(torch.from_numpy(np.ascontiguousarray(getattr(b, name))).cuda())
                setattr(g, name, keep[-1].data_ptr())
        g.slope_mid, g.slope_out, g.x, g.out = b.slope_mid, b.slope_out, x.data_ptr(), out.data_ptr()
        handle.mmp_block2(g)
        keep.append(x)
        x = out
    torch.cuda.synchronize()
    return x


@pytest.mark.parametrize("C", [8, 64], ids=["allocated", "inside-the-stem-output"])
def test_front_end_with_blocks2(handle, fworld, C):
    items = torch.tensor(ITEMS, dtype=torch.long, device="cuda")
    fe, parent = _front(handle, fworld, C), _front(handle, fworld, C, blocks2=None)
    inside = C == 64
    assert fe.stage("layer2").in_fill == inside and fe.row == (32, H2, W2) and fe.fill_row == (C, HP, WP) and parent.row == (16, HP, WP)
    assert parent.bytes_per_item == N_OFF * (C + 32) * HP * WP * 4
    assert fe.bytes_per_item == parent.bytes_per_item + (0 if inside else N_OFF * 2 * 32 * H2 * W2 * 4)
    fe.allocate(CHUNK)
    parent.allocate(CHUNK)
    args = (fworld["d_hist"].data_ptr(), fworld["d_hcount"].data_ptr(), FB, FH)
    chunks = []
    for c0 in range(0, len(ITEMS), CHUNK):
        n, names = min(CHUNK, len(ITEMS) - c0), []
        got = fe.run(*args, items[c0:].data_ptr(), n, lambda what, call: (names.append(what), call())[1])
        assert names == ["input", "layer1", "layer2"]
        want = _direct_layer2(handle, parent.run(*args, items[c0:].data_ptr(), n))
        assert got.shape == want.shape == (n * N_OFF, 32, H2, W2) and got.dtype == torch.float32 and got.is_contiguous()
        assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0 and torch.equal(got, want), c0
        chunks.append(got.clone())
    assert not torch.equal(chunks[0][:N_OFF], chunks[0][N_OFF:]) and not torch.equal(chunks[0][:N_OFF], chunks[1])
    # one index space for run_block: 0 .. 2 layer1, 3 .. 6 layer2
    x = fe.fill(*args, items.data_ptr(), CHUNK)
    for i in range(7):
        fe.run_block(i, CHUNK * N_OFF)
    torch.cuda.synchronize()
    assert torch.equal(fe._out.view(-1)[:chunks[0].numel()].view(chunks[0].shape), chunks[0])
    with pytest.raises(IndexError):
        fe.run_block(7, 1)
    with pytest.raises(ValueError, match="allocate"):
        fe.run(*args, None, CHUNK + 1)
    assert fe.chunk == CHUNK and all(b.w1.is_cuda for b in fe.blocks2) and fe.blocks2[1].wd is None and fe.blocks2[0].stride == 2
    with pytest.raises(ValueError, match="blocks2 needs blocks"):
        _front(handle, fworld, C, blocks=None)
    with pytest.raises(ValueError, match="block 0 takes 32 channels"):
        _front(handle, fworld, C, blocks2=FBLOCKS2[1:])


def test_one_pedestrian_front_end_equals_the_batched_one(handle, fworld):
    batched, single = _front(handle, fworld, 64), _front(handle, fworld, 64)
    batched.allocate(1)
    single.allocate(1)
    for k in range(FB * FH):
        item = torch.tensor([k], dtype=torch.long, device="cuda")
        want = batched.run(fworld["d_hist"].data_ptr(), fworld["d_hcount"].data_ptr(), FB, FH, item.data_ptr(), 1).clone()
        hist = torch.from_numpy(np.ascontiguousarray(fworld["hist"].reshape(FB * FH, 1, 1, 5, 2)[k])).cuda()
        hcount = torch.from_numpy(np.ascontiguousarray(fworld["hcount"].reshape(FB * FH, 1, 1)[k])).cuda()
        got = single.run(hist.data_ptr(), hcount.data_ptr(), 1, 1, None, 1)
        torch.cuda.synchronize()
        assert got.shape == want.shape == (N_OFF, 32, H2, W2) and torch.equal(got, want), k
