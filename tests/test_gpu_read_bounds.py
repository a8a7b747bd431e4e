"""No kernel's result depends on memory outside its arguments: every entry point of include/nmpc_hip.h that takes arrays, called
through ``Handle`` / ``_capi`` with EVERY input array in a guarded buffer (tests/guarded_buffers.py: ``[pad | data | pad]`` in one
ordinary allocation, the pads poisoned). Per case the call runs once on plain exact-size tensors -- that run is compared with
the family's existing reference -- and once per poison (NaN, 0, +big, -big; two declared valid values for integer arrays) and
pad (64 elements, and 61 where the header asks no more than element alignment, which is everywhere). Every output must have the
same bits in every run, and no input pad may change. The batch is at least 2 everywhere: a read past row 0 lands in row 1, a
read past the last row in the pad.

The arrays each call reads, as the header states them. ``test_the_table_matches_the_argument_blocks`` checks the table against
the pointer fields of the ``_capi`` structures (a new field without a guard fails there), and every test asserts that its guarded
inputs are exactly its row.

    entry point                       reads (guarded)                                                     written only
    --------------------------------  ------------------------------------------------------------------  -----------------------
    mmp_input    NmpcMmpArgs          items hist hcount ref_image                                         out
    mmp_stem     NmpcMmpStemArgs      items hist hcount ref_image weight bn_scale bn_shift                out
    mmp_block    NmpcMmpBlockArgs     x w1 s1 b1 w2 s2 b2 wd sd bd                                        out
    mmp_block2   NmpcMmpBlock2Args    x w1 s1 b1 w2 s2 b2 wd sd bd                                        out
    mmp_block3   NmpcMmpBlock3Args    x w1 s1 b1 w2 s2 b2 wd sd bd                                        out
    kf_predict   NmpcKfArgs           run humans hcount kf_traj kf_len kf_P                               dyn_c
    dwa_step     NmpcDwaArgs          run state_c last_u_c dyn_c goal path path_len polys                 U_c min_cost choice counts cost_all cand_all
    assemble     NmpcAssembleArgs     last_u state ref_states speed_ref tuning other_robots map_polygons dyn_obstacles stc_weights dyn_weights   selected
    loop_pre_post  NmpcLoopArgs       run robot last_u humans hist hcount hidx hpath ref_traj ref_len idx_ref goal polys stagger alive collision complete steps clr_dyn clr_stc dev_sum dev_max n_traj traj acts U_c y_c U y   state_c last_u_c refs_c speed_c dyn_c
    snap         NmpcSnapArgs         raw                                                                 n_snapped n_outside hypos
    hypotheses   -                    hypos cur                                                           dyn n_obs
    eval         -                    P U Y C                                                             psi grad f2sq
    solve        -                    P u0 y c0 order                                                     U cost status iters info

(nmpc_loop_pre and nmpc_loop_post share their argument block and are guarded as the pair a time step makes: pre, then post with
the step's controls. ``raw`` / ``hypos`` of snap, the arrays of hypotheses, eval and solve and the dispatch ``order`` are plain arguments, not fields.)

Regions INSIDE an array that the header documents as not read are filled with each real poison in turn and must not change a bit
(``run_poisoned_regions``): ``path[b]`` from ``path_len[b]`` on and columns 2:6 of ``dyn_c`` for nmpc_dwa_step, ``kf_traj`` beyond
the appended row, ``y`` with ``y_is_input = 0``, the leading rows of ``hist[q]`` in front of row ``5 - n`` for the mmp front end,
``ref_traj[b]`` from ``ref_len[b]`` on."""
import functools
import re
import time

import numpy as np
import pytest
import torch

import dyobav_mpcnwta_warehouse_amd as nm
import oracle
from dyobav_mpcnwta_warehouse_amd import _capi
from dyobav_mpcnwta_warehouse_amd.scenarios import ParamLayout
from guarded_buffers import IntPoison, run_guarded, run_poisoned_regions

pytestmark = pytest.mark.gpu
DTYPES = (np.float64, np.float32)


def _table():
    """entry -> (structure name or None, arrays read, arrays written only), parsed from the module text."""
    rows = {}
    for line in __doc__.split("--  -----------------------\n")[1].split("\n\n")[0].splitlines():
        entry, struct, rest = line.split(None, 2)
        read, written = re.split(r"\s{3,}", rest.strip())
        rows[entry] = (None if struct == "-" else struct, tuple(read.split()), tuple(written.split()))
    return rows


TABLE = _table()


def _guard(entry, call, inputs, **kw):
    """``run_guarded`` on the device, after checking that the guarded inputs are the entry's row of the table."""
    assert set(inputs) == set(TABLE[entry][1]), (entry, sorted(inputs), TABLE[entry][1])
    kw.setdefault("odd_pad", [k for k, v in inputs.items() if v is not None])       # element alignment is all the header asks
    return run_guarded(call, inputs, device="cuda", **kw)


def test_the_table_matches_the_argument_blocks():
    assert set(TABLE) == {"mmp_input", "mmp_stem", "mmp_block", "mmp_block2", "mmp_block3", "kf_predict", "dwa_step", "assemble", "snap",
                          "hypotheses", "eval", "solve", "loop_pre_post"}
    import ctypes
    for entry, (struct, read, written) in TABLE.items():
        assert read and not set(read) & set(written), entry
        if struct is None:
            continue
        fields = [n for n, t in getattr(_capi, struct)._fields_ if t is ctypes.c_void_p]
        plain = {"snap": {"raw", "hypos"}}.get(entry, set())
        assert set(fields) == (set(read) | set(written)) - plain, (entry, sorted(set(fields) ^ ((set(read) | set(written)) - plain)))


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.time()
    yield
    print(f"\n[read bounds] {time.time() - t0:.1f} s")


def _own_stream(h):
    h.set_stream(torch.cuda.current_stream().cuda_stream)
    return h


@pytest.fixture(scope="module")
def handle():
    with nm.Handle(nm.default_config_struct()) as h:
        yield _own_stream(h)


_handles = {}


def _handle_for(N, Ndyn=15, ts=0.2):
    """A handle with these dimensions on torch's stream, kept for the module."""
    if (N, Ndyn, ts) not in _handles:
        cfg = nm.default_config_struct()
        cfg.N_hor, cfg.ts, cfg.Ndynobs = N, ts, Ndyn
        _handles[(N, Ndyn, ts)] = _own_stream(nm.Handle(cfg))
    return _handles[(N, Ndyn, ts)]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for h in _handles.values():
        h.close()
    _handles.clear()


def _tdt(dtype):
    return torch.float32 if np.dtype(dtype) == np.float32 else torch.float64


def _ptr(t):
    return None if t is None else t.data_ptr()


# ---- the residual blocks of the mmp network ----------------------------------------------------------------------------------
import mmp_block_reference as b1  # noqa: E402
import mmp_block2_reference as b2  # noqa: E402
import mmp_block3_reference as b3  # noqa: E402

# From each family's CASES the smallest plane with a ragged last tile in both directions (one row and one column of a second
# tile), once with and once without a projection; block3 also with Cin = 24 at stride 1 (a last chunk of sixteen with eight
# channels missing) and Cin = 8 at stride 2. (family, H, W, Cin, stride, projection)
BLOCK_CASES = [(1, 16, 29, 8, 1, True), (1, 16, 29, 16, 1, False),
               (2, 17, 89, 8, 2, True), (2, 9, 45, 32, 1, False),
               (3, 8, 22, 24, 1, True), (3, 8, 22, 64, 1, False), (3, 15, 43, 8, 2, True)]
BLOCK_WEIGHTS = ("w1", "s1", "b1", "w2", "s2", "b2", "wd", "sd", "bd")


@pytest.mark.parametrize("c", BLOCK_CASES, ids=lambda c: f"block{c[0]}-{c[1]}x{c[2]}-c{c[3]}-s{c[4]}")
def test_mmp_blocks(handle, c):
    family, H, W, Cin, stride, projection = c
    mod, entry = {1: (b1, "mmp_block"), 2: (b2, "mmp_block2"), 3: (b3, "mmp_block3")}[family]
    if family == 1:
        assert (H, W) in mod.PLANES and (Cin, projection) in mod.CHANNELS
        x, spec, want, bound = mod.case("random", H, W, Cin, projection)
        shape = (2, mod.C, H, W)
    else:
        assert (H, W, Cin, stride, projection) in mod.CASES
        x, spec, want, bound = mod.case("random", H, W, Cin, stride, projection)
        shape = (2, mod.C) + mod.out_plane(H, W, stride)
    th, tw = (15, 28) if family == 1 else mod.TILE
    assert shape[2] % th == 1 and shape[3] % tw == 1          # ragged both ways
    inputs = {"x": np.array(x[:2], dtype=np.float32)}
    inputs.update({k: None if getattr(spec, k) is None else np.array(getattr(spec, k), dtype=np.float32) for k in BLOCK_WEIGHTS})
    assert (inputs["wd"] is not None) == projection

    def call(t):
        a = {1: _capi.NmpcMmpBlockArgs, 2: _capi.NmpcMmpBlock2Args, 3: _capi.NmpcMmpBlock3Args}[family]()
        a.M, a.Cin, a.H, a.W = 2, Cin, H, W
        if family != 1:
            a.stride = stride
        for k, v in t.items():
            setattr(a, k, _ptr(v))
        a.slope_mid, a.slope_out = spec.slope_mid, spec.slope_out
        out = torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
        a.out = out.data_ptr()
        getattr(handle, entry)(a)
        torch.cuda.synchronize()
        return {"out": out}
    got = _guard(entry, call, inputs)["out"]
    assert np.isfinite(got).all() and (np.abs(got - want[:2]) <= bound[:2]).all()


# ---- nmpc_assemble_params ----------------------------------------------------------------------------------------------------
from oracle import assemble as oa  # noqa: E402


@functools.lru_cache(maxsize=None)
def _assemble_inputs(N, Nother, with_other, dtype):
    """B = 3, two map polygons more than slots would need none of, n_dyn = 3 < Ndynobs (the slots behind are zero padding: a
    pair read past a scenario's obstacles would land there)."""
    rng = np.random.default_rng(300 + N)
    B, n_dyn, M = 3, 3, 5
    f = lambda a: np.ascontiguousarray(a, dtype=dtype)
    state = np.c_[rng.uniform(-3, 3, (B, 2)), rng.uniform(-3, 3, B)]
    refs = np.concatenate([state[:, None, :2] + rng.uniform(-1, 1, (B, N, 2)), rng.uniform(-3, 3, (B, N, 1))], axis=2)
    ctr, half = rng.uniform(-5, 5, (M, 2)), rng.uniform(0.3, 1.0, (M, 2))
    polys = np.array([[1, 1], [-1, 1], [-1, -1], [1, -1]])[None] * half[:, None, :] + ctr[:, None, :]
    dyn = rng.uniform(-4, 4, (B, n_dyn, N + 1, 6))
    dyn[..., 2:4] = rng.uniform(0.2, 0.8, (B, n_dyn, N + 1, 2))
    dyn[..., 4], dyn[..., 5] = 0.0, 1.0
    return dict(last_u=f(rng.uniform(0.1, 1.0, (B, 2))), state=f(state), ref_states=f(refs), speed_ref=f(rng.uniform(0.5, 1.2, B)),
                tuning=f(nm.scenarios.WORK_MODE_Q), other_robots=f(rng.normal(size=(B, 3 * (N + 1) * Nother))) if with_other else None,
                map_polygons=f(polys), dyn_obstacles=f(dyn), stc_weights=f(rng.uniform(1, 10, N)), dyn_weights=f(rng.uniform(1, 10, N)))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("with_other", [True, False], ids=["others", "no-others"])
@pytest.mark.parametrize("N,Nother", [(20, 2), (5, 2), (4, 1)], ids=["N20", "N5", "N4-odd-blocks"])
def test_assemble_params(N, Nother, with_other, dtype):
    """N = 20 and N = 5 with two other robots: every block boundary of the row is even, so the pair mover runs when the pointers
    allow it (pad 64) and the element path when they do not (pad 61 elements); at N = 5 a scenario's obstacles are fewer pairs
    than the mover has threads. (The horizon alone never makes a boundary odd: the block of the other robots, 3 Nother (N + 1)
    long, is the only one that can.) N = 4 with one other robot has odd boundaries and takes the element path always."""
    Nstc, Ndyn = 3, 5
    lay = ParamLayout(N=N, Nother=Nother, Nstc=Nstc, Ndyn=Ndyn)
    cfg = nm.default_config_struct()
    cfg.N_hor, cfg.Nother, cfg.Nstcobs, cfg.Ndynobs = N, Nother, Nstc, Ndyn
    inputs = dict(_assemble_inputs(N, Nother, with_other, np.dtype(dtype)))
    B = inputs["state"].shape[0]
    with nm.Handle(cfg) as h:
        _own_stream(h)
        assert h.np_ == lay.np_ and (lay.os % 2 == 1) == (N == 4)

        def call(t):
            P = torch.full((B, h.np_), float("nan"), dtype=_tdt(dtype), device="cuda")
            sel = torch.full((B, Nstc), -9, dtype=torch.int32, device="cuda")
            h.assemble_params(dtype, B, P, t["last_u"], t["state"], t["ref_states"], t["speed_ref"], t["tuning"], t["stc_weights"],
                              t["dyn_weights"], t["map_polygons"], t["dyn_obstacles"], t["other_robots"], sel)
            torch.cuda.synchronize()
            return {"P": P, "selected": sel}
        got = _guard("assemble", call, inputs)
    d = {k: None if v is None else v.astype(np.float64) for k, v in inputs.items()}
    tol = 1e-11 if dtype == np.float64 else 2e-5
    for b in range(B):
        other = np.zeros(3 * (N + 1) * Nother) if d["other_robots"] is None else d["other_robots"][b]
        p = oa.assemble(d["last_u"][b], d["state"][b], d["ref_states"][b], d["speed_ref"][b], d["tuning"], other, list(d["map_polygons"]),
                        d["dyn_obstacles"][b], d["stc_weights"], d["dyn_weights"], N=N, Nother=Nother, Nstc=Nstc, Ndyn=Ndyn)
        row = got["P"][b].astype(np.float64)                  # the tolerances of tests/test_gpu_assemble.py
        assert not np.isnan(row).any()
        np.testing.assert_allclose(row[:lay.os], p[:lay.os], rtol=tol, atol=tol)
        np.testing.assert_allclose(row[lay.od:], p[lay.od:], rtol=tol, atol=tol)
        np.testing.assert_allclose(row[lay.os:lay.od], p[lay.os:lay.od], rtol=0, atol=1e-6 if dtype == np.float64 else 2e-3)
        assert (row[lay.od + 3 * 6 * (N + 1):lay.od + Ndyn * 6 * (N + 1)] == 0).all()        # the padding slots


# ---- nmpc_dwa_step ---------------------------------------------------------------------------------------------------------------
import dwa_cases as dc  # noqa: E402
import dwa_reference as dr  # noqa: E402

DWA_SEQUENCE = "one rectangle, H = 2, mode 2"
DWA_OUT = ("U_c", "min_cost", "choice", "counts", "cost_all", "cand_all")


@functools.lru_cache(maxsize=None)
def _dwa_inputs(dtype):
    """The three recorded calls of one sequence (M = 1, H = 2, the robot within half a metre of the origin, so that a stray
    pedestrian row of zeros is in reach) as the compact rows of scenarios 0, 2 and 4 of B = 5; scenarios 1 and 3 hold another
    goal and path. Pmax = 4 with three valid nodes: row 3 of every path is documented as not read, and so are columns 2:6 of
    dyn_c. The last call's pedestrians are the last rows of dyn_c: a read of pedestrian H lands in the pad."""
    s = next(q for q in dc.golden()["sequences"] if q["name"] == DWA_SEQUENCE)
    assert s["dyn_mode"] == 2 and len(s["calls"]) == 3 and len(s["polys"]) > 0
    f = lambda x: np.ascontiguousarray(np.asarray(x, dtype=dtype))
    calls, N = s["calls"], 20
    run = np.array([0, 2, 4], dtype=np.int64)
    B, Pmax = 5, 4
    goal = np.tile(np.asarray(s["goal"], dtype=float) + [3.0, -2.0], (B, 1))
    path = np.tile(np.concatenate([np.asarray(s["path"], dtype=float), [[-4.0, 7.0]]])[None] + [1.0, 2.0], (B, 1, 1))
    goal[run], path[run, :3] = np.asarray(s["goal"], dtype=float), np.asarray(s["path"], dtype=float)
    dyn = np.zeros((3, 2, N + 1, 6))
    dyn[..., :2] = np.stack([dc.call_dyn(s, c) for c in calls])
    dyn[..., 2:] = [0.2, 0.3, 0.0, 1.0]
    inputs = dict(run=run, state_c=f([c["state"] for c in calls]), last_u_c=f([c["last_u"] for c in calls]), dyn_c=f(dyn), goal=f(goal),
                  path=f(path), path_len=np.full(B, 3, dtype=np.int64), polys=f(dc.seq_polys(s)))
    assert np.hypot(*inputs["state_c"][-1, :2]) < 0.5
    return s, inputs


def _dwa_call(dtype, mode, cfg, inputs):
    h, N = _dwa_handle(), 20
    n_run, B, cap = 3, 5, 1
    for rng, acc, res in ((cfg.lin_vel_max - cfg.lin_vel_min, cfg.lin_acc_max, cfg.vel_resolution), (2 * cfg.ang_vel_max, cfg.ang_acc_max, cfg.ang_resolution)):
        cap *= int(min(rng, 2 * acc * 0.2) / res * (1 + 1e-9)) + 1           # the host's bound on nv nw (tests/test_gpu_dwa.py)

    def call(t):
        a = _capi.NmpcDwaArgs().set_config(cfg, 0.8)
        a.B, a.n_run, a.H, a.M, a.Pmax, a.cap, a.dyn_mode = B, n_run, 2, int(inputs["polys"].shape[0]), 4, cap, mode
        out = dict(U_c=torch.full((n_run, 2 * N), -7.5e6, dtype=_tdt(dtype), device="cuda"), min_cost=torch.full((n_run,), -7.5e6, dtype=_tdt(dtype), device="cuda"),
                   choice=torch.full((n_run,), -9, dtype=torch.int32, device="cuda"), counts=torch.full((n_run, 2), -9, dtype=torch.int32, device="cuda"),
                   cost_all=torch.full((n_run, cap), -7.5e6, dtype=_tdt(dtype), device="cuda"), cand_all=torch.full((n_run, cap, 2), -7.5e6, dtype=_tdt(dtype), device="cuda"))
        for k, v in {**t, **out}.items():
            setattr(a, k, _ptr(v))
        h.dwa_step(dtype, a)
        torch.cuda.synchronize()
        return out
    return call


def _dwa_handle():
    return _handle_for(20)


DWA_POISONS = {"run": IntPoison((1, 3), 0, 4), "path_len": IntPoison((2, 4), 2, 4)}


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("mode", [1, 2])
def test_dwa_step(mode, dtype):
    s, inputs = _dwa_inputs(np.dtype(dtype))
    cfg = dc.seq_config(s)
    got = _guard("dwa_step", _dwa_call(dtype, mode, cfg, inputs), dict(inputs), int_poisons=DWA_POISONS)
    g = dc.golden()
    tol_c, tol_d = 4 * g["delta_f32"]["cost"], 4 * g["delta_f32"]["dist"]
    d = {k: v.astype(np.float64) if v.dtype.kind == "f" else v for k, v in inputs.items()}
    for a, b in enumerate(inputs["run"]):                  # the comparisons of tests/test_gpu_dwa.py, sections 1 and 2
        want = dr.run_step(d["state_c"][a], d["goal"][b], d["last_u_c"][a], d["path"][b, :3], d["polys"], d["dyn_c"][a], mode, cfg, dtype)
        n = want["nv"] * want["nw"]
        assert tuple(got["counts"][a]) == (want["nv"], want["nw"]) and got["cand_all"][a, :n].tobytes() == want["cand"].astype(dtype).tobytes()
        cost, ref = got["cost_all"][a, :n].astype(np.float64), want["cost"].astype(np.float64)
        ok = np.ones(n, bool) if dtype == np.float64 else ~dr.near_threshold(want, tol_d)
        assert np.array_equal(np.isfinite(cost[ok]), np.isfinite(ref[ok])) and not np.isnan(cost).any()
        fin = ok & np.isfinite(ref)
        assert fin.sum() > n // 2
        err = np.abs(cost[fin] - ref[fin])
        assert (err <= (1e-9 * (1 + np.abs(ref[fin])) if dtype == np.float64 else tol_c)).all(), (a, err.max())
        if dtype == np.float64 and dc.cost_gap(ref) > 1e-6:
            assert got["choice"][a] == want["choice"]
    if mode == 1:
        assert s["calls"][0]["choice"] >= 0
    else:
        for a, c in enumerate(s["calls"]):                 # mode 2 is the recording itself
            assert dtype != np.float64 or got["choice"][a] == c["choice"]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_dwa_step_regions_that_are_not_read(dtype):
    """``path[b]`` from ``path_len[b]`` on; columns 2:6 of ``dyn_c``."""
    s, inputs = _dwa_inputs(np.dtype(dtype))
    beyond = np.zeros(inputs["path"].shape, bool)
    beyond[:, 3:] = True
    columns = np.zeros(inputs["dyn_c"].shape, bool)
    columns[..., 2:] = True
    for mode in (1, 2):
        run_poisoned_regions(_dwa_call(dtype, mode, dc.seq_config(s), inputs), dict(inputs), {"path": beyond, "dyn_c": columns}, device="cuda")


# ---- nmpc_kf_predict -------------------------------------------------------------------------------------------------------------
import kf_cases as kc  # noqa: E402
import kf_reference as kr  # noqa: E402
import test_gpu_kf_predict as tkf  # noqa: E402  (check_call: the comparison with the restatement)

# B = 3, H = 4, cap = 2 (kf_len 0, 1 and cap; the run list 0, 2 ends at the last scenario), and the fuzz set's own group with
# the last scenario alone in the run list (H = 5, cap = 41, dense matrices)
KF_CASES = {"B3-H4-cap2": dict(B=3, H=4, cap=2, N=5, mats="dense", run="alternate", seed=101), "B3-H5-cap41-last": 2}


def _kf_case(which, dtype):
    case = kc.round_inputs(kc.fuzz_group(KF_CASES[which]), dtype)
    d = case["dims"]
    assert d["B"] == 3 and case["run"][-1] == 2
    inputs = {k: np.ascontiguousarray(v, dtype=dtype if k in kr.REAL_KEYS else np.int64) for k, v in case["state"].items()}
    inputs["run"] = case["run"].astype(np.int64)
    return case, d, inputs


def _kf_call(case, d, dtype, masked=None):
    h = _handle_for(d["N"])
    n_run = len(case["run"])

    def call(t):
        a = _capi.NmpcKfArgs().set_matrices(*case["mats"])
        a.B, a.n_run, a.H, a.cap, a.human_size = d["B"], n_run, d["H"], d["cap"], case["human_size"]
        dyn = torch.full((d["B"], d["H"], d["N"] + 1, 6), kc.SENTINEL, dtype=_tdt(dtype), device="cuda")
        a.dyn_c = dyn.data_ptr()
        for k, v in t.items():
            setattr(a, k, _ptr(v))
        h.kf_predict(dtype, a)
        torch.cuda.synchronize()
        traj = t["kf_traj"].clone()
        if masked is not None:
            traj[torch.from_numpy(masked).cuda()] = 0
        return {"dyn_c": dyn, "kf_traj": traj, "kf_len": t["kf_len"], "kf_P": t["kf_P"], "humans": t["humans"], "hcount": t["hcount"]}
    return call


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("which", list(KF_CASES))
def test_kf_predict(which, dtype):
    case, d, inputs = _kf_case(which, dtype)
    B, cap = d["B"], d["cap"]
    poisons = {"run": IntPoison((1, 0), 0, B - 1), "hcount": IntPoison((1, cap), 0, cap + 2), "kf_len": IntPoison((1, cap), 0, cap)}
    got = _guard("kf_predict", _kf_call(case, d, dtype), inputs, int_poisons=poisons)
    before = {k: v for k, v in inputs.items() if k != "run"}
    tkf.check_call(before, got, got["dyn_c"], kc.reference(case), case["run"], d["N"], dtype, which, {})


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("which", list(KF_CASES))
def test_kf_predict_rows_beyond_the_stored_trajectory_are_not_read(which, dtype):
    """``kf_traj[b][h]`` from row ``kf_len`` on (the row a call appends is written, not read; the cases hold SENTINEL there)."""
    case, d, inputs = _kf_case(which, dtype)
    beyond = np.broadcast_to(np.arange(d["cap"])[None, None, :, None] >= inputs["kf_len"][:, :, None, None], inputs["kf_traj"].shape).copy()
    assert beyond.any() and (inputs["kf_traj"][beyond] == np.dtype(dtype).type(kc.SENTINEL)).all()
    run_poisoned_regions(_kf_call(case, d, dtype, masked=beyond), inputs, {"kf_traj": beyond}, device="cuda")


# ---- nmpc_eval_batch, nmpc_solve_batch --------------------------------------------------------------------------------------------
# (N, Ndynobs, pedestrians, hypotheses each) of tests/test_gpu_dims_sweep.py: the 4-slot, 6-slot and LDS obstacle tables at three
# lanes per step, two lanes per step, and the tiny problem
DIMS = [(20, 12, 2, 6), (20, 13, 1, 13), (20, 43, 1, 43), (33, 24, 4, 6), (5, 4, 2, 2)]
KERNELS = {"throughput": dict(latency_waves=1, coop_waves=1), "latency": dict(latency_waves=3, coop_waves=1),
           "cooperative": dict(latency_waves=1, coop_waves=4)}


@functools.lru_cache(maxsize=None)
def _problem(N, Ndyn, n_ped, n_hyp):
    """B = 3 instances, a point to evaluate at, multipliers, penalties; the oracle's psi / grad there and its short solve."""
    lay = ParamLayout(N=N, Ndyn=Ndyn)
    B = 3
    P = nm.scenarios.make_batch(B, lay, seed=100 + N + Ndyn, n_ped=n_ped, n_hyp=n_hyp, ped_mode="oncoming")
    rng = np.random.default_rng(N * 1000 + Ndyn)
    U = np.stack([rng.uniform(-0.3, 1.4, (B, N)), rng.uniform(-0.45, 0.45, (B, N))], axis=2).reshape(B, 2 * N)
    Y = rng.normal(size=(B, 2 * N)) * 2
    C = rng.uniform(1, 200, B)
    pr = oracle.Problem(N, lay.Nother, lay.Nstc, Ndyn)
    return lay, pr, P, U, Y, C


def _cfg(lay, **ov):
    cfg = nm.default_config_struct()
    cfg.N_hor, cfg.Nother, cfg.Nstcobs, cfg.Ndynobs = lay.N, lay.Nother, lay.Nstc, lay.Ndyn
    for k, v in ov.items():
        setattr(cfg, k, v)
    return cfg


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: f"N{d[0]}-dyn{d[1]}")
def test_eval_batch(dims, dtype):
    lay, pr, P, U, Y, C = _problem(*dims)
    B, n = P.shape[0], 2 * lay.N
    inputs = {k: np.ascontiguousarray(v, dtype=dtype) for k, v in (("P", P), ("U", U), ("Y", Y), ("C", C))}
    with nm.Handle(_cfg(lay)) as h:
        _own_stream(h)
        fn = getattr(h._lib, "nmpc_eval_batch_" + _capi._suffix(dtype))

        def call(t):
            out = dict(psi=torch.full((B,), float("nan"), dtype=_tdt(dtype), device="cuda"), grad=torch.full((B, n), float("nan"), dtype=_tdt(dtype), device="cuda"),
                       f2sq=torch.full((B,), float("nan"), dtype=_tdt(dtype), device="cuda"))
            _capi._check(fn(h._h, _ptr(t["P"]), _ptr(t["U"]), _ptr(t["Y"]), _ptr(t["C"]), B, _ptr(out["psi"]), _ptr(out["grad"]), _ptr(out["f2sq"])))
            torch.cuda.synchronize()
            return out
        got = _guard("eval", call, inputs)
    tp, tg = (1e-11, 1e-10) if dtype == np.float64 else (5e-5, 5e-4)          # tests/test_gpu_dims_sweep.py
    for i in range(B):
        v, g = oracle.psi(pr, U[i], C[i], Y[i], P[i])
        assert got["psi"][i] == pytest.approx(v, rel=tp), i
        np.testing.assert_allclose(got["grad"][i], g, rtol=0, atol=tg * max(1.0, np.abs(g).max()))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: f"N{d[0]}-dyn{d[1]}")
def test_solve_batch(dims, kernel, dtype):
    """One outer x three inner iterations from a given start, multipliers (``y_is_input = 1``) and penalties, with a device-side
    dispatch order. The same call with ``y_is_input = 0`` must not read ``y``: every poison in it gives the bits of zeros."""
    lay, pr, P, U, Y, C = _problem(*dims)
    B, n = P.shape[0], 2 * lay.N
    f = lambda a: np.ascontiguousarray(a, dtype=dtype)
    inputs = dict(P=f(P), u0=f(0.5 * U), y=f(0.1 * Y), c0=f(C), order=np.array([2, 0, 1], dtype=np.int32))
    short = dict(max_outer_iterations=1, max_inner_iterations=3, lip_eps_f64=1e-4, lip_delta_f64=1e-4)
    with nm.Handle(_cfg(lay, **short, **KERNELS[kernel])) as h:
        _own_stream(h)

        def solve(t, y_is_input):
            h.set_dispatch_order(t["order"])
            out = dict(U=torch.full((B, n), float("nan"), dtype=_tdt(dtype), device="cuda"), cost=torch.full((B,), float("nan"), dtype=_tdt(dtype), device="cuda"),
                       status=torch.full((B,), -9, dtype=torch.int32, device="cuda"), iters=torch.full((B, 2), -9, dtype=torch.int32, device="cuda"),
                       info=torch.full((B, 8), float("nan"), dtype=_tdt(dtype), device="cuda"))
            h.solve_raw(dtype, t["P"], B, out["U"], out["cost"], out["status"], out["iters"], t["u0"], t["y"], y_is_input, t["c0"], out["info"], True)
            torch.cuda.synchronize()
            out["y"] = t["y"]
            return out
        got = _guard("solve", lambda t: solve(t, True), inputs, int_poisons={"order": IntPoison((0, 2), 0, B - 1)})
        everywhere = np.ones((B, n), bool)
        cold = run_poisoned_regions(lambda t: {k: v for k, v in solve(t, False).items()}, dict(inputs, y=f(np.zeros((B, n)))), {"y": everywhere}, device="cuda")
    assert set(np.unique(got["status"])) <= {0, 1} and np.isfinite(got["U"]).all() and np.isfinite(got["y"]).all()
    assert not np.array_equal(cold["U"], got["U"])        # the multipliers given were used
    opt = lambda c: oracle.Options(max_outer=1, max_inner=3, lip_delta=1e-4, lip_eps=1e-4, initial_penalty=float(c))
    want = np.stack([oracle.solve(pr, opt(inputs["c0"][i]), inputs["P"][i].astype(np.float64), inputs["u0"][i], inputs["y"][i])[0] for i in range(B)])
    du = np.abs(got["U"].astype(np.float64) - want).max(axis=1)
    tol = 1e-7 if dtype == np.float64 else 2e-2                                # tests/test_gpu_dims_sweep.py
    assert np.median(du) < tol and du.max() < 50 * tol, (np.median(du), du.max())


# ---- nmpc_hypotheses_to_ellipses -----------------------------------------------------------------------------------------------------
import fuzz_hypotheses as fz  # noqa: E402
import hypotheses_cases as hc  # noqa: E402


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_hypotheses_to_ellipses(dtype):
    """B = 2, N = 5, P = 7, H = 2 (nine groups of seven points in a wavefront: one pass, the last lane idle)."""
    B, N, P, H, Ndyn = 2, 5, 7, 2, 4
    hypos, cur = hc.blobs(B, N, P, H, 1.0, 7, dtype)
    par = hc.DEFAULT
    inputs = {"hypos": np.ascontiguousarray(hypos, dtype=dtype), "cur": np.ascontiguousarray(cur, dtype=dtype)}
    with fz.handle(N, Ndyn) as h:
        _own_stream(h)

        def call(t):
            dyn = torch.full((B, Ndyn, N + 1, 6), float("nan"), dtype=_tdt(dtype), device="cuda")
            nobs = torch.full((B,), -7, dtype=torch.int32, device="cuda")
            rc = fz.call(h, dtype, t["hypos"], P, t["cur"], H, par, B, dyn, nobs)
            torch.cuda.synchronize()
            assert rc == 0, h._lib.nmpc_last_error()
            return {"dyn": dyn, "n_obs": nobs}
        got = _guard("hypotheses", call, inputs)
    want, want_n = fz.reference(hypos, cur, par, Ndyn)
    msg = fz.compare(dtype, got["dyn"].astype(np.float64), got["n_obs"], hypos, cur, par, Ndyn, want, want_n)
    assert msg is None, msg


# ---- nmpc_mmp_input, nmpc_mmp_stem -----------------------------------------------------------------------------------------------
import mmp_cases as mc  # noqa: E402
import mmp_reference as mr  # noqa: E402
import mmp_stem_reference as msr  # noqa: E402

# 37 x 41 = 1517 floats per plane: dword stores; 6 x 7 = 42: dwordx2; 6 x 8 = 48: dwordx4 (an aligned ``out``)
MMP_MAPS = {(37, 41): 1, (6, 7): 2, (6, 8): 4}
# (past-trajectory length, newest centre in pixels, step per entry): 2 scenarios x 2 pedestrians with 1, 3, 7 and 4 past positions
MMP_PEDESTRIANS = ((1, (3.0, 2.0), (0.0, 0.0)), (3, (4.3125, 1.625), (0.25, 0.5)), (7, (1.5, 3.5), (0.5, -0.25)), (4, (5.25, 4.0), (-0.75, 0.25)))
MMP_ITEMS = (0, 3)                  # the first and the last pedestrian (ascending, as the header asks)
MMP_POISONS = {"items": IntPoison((1, 2), 0, 3), "hcount": IntPoison((1, 9), 0, 9)}
FLT_MIN = float(np.finfo(np.float32).tiny)


@functools.lru_cache(maxsize=None)
def _mmp_inputs(Hm, Wm, dtype):
    tf = mc.TRANSFORMS["plain"]
    trajs = [mc.forward(tf, np.array(end)[None, :] - np.arange(n - 1, -1, -1)[:, None] * np.array(step)[None, :], 1.0) for n, end, step in MMP_PEDESTRIANS]
    hist, hcount = mc.hist_arrays(trajs)
    assert list(hcount) == [1, 3, 7, 4] and np.array_equal(hist.astype(np.float32).astype(np.float64), hist)      # dyadic: exact in float32
    rng = np.random.default_rng(Hm * 100 + Wm)
    ref = np.where(rng.random((Hm, Wm)) < 0.25, rng.integers(0, 200, (Hm, Wm)), 255).astype(np.float32)
    inputs = dict(items=np.array(MMP_ITEMS, dtype=np.int64), hist=np.ascontiguousarray(hist.reshape(2, 2, 5, 2), dtype=dtype), hcount=hcount.reshape(2, 2), ref_image=ref)
    return tf, trajs, inputs


def _mmp_args(a, tf, n_off, Hm, Wm, t):
    a.set_transform(tf, 1.0, 20.0)
    a.B, a.H, a.n_item, a.n_off, a.Hm, a.Wm = 2, 2, len(MMP_ITEMS), n_off, Hm, Wm
    for k, v in t.items():
        setattr(a, k, _ptr(v))
    return a


def _unread_rows_of_hist(inputs):
    """The leading rows of ``hist[q]`` in front of row ``5 - n``."""
    n = np.minimum(inputs["hcount"], 5)
    mask = np.broadcast_to(np.arange(5)[None, None, :, None] < (5 - n)[:, :, None, None], inputs["hist"].shape).copy()
    assert mask.any()
    return {"hist": mask}


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("shape", list(MMP_MAPS), ids=lambda s: f"{s[0]}x{s[1]}")
def test_mmp_input(handle, shape, dtype):
    Hm, Wm = shape
    tf, trajs, inputs = _mmp_inputs(Hm, Wm, np.dtype(dtype))
    n_off = 2
    V = MMP_MAPS[shape]
    assert (Hm * Wm) % V == 0 and (V == 4 or (Hm * Wm) % (2 * V))

    def call(t):
        out = torch.full((len(MMP_ITEMS), n_off, 7, Hm, Wm), float("nan"), dtype=torch.float32, device="cuda")
        a = _mmp_args(_capi.NmpcMmpArgs(), tf, n_off, Hm, Wm, t)
        a.out = out.data_ptr()
        handle.mmp_input(dtype, a)
        torch.cuda.synchronize()
        return {"out": out}
    got = _guard("mmp_input", call, dict(inputs), int_poisons=MMP_POISONS)["out"]
    run_poisoned_regions(call, dict(inputs), _unread_rows_of_hist(inputs), device="cuda")
    for i, q in enumerate(MMP_ITEMS):                      # the comparison of tests/test_gpu_mmp_input.py, with the restatement
        want = mr.input_stack(mr.input_planes(mr.to_pixels(trajs[q], tf, 1.0), inputs["ref_image"]), n_off)
        steps = mr.ulp_distance_f32(got[i, :, :5], want[:, :5])
        dist = np.abs(got[i, :, :5].astype(np.float64) - want[:, :5].astype(np.float64))
        assert np.isfinite(got[i]).all() and ((steps <= 1) | (dist <= FLT_MIN)).all() and np.array_equal(got[i, :, 5:], want[:, 5:]), q


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("C", [8, 16])
def test_mmp_stem(handle, C, dtype):
    Hm, Wm = 37, 41
    tf, trajs, inputs = _mmp_inputs(Hm, Wm, np.dtype(dtype))
    spec = msr.random_spec(C, 50 + C)
    inputs = dict(inputs, weight=np.ascontiguousarray(spec.weight, dtype=np.float32), bn_scale=np.ascontiguousarray(spec.scale, dtype=np.float32),
                  bn_shift=np.ascontiguousarray(spec.shift, dtype=np.float32))
    n_off = 2
    shape = (len(MMP_ITEMS), n_off, C) + _capi.mmp_stem_shape(Hm, Wm)

    def call(t):
        out = torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
        a = _mmp_args(_capi.NmpcMmpStemArgs(), tf, n_off, Hm, Wm, t)
        a.C, a.slope, a.out = C, spec.slope, out.data_ptr()
        handle.mmp_stem(dtype, a)
        torch.cuda.synchronize()
        return {"out": out}
    got = _guard("mmp_stem", call, inputs, int_poisons=MMP_POISONS)["out"]
    run_poisoned_regions(call, inputs, _unread_rows_of_hist(inputs), device="cuda")
    for i, q in enumerate(MMP_ITEMS):                      # the bound of tests/test_gpu_mmp_stem.py: 352 x 2^-24 x (|scale| S + |shift|)
        want, bound = msr.stage(mr.to_pixels(trajs[q], tf, 1.0), inputs["ref_image"], n_off, spec)
        assert np.isfinite(got[i]).all() and (np.abs(got[i] - want) <= 352 * msr.U * bound).all(), q


# ---- nmpc_snap_hypotheses --------------------------------------------------------------------------------------------------------
import snap_reference as snr  # noqa: E402
from test_snap_cpu import load_maps as load_snap_maps  # noqa: E402


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_snap_hypotheses(golden_dir, dtype):
    """The smallest golden map (synthetic, 24 x 31); B = 2 scenarios x 2 offsets, 2 pedestrians x 3 hypotheses = 6 points per
    offset; half of the points in occupied cells, a quarter on integer coordinates (exact ties between edge pixels)."""
    _, occupied, edge = load_snap_maps(golden_dir)[0]["synthetic"]
    B, N, n_ped, K = 2, 2, 2, 3
    rng = np.random.default_rng(61)
    Hm, Wm = occupied.shape
    rr, cc = np.nonzero(occupied)
    j = rng.integers(len(rr), size=(B, N, n_ped * K))
    inside = rng.random((B, N, n_ped * K)) < 0.5
    cell = np.stack([np.where(inside, cc[j], rng.integers(Wm, size=j.shape)), np.where(inside, rr[j], rng.integers(Hm, size=j.shape))], axis=-1)
    raw = cell + rng.integers(0, 8, cell.shape) / 8.0 * (rng.random(cell.shape[:-1] + (1,)) >= 0.25)          # exact in float32
    tf = mc.TRANSFORMS["reversed"]
    want, ns_w, no_w = snr.snap(raw, n_ped, K, occupied, edge, tf, 2.0)
    assert 0 < ns_w.sum() < raw.size // 2
    with nm.Handle(_cfg(ParamLayout(N=N))) as h:
        _own_stream(h)
        h.set_map(occupied, edge)

        def call(t):
            out = torch.full(t["raw"].shape, float("nan"), dtype=_tdt(dtype), device="cuda")
            ns = torch.full((B, N, n_ped), -1, dtype=torch.int32, device="cuda")
            no = torch.full((B,), -1, dtype=torch.int32, device="cuda")
            h.snap_hypotheses(dtype, t["raw"], out, n_ped, K, tf, 2.0, ns, no)
            torch.cuda.synchronize()
            return {"hypos": out, "n_snapped": ns, "n_outside": no}
        got = _guard("snap", call, {"raw": np.ascontiguousarray(raw, dtype=dtype)})
    assert np.array_equal(got["hypos"], want.astype(dtype)) and np.array_equal(got["n_snapped"], ns_w) and np.array_equal(got["n_outside"], no_w.sum(axis=1))


# ---- nmpc_loop_pre, nmpc_loop_post -----------------------------------------------------------------------------------------------
import step_cases as sc  # noqa: E402
import step_reference as stp  # noqa: E402
import test_gpu_step_kernels as tsk  # noqa: E402  (check_call_pair: the comparison with the restatement)

# the smallest groups of step_cases.FUZZ_GROUPS with a run list with gaps: n_hyp = 1 (N 33, H 63) and n_hyp = 3 (N 64, H 5)
LOOP_GROUPS = {"n_hyp1": 5, "n_hyp3": 7}
LOOP_COMPACT = ("state_c", "last_u_c", "refs_c", "speed_c", "dyn_c")


@functools.lru_cache(maxsize=None)
def _loop_case(g, dtype):
    case = sc.round_inputs(sc.fuzz_group(g), dtype)
    assert case["run"] is not None and case["dims"]["n_hyp"] in (1, 3)
    inputs = {k: np.ascontiguousarray(v, dtype=dtype if k in stp.REAL_KEYS else np.int64 if k in stp.INT_KEYS else np.uint8)
              for k, v in case["state"].items()}
    real = lambda x: None if x is None else np.ascontiguousarray(x, dtype=dtype)
    inputs.update(run=case["run"].astype(np.int64), stagger=real(case["stagger"]), U_c=real(case["U_c"]), y_c=real(case["y_c"]))
    return case, inputs


def _loop_poisons(case):
    d, B = case["dims"], case["dims"]["B"]
    flag = IntPoison((0, 1), 0, 1)
    return dict(run=IntPoison((1, B - 2), 0, B - 1), hcount=IntPoison((1, 5), 0, 1 << 40), hidx=IntPoison((0, d["W"]), 0, d["W"]),
                ref_len=IntPoison((1, d["Lmax"]), 1, d["Lmax"]), idx_ref=IntPoison((0, 1), 0, d["Lmax"] - 1),
                steps=IntPoison((0, 1), 0, sc.MAX_STEPS), alive=flag, collision=flag, complete=flag)


def _loop_call(case, dtype):
    """One ``nmpc_loop_pre`` call, then one ``nmpc_loop_post`` call with the case's controls and multipliers, on the tensors
    given: -> the compact buffers behind each call and the state behind each call."""
    d, c = case["dims"], case["consts"]
    N, H, nh, B = d["N"], d["H"], max(1, d["n_hyp"]), d["B"]
    n_run = len(case["run"])
    h = tsk._handle(N, float(np.float64(case.get("handle_ts", sc.TS))))
    state_keys = tuple(case["state"])

    def call(t):
        sent = lambda *shape: torch.full(shape, tsk.SENTINEL, dtype=_tdt(dtype), device="cuda")
        out = {}
        for post in (False, True):
            comp = dict(state_c=sent(n_run, 3), last_u_c=sent(n_run, 2), refs_c=sent(n_run, N, 3), speed_c=sent(n_run), dyn_c=sent(n_run, H * nh, N + 1, 6),
                        U_c=t["U_c"] if post else sent(n_run, 2 * N), y_c=t["y_c"] if post else sent(n_run, 2 * N))
            a = _capi.NmpcLoopArgs()
            a.B, a.n_run, a.H, a.W, a.Lmax, a.M, a.step, a.max_steps = B, n_run, H, d["W"], d["Lmax"], d["M"], case["step"], sc.MAX_STEPS
            a.base_speed, a.lin_vel_max, a.human_size, a.human_vmax = c["base_speed"], d["lin_vel_max"], c["human_size"], c["human_vmax"]
            a.n_hyp, a.hyp_fan_rad, a.hyp_radius0, a.hyp_radius_growth = d["n_hyp"], c["hyp_fan"], c["hyp_r0"], c["hyp_grow"]
            a.gather_y = 1
            for k in state_keys:
                setattr(a, k, _ptr(t[k]))
            a.run = _ptr(t["run"])
            a.stagger = _ptr(t["stagger"]) if post else None
            for k, v in comp.items():
                setattr(a, k, v.data_ptr())
            h.loop_step(dtype, a, post=post)
            torch.cuda.synchronize()
            tag = "post" if post else "pre"
            out.update({f"{tag}/{k}": v.clone() for k, v in comp.items()})
            out.update({f"after_{tag}/{k}": t[k].clone() for k in state_keys})
        return out
    return call


def _split(got, tag):
    return {k.split("/", 1)[1]: v for k, v in got.items() if k.startswith(tag + "/")}


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("which", list(LOOP_GROUPS))
def test_loop_pre_and_post(which, dtype):
    case, inputs = _loop_case(LOOP_GROUPS[which], np.dtype(dtype))
    got = _guard("loop_pre_post", _loop_call(case, dtype), dict(inputs), int_poisons=_loop_poisons(case))
    before = {k: inputs[k] for k in case["state"]}
    # (scenarios whose decisions sit within rounding of a threshold are compared with the device's decision forced; their share
    # is a figure of the whole fuzz set, which tests/test_gpu_step_kernels.py asserts)
    tsk.check_call_pair(case, dtype, before, _split(got, "pre"), _split(got, "after_pre"), _split(got, "post"), _split(got, "after_post"), which, {}, {})


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_loop_pre_does_not_read_the_reference_trajectory_beyond_its_length(dtype):
    """``ref_traj[b]`` from ``ref_len[b]`` on."""
    case, inputs = _loop_case(LOOP_GROUPS["n_hyp1"], np.dtype(dtype))
    beyond = np.broadcast_to(np.arange(case["dims"]["Lmax"])[None, :, None] >= inputs["ref_len"][:, None, None], inputs["ref_traj"].shape).copy()
    assert beyond.any()
    call = _loop_call(case, dtype)
    rest = lambda t: {k: v for k, v in call(t).items() if not k.endswith("/ref_traj")}        # (the array itself comes back as it went in)
    run_poisoned_regions(rest, dict(inputs), {"ref_traj": beyond}, device="cuda")
