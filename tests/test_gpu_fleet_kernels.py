"""The two fleet kernels (csrc/nmpc_fleet.h) ONE call at a time through the C ABI (nmpc_fleet_exchange_* / nmpc_fleet_post_*),
fp32 and fp64, against tests/fleet_reference.py -- the numpy statement whose rollout and layout tests/test_fleet_reference_cpu.py
ties to the reference project and to the oracle's cost.

Bars (those of tests/test_gpu_step_kernels.py). fp64: 1e-12 x the coordinate scale (fleet_cases.COORD). fp32: four times the
float32 error of the numpy reference against its float64 self on the same float32-rounded inputs, measured here over the cases
of the test. Copies (c_0, the peers at rest) are compared bit for bit. Discrete outcomes -- which peer in which slot, the
collision flags -- are compared wherever the reference's margin exceeds 16 eps x the largest coordinate; below it the robot is
left out (at most 1 % of a test's robots, never on the constructed ties, which are compared exactly).

Shapes: G = 3 groups; R in {1, 2, 3, Nother - 1, Nother, Nother + 1} for Nother in {1, 2, 3, 10} (Nother = 1: capacity 0, an
all-zero block), R = 64 once; N in {5, 20}; U_prev NULL; stopped members; a compact run list that drops members of the middle
group and the whole last group; equal distances; a pair exactly vehicle_width apart and one float to either side; completion
and collision in one step; a parked peer hit by a running one; other_c pre-filled with NaN.
"""
import numpy as np
import pytest

import fleet_cases as fc
import fleet_reference as fr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    fc.close_handles()


def _thr(dtype):
    return 16 * float(np.finfo(dtype).eps) * fc.COORD


def _check_exchange(h, dtype, case, Nother, run, with_U, stats):
    """One call against the reference. ``stats``: dict collecting 'robots', 'excluded', 'twin' (float32 twin error), 'worst'."""
    R, N = case["R"], case["N"]
    U = case["U"] if with_U else None
    got, t = fc.call_exchange(h, dtype, case["robot"], U, case["alive"], R, run=run)
    # every element was overwritten: nothing of the NaN pre-fill is left
    assert np.isfinite(got).all(), "elements of other_c were not written"
    # the inputs are inputs
    assert np.array_equal(t["robot"].cpu().numpy().astype(np.float64), case["robot"])
    assert np.array_equal(t["alive"].cpu().numpy(), case["alive"])
    if U is not None:
        assert np.array_equal(t["U"].cpu().numpy().astype(np.float64), U)
    want, peers, margins = fr.exchange(case["robot"], U, case["alive"], R, N, Nother, fc.TS, run=run)
    assert got.shape == want.shape
    rows = np.arange(case["B"]) if run is None else run
    sure = margins > _thr(dtype)
    stats["robots"] += len(rows)
    stats["excluded"] += int((~sure).sum())
    if np.dtype(dtype) == np.float32:
        twin, tp, _ = fr.exchange(case["robot"], U, case["alive"], R, N, Nother, fc.TS, run=run, dtype=np.float32)
        same = np.array([tp[a] == peers[a] for a in range(len(rows))], dtype=bool)
        ok = sure & same
        if ok.any():
            stats["twin"] = max(stats["twin"], float(np.abs(twin[ok].astype(np.float64) - want[ok]).max()))
    L = fr.block_len(N, Nother)
    for a in range(len(rows)):
        if not sure[a]:
            continue
        g, w = got[a].astype(np.float64), want[a]
        # slot 0 and the unused slots are zeros, exactly
        used = np.zeros(L, dtype=bool)
        for s in range(1, len(peers[a]) + 1):
            used[3 * s:3 * s + 3] = True
            used[fr.c_index(s, 0, N, Nother):fr.c_index(s, 0, N, Nother) + 3 * N] = True
        assert not g[~used].any(), (rows[a], "a slot that must be zero is not")
        for s, m in enumerate(peers[a], start=1):
            # c_0 is a copy: which peer sits in which slot, bit for bit
            assert np.array_equal(g[3 * s:3 * s + 3], case["robot"][m]), (rows[a], s, m, g[3 * s:3 * s + 3], case["robot"][m])
            i0 = fr.c_index(s, 0, N, Nother)
            if U is None or not case["alive"][m]:
                assert np.array_equal(g[i0:i0 + 3 * N], np.tile(case["robot"][m], N)), (rows[a], s, "a peer at rest is its state, N times")
        stats["worst"] = max(stats["worst"], float(np.abs(g - w).max()))
        stats["rows"].append((g, w))


def _finish(dtype, stats, where):
    assert stats["excluded"] <= 0.01 * stats["robots"], (where, stats["excluded"], stats["robots"])
    bound = 1e-12 * fc.COORD if np.dtype(dtype) == np.float64 else 4 * stats["twin"]
    print(f"{where}: {stats['robots']} robots, {stats['excluded']} below the margin; worst |error| {stats['worst']:.3e}, bound {bound:.3e}"
          + (f" (4 x the reference's float32 twin error {stats['twin']:.3e})" if np.dtype(dtype) == np.float32 else ""))
    for g, w in stats["rows"]:
        assert np.abs(g - w).max() <= bound, (where, float(np.abs(g - w).max()), bound)


def _stats():
    return dict(robots=0, excluded=0, twin=0.0, worst=0.0, rows=[])


@pytest.mark.parametrize("N", [5, 20])
@pytest.mark.parametrize("Nother", [1, 2, 3, 10])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_exchange_against_the_reference(dtype, Nother, N):
    h = fc.handle(N, Nother)
    stats = _stats()
    for R in fc.group_sizes(Nother):
        case = fc.make_case(20261, R, N, dtype)
        for run in fc.run_lists(R):
            for with_U in (True, False):
                _check_exchange(h, dtype, case, Nother, run, with_U, stats)
    _finish(dtype, stats, f"exchange {np.dtype(dtype).name} Nother={Nother} N={N}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_exchange_with_64_members(dtype):
    h = fc.handle(20, 10)
    stats = _stats()
    case = fc.make_case(20262, 64, 20, dtype, spread=6.0)
    for run in fc.run_lists(64):
        _check_exchange(h, dtype, case, 10, run, True, stats)
    _finish(dtype, stats, f"exchange {np.dtype(dtype).name} R=64")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_exchange_equal_distances_go_to_the_lower_index(dtype):
    # member 2 between mirror images on integer coordinates: 1 and 3 tie at 1, 0 and 4 at 2; seen from 0 and 4, 1 and 3 tie at sqrt(5)
    robot = np.array([[-2, 0, 0.5], [0, 1, 1.0], [0, 0, 1.5], [0, -1, 2.0], [2, 0, 2.5]], dtype=np.float64)
    robot = np.concatenate([robot, robot + [[7.0, 3.0, 0.0]], robot[::-1] + [[-5.0, 2.0, 0.0]]])      # three groups; the last one reversed
    alive = np.ones(15, dtype=np.uint8)
    for Nother, N in ((3, 5), (2, 5), (10, 20)):
        h = fc.handle(N, Nother)
        got, _ = fc.call_exchange(h, dtype, robot, None, alive, 5)
        want, peers, margins = fr.exchange(robot, None, alive, 5, N, Nother, fc.TS)
        assert margins[2] == 0.0 and margins[7] == 0.0 and margins[12] == 0.0          # the ties are ties
        assert peers[2][:min(2, Nother - 1)] == [1, 3][:Nother - 1] and peers[12][:min(2, Nother - 1)] == [11, 13][:Nother - 1]
        # everything here is a copy of integer-valued states: the whole block, bit for bit
        assert np.array_equal(got.astype(np.float64), want), (Nother, N)


def _post_state(B, dtype, clr=np.inf):
    z = lambda v=0: np.full(B, v, dtype=np.uint8)
    return dict(clr_fleet=np.full(B, clr, dtype=np.float64), collision=z(), complete=z(), alive=z(1), collision_fleet=z())


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_post_against_the_reference(dtype):
    h = fc.handle(5, 3)
    robots = excluded = hits = misses = 0
    twin = worst = 0.0
    pairs = []
    rng = np.random.default_rng(20263)
    for R in (1, 2, 3, 9, 10, 11, 64):
        case = fc.make_case(20263, R, 5, dtype, spread=0.8 if R < 9 else 3.0)       # close enough that some pairs collide
        B = case["B"]
        st = _post_state(B, dtype)
        st["clr_fleet"] = np.asarray(np.where(rng.random(B) < 0.5, np.inf, rng.uniform(0.0, 6.0, B)), dtype=dtype).astype(np.float64)
        st["complete"] = (rng.random(B) < 0.3).astype(np.uint8)
        st["alive"] = np.where(st["complete"] == 1, 0, case["alive"]).astype(np.uint8)
        for run in fc.run_lists(R):
            got, _ = fc.call_post(h, dtype, case["robot"], R, st, run=run)
            want, margins = fr.post(case["robot"], R, fc.WIDTH, st["clr_fleet"], st["collision"], st["complete"], st["alive"],
                                    st["collision_fleet"], run=run)
            rows = np.arange(B) if run is None else run
            rest = np.setdiff1d(np.arange(B), rows)
            sure = margins > _thr(dtype)
            robots += len(rows)
            excluded += int((~sure).sum())
            for k in fc.POST_KEYS:      # a robot outside the run list is never written
                assert np.array_equal(got[k][rest].astype(np.float64), np.asarray(st[k])[rest].astype(np.float64)), (R, k)
            for k in fc.POST_KEYS[1:]:
                assert np.array_equal(got[k][rows[sure]], want[k][rows[sure]]), (R, k)
            g, w = got["clr_fleet"][rows].astype(np.float64), want["clr_fleet"][rows]
            assert np.array_equal(np.isinf(g), np.isinf(w))
            fin = np.isfinite(w)
            if fin.any():
                worst = max(worst, float(np.abs(g[fin] - w[fin]).max()))
                pairs.append((g[fin], w[fin]))
                if np.dtype(dtype) == np.float32:
                    t32, _ = fr.post(case["robot"], R, fc.WIDTH, st["clr_fleet"], st["collision"], st["complete"], st["alive"],
                                     st["collision_fleet"], run=run, dtype=np.float32)
                    twin = max(twin, float(np.abs(t32["clr_fleet"][rows][fin].astype(np.float64) - w[fin]).max()))
        hits += int(want["collision_fleet"].sum())
        misses += int((want["collision_fleet"][want["alive"] == 1] == 0).sum())
    assert hits >= 10 and misses >= 10, (hits, misses)        # both answers occur
    assert excluded <= 0.01 * robots, (excluded, robots)
    bound = 1e-12 * fc.COORD if np.dtype(dtype) == np.float64 else 4 * twin
    print(f"post {np.dtype(dtype).name}: {robots} robots, {excluded} below the margin; worst |error| of clr_fleet {worst:.3e}, bound {bound:.3e}")
    for g, w in pairs:
        assert np.abs(g - w).max() <= bound


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_post_constructed_decisions(dtype):
    """Exact decisions: `<=` at exactly vehicle_width (axis-aligned: the distance is exact) and one float to either side; a
    completion and a collision in one step; a parked robot hit by a running one keeps its record."""
    h = fc.handle(5, 3)
    t = np.dtype(dtype).type
    w = t(fc.WIDTH)
    below, above = np.nextafter(w, t(0)), np.nextafter(w, t(1))
    a = -float(w) / 2       # (a + d has the finer spacing of w / 2: the difference is d exactly)
    robot = np.array([[a, 3, 0], [a + float(w), 3, 0],              # group 0: exactly the width -> both collide
                      [7, a, 0], [7, a + float(below), 0],          # group 1: one float below -> both collide
                      [-9, a, 0], [-9, a + float(above), 0],        # group 2: one float above -> none
                      [4, 4, 0], [4.2, 4, 0],                       # group 3: 6 completed this very step, is hit: the collision wins
                      [-4, -4, 0], [-4, -4.3, 0]], dtype=np.float64)  # group 4: 9 is parked (not in the run list), 8 runs into it
    for i, d in ((0, w), (2, below), (4, above)):
        assert t(robot[i + 1, 0 if i == 0 else 1]) - t(robot[i, 0 if i == 0 else 1]) == d
    st = _post_state(10, dtype)
    st["complete"][6], st["alive"][6] = 1, 0
    st["complete"][9], st["alive"][9], st["clr_fleet"][9] = 1, 0, 2.5
    run = np.arange(9, dtype=np.int64)
    got, _ = fc.call_post(h, dtype, robot, 2, st, run=run)
    want, _ = fr.post(robot, 2, fc.WIDTH, st["clr_fleet"], st["collision"], st["complete"], st["alive"], st["collision_fleet"], run=run,
                      dtype=dtype)
    assert want["collision"].tolist() == [1, 1, 1, 1, 0, 0, 1, 1, 1, 0]
    assert want["complete"].tolist() == [0] * 9 + [1] and want["alive"].tolist() == [0, 0, 0, 0, 1, 1, 0, 0, 0, 0]
    for k in fc.POST_KEYS[1:]:
        assert np.array_equal(got[k], want[k]), k
    assert got["clr_fleet"][9] == 2.5                                  # the parked robot's record
    assert got["clr_fleet"][0] == w and got["clr_fleet"][2] == below and got["clr_fleet"][4] == above
    assert np.allclose(got["clr_fleet"][:9].astype(np.float64), want["clr_fleet"][:9].astype(np.float64), rtol=4 * float(np.finfo(dtype).eps), atol=0)
    # width <= 0 means the handle's vehicle_width; an explicit one is taken
    got2, _ = fc.call_post(h, dtype, robot, 2, st, run=run, width=float(below))
    assert got2["collision"].tolist() == [0, 0, 1, 1, 0, 0, 1, 1, 1, 0]


def test_bad_inputs_are_refused_with_one_sentence():
    import torch
    import dyobav_mpcnwta_warehouse_amd as nm
    from dyobav_mpcnwta_warehouse_amd import _capi
    h = fc.handle(5, 3)
    robot = torch.zeros(6, 3, dtype=torch.float64, device="cuda")
    flags = [torch.zeros(6, dtype=torch.uint8, device="cuda") for _ in range(3)]
    clr = torch.zeros(6, dtype=torch.float64, device="cuda")
    out = torch.zeros(6, fr.block_len(5, 3), dtype=torch.float64, device="cuda")

    def args(**kw):
        a = _capi.NmpcFleetArgs()
        a.B, a.R, a.n_run = 6, 2, 6
        a.robot, a.alive, a.collision, a.complete = robot.data_ptr(), flags[0].data_ptr(), flags[1].data_ptr(), flags[2].data_ptr()
        a.clr_fleet, a.other_c = clr.data_ptr(), out.data_ptr()
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    for call in (h.fleet_exchange, h.fleet_post):
        for kw in (dict(R=0), dict(R=65, B=130, n_run=130), dict(R=4), dict(robot=None), dict(n_run=7), dict(n_run=3), dict(n_run=-1)):
            with pytest.raises(nm.NmpcError) as e:
                call(np.float64, args(**kw))
            msg = str(e.value)
            assert "nmpc_fleet" in msg and msg.count(". ") == 0, (kw, msg)
        with pytest.raises(nm.NmpcError):
            call(np.float64, None)
    for kw in (dict(other_c=None), dict(alive=None, U_prev=out.data_ptr())):
        with pytest.raises(nm.NmpcError):
            h.fleet_exchange(np.float64, args(**kw))
    for kw in (dict(alive=None), dict(clr_fleet=None), dict(collision=None), dict(complete=None)):
        with pytest.raises(nm.NmpcError):
            h.fleet_post(np.float64, args(**kw))
    # n_run = 0 does nothing
    h.fleet_exchange(np.float64, args(n_run=0))
    h.fleet_post(np.float64, args(n_run=0))
    torch.cuda.synchronize()
