"""tests/handle_history.py without a device: the tour holds every ordered pair of plans with both batches on either side;
run_tour reports the right pair on fake handles whose answers depend on their history -- by one step, only after a larger
batch, only two calls back -- and passes an honest one; and the tour's ten batch sizes reach the plans they claim, by
csrc/nmpc_plan.h compiled with g++ (the driver of tests/test_plan_cpu.py) at 1 024 SIMDs."""
import numpy as np
import pytest

import handle_history as hh
from plan_cases import PLAN_IDS, plans
from test_plan_cpu import LATENCY, THROUGHPUT, _case, plan  # noqa: F401  (plan: the module's fixture, the g++ driver)


# ---- the tour -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_tour_holds_every_ordered_pair_once(n):
    t = hh.tour(n)
    assert len(t) == n * n + 1 and t[0][0] == t[-1][0]
    plan_pairs = [(a[0], b[0]) for a, b in hh.pairs(t)]
    assert sorted(plan_pairs) == [(i, j) for i in range(n) for j in range(n)]
    for p in range(n):                                      # the k-th visit of a plan takes a / b by the parity of k
        assert [w for q, w in t if q == p] == ["ab"[k % 2] for k in range(sum(q == p for q, _ in t))]


def test_tour_of_the_five_plans_has_both_batches_on_both_sides():
    t = hh.tour(5)
    assert len(t) == 26 and len({(a[0], b[0]) for a, b in hh.pairs(t)}) == 25
    previous, current = {a for a, _ in hh.pairs(t)}, {b for _, b in hh.pairs(t)}
    every = {(p, w) for p in range(5) for w in "ab"}
    assert previous == every and current == every
    # consecutive visits of one plan (the pair (p, p)) alternate between a and b: data, size and pair member all change
    assert all(a[1] != b[1] for a, b in hh.pairs(t) if a[0] == b[0])


# ---- run_tour on fake handles -------------------------------------------------------------------------------------------------
class Fake:
    """solve() answers from P alone (row sums), plus whatever `leak(history of B, B)` adds to the iteration counts."""

    def __init__(self, leak=None):
        self.leak, self.seen = leak, []

    def solve(self, P):
        B = len(P)
        s = P.sum(axis=1)
        extra = self.leak(self.seen, B) if self.leak else 0
        self.seen.append(B)
        self.li = dict(family="latency", axis_aligned=2, staged_outer_iterations=0, polish_selected=0, tail_handed_off=0, deep_parked=0,
                       order_source=2)
        return dict(U=np.stack([s, -s], axis=1), y=np.stack([s * 0, s], axis=1), cost=s * s, status=(s > 0).astype(np.int32),
                    iters=np.stack([np.arange(B), np.arange(B) + extra], axis=1).astype(np.int32), info=np.tile(s[:, None], (1, 8)))

    def last_launch_info(self):
        return self.li


SIZES = {0: (5, 6), 1: (9, 12), 2: (17, 20)}                 # plan -> (B of a, B of b): the tour's first two steps do not shrink


def _fake_tour(leak):
    visits = hh.tour(3)
    rng = np.random.default_rng(1)
    batches = {(p, w): rng.normal(size=(SIZES[p]["ab".index(w)], 4)) for p in range(3) for w in "ab"}
    refs = {v: hh.call(Fake(), batches[v]) for v in batches}
    return visits, batches, refs, (lambda: Fake(leak))


def test_run_tour_passes_an_honest_handle():
    visits, batches, refs, fresh = _fake_tour(None)
    hh.run_tour(fresh(), visits, refs, batches, want={p: dict(family="latency", order_source=2) for p in range(3)}, fresh=fresh)


def test_run_tour_names_the_pair_of_a_one_step_leak():
    """The previous call's B is added to an iteration count: the very first pair fails, and fails alone."""
    visits, batches, refs, fresh = _fake_tour(lambda seen, B: seen[-1] if seen else 0)
    with pytest.raises(hh.HistoryMismatch) as e:
        hh.run_tour(fresh(), visits, refs, batches, fresh=fresh)
    assert e.value.position == 1 and e.value.pair == (visits[0], visits[1]) and e.value.pair_alone is True
    B = len(batches[visits[1]])
    assert f"iters differs from the fresh handle's in {B} of {B} instances" in str(e.value) and "one-step leak" in str(e.value)


def test_run_tour_names_the_pair_of_a_leak_behind_a_larger_batch():
    """The leak shows only where the previous batch was LARGER (rows beyond this call's B left in a grow-only buffer)."""
    visits, batches, refs, fresh = _fake_tour(lambda seen, B: 1 if seen and seen[-1] > B else 0)
    first = next(i for i, (a, b) in enumerate(hh.pairs(visits), 1) if len(batches[a]) > len(batches[b]))
    assert first > 1                                        # (pairs before it pass: the previous batch was no larger)
    with pytest.raises(hh.HistoryMismatch) as e:
        hh.run_tour(fresh(), visits, refs, batches, fresh=fresh)
    assert e.value.position == first and e.value.pair == (visits[first - 1], visits[first]) and e.value.pair_alone is True
    assert len(batches[e.value.pair[0]]) > len(batches[e.value.pair[1]])


def test_run_tour_tells_a_longer_history_from_a_one_step_leak():
    """The leak comes from TWO calls back: the report names the pair at which it shows and says that the pair alone is clean."""
    visits, batches, refs, fresh = _fake_tour(lambda seen, B: seen[-2] if len(seen) >= 2 else 0)
    with pytest.raises(hh.HistoryMismatch) as e:
        hh.run_tour(fresh(), visits, refs, batches, fresh=fresh)
    assert e.value.position == 2 and e.value.pair == (visits[1], visits[2]) and e.value.pair_alone is False
    assert "does NOT reproduce" in str(e.value)


def test_run_tour_checks_the_plan_and_the_launch_info():
    visits, batches, refs, fresh = _fake_tour(None)
    with pytest.raises(hh.HistoryMismatch, match="not the intended plan: order_source = 2, expected 3"):
        hh.run_tour(fresh(), visits, refs, batches, want={p: dict(order_source=3) for p in range(3)}, fresh=fresh)

    class Sticky(Fake):                                     # (a tail hand-off reported one call too long)
        def last_launch_info(self):
            return dict(self.li, tail_handed_off=256 if len(self.seen) > 1 else 0)
    with pytest.raises(hh.HistoryMismatch, match="launch info tail_handed_off = 256, fresh handle 0") as e:
        hh.run_tour(Sticky(), visits, refs, batches, fresh=Sticky)
    assert e.value.position == 1 and e.value.pair_alone is True


def test_compare_counts_instances_and_takes_nans_as_equal():
    r, li = hh.call(Fake(), np.arange(24.0).reshape(6, 4))
    r["cost"][2] = np.nan
    other = {k: v.copy() for k, v in r.items()}
    hh.compare((other, li), (r, li), "nan")
    other["U"][1, 1] += 1e-12
    other["U"][4] = 0
    with pytest.raises(hh.HistoryMismatch, match="U differs from the fresh handle's in 2 of 6 instances"):
        hh.compare((other, li), (r, li), "two rows")
    other = {k: v.copy() for k, v in r.items()}
    other["info"][:, 6:] += 1                               # launch diagnostics: not compared
    hh.compare((other, li), (r, li), "diagnostics")
    other["info"][3, 5] += 1
    with pytest.raises(hh.HistoryMismatch, match="info differs from the fresh handle's in 1 of 6"):
        hh.compare((other, li), (r, li), "info")
    with pytest.raises(hh.HistoryMismatch, match="deep_parked > tail_handed_off"):
        hh.compare((r, dict(li, deep_parked=1)), (r, li), "deep parks")


# ---- the tour's sizes reach the plans they claim ----------------------------------------------------------------------------
DIMS, HINT_ROWS = (20, 10, 10, 15), 10


def test_tour_sizes_reach_their_plans_at_1024_simds(plan):
    S = 1024
    park = max(32, S // 4)
    table = plans(S)
    assert [name for name, *_ in table] == PLAN_IDS
    sizes = hh.tour_sizes(S)
    family = {"latency": LATENCY, "throughput": THROUGHPUT}
    for (name, dtype, B, want, two_waves), (Ba, Bb) in zip(table, sizes):
        assert Ba == B and abs(Bb - Ba) % 2 == 1 and abs(Bb - Ba) % 64 != 0 and 0 < abs(Bb - Ba) < 64, (name, Ba, Bb)
        elem = np.dtype(dtype).itemsize
        for r, Bx in zip(plan([_case(DIMS, HINT_ROWS, elem, Bx, S) for Bx in (Ba, Bb)]), (Ba, Bb)):
            assert r["mode"] == family[want["family"]], (name, Bx, r)
            assert r["last_order"] == want["order_source"] and r["last_staged"] == want["staged_outer_iterations"], (name, Bx, r)
            assert r["last_tail"] == want["tail_handed_off"] and want["tail_handed_off"] in (0, park), (name, Bx, r)
            assert r["threads"] == (128 if two_waves else r["threads"]) and r["reg_slots"] == (4 if elem == 4 else 0), (name, Bx, r)
            assert r["has_axis"] == (elem == 4), (name, r)      # fp32: a kernel pair, the member decided on the device
    # b is the smaller batch wherever the plan leaves room below a; the pilot plan begins AT a (one instance fewer: another plan)
    below = plan([_case(DIMS, HINT_ROWS, 4, 24 * S - 1, S)])[0]
    assert below["last_order"] == 2 and below["last_staged"] == 0
    assert [Bb < Ba for Ba, Bb in sizes] == [name != "throughput-pilot-tail" for name in PLAN_IDS]


def test_sizes_of_the_workspace_and_staged_cooperative_cases(plan):
    """What tests/test_gpu_handle_history.py states about its other configurations, at 1 024 SIMDs: N = 40 with 160 rows runs the
    on-chip cooperative kernel in fp32 and streams the table through the workspace in fp64 (automatic, and on one wavefront
    with latency_waves = coop_waves = 1, reg_table = -1); the staged cooperative plan (kCoopStageFills fills) is reached in
    fp64 on the tour's dimensions with coop_waves = 4 from B = 2 S on -- two workgroups of four wavefronts per CU."""
    S = 1024
    big = (40, 10, 10, 160)
    f32, f64, one = plan([_case(big, 0, 4, 6, S), _case(big, 0, 8, 6, S), _case(big, 0, 8, 6, S, latency_waves=1, coop_waves=1, reg_table=-1)])
    assert f32["mode"] == 2 and f32["threads"] == 512 and not f32["uses_ws"] and f32["reg_slots"] == 12
    assert f64["mode"] == 2 and f64["threads"] == 256 and f64["uses_ws"] and f64["pair"]
    assert one["mode"] == THROUGHPUT and one["threads"] == 64 and one["uses_ws"]
    at, below = plan([_case(DIMS, HINT_ROWS, 8, 2 * S, S, coop_waves=4), _case(DIMS, HINT_ROWS, 8, 2 * S - 1, S, coop_waves=4)])
    assert at["mode"] == 2 and at["resident"] == S // 2 and not at["uses_ws"], at
    assert at["last_staged"] == 1 and at["last_order"] == 3 and at["launch_rounds"] == 2, at
    assert below["mode"] == 2 and below["last_staged"] == 0 and below["last_order"] == 0, below
