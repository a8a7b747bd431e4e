"""One handle through a history of calls. A handle (nmpc_handle_s, csrc/nmpc_capi.hip) carries counters, flags, grow-only
buffers, staging buffers, a dispatch order and the polish's selection from call to call; most of it is right only by an
invariant that every call leaves behind for the next one. The property checked with the help of this module: a call's result
on a handle with ANY history equals, bit for bit, its result on a handle just created with the same configuration.

* tour_sizes / tour_batch: two batches per plan of tests/plan_cases.py -- `a` as plan_batch makes it (axis-aligned ellipses), `b`
  with another seed, another size inside the same plan thresholds and a rotated ellipse in every seventh instance -- so that
  consecutive visits of a plan differ in data, in size and in the member of the kernel pair that the device picks.
* tour(n): a closed walk over n plans with every ordered pair (previous, current), a plan behind itself included.
* compare: the comparison of plan_cases.same() plus the timing-independent fields of nmpc_last_launch_info.
* run_tour: the visits on one handle, each against its fresh-handle reference; the first mismatch is reported with its pair,
  its position, and whether the pair alone on a new handle reproduces it (a one-step leak) or not (a longer history).

Nothing here touches a device when it is imported; tests/test_handle_history_cpu.py runs run_tour on fake handles."""
import numpy as np

KEYS = ("U", "y", "cost", "status", "iters")
# nmpc_last_launch_info without what depends on timing (deep_parked: only deep_parked <= tail_handed_off)
LAUNCH_KEYS = ("family", "axis_aligned", "staged_outer_iterations", "polish_selected", "tail_handed_off", "order_source")
ODD = 37                                        # what batch `b` differs by: odd, hence no multiple of 64 (nor of a 256-thread block)


class HistoryMismatch(AssertionError):
    """A call on a used handle differs from the same call on a fresh one. `pair` = (previous visit, current visit),
    `position` = index of the current visit in the tour, `pair_alone` = whether the pair by itself on a new handle reproduces
    the mismatch (None: not tried)."""

    def __init__(self, msg, pair=None, position=None, pair_alone=None):
        super().__init__(msg)
        self.pair, self.position, self.pair_alone = pair, position, pair_alone


# ---- the plans' two batches ---------------------------------------------------------------------------------------------------
def tour_sizes(S=None):
    """[(B of batch a, B of batch b)] per plan of plan_cases.plans(S). b is a little smaller wherever the plan's thresholds
    leave room below a; the pilot plan begins AT a = 24 S = eight fills of 3 S (csrc/nmpc_plan.h, kProxyFills: below it the
    order comes from one evaluation), so there b is a little larger. tests/test_handle_history_cpu.py evaluates plan_solve for
    all ten sizes."""
    from plan_cases import plans
    return [(B, B + ODD if name == "throughput-pilot-tail" else B - ODD) for name, _, B, _, _ in plans(S)]


def rotate_every_seventh(P, lay):
    """A rotated ellipse in every seventh instance, as tests/test_gpu_tail.py writes it (a rotated circle would still be
    axis-aligned): the call goes to the general member of the kernel pair (axis_aligned = 0: decided on the device)."""
    B = P.shape[0]
    rows = P[:, lay.od:lay.od + lay.Ndyn * (lay.N + 1) * 6].reshape(B, lay.Ndyn, lay.N + 1, 6)
    assert np.shares_memory(rows, P)
    rows[::7, 3, :, 4] = 0.4
    rows[::7, 3, :, 2] *= 1.3
    return P


def tour_batch(idx, which, S=None):
    """Batch `which` ('a' / 'b') of plan idx."""
    from plan_cases import LAY, plan_batch, plans
    _, dtype, _, _, _ = plans(S)[idx]
    Ba, Bb = tour_sizes(S)[idx]
    if which == "a":
        return plan_batch(Ba, dtype, seed=100 + idx)
    return rotate_every_seventh(plan_batch(Bb, dtype, seed=300 + idx), LAY)


# ---- the tour ----------------------------------------------------------------------------------------------------------------
def tour(n):
    """n * n + 1 visits [(plan, 'a' | 'b')]: a closed walk through every ordered pair (previous plan, current plan) of n plans
    exactly once -- an Euler circuit of the complete directed graph with loops (Hierholzer) -- in which the k-th visit of a plan
    takes batch a or b by the parity of k."""
    nxt, stack, walk = [0] * n, [0], []
    while stack:
        v = stack[-1]
        if nxt[v] < n:
            stack.append(nxt[v])
            nxt[v] += 1
        else:
            walk.append(stack.pop())
    walk.reverse()
    assert len(walk) == n * n + 1 and walk[0] == walk[-1]
    return with_batches(walk)


def with_batches(walk):
    seen, visits = {}, []
    for p in walk:
        visits.append((p, "ab"[seen.get(p, 0) % 2]))
        seen[p] = seen.get(p, 0) + 1
    return visits


def pairs(visits):
    return [(visits[i - 1], visits[i]) for i in range(1, len(visits))]


# ---- the comparison -----------------------------------------------------------------------------------------------------------
def differing(a, b):
    """Number of instances (rows) in which a and b differ, NaNs equal; None if the shapes differ."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return None
    ne = a != b
    if a.dtype.kind == "f":
        ne &= ~(np.isnan(a) & np.isnan(b))
    return int(ne.reshape(ne.shape[0], -1).any(axis=1).sum()) if ne.ndim else int(ne)


def compare(got, want, what):
    """got, want: (result arrays of Handle.solve, nmpc_last_launch_info or None). U, y, cost, status, iters and info[:, :6]
    bit for bit with NaNs equal (info[:, 6], [7] are launch diagnostics), the timing-independent fields of the launch info equal,
    deep_parked <= tail_handed_off. Raises HistoryMismatch naming the array and the number of differing instances."""
    (r, li), (r0, li0) = got, want
    for k in KEYS + ("info",):
        if r0.get(k) is None:
            continue
        a, b = (r[k][:, :6], r0[k][:, :6]) if k == "info" else (r[k], r0[k])
        d = differing(a, b)
        if d is None:
            raise HistoryMismatch(f"{what}: {k} has shape {np.shape(a)} {np.asarray(a).dtype}, fresh handle {np.shape(b)} {np.asarray(b).dtype}")
        if d:
            raise HistoryMismatch(f"{what}: {k} differs from the fresh handle's in {d} of {len(b)} instances")
    if li0 is not None:
        for k in LAUNCH_KEYS:
            if li[k] != li0[k]:
                raise HistoryMismatch(f"{what}: launch info {k} = {li[k]}, fresh handle {li0[k]} ({li} / {li0})")
        if not li["deep_parked"] <= li["tail_handed_off"]:
            raise HistoryMismatch(f"{what}: deep_parked > tail_handed_off: {li}")


def call(handle, P):
    r = handle.solve(P)
    return r, handle.last_launch_info()


def run_tour(handle, visits, refs, batches, want=None, fresh=None, names=None):
    """The visits on one handle. refs[visit] = (result, launch info) of a fresh handle, batches[visit] = P, want[plan] = the
    launch-info fields that show the intended plan (plan_cases.check_plan), fresh() = a new handle for the re-run of a failing
    pair, names[plan] for the report. Raises HistoryMismatch at the first visit that differs."""
    def label(v):
        return "nothing" if v is None else f"{names[v[0]] if names else v[0]}/{v[1]} (B = {len(batches[v])})"
    prev = None
    for pos, v in enumerate(visits):
        got = call(handle, batches[v])
        what = f"visit {pos} of {len(visits)}: {label(v)} after {label(prev)}"
        try:
            if want is not None:
                for k, val in want[v[0]].items():
                    if got[1][k] != val:
                        raise HistoryMismatch(f"{what}: not the intended plan: {k} = {got[1][k]}, expected {val} ({got[1]})")
            compare(got, refs[v], what)
        except HistoryMismatch as e:
            alone = None
            if fresh is not None and prev is not None:
                h2 = fresh()
                try:
                    call(h2, batches[prev])
                    try:
                        compare(call(h2, batches[v]), refs[v], what)
                        alone = False
                    except HistoryMismatch:
                        alone = True
                finally:
                    getattr(h2, "close", lambda: None)()
            verdict = {None: "the pair alone was not re-run", True: "the pair alone on a new handle reproduces it: a one-step leak",
                       False: "the pair alone on a new handle does NOT reproduce it: a longer history is needed"}[alone]
            raise HistoryMismatch(f"{e}; {verdict}", pair=(prev, v), position=pos, pair_alone=alone) from None
        prev = v
