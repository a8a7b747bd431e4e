"""Capacity failures inside scheduled batches. With nmpc_config.max_active_dynobs = K, an instance with K + 1 non-zero
obstacle slots is not solved (status 4, NMPC_CAPACITY_EXCEEDED). Inside the plans of run_solve such an instance goes
through the one-evaluation ranking, the pilot launch and the tail hand-off like any other; it must come out with exactly
the documented failure values and leave every other instance's bits alone. The evaluation entry points report the same
instances as NaN in every output (what the one-evaluation ranking reads), whatever the handle's buffers held before."""
import numpy as np
import pytest

import dyobav_mpcnwta_warehouse_amd as nm
from test_gpu_plan_warmstart import HINT, LAY, PLAIN, PLAN_IDS, check_plan, plan_batch, plan_cfg, plans, same

pytestmark = pytest.mark.gpu


def _rows(P):
    return P[:, LAY.od:LAY.od + LAY.Ndyn * (LAY.N + 1) * 6].reshape(P.shape[0], LAY.Ndyn, LAY.N + 1, 6)


def _offenders(P, frac, seed):
    """About `frac` of the instances get a (HINT + 1)-th non-zero slot: a copy of their live row 0 in padding slot HINT."""
    rows = _rows(P)
    assert not rows[:, HINT:].any() and rows[:, HINT - 1].any()          # (HINT live rows, the rest padding)
    off = np.sort(np.random.default_rng(seed).choice(P.shape[0], max(1, int(frac * P.shape[0])), replace=False))
    rows[off, HINT] = rows[off, 0]
    return off


@pytest.mark.parametrize("member", ["axis-aligned", "general"])
@pytest.mark.parametrize("idx", range(4), ids=PLAN_IDS[:4])
def test_capacity_failures_inside_scheduled_batches(idx, member):
    name, dtype, B, want, _ = plans()[idx]
    assert dtype == np.float32
    P = plan_batch(B, dtype, seed=200 + idx)
    if member == "general":                      # rotated ellipses: the general member of the kernel pair
        rows = _rows(P)
        rows[::7, 3, :, 4] = 0.4
        rows[::7, 3, :, 2] *= 1.3
    off = _offenders(P, 0.03, seed=idx)
    ok = np.ones(B, bool)
    ok[off] = False
    rng = np.random.default_rng(300 + idx)
    y0 = (rng.normal(size=(B, 2 * LAY.N)) * 2).astype(dtype)          # (multipliers passed as input: y_is_input = 1)
    res = {}
    for run, ov, Q in (("automatic", {}, P), ("plain", PLAIN, P), ("plain-zeroed", PLAIN, None)):
        if Q is None:
            Q = P.copy()
            _rows(Q)[off, HINT] = 0
        with nm.Handle(plan_cfg(**ov)) as h:
            res[run] = h.solve(Q, y0=y0)
            li = h.last_launch_info()
        if run == "automatic":
            print("plan:", name, member, B, len(off), li)
            check_plan(li, want)
            if want["tail_handed_off"]:
                assert (res[run]["info"][ok, 7] > 0).any()
    for run in ("automatic", "plain"):
        r = res[run]
        # the offenders: exactly the failure values nmpc_hip.h documents
        assert (r["status"][off] == 4).all() and np.isnan(r["U"][off]).all() and np.isnan(r["cost"][off]).all(), run
        assert (r["iters"][off] == 0).all() and (r["info"][off] == 0).all(), run
        assert np.array_equal(r["y"][off], y0[off]), run                  # (multipliers not written: the input comes back)
        assert (r["status"][ok] != 4).all() and np.isfinite(r["U"][ok]).all(), run
    same(res["automatic"], res["plain"], (name, member), rows=ok)
    same(res["automatic"], res["plain-zeroed"], (name, member, "zeroed"), rows=ok)
    assert (res["plain-zeroed"]["status"] != 4).all()


@pytest.mark.parametrize("mode", ["throughput", "cooperative"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_eval_of_over_capacity_instances_is_nan(dtype, mode):
    """nmpc_eval_batch_* on one handle: a clean batch first (the handle's psi / grad / ||F2||^2 buffers then hold finite
    values), then the same batch with over-capacity instances. Their psi, grad row and f2sq are NaN; the other instances
    keep their values bit for bit."""
    B, n = 96, 2 * LAY.N
    P = nm.scenarios.make_batch(B, LAY, seed=61, n_ped=2, n_hyp=5).astype(dtype)
    rng = np.random.default_rng(62)
    U = np.empty((B, n), dtype)
    U[:, 0::2] = rng.uniform(0, 1.2, (B, LAY.N))
    U[:, 1::2] = rng.uniform(-0.5, 0.5, (B, LAY.N))
    Y = (rng.normal(size=(B, n)) * 3).astype(dtype)
    C = rng.uniform(1, 100, B).astype(dtype)
    ov = dict(coop_waves=4, reg_table=-1, latency_waves=1) if mode == "cooperative" else {}
    with nm.Handle(plan_cfg(**ov)) as h:
        clean = h.eval(P, U, Y, C)
        assert h.last_launch_info()["family"] == mode
        assert np.isfinite(clean["psi"]).all() and np.isfinite(clean["grad"]).all() and np.isfinite(clean["f2sq"]).all()
        Q = P.copy()
        off = _offenders(Q, 0.1, seed=63)
        bad = h.eval(Q, U, Y, C)
    ok = np.ones(B, bool)
    ok[off] = False
    for k in ("psi", "f2sq", "grad"):
        assert np.isnan(bad[k][off]).all(), (k, dtype, mode)
        assert np.array_equal(bad[k][ok], clean[k][ok]), (k, dtype, mode)
