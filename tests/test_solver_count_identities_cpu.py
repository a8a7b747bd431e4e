"""CPU test: how many line-search candidates were rejected and how often the Lipschitz estimate was doubled follows from the
counts a solve returns. tests/test_gpu_solver_boundaries.py uses these identities to assert that a batch took the paths it
is meant to exercise; here they are held against the oracle's iteration trace, which counts both events directly.

Per solve, with ncap = the inner solves that ran into max_inner (such a solve completes one step more than it counts: the
cap is found behind the step that follows the one that reached it):
    gradient evaluations  = 2 outer + inner + ncap + rejected candidates
    cost-only evaluations = outer + inner + ncap + Lipschitz doublings
(two gradients per PANOCEngine::init; one candidate per step, the first step of an inner solve's being u_half; one
Lipschitz test per step; one evaluation with c = 0 per outer iteration.)"""
import numpy as np
import pytest

import dyobav_mpcnwta_warehouse_amd as nm
import oracle


@pytest.mark.parametrize("N,rows,family,dtype", [(20, (4, 10), "toward_robot", np.float32), (20, (3, 5), "passing", np.float32),
                                                  (12, (2, 6), "toward_robot", np.float64)])
def test_counts_give_rejections_and_doublings(N, rows, family, dtype):
    lay = nm.scenarios.ParamLayout(N, 10, 10, 40)
    P = nm.scenarios.make_batch(6, lay, seed=3, n_ped=rows[0], n_hyp=rows[1], ped_mode=family)
    pr = oracle.Problem(N, 10, 10, 40)
    max_inner = 40
    op = oracle.Options(max_outer=3, max_inner=max_inner, lip_eps=1e-2, lip_delta=1e-2)
    rejected_any = doubled_any = capped_any = 0
    for p in P:
        _, _, r, head, _ = oracle.solve_trace(pr, op, p, dtype=dtype)
        outer, inner = int(r["outer_iters"]), int(r["inner_iters"])
        points, grads = int(r["n_points"]), int(r["n_grad_evals"])
        steps = np.bincount(head[:, oracle.TRACE_FIELDS.index("outer")].astype(int), minlength=outer + 1)
        ncap = int((steps == max_inner + 1).sum())
        assert len(head) == inner + ncap
        rejected = int(head[:, oracle.TRACE_FIELDS.index("ls_halvings")].sum())
        doubled = int(head[:, oracle.TRACE_FIELDS.index("lip_doublings")].sum())
        assert grads == 2 * outer + inner + ncap + rejected
        assert points - grads == outer + inner + ncap + doubled
        # the bounds the GPU test uses, which do without ncap
        assert rejected >= grads - inner - 3 * outer and doubled >= points - grads - inner - 2 * outer
        rejected_any += rejected
        doubled_any += doubled
        capped_any += ncap
    assert rejected_any > 0 and doubled_any > 0
    if family == "toward_robot" and N == 20:
        assert capped_any > 0          # (both forms of an inner solve's end are covered)
