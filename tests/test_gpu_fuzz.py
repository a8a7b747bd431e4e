"""Reduced runs of the randomised differential checks (tests/fuzz_eval.py, fuzz_solve.py, fuzz_assemble.py, fuzz_hypotheses.py) with fixed
seeds, so that the driver-run GPU suite -- not a text file under profiles/ -- covers every lane-map / table boundary with
obstacles ON the path: random dimensions with the table boundaries over-represented, every evaluation code path
(register / LDS / global table, axis-aligned and general variants, cooperative with 2-4 wavefronts, on-chip cooperative
with and without helper lanes), short solves with every solver kernel, the assembly kernel, the hypothesis-clustering
kernels; all against the oracle."""
import pytest

pytestmark = pytest.mark.gpu

# seeds and case counts of the runs below (tests/kernel_census.py --fuzz replays them on the CPU: which kernels they reach)
EVAL_SEEDS, EVAL_CASES = (11, 12, 13), 500
SOLVE_RUNS = ((21, 1, 4, 400), (22, 1, 4, 400), (23, 3, 15, 150))     # seed, outer, inner, cases
SOLVE_F32_SEEDS, SOLVE_F32_CASES = (24, 25), 200


def _collect():
    lines = []
    return lines, lines.append


@pytest.mark.parametrize("seed", EVAL_SEEDS)
def test_fuzz_eval(seed):
    import fuzz_eval
    lines, out = _collect()
    rc = fuzz_eval.run(cases=EVAL_CASES, seed=seed, out=out)
    print("\n".join(lines))
    assert rc == 0, lines[-1]


@pytest.mark.parametrize("seed,outer,inner,cases", SOLVE_RUNS)
def test_fuzz_solve(seed, outer, inner, cases):
    import fuzz_solve
    lines, out = _collect()
    rc = fuzz_solve.run(cases=cases, seed=seed, n_outer=outer, n_inner=inner, out=out)
    print("\n".join(lines))
    assert rc == 0, lines[-1]


@pytest.mark.parametrize("seed", SOLVE_F32_SEEDS)
def test_fuzz_solve_fp32(seed):
    """fp32 short solves, the fp32-only kernels included, against the fp32 oracle at the wide Lipschitz step."""
    import numpy as np
    import fuzz_solve
    lines, out = _collect()
    rc = fuzz_solve.run(cases=SOLVE_F32_CASES, seed=seed, n_outer=1, n_inner=4, out=out, dtype=np.float32)
    print("\n".join(lines))
    assert rc == 0, lines[-1]


def test_fuzz_assemble():
    import fuzz_assemble
    lines, out = _collect()
    rc = fuzz_assemble.run(cases=600, seed=31, out=out)
    print("\n".join(lines))
    assert rc == 0, lines[-1]


def test_fuzz_hypotheses():
    import fuzz_hypotheses
    lines, out = _collect()
    rc = fuzz_hypotheses.run(cases=30, seed=41, out=out)
    print("\n".join(lines))
    assert rc == 0, lines[-1]
