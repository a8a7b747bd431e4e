"""Reduced runs of the randomised differential checks (tests/fuzz_eval.py, fuzz_solve.py, fuzz_assemble.py, fuzz_hypotheses.py) with fixed
seeds, so that the driver-run GPU suite -- not a text file under profiles/ -- covers every lane-map / table boundary with
obstacles ON the path: random dimensions with the table boundaries over-represented, every evaluation code path
(register / LDS / global table, axis-aligned and general variants, cooperative with 2-4 wavefronts, on-chip cooperative
with and without helper lanes), short solves with every solver kernel, the assembly kernel, the hypothesis-clustering
kernels; all against the oracle."""
import pytest

pytestmark = pytest.mark.gpu


def _collect():
    lines = []
    return lines, lines.append


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_fuzz_eval(seed):
    import fuzz_eval
    lines, out = _collect()
    rc = fuzz_eval.run(cases=500, seed=seed, out=out)
    print("\n".join(lines))
    assert rc == 0, lines[-1]


@pytest.mark.parametrize("seed,outer,inner,cases", [(21, 1, 4, 400), (22, 1, 4, 400), (23, 3, 15, 150)])
def test_fuzz_solve(seed, outer, inner, cases):
    import fuzz_solve
    lines, out = _collect()
    rc = fuzz_solve.run(cases=cases, seed=seed, n_outer=outer, n_inner=inner, out=out)
    print("\n".join(lines))
    assert rc == 0, lines[-1]


@pytest.mark.parametrize("seed", [24, 25])
def test_fuzz_solve_fp32(seed):
    """fp32 short solves, the fp32-only kernels included, against the fp32 oracle at the wide Lipschitz step."""
    import numpy as np
    import fuzz_solve
    lines, out = _collect()
    rc = fuzz_solve.run(cases=200, seed=seed, n_outer=1, n_inner=4, out=out, dtype=np.float32)
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
