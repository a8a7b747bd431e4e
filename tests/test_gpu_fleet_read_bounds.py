"""Do the fleet kernels (csrc/nmpc_fleet.h) read outside the arrays they are given? Both run on guarded and shifted buffers in the
manner of tests/test_gpu_read_bounds.py (tests/guarded_buffers.py: every input in the middle of one allocation whose pads hold
NaN, 0, +big or -big -- declared valid values for the integer and byte arrays -- at pads of 64 and 61 elements): the outputs must
have the bits of the plain run whatever the pads hold, and no pad may be written. The plain run is compared with the numpy
reference by tests/test_gpu_fleet_kernels.py; here only its independence of the surroundings is asked.

Shapes: the last group is full and the run list ends with the last robot (a read past the end of robot / U / alive would land in
the pad), R = 64 fills every lane, R = 11 > capacity leaves lanes that rank but do not roll, R = 1 has no peer at all."""
import numpy as np
import pytest

import fleet_cases as fc
from guarded_buffers import IntPoison, run_guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    fc.close_handles()


def _runs(R):
    B = fc.G * R
    return [None, np.array([b for b in range(B) if b % 2 == 1 or b == B - 1], dtype=np.int64)]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("R,N,Nother", [(1, 5, 3), (3, 5, 2), (11, 20, 10), (64, 20, 10), (4, 5, 1)])
def test_exchange_reads_nothing_outside_its_arrays(dtype, R, N, Nother):
    h = fc.handle(N, Nother)
    case = fc.make_case(20264, R, N, dtype)
    B = case["B"]
    for run in _runs(R):
        for with_U in (True, False):
            inputs = dict(robot=case["robot"].astype(dtype), U=case["U"].astype(dtype) if with_U else None, alive=case["alive"], run=run)

            def call(t):
                out, _ = fc.call_exchange(h, dtype, None, None, None, R, tensors=t)
                return dict(other_c=out)
            poisons = dict(alive=IntPoison((0, 1), 0, 1))
            if run is not None:
                poisons["run"] = IntPoison((0, B - 1), 0, B - 1)
            plain = run_guarded(call, inputs, int_poisons=poisons, odd_pad=("robot", "U"), device="cuda")
            assert np.isfinite(plain["other_c"]).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("R", [1, 3, 11, 64])
def test_post_reads_nothing_outside_its_arrays(dtype, R):
    h = fc.handle(5, 3)
    case = fc.make_case(20265, R, 5, dtype, spread=1.0)
    B = case["B"]
    rng = np.random.default_rng(R)
    flag = lambda p: (rng.random(B) < p).astype(np.uint8)
    for run in _runs(R):
        inputs = dict(robot=case["robot"].astype(dtype), run=run, clr_fleet=rng.uniform(0.2, 5.0, B).astype(dtype), collision=flag(0.2),
                      complete=flag(0.2), alive=flag(0.7), collision_fleet=flag(0.1))

        def call(t):
            out, _ = fc.call_post(h, dtype, None, R, None, tensors=t)
            return out
        poisons = {k: IntPoison((0, 1), 0, 1) for k in fc.POST_KEYS[1:]}
        if run is not None:
            poisons["run"] = IntPoison((0, B - 1), 0, B - 1)
        run_guarded(call, inputs, outputs=fc.POST_KEYS, int_poisons=poisons, odd_pad=("robot", "clr_fleet"), device="cuda")
