"""Handle teardown gives the device memory back. BatchEvaluator, bench.py and the tests create one handle per run; a
buffer that nmpc_destroy forgets stays allocated for the life of the process. The run_solve plan with a dispatch order
from one evaluation keeps its own buffer (nominal controls, zero multipliers, penalties, psi, ||F2||^2:
(2 B 2N + 3 B) elements), so every handle here takes that plan."""
import numpy as np
import pytest
import torch

import dyobav_mpcnwta_warehouse_amd as nm
from test_gpu_plan_warmstart import LAY, n_simd, plan_batch, plan_cfg

pytestmark = pytest.mark.gpu


def test_destroyed_handles_return_their_device_memory():
    B, reps = 12 * n_simd(), 40         # between one and eight device fills of the 4-slot throughput kernels
    P = plan_batch(B, np.float32, seed=71)
    per_handle = (2 * B * 2 * LAY.N + 3 * B) * 4     # the evaluation-order buffer alone
    cfg = plan_cfg(max_inner_iterations=2, max_outer_iterations=1)

    def one():
        with nm.Handle(cfg) as h:
            h.solve(P, want_info=False)
            assert h.last_launch_info()["order_source"] == 2

    one()                                # (runtime and code-object setup before the first reading)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(reps):
        one()
    torch.cuda.synchronize()
    drop = free0 - torch.cuda.mem_get_info(0)[0]
    # a forgotten buffer would cost reps * per_handle (~160 MB at 256 CUs); allow a quarter of it for allocator noise
    print(f"device memory after {reps} handles: {drop / 2**20:.1f} MiB less free (a leak of the buffer: {reps * per_handle / 2**20:.0f} MiB)")
    assert drop < reps * per_handle / 4, (drop, reps * per_handle)
