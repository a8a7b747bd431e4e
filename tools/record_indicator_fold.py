#!/usr/bin/env python3
"""Record the fixtures of tests/test_gpu_indicator_fold.py: tests/golden/indicator_fold/<shape>.npz.

    NMPC_HIP_LIBRARY=build/libnmpc_parent.so python tools/record_indicator_fold.py [out_dir]

Run it with the library of the commit whose bits are the yardstick (NMPC_HIP_LIBRARY: a build of the same C ABI), on the
MI355X: the fixtures of the indicator fold were recorded with the library of the commit BEFORE the fold. The batches are
the constructed ones of tests/indicator_fold_cases.py; a batch that lacks one of its situations is not recorded.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import indicator_fold_cases as cases  # noqa: E402

FULL = ("rows42", "rows12")   # tables without a dummy row

if __name__ == "__main__":
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "indicator_fold")
    os.makedirs(out_dir, exist_ok=True)
    print("library:", os.environ.get("NMPC_HIP_LIBRARY", "in-tree"))
    for shape in cases.SHAPES:
        sit = cases.situations(shape, cases.make_batch(shape))
        missing = [k for k, v in sit.items() if not v and not (k == "dummies" and shape in FULL)]
        assert not missing, (shape, missing)
        for rotate in ((False, True) if shape == "rows40" else (False,)):
            name = shape + ("_rotated" if rotate else "")
            res = cases.run_all(shape, rotate)
            np.savez_compressed(os.path.join(out_dir, name + ".npz"), **res)
            st = res["solve/throughput/status"]
            print(name, "recorded:", len(res), "arrays; solve statuses", np.unique(st, return_counts=True),
                  "inner iterations", res["solve/throughput/iters"][:, 1].tolist(), flush=True)
