"""The folded ellipse indicators of the axis-aligned fp32 register-table kernels, bit for bit against the plain form.

csrc/nmpc_device.h forms max(0, 1 - d^T M d) of an axis-aligned ellipse with the clamp modifier of its second FMA
(unit_clamp_floor: the indicator cannot exceed 1 after rounding) and, in the gated passes without a t = 0 half, selects
the hard gradient's -2 on the penalty factor. Neither may change a bit. The yardstick is the library of the commit before
the fold: tests/golden/indicator_fold/*.npz, recorded with it on an MI355X by tools/record_indicator_fold.py on the
constructed batches of tests/indicator_fold_cases.py (8 instances, N = 20; 19, 40 and 42 rows on the 14-slot kernel, 12 on the
4-slot and 15 on the 6-slot pair; zero, nominal and two random control sets).

A batch that stopped holding a situation it was built for fails test_batches_hold_their_situations; a fixture recorded on
other inputs fails on its input hash.
"""
import os

import numpy as np
import pytest

import dyobav_mpcnwta_warehouse_amd as nm  # noqa: F401  (the package before the cases module, as everywhere in the suite)
import indicator_fold_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "indicator_fold")
FULL = ("rows42", "rows12")   # tables without a dummy row
_RUNS = {}


def _run(name):
    """The loaded library's results on one fixture's batch, computed once."""
    if name not in _RUNS:
        shape, _, rot = name.partition("_")
        _RUNS[name] = cases.run_all(shape, rot == "rotated")
    return _RUNS[name]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _assert_same(name, keys):
    got, want = _run(name), np.load(os.path.join(GOLDEN, name + ".npz"))
    assert np.array_equal(got["inputs_sha256"], want["inputs_sha256"]), (name, "the fixture was recorded on other inputs")
    keys = [k for k in want.files if k.startswith(keys)]
    assert keys, name
    for k in keys:
        g, w = _bits(got[k]), _bits(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (name, k, g.shape, w.shape)
        assert np.array_equal(g, w), (name, k, "differing entries", int((g != w).sum()), "of", g.size)


@pytest.mark.parametrize("shape", list(cases.SHAPES))
def test_batches_hold_their_situations(shape):
    sit = cases.situations(shape, cases.make_batch(shape))
    print(shape, sit)
    assert sit.pop("dummies") == (shape not in FULL), shape
    assert all(sit.values()), (shape, [k for k, v in sit.items() if not v])


def test_some_batch_has_dummy_rows_and_some_has_none():
    d = [cases.SHAPES[s][0] < 3 * cases.SHAPES[s][1] for s in cases.SHAPES]
    assert any(d) and not all(d)


@pytest.mark.parametrize("shape", list(cases.SHAPES))
def test_evaluations_keep_their_bits(shape):
    """psi, gradient and sum F2^2 of eval_kernel, with and without the gradient, for the four control sets."""
    got = _run(shape)
    for c in cases.CONTROLS:   # the evaluations are not trivial: finite, and the obstacle terms are in them
        assert np.isfinite(got[f"eval/{c}/grad/psi"]).all() and np.isfinite(got[f"eval/{c}/grad/grad"]).all(), (shape, c)
    assert (got["eval/nominal/grad/f2sq"] > 0).all(), shape          # (a violated hard ellipse in every instance)
    _assert_same(shape, "eval/")


@pytest.mark.parametrize("shape", list(cases.SHAPES))
def test_solves_keep_their_bits(shape):
    """U, cost, status, iters, info[:, :6]: the throughput kernel, the latency family's tail member and its flat form."""
    got = _run(shape)
    assert (got["solve/throughput/iters"][:, 1] > 0).all(), shape
    _assert_same(shape, "solve/")
    for k in cases.SOLVE_KEYS:   # the tail member returns the throughput kernel's bits (tests/test_gpu_solver_boundaries.py)
        a, b = _bits(got[f"solve/throughput/{k}"]), _bits(got[f"solve/tail/{k}"])
        assert np.array_equal(a, b), (shape, k, int((a != b).sum()))


def test_general_member_is_unchanged():
    """One rotated batch at 40 rows: the general member keeps the plain maximum (its indicators can exceed 1 by an ulp)."""
    _assert_same("rows40_rotated", ("eval/", "solve/"))
