"""tests/guarded_buffers.py on the CPU: three functions that misbehave the way a kernel would must be caught, each by the poison
that can show it and under the name of the array it strays from; a well-behaved function passes; undeclared or out-of-range
integer poisons are refused. No device needed.

The misbehaving functions read through the tensor's underlying storage, as a kernel reads through a pointer. On a plain
exact-size tensor there is no storage outside the data, so there they take a finite stand-in -- the other test data that
neighbours an exact-size array in a caching allocator, which is why such reads pass every test on exact-size tensors."""
import numpy as np
import pytest
import torch

from guarded_buffers import PADS, IntPoison, guarded, real_poisons, run_guarded, run_poisoned_regions


def _storage(t):
    """The whole allocation a tensor lives in, flat, and the data's first index in it."""
    flat = torch.empty(0, dtype=t.dtype).set_(t.untyped_storage())
    return flat, t.storage_offset()


def _before(t, stand_in):
    flat, off = _storage(t)
    return flat[off - 1] if off > 0 else torch.tensor(stand_in, dtype=t.dtype)


def _behind(t, stand_in):
    flat, off = _storage(t)
    end = off + t.numel()
    return flat[end] if end < flat.numel() else torch.tensor(stand_in, dtype=t.dtype)


def weighted_sum_ok(t):
    return {"s": (t["x"] * t["w"]).sum(dim=1)}


def zero_weight_on_the_element_in_front(t):
    """Row sums, plus 0 * x[-1]: a halo load that is multiplied by a zero weight."""
    return {"s": (t["x"] * t["w"]).sum(dim=1) + 0.0 * _before(t["x"], 0.5)}


def min_over_one_too_many(t):
    """The smallest element of x by a kernel's `if (v < best) best = v`, in a loop that runs to i <= n."""
    best, v = t["x"].min(), _behind(t["x"], 7.0)
    return {"m": torch.where(v < best, v, best).reshape(1)}


def index_one_past_the_list(t):
    """Gathers rows[run[a]] for a <= n_run: the entry behind the list is used as a row index."""
    run = torch.cat([t["run"], _behind(t["run"], 0).reshape(1)])
    return {"g": t["rows"][run].sum(dim=0)}


X = np.random.default_rng(0).uniform(1.0, 2.0, (3, 5))
W = np.random.default_rng(1).uniform(1.0, 2.0, (3, 5))
ROWS = np.arange(12.0).reshape(4, 3) ** 2
RUN = np.array([0, 2], dtype=np.int64)
RUN_POISON = {"run": IntPoison((1, 3), 0, 3)}


def test_guarded_layout_on_the_cpu():
    for dtype in (np.float32, np.float64):
        for label, value in real_poisons(dtype):
            for pad in PADS:
                a = np.arange(10, dtype=dtype).reshape(2, 5)
                data, g = guarded(a, value, pad, "cpu", "a")
                assert data.shape == (2, 5) and data.is_contiguous() and np.array_equal(data.numpy(), a)
                assert g.base.numel() == 10 + 2 * pad and data.data_ptr() == g.base.data_ptr() + pad * a.itemsize
                assert g.base[:pad].numpy().tobytes() == np.full(pad, value, dtype).tobytes() == g.base[-pad:].numpy().tobytes()
                assert g.pads_intact()
                g.base[pad - 1] = 1.0                      # a write through the pointer, one element in front
                assert not g.pads_intact()
                with pytest.raises(AssertionError, match="'a'"):
                    g.check()
                g.repoison()
                assert g.pads_intact()
                g.base[pad + 10] = 1.0
                assert not g.pads_intact()
    assert real_poisons(np.float32)[2][1] == 3e38 and real_poisons(np.float64)[3][1] == -1e300
    assert np.isfinite(np.float32(3e38)) and PADS == (64, 61)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_well_behaved_function_passes(dtype):
    x, w = X.astype(dtype), W.astype(dtype)
    out = run_guarded(weighted_sum_ok, {"x": x, "w": w}, ["s"], odd_pad=("x", "w"))
    assert np.array_equal(out["s"], (torch.from_numpy(x) * torch.from_numpy(w)).sum(dim=1).numpy())
    out = run_guarded(lambda t: {"g": t["rows"][t["run"]].sum(dim=0)}, {"rows": ROWS, "run": RUN}, int_poisons=RUN_POISON, odd_pad=("run",))
    assert np.array_equal(out["g"], ROWS[0] + ROWS[2])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_zero_times_a_stray_load_is_caught_by_nan_only(dtype):
    inputs = {"x": X.astype(dtype), "w": W.astype(dtype)}
    with pytest.raises(AssertionError, match=r"outside input 'x': poison nan, pad 64") as e:
        run_guarded(zero_weight_on_the_element_in_front, inputs)
    assert "s (rows [0, 1, 2] of 3)" in str(e.value) and "'w'" not in str(e.value)
    run_guarded(zero_weight_on_the_element_in_front, inputs, poisons=("zero", "+big", "-big"))   # 0 * finite = 0: all blind


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_min_over_one_too_many_is_caught_by_a_finite_poison_only(dtype):
    inputs = {"x": X.astype(dtype), "w": W.astype(dtype)}
    run_guarded(min_over_one_too_many, inputs, poisons=("nan",))       # NaN misses it: `NaN < best` is false
    with pytest.raises(AssertionError, match=r"outside input 'x': poison zero, pad 64"):
        run_guarded(min_over_one_too_many, inputs)
    with pytest.raises(AssertionError, match=r"outside input 'x': poison -big, pad 64"):
        run_guarded(min_over_one_too_many, inputs, poisons=("nan", "+big", "-big"))
    run_guarded(min_over_one_too_many, inputs, poisons=("nan", "+big"))    # and a large value never wins a min


def test_an_index_one_past_a_list_is_caught_and_names_the_list():
    with pytest.raises(AssertionError, match=r"outside input 'run': poison nan, pad 64"):
        run_guarded(index_one_past_the_list, {"rows": ROWS, "run": RUN}, int_poisons=RUN_POISON)
    # (run 0 pairs the real poison "nan" with the first integer poison, row 1; the plain run's stand-in was row 0)


def test_a_write_through_an_input_pointer_is_caught():
    def writes_in_front(t):
        flat, off = _storage(t["x"])
        if off > 0:
            flat[off - 1] = 4.0
        return weighted_sum_ok(t)
    with pytest.raises(AssertionError, match=r"pads of input 'x' were written"):
        run_guarded(writes_in_front, {"x": X, "w": W})


def test_the_odd_pad_is_used_only_where_it_is_declared():
    seen = []

    def call(t):
        seen.append({k: v.storage_offset() for k, v in t.items()})
        return weighted_sum_ok(t)
    run_guarded(call, {"x": X, "w": W}, odd_pad=("w",))
    assert seen[0] == {"x": 0, "w": 0} and seen[1:5] == [{"x": 64, "w": 64}] * 4 and seen[5:] == [{"x": 64, "w": 61}] * 4
    del seen[:]
    run_guarded(call, {"x": X, "w": W})
    assert len(seen) == 5                                  # no odd-pad runs without an array that takes one


def test_integer_poisons_must_be_declared_valid_and_different():
    ok = lambda t: {"g": t["rows"][t["run"]].sum(dim=0)}
    inputs = {"rows": ROWS, "run": RUN}
    with pytest.raises(ValueError, match="needs a declared IntPoison"):
        run_guarded(ok, inputs)
    for bad in (IntPoison((1, 4), 0, 3), IntPoison((-1, 1), 0, 3), IntPoison((1, 1), 0, 3), IntPoison((1, 2 ** 40), 0, 3)):
        with pytest.raises(ValueError, match="run"):
            run_guarded(ok, inputs, int_poisons={"run": bad})
    with pytest.raises(ValueError, match="holds values outside"):
        run_guarded(ok, inputs, int_poisons={"run": IntPoison((0, 1), 0, 1)})
    with pytest.raises(ValueError, match="real array"):
        run_guarded(ok, inputs, int_poisons={"run": RUN_POISON["run"], "rows": IntPoison((0, 1), 0, 3)})
    with pytest.raises(ValueError, match="no such inputs"):
        run_guarded(ok, inputs, int_poisons={"run": RUN_POISON["run"], "rnu": RUN_POISON["run"]})
    with pytest.raises(TypeError):
        run_guarded(ok, inputs, int_poisons={"run": (1, 3)})


def test_regions_documented_as_not_read():
    length = 3
    head = lambda t: {"s": t["path"][:length].sum(dim=0)}
    whole = lambda t: {"s": t["path"][:length].sum(dim=0) + 0.0 * t["path"][length]}
    path = np.arange(10.0).reshape(5, 2)
    mask = np.zeros((5, 2), dtype=bool)
    mask[length:] = True
    assert np.array_equal(run_poisoned_regions(head, {"path": path}, {"path": mask})["s"], path[:3].sum(axis=0))
    with pytest.raises(AssertionError, match=r"region of 'path'.*poison nan"):
        run_poisoned_regions(whole, {"path": path}, {"path": mask})
    with pytest.raises(ValueError):
        run_poisoned_regions(head, {"path": path}, {"path": np.zeros((5, 2), dtype=bool)})
