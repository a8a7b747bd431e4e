"""Guarded input buffers (test infrastructure): does a result depend on memory outside the arrays it was given?

The suite wraps every OUTPUT in sentinels; this module does the same for the read side. ``guarded`` puts an array into the middle
of one ordinary allocation ``[pad | data | pad]`` whose pads hold a chosen poison, and ``run_guarded`` runs a callable once on
plain exact-size tensors and once per (poison, pad) combination with every input guarded. It asserts

  (a) every output has the same bits (``tobytes()``) in every run, the plain one included, and
  (b) the pads of every input are unchanged after each guarded run: nothing writes through an input pointer.

A read one element past a row, a plane, a weight tensor or a list lands in the pad (or, inside a batch, in the next row) and
changes the bits under at least one poison. The allocation is an ordinary one, so such a read stays inside the test's own
memory: nothing here can fault, and nothing is placed at the end of a mapping.

Poisons for real arrays (``real_poisons``): NaN, 0.0, +big and -big, with big = 3e38 for float32 and 1e300 for float64. NaN alone
is blind wherever the stray value goes through a comparison (``x < best`` is false for NaN, so a NaN never wins a min or a max);
zero and the two large values can win one; and a value multiplied by a zero weight only shows as NaN.

Poisons for integer and byte arrays are DECLARED per array (``IntPoison``): two values that are valid for that array -- the index
of another valid row, a count within the documented range -- but differ from what the array holds, so that a stray read changes
the result and can never become an out-of-range index. Values outside the declared range are refused, and so is an integer array
without a declaration: there are no garbage bit patterns here.

Pads are counted in elements. 64 keeps whatever alignment the data had; 61 breaks everything above element alignment and is used
for the arrays named in ``odd_pad`` (those of which the interface asks no more than element alignment), which drives
pointer-dependent vector paths both ways.

The module works on any torch device, ``"cpu"`` included (tests/test_guarded_buffers_cpu.py)."""
from __future__ import annotations

from typing import Callable, Dict, Iterable, Mapping, NamedTuple, Optional, Sequence

import numpy as np
import torch

PADS = (64, 61)
BIG = {np.dtype(np.float32): 3e38, np.dtype(np.float64): 1e300}


def real_poisons(dtype):
    """The four poisons of a real array: (label, value)."""
    big = BIG[np.dtype(dtype)]
    return (("nan", float("nan")), ("zero", 0.0), ("+big", big), ("-big", -big))


REAL_LABELS = tuple(label for label, _ in real_poisons(np.float32))


class IntPoison(NamedTuple):
    """Two poison values of an integer / byte array and the closed range [lo, hi] of values that are valid in it."""
    values: Sequence[int]
    lo: int
    hi: int


def _check_int_poison(name, array, p):
    if not isinstance(p, IntPoison):
        raise TypeError(f"{name}: integer arrays take an IntPoison(values, lo, hi), got {type(p).__name__}")
    if len(p.values) != 2 or p.values[0] == p.values[1]:
        raise ValueError(f"{name}: an IntPoison has two different values, got {tuple(p.values)}")
    for v in p.values:
        if int(v) != v or not (p.lo <= v <= p.hi):
            raise ValueError(f"{name}: poison {v} is outside the valid range [{p.lo}, {p.hi}] declared for this array")
    a = np.asarray(array)
    if a.size and (a.min() < p.lo or a.max() > p.hi):
        raise ValueError(f"{name}: the array itself holds values outside the declared range [{p.lo}, {p.hi}]")


class Guard:
    """One allocation ``[pad | data | pad]``: ``data`` is the contiguous view in the middle."""

    def __init__(self, name, array, poison, pad, device):
        a = np.ascontiguousarray(array)
        self.name, self.poison, self.pad, self.n = name, poison, int(pad), int(a.size)
        if self.pad < 1:
            raise ValueError(f"{name}: pad must be at least one element, got {pad}")
        src = torch.from_numpy(a.reshape(-1).copy())
        self.base = torch.empty(self.n + 2 * self.pad, dtype=src.dtype, device=device)
        self.base[self.pad:self.pad + self.n] = src.to(device)
        self.data = self.base[self.pad:self.pad + self.n].view(a.shape)
        assert self.data.is_contiguous() and self.data.data_ptr() == self.base.data_ptr() + self.pad * a.itemsize
        self._want = np.full(self.pad, poison, dtype=a.dtype).tobytes()
        self.repoison()

    def repoison(self):
        self.base[:self.pad] = self.poison
        self.base[self.pad + self.n:] = self.poison

    def pads_intact(self):
        front = self.base[:self.pad].cpu().numpy().tobytes()
        back = self.base[self.pad + self.n:].cpu().numpy().tobytes()
        return front == self._want and back == self._want

    def check(self):
        assert self.pads_intact(), f"the pads of input {self.name!r} were written (poison {self.poison}, pad {self.pad})"


def guarded(array, poison, pad=64, device="cpu", name="array"):
    """``array`` (numpy) in the middle of one allocation ``[pad | data | pad]`` on ``device``, both pads filled with ``poison``;
    ``pad`` is counted in elements. Returns ``(data, guard)``: the contiguous tensor view of the data, and the object that
    re-poisons (``guard.repoison()``) and checks (``guard.check()``, ``guard.pads_intact()``) the pads."""
    g = Guard(name, array, poison, pad, device)
    return g.data, g


def _plain(array, device):
    return torch.from_numpy(np.ascontiguousarray(array).copy()).to(device)


def _to_numpy(v):
    if hasattr(v, "detach"):
        v = v.detach().cpu().numpy()
    return np.ascontiguousarray(v)


def _is_real(a):
    return np.asarray(a).dtype.kind == "f"


def _differing_rows(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return f"shape / type {a.shape} {a.dtype} against {b.shape} {b.dtype}"
    if a.ndim == 0:
        return "the value"
    rows = [i for i in range(a.shape[0]) if a[i].tobytes() != b[i].tobytes()]
    return f"rows {rows} of {a.shape[0]}"


def _compare(want, got):
    """Names and rows of the outputs whose bits differ."""
    assert set(want) == set(got), (sorted(want), sorted(got))
    return [f"{k} ({_differing_rows(want[k], got[k])})" for k in sorted(want) if want[k].tobytes() != got[k].tobytes()]


def run_guarded(call: Callable[[Dict[str, Optional[torch.Tensor]]], Mapping[str, object]], inputs: Mapping[str, Optional[np.ndarray]],
                outputs: Optional[Sequence[str]] = None, int_poisons: Optional[Mapping[str, IntPoison]] = None, odd_pad: Iterable[str] = (), device="cpu", pads=PADS,
                poisons=REAL_LABELS):
    """Run ``call`` on plain tensors, then once per (poison, pad) with every input guarded; assert (a) and (b) of the module text.

    ``call(tensors)`` gets one tensor per name of ``inputs`` (``None`` stays ``None``: an optional array that is absent) and
    returns named outputs (tensors or numpy arrays); ``outputs`` names the ones that are compared and returned (default: all of
    them, and the same names must come back from every run). It must build everything else it needs itself, outputs included, and may
    modify the inputs (an in/out array): every run gets fresh copies. An in/out array belongs among the returned outputs.
    ``int_poisons`` declares the two poison values of every integer / byte input; real inputs get the four of ``real_poisons``.
    Run k uses the k-th real poison and the (k % 2)-th integer poison. Inputs named in ``odd_pad`` get the odd pad in the odd-pad
    runs, the others keep 64. When a run differs, the array that matters is named by changing the poison of one input at a time.

    Returns the outputs of the plain run (numpy), for the caller's comparison with its reference."""
    int_poisons = dict(int_poisons or {})
    odd_pad = set(odd_pad)
    unknown = (set(int_poisons) | odd_pad) - set(inputs)
    if unknown:
        raise ValueError(f"no such inputs: {sorted(unknown)}")
    for name, a in inputs.items():
        if a is None:
            continue
        if _is_real(a):
            if name in int_poisons:
                raise ValueError(f"{name}: a real array takes the real poisons, not an IntPoison")
            if np.asarray(a).dtype not in BIG:
                raise ValueError(f"{name}: no poison set for {np.asarray(a).dtype}")
        else:
            if name not in int_poisons:
                raise ValueError(f"{name}: an integer / byte array needs a declared IntPoison (no garbage bit patterns)")
            _check_int_poison(name, a, int_poisons[name])

    def poison_of(name, a, k):
        """Poison number k (an index into REAL_LABELS) of an input."""
        if _is_real(a):
            return real_poisons(np.asarray(a).dtype)[k][1]
        return int(int_poisons[name].values[k % 2])

    def one_run(k, pad, other=None):
        """Outputs with every input guarded by poison k (``other`` = (name, k'): that one by poison k' instead; k = None: plain
        exact-size tensors); also the guards whose pads were written."""
        tensors, guards = {}, []
        for name, a in inputs.items():
            if a is None:
                tensors[name] = None
            elif k is None:
                tensors[name] = _plain(a, device)
            else:
                p = pad if (pad == 64 or name in odd_pad) else 64
                kk = other[1] if other is not None and other[0] == name else k
                tensors[name], g = guarded(a, poison_of(name, a, kk), p, device, name)
                guards.append(g)
        res = call(tensors)
        missing = [key for key in (outputs or ()) if key not in res]
        if missing:
            raise KeyError(f"the call did not return the outputs {missing}")
        out = {key: _to_numpy(v).copy() for key, v in res.items() if outputs is None or key in outputs}
        return out, [g for g in guards if not g.pads_intact()]

    def culprits(k, pad, got):
        """The inputs whose OWN pads decide the outputs: with every input guarded by poison k, changing the poison of that one
        input alone changes a bit. (Guarding one input at a time would not tell: a stray read of an exact-size tensor lands in
        whatever the allocator holds there, so such a run compares with nothing.)"""
        found = []
        for name, a in inputs.items():
            if a is None:
                continue
            others = [j for j in range(len(REAL_LABELS)) if j != k] if _is_real(a) else [k + 1]
            if any(_compare(got, one_run(k, pad, other=(name, j))[0]) for j in others):
                found.append(name)
        return found

    plain, _ = one_run(None, None)
    for pad in pads:
        if pad != 64 and not odd_pad:
            continue
        for label in poisons:
            k = REAL_LABELS.index(label)
            got, written = one_run(k, pad)
            for g in written:
                raise AssertionError(f"the pads of input {g.name!r} were written through the input pointer "
                                     f"(poison {label} = {g.poison}, pad {g.pad})")
            diff = _compare(plain, got)
            if diff:
                found = culprits(k, pad, got)
                what = (" and ".join(repr(c) for c in found) if found else
                        "an input that could not be told (no single pad decides the bits: the plain run itself may have read stray memory)")
                raise AssertionError(f"outputs {', '.join(diff)} depend on memory outside input {what}: "
                                     f"poison {label}, pad {pad} elements")
    return plain


def run_poisoned_regions(call, inputs: Mapping[str, Optional[np.ndarray]], regions: Mapping[str, np.ndarray], device="cpu"):
    """Regions INSIDE an array that the interface says are not read: ``regions[name]`` is a boolean mask of ``inputs[name]`` (a
    real array). ``call`` (as in ``run_guarded``, on plain tensors) runs once on the data as given and once per real poison with
    every masked element replaced; the outputs must have the same bits. Returns the outputs of the first run."""
    def run(arrays):
        return {key: _to_numpy(v).copy() for key, v in call({n: None if a is None else _plain(a, device) for n, a in arrays.items()}).items()}
    want = run(inputs)
    for name, mask in regions.items():
        a = np.asarray(inputs[name])
        if not _is_real(a) or mask.shape != a.shape or mask.dtype != np.bool_ or not mask.any():
            raise ValueError(f"{name}: a region is a non-empty boolean mask of a real array")
        for label, value in real_poisons(a.dtype):
            filled = dict(inputs)
            filled[name] = np.where(mask, np.asarray(value, dtype=a.dtype), a)
            diff = _compare(want, run(filled))
            assert not diff, f"outputs {', '.join(diff)} depend on the region of {name!r} that is documented as not read: poison {label}"
    return want
