"""``MmpFrontEnd``: what runs on the device in front of the caller's network in the multi-hypothesis predictor (``mmp``) stage,
stated once for ``evaluate.BatchEvaluator``, ``mmp_interface.MmpInterface`` and ``tools/mmp_evaluate_profile.py``: the *fill* --
the input stack ``[7, Hm, Wm]`` per pedestrian and time offset (``nmpc_mmp_input_*``, csrc/nmpc_mmp.h) or, with ``stem``, the
network's first layer fused with it, ``[C, Hp, Wp]`` (``nmpc_mmp_stem_*``, csrc/nmpc_mmp_stem.h) -- then, with ``blocks``, the
residual blocks of ``layer1``, one launch each between two 16-channel buffers (``nmpc_mmp_block_f32``, csrc/nmpc_mmp_block.h),
then, with ``blocks2``, those of ``layer2``, one launch each between two 32-channel buffers on the strided plane
(``nmpc_mmp_block2_f32``, csrc/nmpc_mmp_block2.h), then, with ``blocks3``, those of ``layer3``, one launch each between two
64-channel buffers on the plane strided once more (``nmpc_mmp_block3_f32``, csrc/nmpc_mmp_block3.h), then, with ``blocks4``, those of
``layer4``, one launch each between two 128-channel buffers on the plane strided a third time (``nmpc_mmp_block4_f32``,
csrc/nmpc_mmp_block4.h), then, with ``head``, the pool and both linear layers in one launch (``nmpc_mmp_head_f32``,
csrc/nmpc_mmp_head.h), after which no network is left for the caller to run. The object owns the folded weights on the device, the argument structs and
the buffers they point to; the structs of these kernels are built nowhere else in the package."""
from __future__ import annotations

import numpy as np

from . import _capi
from .mmp_stem import (BLOCK2_CHANNELS, BLOCK3_CHANNELS, BLOCK4_CHANNELS, BLOCK_CHANNELS, block2_plane, check_blocks,
                       check_blocks2, check_blocks3, check_blocks4, check_head, check_spec, head_features)

_BLOCK_ARRAYS = ("w1", "s1", "b1", "w2", "s2", "b2", "wd", "sd", "bd")
_HEAD_ARRAYS = ("w1", "c1", "w2", "c2")
_ABSENT = object()


class MmpFrontEnd:
    def __init__(self, handle: _capi.Handle, dtype, device, Hm: int, Wm: int, n_off: int, transform, rescale: float, sigma: float,
                 ref_image, stem=None, blocks=None, blocks2=None, blocks3=None, blocks4=None, head=None):
        """``dtype``: the element type of ``hist``; ``ref_image``: the float32 label image ``[Hm, Wm]`` on ``device``; ``transform``: the
        :class:`.snap.WorldTransform` between map pixels and the world of ``hist``; ``stem`` / ``blocks``: :class:`.mmp_stem.StemSpec` /
        ``BlockSpec`` s; ``blocks2`` (needs ``blocks``): the ``Block2Spec`` s of layer2; ``blocks3`` (needs ``blocks2``): the ``Block3Spec`` s of layer3. ``fill_row``: a row of what the fill writes;
        ``row``: a row of what the network sees; ``bytes_per_item``: the buffers one pedestrian takes -- with blocks the stem's
        output and the two buffers the blocks alternate between. The two
        32-channel buffers of layer2 lie INSIDE the stem's output, which is idle once layer1's first block has read it, where they fit
        (``2 * 32 * H2 * W2 <= C * Hp * Wp``: the 64-channel stem) and are allocated and counted otherwise. The two 64-channel buffers of
        layer3 lie behind them in the same place where everything fits (``2 * 32 * H2 * W2 + 2 * 64 * H3 * W3 <= C * Hp * Wp``) and are
        allocated and counted otherwise. ``blocks4`` (needs ``blocks3``): the ``Block4Spec`` s of layer4; their two 128-channel buffers lie
        behind layer3's in the same place where everything fits, and are allocated and counted otherwise. ``head`` (needs
        ``blocks4``): the ``HeadSpec`` of the network's end, whose ``F`` must be ``128 * (H4 // 2) * (W4 // 2)`` for the plane that
        arrives; its output ``[rows, O]`` is always allocated and counted, and ``row`` is then ``(O,)``."""
        import torch
        stem, blocks, blocks2, blocks3, blocks4, head = self.check_specs(stem, blocks, blocks2=blocks2, blocks3=blocks3, blocks4=blocks4, head=head)
        self.h, self.dt, self.dev, self.n_off = handle, np.dtype(dtype), device, int(n_off)
        dev = lambda v: None if v is None else torch.as_tensor(v, device=device)
        self.stem = None if stem is None else stem._replace(weight=dev(stem.weight), scale=dev(stem.scale), shift=dev(stem.shift))
        self.blocks = None if blocks is None else tuple(b._replace(**{n: dev(getattr(b, n)) for n in _BLOCK_ARRAYS}) for b in blocks)
        self.blocks2 = None if blocks2 is None else tuple(b._replace(**{n: dev(getattr(b, n)) for n in _BLOCK_ARRAYS}) for b in blocks2)
        self.blocks3 = None if blocks3 is None else tuple(b._replace(**{n: dev(getattr(b, n)) for n in _BLOCK_ARRAYS}) for b in blocks3)
        self.blocks4 = None if blocks4 is None else tuple(b._replace(**{n: dev(getattr(b, n)) for n in _BLOCK_ARRAYS}) for b in blocks4)
        self.head = None if head is None else head._replace(**{n: dev(getattr(head, n)) for n in _HEAD_ARRAYS})
        self.ref = ref_image
        if stem is None:
            self.fill_row = (7, int(Hm), int(Wm))
            a, self._fill = _capi.NmpcMmpArgs(), handle.mmp_input
        else:
            self.fill_row = (int(stem.weight.shape[0]),) + _capi.mmp_stem_shape(Hm, Wm)
            a, self._fill = _capi.NmpcMmpStemArgs(), handle.mmp_stem
            a.C, a.slope = self.fill_row[0], stem.slope
            a.weight, a.bn_scale, a.bn_shift = self.stem.weight.data_ptr(), self.stem.scale.data_ptr(), self.stem.shift.data_ptr()
        a.set_transform(transform, rescale, sigma)
        a.n_off, a.Hm, a.Wm, a.ref_image = self.n_off, int(Hm), int(Wm), ref_image.data_ptr()
        self.row, self.bytes_per_item = self.fill_row, self.n_off * int(np.prod(self.fill_row)) * 4
        if blocks is not None:
            C, Hp, Wp = self.fill_row
            self.row, self.bytes_per_item = (BLOCK_CHANNELS, Hp, Wp), self.n_off * (C + 2 * BLOCK_CHANNELS) * Hp * Wp * 4
        self._pp2_in_fill = False
        if blocks2 is not None:
            plane = self.row[1:]
            self._planes2 = []                                   # the input plane of every layer-2 block, then the last one's output
            for b in blocks2:
                self._planes2.append(plane)
                plane = block2_plane(*plane, b.stride)
            self._planes2.append(plane)
            self._pp2_row = (BLOCK2_CHANNELS,) + self._planes2[1]  # (planes only shrink: the first block's output is the largest)
            self._pp2_in_fill = 2 * int(np.prod(self._pp2_row)) <= int(np.prod(self.fill_row))
            self.row = (BLOCK2_CHANNELS,) + plane
            if not self._pp2_in_fill:
                self.bytes_per_item += self.n_off * 2 * int(np.prod(self._pp2_row)) * 4
        self._pp3_in_fill = False
        if blocks3 is not None:
            self._planes3 = []                                   # the input plane of every layer-3 block, then the last one's output
            for b in blocks3:
                self._planes3.append(plane)
                plane = block2_plane(*plane, b.stride)
            self._planes3.append(plane)
            self._pp3_row = (BLOCK3_CHANNELS,) + self._planes3[1]
            self._pp3_in_fill = self._pp2_in_fill and 2 * int(np.prod(self._pp2_row)) + 2 * int(np.prod(self._pp3_row)) <= int(np.prod(self.fill_row))
            self.row = (BLOCK3_CHANNELS,) + plane
            if not self._pp3_in_fill:
                self.bytes_per_item += self.n_off * 2 * int(np.prod(self._pp3_row)) * 4
        self._pp4_in_fill = False
        if blocks4 is not None:
            self._planes4 = []                                   # the input plane of every layer-4 block, then the last one's output
            for b in blocks4:
                self._planes4.append(plane)
                plane = block2_plane(*plane, b.stride)
            self._planes4.append(plane)
            self._pp4_row = (BLOCK4_CHANNELS,) + self._planes4[1]
            self._pp4_in_fill = self._pp3_in_fill and (2 * int(np.prod(self._pp2_row)) + 2 * int(np.prod(self._pp3_row))
                                                       + 2 * int(np.prod(self._pp4_row)) <= int(np.prod(self.fill_row)))
            self.row = (BLOCK4_CHANNELS,) + plane
            if not self._pp4_in_fill:
                self.bytes_per_item += self.n_off * 2 * int(np.prod(self._pp4_row)) * 4
        if head is not None:
            F, want = int(head.w1.shape[1]), head_features(*self.row)
            if F != want or min(self.row[1:]) < 2:
                raise ValueError(f"HeadSpec: fc1 takes F = {F} values, but the pooled {self.row[0]} x {self.row[1]} x {self.row[2]} plane of layer4 "
                                 f"gives {self.row[0]} x {self.row[1] // 2} x {self.row[2] // 2} = {want}")
            self._head_in = self.row
            self.row = (int(head.w2.shape[0]),)
            self.bytes_per_item += self.n_off * self.row[0] * 4
        self._fill_args, self._block_args, self._block2_args, self._block3_args, self._block4_args, self._head_args, self.chunk = a, (), (), (), (), None, 0

    @staticmethod
    def check_specs(stem, blocks, prefix: str = "", blocks2=_ABSENT, blocks3=_ABSENT, blocks4=_ABSENT, head=_ABSENT):
        """``(stem, blocks)`` checked, either may be ``None``; ``prefix``: what the caller's argument names carry in front. With
        ``blocks2=`` given (``None`` included): ``(stem, blocks, blocks2)``; with ``blocks3=`` given as well: ``(stem, blocks, blocks2,
        blocks3)``; with ``blocks4=``: five values; with ``head=`` as well: six."""
        if blocks4 is not _ABSENT or head is not _ABSENT:
            stem, blocks, blocks2, blocks3 = MmpFrontEnd.check_specs(stem, blocks, prefix, blocks2=None if blocks2 is _ABSENT else blocks2,
                                                                     blocks3=None if blocks3 is _ABSENT else blocks3)
            blocks4 = None if blocks4 is _ABSENT else blocks4
            if blocks4 is not None:
                if blocks3 is None:
                    raise ValueError(f"{prefix}blocks4 needs {prefix}blocks3 (the blocks of layer4 run on the fused layer3's output)")
                blocks4 = check_blocks4(blocks3, blocks4)
            if head is _ABSENT:
                return stem, blocks, blocks2, blocks3, blocks4
            if head is not None:
                if blocks4 is None:
                    raise ValueError(f"{prefix}head needs {prefix}blocks4 (the head runs on the fused layer4's output)")
                head = check_head(head)
            return stem, blocks, blocks2, blocks3, blocks4, head
        if blocks3 is not _ABSENT:
            stem, blocks, blocks2 = MmpFrontEnd.check_specs(stem, blocks, prefix, blocks2=None if blocks2 is _ABSENT else blocks2)
            if blocks3 is not None:
                if blocks2 is None:
                    raise ValueError(f"{prefix}blocks3 needs {prefix}blocks2 (the blocks of layer3 run on the fused layer2's output)")
                blocks3 = check_blocks3(blocks2, blocks3)
            return stem, blocks, blocks2, blocks3
        if blocks2 is not _ABSENT:
            stem, blocks = MmpFrontEnd.check_specs(stem, blocks, prefix)
            if blocks2 is not None:
                if blocks is None:
                    raise ValueError(f"{prefix}blocks2 needs {prefix}blocks (the blocks of layer2 run on the fused layer1's output)")
                blocks2 = check_blocks2(blocks, blocks2)
            return stem, blocks, blocks2
        if stem is not None:
            stem = check_spec(stem)
        if blocks is not None:
            if stem is None:
                raise ValueError(f"{prefix}blocks needs {prefix}stem (the blocks run on the fused first layer's output)")
            blocks = check_blocks(stem, blocks)
        return stem, blocks

    def allocate(self, chunk: int):
        """The buffers for up to ``chunk`` pedestrians per ``run``, and the kernels' structs wired to them (kept while they suffice)."""
        import torch
        if chunk <= self.chunk:
            return
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=self.dev)
        self._fill_buf = self._out = new(chunk, self.n_off, *self.fill_row)
        self._fill_args.out = self._fill_buf.data_ptr()
        args, args2, args3, args4 = [], [], [], []
        if self.blocks is not None:
            self._pp = new(2, chunk, self.n_off, BLOCK_CHANNELS, *self.fill_row[1:])
            for i, b in enumerate(self.blocks):
                a = _capi.NmpcMmpBlockArgs()
                a.Cin, a.H, a.W = int(b.w1.shape[1]), self.fill_row[1], self.fill_row[2]
                for name in _BLOCK_ARRAYS:
                    setattr(a, name, None if getattr(b, name) is None else getattr(b, name).data_ptr())
                a.slope_mid, a.slope_out = b.slope_mid, b.slope_out
                a.x, a.out = self._out.data_ptr(), self._pp[i % 2].data_ptr()
                self._out = self._pp[i % 2]
                args.append(a)
        if self.blocks2 is not None:
            rows, n2 = chunk * self.n_off, int(np.prod(self._pp2_row))
            # (inside the stem's output: layer1's first block has read it before the first block of layer2 writes)
            self._pp2 = self._fill_buf.view(-1)[:2 * rows * n2].view(2, rows * n2) if self._pp2_in_fill else new(2, rows * n2)
            for i, b in enumerate(self.blocks2):
                a = _capi.NmpcMmpBlock2Args()
                a.Cin, (a.H, a.W), a.stride = int(b.w1.shape[1]), self._planes2[i], b.stride
                for name in _BLOCK_ARRAYS:
                    setattr(a, name, None if getattr(b, name) is None else getattr(b, name).data_ptr())
                a.slope_mid, a.slope_out = b.slope_mid, b.slope_out
                a.x, a.out = self._out.data_ptr(), self._pp2[i % 2].data_ptr()
                self._out = self._pp2[i % 2]
                args2.append(a)
        if self.blocks3 is not None:
            rows, n3 = chunk * self.n_off, int(np.prod(self._pp3_row))
            # (inside the stem's output, behind layer2's two buffers)
            behind = 2 * rows * int(np.prod(self._pp2_row))
            self._pp3 = self._fill_buf.view(-1)[behind:behind + 2 * rows * n3].view(2, rows * n3) if self._pp3_in_fill else new(2, rows * n3)
            for i, b in enumerate(self.blocks3):
                a = _capi.NmpcMmpBlock3Args()
                a.Cin, (a.H, a.W), a.stride = int(b.w1.shape[1]), self._planes3[i], b.stride
                for name in _BLOCK_ARRAYS:
                    setattr(a, name, None if getattr(b, name) is None else getattr(b, name).data_ptr())
                a.slope_mid, a.slope_out = b.slope_mid, b.slope_out
                a.x, a.out = self._out.data_ptr(), self._pp3[i % 2].data_ptr()
                self._out = self._pp3[i % 2]
                args3.append(a)
        if self.blocks4 is not None:
            rows, n4 = chunk * self.n_off, int(np.prod(self._pp4_row))
            # (inside the stem's output, behind layer2's and layer3's buffers)
            behind = 2 * rows * (int(np.prod(self._pp2_row)) + int(np.prod(self._pp3_row)))
            self._pp4 = self._fill_buf.view(-1)[behind:behind + 2 * rows * n4].view(2, rows * n4) if self._pp4_in_fill else new(2, rows * n4)
            for i, b in enumerate(self.blocks4):
                a = _capi.NmpcMmpBlock4Args()
                a.Cin, (a.H, a.W), a.stride = int(b.w1.shape[1]), self._planes4[i], b.stride
                for name in _BLOCK_ARRAYS:
                    setattr(a, name, None if getattr(b, name) is None else getattr(b, name).data_ptr())
                a.slope_mid, a.slope_out = b.slope_mid, b.slope_out
                a.x, a.out = self._out.data_ptr(), self._pp4[i % 2].data_ptr()
                self._out = self._pp4[i % 2]
                args4.append(a)
        self._head_args = None
        if self.head is not None:
            a = _capi.NmpcMmpHeadArgs()
            (a.C, a.H, a.W), a.O, a.slope = self._head_in, self.row[0], self.head.slope
            for name in _HEAD_ARRAYS:
                setattr(a, name, getattr(self.head, name).data_ptr())
            self._head_out = new(chunk * self.n_off, self.row[0])
            a.x, a.out = self._out.data_ptr(), self._head_out.data_ptr()
            self._head_args = a
        self._block_args, self._block2_args, self._block3_args, self._block4_args, self.chunk = tuple(args), tuple(args2), tuple(args3), tuple(args4), chunk

    def fill(self, hist: int, hcount: int, B: int, H: int, items, n: int):
        """The fill alone for ``n`` pedestrians: ``hist`` ``[B, H, 5, 2]`` / ``hcount`` ``[B, H]`` device pointers, ``items`` a device
        pointer to their int64 indices or ``None`` = 0 .. n - 1. Returns its output ``[n * n_off, *fill_row]``."""
        if not 0 <= n <= self.chunk:
            raise ValueError(f"{n} items; allocate() was called for {self.chunk}")
        a = self._fill_args
        a.B, a.H, a.n_item, a.hist, a.hcount, a.items = B, H, n, hist, hcount, items
        self._fill(self.dt, a)
        return self._fill_buf.view(-1, *self.fill_row)[:n * self.n_off]

    def run_block(self, i: int, rows: int):
        """Block ``i`` alone on the first ``rows`` rows of its input buffer (what ``fill`` or block ``i - 1`` left there). ONE index
        space covers all stages: ``0 .. len(blocks) - 1`` are the blocks of layer1, ``len(blocks) ..`` those of layer2, then those of
        layer3, then those of layer4."""
        if not 0 <= rows <= self.chunk * self.n_off:
            raise ValueError(f"{rows} rows; allocate() was called for {self.chunk * self.n_off}")
        n1, n2, n3, n4 = len(self._block_args), len(self._block2_args), len(self._block3_args), len(self._block4_args)
        if not 0 <= i < n1 + n2 + n3 + n4:
            raise IndexError(f"block {i} of {n1} + {n2}" + (f" + {n3}" if n3 else "") + (f" + {n4}" if n4 else ""))
        if i < n1:
            self._block_args[i].M = rows
            self.h.mmp_block(self._block_args[i])
        elif i < n1 + n2:
            self._block2_args[i - n1].M = rows
            self.h.mmp_block2(self._block2_args[i - n1])
        elif i < n1 + n2 + n3:
            self._block3_args[i - n1 - n2].M = rows
            self.h.mmp_block3(self._block3_args[i - n1 - n2])
        else:
            self._block4_args[i - n1 - n2 - n3].M = rows
            self.h.mmp_block4(self._block4_args[i - n1 - n2 - n3])

    def run_blocks(self, rows: int):
        """All blocks of layer1, one after the other, on the first ``rows`` rows of the fill's output. Returns the last one's
        ``[rows, 16, Hp, Wp]``."""
        for i in range(len(self._block_args)):
            self.run_block(i, rows)
        return self._pp[(len(self._block_args) - 1) % 2].view(-1, BLOCK_CHANNELS, *self.fill_row[1:])[:rows]

    def run_blocks2(self, rows: int):
        """All blocks of layer2, one after the other, on the first ``rows`` rows of what ``run_blocks`` left. Returns the last one's
        ``[rows, 32, H2, W2]`` (``[rows, *row]`` without blocks3)."""
        n1 = len(self._block_args)
        for i in range(len(self._block2_args)):
            self.run_block(n1 + i, rows)
        row = (BLOCK2_CHANNELS,) + self._planes2[-1]
        return self._pp2[(len(self._block2_args) - 1) % 2][:rows * int(np.prod(row))].view(rows, *row)

    def run_blocks3(self, rows: int):
        """All blocks of layer3, one after the other, on the first ``rows`` rows of what ``run_blocks2`` left. Returns the last one's
        ``[rows, 64, H3, W3]`` (``[rows, *row]`` without blocks4)."""
        n12 = len(self._block_args) + len(self._block2_args)
        for i in range(len(self._block3_args)):
            self.run_block(n12 + i, rows)
        row = (BLOCK3_CHANNELS,) + self._planes3[-1]
        return self._pp3[(len(self._block3_args) - 1) % 2][:rows * int(np.prod(row))].view(rows, *row)

    def run_blocks4(self, rows: int):
        """All blocks of layer4, one after the other, on the first ``rows`` rows of what ``run_blocks3`` left. Returns the last one's
        ``[rows, 128, H4, W4]`` (``[rows, *row]`` without a head)."""
        n123 = len(self._block_args) + len(self._block2_args) + len(self._block3_args)
        for i in range(len(self._block4_args)):
            self.run_block(n123 + i, rows)
        row = (BLOCK4_CHANNELS,) + self._planes4[-1]
        return self._pp4[(len(self._block4_args) - 1) % 2][:rows * int(np.prod(row))].view(rows, *row)

    def run_head(self, rows: int):
        """The head on the first ``rows`` rows of what ``run_blocks4`` left. Returns ``[rows, O]``."""
        if not 0 <= rows <= self.chunk * self.n_off:
            raise ValueError(f"{rows} rows; allocate() was called for {self.chunk * self.n_off}")
        if self._head_args is None:
            raise ValueError("no head was given" if self.head is None else "allocate() has not been called")
        self._head_args.M = rows
        self.h.mmp_head(self._head_args)
        return self._head_out[:rows]

    def run(self, hist: int, hcount: int, B: int, H: int, items, n: int, part=None):
        """One chunk: fill, then the blocks on its ``n * n_off`` rows (arguments as in ``fill``). ``part(name, call)``, if given,
        makes the launches in place of a plain ``call()`` and returns its result: ``"input"``, then with blocks ``"layer1"``, then with
        blocks2 ``"layer2"``, then with blocks3 ``"layer3"``, then with blocks4 ``"layer4"``, then with a head ``"head"``.
        Returns the view ``[n * n_off, *row]`` the network is to be called on -- with a head the network's output ``[n * n_off, O]``
        itself; the next ``run`` overwrites it."""
        part = part or (lambda name, call: call())
        x = part("input", lambda: self.fill(hist, hcount, B, H, items, n))
        if self._block_args:
            x = part("layer1", lambda: self.run_blocks(n * self.n_off))
        if self._block2_args:
            x = part("layer2", lambda: self.run_blocks2(n * self.n_off))
        if self._block3_args:
            x = part("layer3", lambda: self.run_blocks3(n * self.n_off))
        if self._block4_args:
            x = part("layer4", lambda: self.run_blocks4(n * self.n_off))
        if self._head_args is not None:
            x = part("head", lambda: self.run_head(n * self.n_off))
        return x
