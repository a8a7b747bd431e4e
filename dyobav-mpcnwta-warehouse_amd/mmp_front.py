"""``MmpFrontEnd``: what runs on the device in front of the caller's network in the multi-hypothesis predictor (``mmp``) stage,
stated once for ``evaluate.BatchEvaluator``, ``mmp_interface.MmpInterface`` and ``tools/mmp_evaluate_profile.py``: the *fill* --
the input stack ``[7, Hm, Wm]`` per pedestrian and time offset (``nmpc_mmp_input_*``, csrc/nmpc_mmp.h) or, with ``stem``, the
network's first layer fused with it, ``[C, Hp, Wp]`` (``nmpc_mmp_stem_*``, csrc/nmpc_mmp_stem.h) -- then one *stage* per residual
stage whose specs were given (``blocks`` .. ``blocks4``: the rows of ``mmp_stem.STAGES``, ``layer1`` .. ``layer4``), one launch per
block between the stage's two buffers (``nmpc_mmp_block_f32`` .. ``nmpc_mmp_block4_f32``, csrc/nmpc_mmp_block.h ..
nmpc_mmp_block4.h), then, with ``head``, the pool and both linear layers in one launch (``nmpc_mmp_head_f32``,
csrc/nmpc_mmp_head.h), after which no network is left for the caller to run. The object owns the folded weights on the device, the
argument structs and the buffers they point to; the structs of these kernels are built nowhere else in the package."""
from __future__ import annotations

import numpy as np

from . import _capi
from .mmp_stem import STAGES, block2_plane, check_head, check_spec, check_stage, head_features, pack_block1_f16, pack_block2_f16, pack_block3_f16, pack_block4_f16

_BLOCK_ARRAYS = ("w1", "s1", "b1", "w2", "s2", "b2", "wd", "sd", "bd")
_HEAD_ARRAYS = ("w1", "c1", "w2", "c2")
_ABSENT = object()
SPEC_NAMES = ("stem",) + tuple(st.arg for st in STAGES) + ("head",)     # the spec keywords, in the order of ``check_specs``' tuple
# beside each row of STAGES: the struct of its kernel and the Handle method that launches it
_DEVICE = ((_capi.NmpcMmpBlockArgs, "mmp_block"), (_capi.NmpcMmpBlock2Args, "mmp_block2"), (_capi.NmpcMmpBlock3Args, "mmp_block3"),
           (_capi.NmpcMmpBlock4Args, "mmp_block4"))
# ``half=``: the stages that have a kernel with binary16 MFMA operands -- how their checked specs are packed, the struct, the method
_HALF = {"layer3": (pack_block3_f16, _capi.NmpcMmpBlock3F16Args, "mmp_block3_f16"),
         "layer4": (pack_block4_f16, _capi.NmpcMmpBlock4F16Args, "mmp_block4_f16")}
# ``operands=``: every stage that has such a kernel -- ``half``'s, and layer2, which ``half`` refuses
_F16 = {"layer2": (pack_block2_f16, _capi.NmpcMmpBlock2F16Args, "mmp_block2_f16"), **_HALF}
_OPERANDS = ("f32", "f16")
# ``activations="f16"``: the Handle method of such a stage that takes the form of x and of out in memory beside the struct
# ``precision="f16"``: every stage, layer1 included, which ``operands`` and ``half`` keep refusing
_F16_ALL = {"layer1": (pack_block1_f16, _capi.NmpcMmpBlockF16Args, "mmp_block_f16"), **_F16}
_F16_IO = {name: launch + "_io" for name, (_, _, launch) in _F16_ALL.items()}
# what each keyword behind ``stem`` needs in front of it, as ``check_specs`` says it
_NEEDS = (("the blocks run on the fused first layer's output",)
          + tuple(f"the blocks of {st.layer} run on the fused {prev.layer}'s output" for prev, st in zip(STAGES, STAGES[1:]))
          + (f"the head runs on the fused {STAGES[-1].layer}'s output",))


class Stage:
    """One residual stage of a front end (``MmpFrontEnd.stages``)."""

    def __init__(self, name, channels, specs, cins, Args, launch, planes, reads_fill):
        self.name, self.channels = name, channels           # "layer1" ..; the output channels of its blocks
        self.specs, self.cins = specs, cins                 # its specs with their arrays on the device (packed ones on f16 operands); each block's Cin
        self.Args, self.launch = Args, launch               # the struct of its kernel, the Handle method that launches it
        self.planes = planes                                # the input plane of every block, then the last one's output
        self.buf_row = (channels,) + planes[1]              # a row of its two buffers (planes only shrink: the first output is the largest)
        self.reads_fill = reads_fill                        # its first block reads the fill's output, so its buffers cannot lie there
        self.in_fill, self.offset = False, None             # the buffers lie inside the fill's output, that many floats into each row
        self.pp, self.args = None, ()                       # allocate(): the two buffers [2, rows * prod(buf_row)], one struct per block
        self.io = None                                      # with binary16 activations: per block (x_f16, out_f16), which ``launch`` then takes

    @property
    def out_f16(self) -> bool:
        """Whether the last block's output lies in its buffer as binary16 in the octet form."""
        return self.io is not None and bool(self.io[-1][1])

    def run(self, j: int, rows: int):
        """Launches block ``j`` of the stage on ``rows`` rows."""
        a = self.args[j]
        a.M = rows
        return self.launch(a) if self.io is None else self.launch(a, *self.io[j])


class MmpFrontEnd:
    def __init__(self, handle: _capi.Handle, dtype, device, Hm: int, Wm: int, n_off: int, transform, rescale: float, sigma: float,
                 ref_image, stem=None, blocks=None, blocks2=None, blocks3=None, blocks4=None, head=None, half=(),
                 operands=None, activations=None, precision=None, fill=None):
        """``dtype``: the element type of ``hist``; ``ref_image``: the float32 label image ``[Hm, Wm]`` on ``device``; ``transform``: the
        :class:`.snap.WorldTransform` between map pixels and the world of ``hist``; ``stem``: a :class:`.mmp_stem.StemSpec`; ``blocks``
        .. ``blocks4``: the specs of ``layer1`` .. ``layer4`` (``mmp_stem.STAGES``), each needing the one before it; ``head`` (needs
        ``blocks4``): the ``HeadSpec`` of the network's end, whose ``F`` must be ``128 * (H4 // 2) * (W4 // 2)`` for the plane that
        arrives. ``fill_row``: a row of what the fill writes; ``row``: a row of what the network sees (with a head ``(O,)``: its
        output); ``bytes_per_item``: the buffers one pedestrian takes. ``stages``: one :class:`Stage` per stage given.
        ``half``: the names of the stages to run on binary16 MFMA operands with float32 accumulation -- ``"layer3"`` (needs
        ``blocks3``; ``nmpc_mmp_block3_f16``, csrc/nmpc_mmp_block3_f16.h, whose header states the rounding rule), ``"layer4"`` (with
        ``blocks4``; ``nmpc_mmp_block4_f16``, csrc/nmpc_mmp_block4_f16.h, the same rule), both, or ``()``; such a stage's
        record then carries the packed specs, that kernel's struct and its launch method, and nothing else differs: the buffers
        stay float32 where they were.
        ``operands``: a mapping stage name -> ``"f32"`` or ``"f16"``, the general form of ``half`` (``half=("layer3",)`` means
        ``operands={"layer3": "f16"}``; both may be given where they do not contradict each other). ``"f16"`` is accepted for
        ``"layer2"`` (``nmpc_mmp_block2_f16``, csrc/nmpc_mmp_block2_f16.h, the same rule; ``half`` keeps refusing it), ``"layer3"``
        and ``"layer4"``, each needing its blocks; ``"f32"`` for any stage. ``None``, ``{}`` or all ``"f32"`` changes no bit.
        ``self.half`` is what ``check_half`` returned, ``self.operands`` what ``check_operands`` did: the operand type of every
        stage given.
        ``activations``: ``None`` or ``"f32"`` changes no bit and no launch. ``"f16"`` (needs a stage on f16 operands): every tensor
        that a block on f16 operands writes AND a block on f16 operands reads -- across stage borders too -- lies in memory as
        binary16 in the octet form ``[rows, C / 8, H, W, 8]`` (``mmp_stem.pack_activations_f16``, csrc/nmpc_mmp_block_f16.h, whose rule
        then rounds ``out`` once, after the last LeakyReLU), launched through ``nmpc_mmp_block{2,3,4}_f16_io``; with layer2 .. layer4 on
        ``"f16"`` that is 12 of their 13 blocks' inputs. Every other tensor stays float32 NCHW: what layer1 or a float32 stage writes,
        what a float32 stage, the head or the caller's network reads. A binary16 tensor lies in the same two buffers of its stage, in
        the front half of the float slot; the placement rule and ``bytes_per_item`` do not change: the halved footprint is not
        exploited. ``self.activations`` is ``"f32"`` or ``"f16"``; a stage's ``io`` holds the two flags of each of its blocks.
        ``precision``: the switch for the whole network. ``None`` or ``"f32"`` changes no bit and no launch. ``"f16"`` (needs
        ``blocks``): EVERY stage given runs on f16 operands, layer1 included (``nmpc_mmp_block_f16``, csrc/nmpc_mmp_block1_f16.h, the
        same rule) -- which ``operands`` and ``half`` keep refusing in their own words --, together with ``activations="f16"``: every
        tensor between two blocks is binary16 in the octet form, layer1's own and the border to layer2 included; layer1's first block
        still reads the fill's float32 output, the last block still writes float32 NCHW. ``self.operands`` then reports ``"f16"`` for
        every stage given and ``self.activations`` ``"f16"``. Refused beside an ``operands`` entry ``"f32"`` for a stage given or
        ``activations="f32"``; accepted beside ``half`` / ``operands`` / ``activations`` that agree (``check_precision``).
        ``fill``: the form of the fill's output in memory. ``None`` or ``"f32"`` changes no bit, no launch and no buffer. ``"f16"``
        (needs ``stem`` and ``precision="f16"``; ``check_fill``): the fused first layer writes binary16 in the octet form
        (``nmpc_mmp_stem_io_*`` with ``out_f16 = 1``, csrc/nmpc_mmp_stem.h) and layer1's first block reads it as such, its flags
        ``(1, 1)``. That block rounds the float32 values by the same rule when it stages them, and so does its projection, so
        behind a first block WITH a projection (the reference's 64 -> 16) every bit is that of ``precision="f16"`` alone; without one
        the block's identity is the binary16 value, as the rule's last clause says. The fill's buffer is half of what it was, and
        ``bytes_per_item`` says so; ``fill()`` then returns a decoded float32 COPY. ``self.fill_f16`` reports the choice.

        Where a stage's two buffers lie is one rule, evaluated in BYTES (``place_stages``): the fill's output (the stem's,
        ``[C, Hp, Wp]`` per row) is idle once layer1's first block has read it, so the buffers of the stages behind layer1 are laid
        INSIDE it one behind the other, at a running offset, as long as the sum still fits (``4 * (2 * 32 * H2 * W2 + 2 * 64 * H3 *
        W3 + 2 * 128 * H4 * W4) <= e * C * Hp * Wp``, ``e`` = 4 bytes, or 2 with ``fill="f16"``: the 64-channel stem); from the first
        stage that does not fit on they are allocated and counted in ``bytes_per_item``. Layer1 itself reads the fill's output
        (``Stage.reads_fill``), so its buffers are always allocated and counted. The head's output ``[rows, O]`` is always allocated
        and counted."""
        import torch
        specs = self.check_specs(stem, blocks, blocks2=blocks2, blocks3=blocks3, blocks4=blocks4, head=head)
        stem, head = specs[0], specs[-1]
        self.operands = self.check_operands(operands, half, specs)
        self.half = self.check_half(half, specs)
        self.operands, self.activations = self.check_precision(precision, operands, half, activations, specs)
        self.fill_f16 = self.check_fill(fill, precision, specs) == "f16"
        self.h, self.dt, self.dev, self.n_off = handle, np.dtype(dtype), device, int(n_off)
        bits = lambda a: a.view(np.int16) if a.dtype == np.uint16 else a          # (packed binary16 bit patterns travel as int16)
        dev = lambda spec, names: spec._replace(**{n: torch.as_tensor(bits(getattr(spec, n)), device=device) for n in names if getattr(spec, n) is not None})
        self.stem = None if stem is None else dev(stem, ("weight", "scale", "shift"))
        self.ref = ref_image
        if stem is None:
            self.fill_row = (7, int(Hm), int(Wm))
            a, self._fill = _capi.NmpcMmpArgs(), handle.mmp_input
        else:
            self.fill_row = (int(stem.weight.shape[0]),) + _capi.mmp_stem_shape(Hm, Wm)
            a, self._fill = _capi.NmpcMmpStemArgs(), handle.mmp_stem
            if self.fill_f16:
                self._fill = lambda dt, args: handle.mmp_stem_io(dt, args, 1)
            a.C, a.slope = self.fill_row[0], stem.slope
            a.weight, a.bn_scale, a.bn_shift = self.stem.weight.data_ptr(), self.stem.scale.data_ptr(), self.stem.shift.data_ptr()
        a.set_transform(transform, rescale, sigma)
        a.n_off, a.Hm, a.Wm, a.ref_image = self.n_off, int(Hm), int(Wm), ref_image.data_ptr()
        fill_size = int(np.prod(self.fill_row))
        self._fill_bytes = fill_size * (2 if self.fill_f16 else 4)              # of a row of the fill's buffer
        self.row, self.bytes_per_item = self.fill_row, self.n_off * self._fill_bytes
        self.stages = []
        for table, (Args, launch), given in zip(STAGES, _DEVICE, specs[1:-1]):
            if given is not None and self.operands[table.layer] == "f16":
                pack, Args, launch = _F16_ALL[table.layer]
                cins, given = tuple(int(b.w1.shape[1]) for b in given), tuple(pack(b) for b in given)
            elif given is not None:
                cins = tuple(int(b.w1.shape[1]) for b in given)
            setattr(self, table.arg, None if given is None else tuple(dev(b, _BLOCK_ARRAYS) for b in given))
            if given is None:
                continue
            planes = [self.row[1:]]
            for b in given:
                planes.append(block2_plane(*planes[-1], getattr(b, "stride", 1)))       # (layer1's blocks have no stride: 1)
            st = Stage(table.layer, table.channels, getattr(self, table.arg), cins, Args, getattr(handle, launch), planes, reads_fill=not self.stages)
            self.row = (st.channels,) + planes[-1]
            self.stages.append(st)
        slots = [2 * int(np.prod(st.buf_row)) * 4 for st in self.stages]       # bytes of a row of each stage's two float-sized buffers
        for st, slot, at in zip(self.stages, slots, self.place_stages(self._fill_bytes, slots)):
            st.in_fill = at is not None
            if st.in_fill:
                st.offset = at // 4                         # (floats: every slot is a multiple of 4 bytes)
            else:
                self.bytes_per_item += self.n_off * slot
        if self.activations == "f16":
            # a tensor is binary16 where the block that writes it and the block that reads it both run on f16 operands
            f16 = [self.operands[st.name] == "f16" for st in self.stages for _ in st.specs]
            # in front of block k: between[k] (the first tensor is the fill's: binary16 with ``fill="f16"``, which needs layer1 on f16)
            between = [self.fill_f16] + [a and b for a, b in zip(f16, f16[1:])] + [False]
            k = 0
            for st in self.stages:
                if self.operands[st.name] == "f16":
                    st.launch = getattr(handle, _F16_IO[st.name])
                    st.io = tuple((int(between[k + j]), int(between[k + j + 1])) for j in range(len(st.specs)))
                k += len(st.specs)
        self.head =None if head is None else dev(head, _HEAD_ARRAYS)      # (uploaded last: the weights keep the order of the network)
        if head is not None:
            F, want = int(head.w1.shape[1]), head_features(*self.row)
            if F != want or min(self.row[1:]) < 2:
                raise ValueError(f"HeadSpec: fc1 takes F = {F} values, but the pooled {self.row[0]} x {self.row[1]} x {self.row[2]} plane of layer4 "
                                 f"gives {self.row[0]} x {self.row[1] // 2} x {self.row[2] // 2} = {want}")
            self._head_in = self.row
            self.row = (int(head.w2.shape[0]),)
            self.bytes_per_item += self.n_off * self.row[0] * 4
        self._fill_args, self._head_args, self.chunk = a, None, 0

    @staticmethod
    def check_specs(stem, blocks, prefix: str = "", blocks2=_ABSENT, blocks3=_ABSENT, blocks4=_ABSENT, head=_ABSENT):
        """``(stem, blocks)`` checked, either may be ``None``; ``prefix``: what the caller's argument names carry in front. The last
        keyword given (``None`` included) decides the length: with ``blocks2=`` ``(stem, blocks, blocks2)``, with ``blocks3=`` four
        values, with ``blocks4=`` five, with ``head=`` six (``SPEC_NAMES``); a keyword left out in front of it counts as ``None``.
        Every spec needs the one before it."""
        given = [blocks, blocks2, blocks3, blocks4, head]
        given = given[:max(i for i, v in enumerate(given) if i == 0 or v is not _ABSENT) + 1]
        out = [None if stem is None else check_spec(stem)]
        for k, v in enumerate(given):
            v = None if v is _ABSENT else v
            if v is not None:
                if out[-1] is None:
                    raise ValueError(f"{prefix}{SPEC_NAMES[k + 1]} needs {prefix}{SPEC_NAMES[k]} ({_NEEDS[k]})")
                v = check_stage(k, out[-1], v) if k < len(STAGES) else check_head(v)
            out.append(v)
        return tuple(out)

    @staticmethod
    def check_half(half, specs, prefix: str = "") -> tuple:
        """``half`` as a tuple of stage names, checked against the checked ``specs`` of ``check_specs`` (all six)."""
        half = (half,) if isinstance(half, str) else tuple(half)
        for name in half:
            k = next((i for i, st in enumerate(STAGES) if st.layer == name), None)
            if name not in _HALF or (name == "layer4" and specs[1 + k] is None):
                raise ValueError(f"{prefix}half: {name!r}: only layer3 has an f16 kernel, and layer4 where {prefix}blocks4 is given")
            if specs[1 + k] is None:
                raise ValueError(f"{prefix}half: {name!r} needs {prefix}{STAGES[k].arg}")
        return tuple(dict.fromkeys(half))

    @staticmethod
    def check_operands(operands, half, specs, prefix: str = "") -> dict:
        """The operand type, ``"f32"`` or ``"f16"``, of every stage whose specs were given, from ``operands`` (a mapping stage name
        -> type, or ``None``) and ``half``, checked against the checked ``specs`` of ``check_specs`` (all six). ``half`` goes
        through ``check_half`` first, so its refusals speak first and unchanged. ``"f32"`` for a stage whose blocks are not given
        is accepted and names nothing."""
        half = MmpFrontEnd.check_half(half, specs, prefix)
        operands = {} if operands is None else dict(operands)
        for name, value in operands.items():
            k = next((i for i, st in enumerate(STAGES) if st.layer == name), None)
            if value not in _OPERANDS:
                raise ValueError(f"{prefix}operands: {name!r}: {value!r} is neither 'f32' nor 'f16'")
            if k is None or (value == "f16" and name not in _F16):
                raise ValueError(f"{prefix}operands: {name!r}: only layer2, layer3 and layer4 have an f16 kernel")
            if value == "f16" and specs[1 + k] is None:
                raise ValueError(f"{prefix}operands: {name!r} needs {prefix}{STAGES[k].arg}")
            if value == "f32" and name in half:
                raise ValueError(f"{prefix}operands: {name!r} is 'f32', but {prefix}half names it")
        return {st.layer: "f16" if st.layer in half or operands.get(st.layer) == "f16" else "f32"
                for k, st in enumerate(STAGES) if specs[1 + k] is not None}

    @staticmethod
    def check_activations(activations, operands, prefix: str = "") -> str:
        """``activations`` as ``"f32"`` (also for ``None``) or ``"f16"``, checked against what ``check_operands`` returned."""
        if activations is not None and activations not in _OPERANDS:
            raise ValueError(f"{prefix}activations: {activations!r} is none of None, 'f32' and 'f16'")
        if activations == "f16" and "f16" not in operands.values():
            raise ValueError(f"{prefix}activations: 'f16' needs a stage on f16 operands ({prefix}operands)")
        return activations or "f32"

    @staticmethod
    def check_precision(precision, operands, half, activations, specs, prefix: str = "") -> tuple:
        """``(operands, activations)`` as ``check_operands`` and ``check_activations`` return them, under ``precision``: ``None`` or
        ``"f32"`` changes neither; ``"f16"`` makes every stage given ``"f16"``, layer1 included, and the activations ``"f16"``.
        ``operands``, ``half`` and ``activations`` are the caller's own values and go through ``check_operands`` and
        ``check_activations`` first, so their refusals speak first and unchanged (``activations="f16"`` counts ``precision="f16"`` as
        the stage on f16 operands it needs). One sentence per refusal: a value that is none of the three; ``"f16"`` without
        ``blocks``; ``"f16"`` beside an ``operands`` entry ``"f32"`` of a stage given; ``"f16"`` beside ``activations="f32"``."""
        ops = MmpFrontEnd.check_operands(operands, half, specs, prefix)
        whole = isinstance(precision, str) and precision == "f16"
        act = MmpFrontEnd.check_activations(activations, {name: "f16" for name in ops} if whole else ops, prefix)
        if precision is not None and not (isinstance(precision, str) and precision in _OPERANDS):
            raise ValueError(f"{prefix}precision: {precision!r} is none of None, 'f32' and 'f16'")
        if not whole:
            return ops, act
        if specs[1] is None:
            raise ValueError(f"{prefix}precision: 'f16' needs {prefix}blocks (the whole network on f16 operands begins with layer1)")
        for name, value in (operands or {}).items():
            if value == "f32" and name in ops:
                raise ValueError(f"{prefix}precision: 'f16', but {prefix}operands says {name!r} is 'f32'")
        if activations == "f32":
            raise ValueError(f"{prefix}precision: 'f16', but {prefix}activations is 'f32'")
        return {name: "f16" for name in ops}, "f16"

    @staticmethod
    def check_fill(fill, precision, specs, prefix: str = "") -> str:
        """``fill`` as ``"f32"`` (also for ``None``) or ``"f16"``, checked against the caller's ``precision`` and the checked ``specs`` of
        ``check_specs`` (all six). It is called behind ``check_precision``, so earlier refusals speak first and unchanged. One
        sentence per refusal: a value that is none of the three; ``"f16"`` without a stem; ``"f16"`` without ``precision="f16"``."""
        if fill is not None and not (isinstance(fill, str) and fill in _OPERANDS):
            raise ValueError(f"{prefix}fill: {fill!r} is none of None, 'f32' and 'f16'")
        if fill == "f16" and specs[0] is None:
            raise ValueError(f"{prefix}fill: 'f16' needs {prefix}stem (the input stack stays float32: only the fused first layer writes binary16)")
        if fill == "f16" and not (isinstance(precision, str) and precision == "f16"):
            raise ValueError(f"{prefix}fill: 'f16' needs {prefix}precision = 'f16' (layer1's first block reads binary16 only on f16 operands)")
        return fill or "f32"

    @staticmethod
    def place_stages(fill_bytes: int, slots) -> tuple:
        """Where each stage's two buffers lie, in BYTES of a row: ``fill_bytes`` is a row of the fill's output, ``slots`` the bytes of
        a row of each stage's two buffers, first stage first. Per stage the byte offset into the fill's row, or ``None`` = allocated
        on its own. The first stage reads the fill's output and is never inside it; the others are laid inside one behind the
        other while the running sum still fits, and from the first that does not fit on none is."""
        out, offset, inside = [], 0, True
        for k, slot in enumerate(slots):
            inside = inside and (k == 0 or offset + slot <= fill_bytes)
            if k == 0 or not inside:
                out.append(None)
            else:
                out.append(offset)
                offset += slot
        return tuple(out)

    def stage(self, name: str):
        """The :class:`Stage` called ``name`` (``"layer1"`` ..), or ``None`` if its specs were not given."""
        return next((st for st in self.stages if st.name == name), None)

    def allocate(self, chunk: int):
        """The buffers for up to ``chunk`` pedestrians per ``run``, and the kernels' structs wired to them (kept while they suffice)."""
        import torch
        if chunk <= self.chunk:
            return
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=self.dev)
        rows = chunk * self.n_off
        # (binary16 in the octet form: the same rows at half the bytes, kept as floats for the stages' views into it)
        self._fill_buf = x = new(chunk, self.n_off, self._fill_bytes // 4) if self.fill_f16 else new(chunk, self.n_off, *self.fill_row)
        self._fill_args.out = x.data_ptr()
        for st in self.stages:
            n, args = int(np.prod(st.buf_row)), []
            st.pp = self._fill_buf.view(-1)[rows * st.offset:rows * (st.offset + 2 * n)].view(2, rows * n) if st.in_fill else new(2, rows * n)
            for i, b in enumerate(st.specs):
                a = st.Args()
                a.Cin, (a.H, a.W) = st.cins[i], st.planes[i]
                for name, v in zip(b._fields, b):           # the weights' pointers, the slopes and, where the stage has one, the stride
                    setattr(a, name, v.data_ptr() if torch.is_tensor(v) else v)
                a.x, a.out = x.data_ptr(), st.pp[i % 2].data_ptr()
                x = st.pp[i % 2]
                args.append(a)
            st.args = tuple(args)
        self._out = x                                       # what the last block writes
        self._head_args = None
        if self.head is not None:
            a = _capi.NmpcMmpHeadArgs()
            (a.C, a.H, a.W), a.O, a.slope = self._head_in, self.row[0], self.head.slope
            for name in _HEAD_ARRAYS:
                setattr(a, name, getattr(self.head, name).data_ptr())
            self._head_out = new(rows, self.row[0])
            a.x, a.out = x.data_ptr(), self._head_out.data_ptr()
            self._head_args = a
        self.chunk = chunk

    def fill(self, hist: int, hcount: int, B: int, H: int, items, n: int):
        """The fill alone for ``n`` pedestrians: ``hist`` ``[B, H, 5, 2]`` / ``hcount`` ``[B, H]`` device pointers, ``items`` a device
        pointer to their int64 indices or ``None`` = 0 .. n - 1. Returns its output ``[n * n_off, *fill_row]``: a view of its
        buffer, or, with ``fill="f16"``, a decoded float32 COPY of it, made with torch operations on the device -- ``run`` makes
        the same launch and never decodes."""
        self._launch_fill(hist, hcount, B, H, items, n)
        return self._fill_out(n)

    def _launch_fill(self, hist: int, hcount: int, B: int, H: int, items, n: int):
        """The launch of ``fill``, and nothing else."""
        if not 0 <= n <= self.chunk:
            raise ValueError(f"{n} items; allocate() was called for {self.chunk}")
        a = self._fill_args
        a.B, a.H, a.n_item, a.hist, a.hcount, a.items = B, H, n, hist, hcount, items
        self._fill(self.dt, a)

    def _fill_out(self, n: int):
        """What ``fill`` returns, from what the launch left in the fill's buffer."""
        import torch
        rows = n * self.n_off
        if not self.fill_f16:
            return self._fill_buf.view(-1, *self.fill_row)[:rows]
        C, H, W = self.fill_row
        octets = self._fill_buf.view(torch.int16).view(-1)[:rows * C * H * W].view(torch.float16).view(rows, C // 8, H, W, 8)
        return octets.permute(0, 1, 4, 2, 3).reshape(rows, C, H, W).float()

    def _check_rows(self, rows: int):
        if not 0 <= rows <= self.chunk * self.n_off:
            raise ValueError(f"{rows} rows; allocate() was called for {self.chunk * self.n_off}")

    def run_block(self, i: int, rows: int):
        """Block ``i`` alone on the first ``rows`` rows of its input buffer (what ``fill`` or block ``i - 1`` left there). ONE index
        space covers all stages: ``0 .. len(blocks) - 1`` are the blocks of layer1, ``len(blocks) ..`` those of layer2, then those of
        layer3, then those of layer4."""
        self._check_rows(rows)
        j = i
        for st in self.stages:
            if 0 <= j < len(st.args):
                return st.run(j, rows)
            j -= len(st.args)
        counts = [len(st.args) for st in self.stages] + [0, 0]
        raise IndexError(f"block {i} of " + " + ".join(str(c) for c in counts[:2] + [c for c in counts[2:] if c]))

    def run_stage(self, name: str, rows: int):
        """All blocks of stage ``name``, one after the other, on the first ``rows`` rows of what the stage in front (for layer1 the
        fill) left. Returns the last one's float32 ``[rows, channels, H, W]``: a view of the stage's buffer, or, where that tensor
        is binary16 in memory (``activations="f16"``, the next stage on f16 operands too), a decoded COPY of it, made with torch
        operations on the device -- ``run`` launches the same blocks and never decodes."""
        st = self.stage(name)
        self._launch_stage(st, rows)
        return self._stage_out(st, rows)

    def _launch_stage(self, st: Stage, rows: int):
        """The launches of ``run_stage``, and nothing else."""
        self._check_rows(rows)
        for j in range(len(st.args)):
            st.run(j, rows)

    def _stage_out(self, st: Stage, rows: int):
        """What ``run_stage`` returns, from what the last block of ``st`` left in its buffer."""
        import torch
        C, (H, W) = st.channels, st.planes[-1]
        buf = st.pp[(len(st.args) - 1) % 2]
        if not st.out_f16:
            return buf[:rows * C * H * W].view(rows, C, H, W)
        octets = buf.view(torch.int16)[:rows * C * H * W].view(torch.float16).view(rows, C // 8, H, W, 8)
        return octets.permute(0, 1, 4, 2, 3).reshape(rows, C, H, W).float()

    def run_blocks(self, rows: int):
        """``run_stage("layer1", rows)``: ``[rows, 16, Hp, Wp]``."""
        return self.run_stage("layer1", rows)

    def run_blocks2(self, rows: int):
        """``run_stage("layer2", rows)``: ``[rows, 32, H2, W2]``."""
        return self.run_stage("layer2", rows)

    def run_blocks3(self, rows: int):
        """``run_stage("layer3", rows)``: ``[rows, 64, H3, W3]``."""
        return self.run_stage("layer3", rows)

    def run_blocks4(self, rows: int):
        """``run_stage("layer4", rows)``: ``[rows, 128, H4, W4]``."""
        return self.run_stage("layer4", rows)

    def run_head(self, rows: int):
        """The head on the first ``rows`` rows of what ``run_blocks4`` left. Returns ``[rows, O]``."""
        self._check_rows(rows)
        if self._head_args is None:
            raise ValueError("no head was given" if self.head is None else "allocate() has not been called")
        self._head_args.M = rows
        self.h.mmp_head(self._head_args)
        return self._head_out[:rows]

    def run(self, hist: int, hcount: int, B: int, H: int, items, n: int, part=None):
        """One chunk: fill, then the stages on its ``n * n_off`` rows (arguments as in ``fill``). ``part(name, call)``, if given,
        makes the launches in place of a plain ``call()`` and returns its result: ``"input"``, then one per stage under its name,
        ``"layer1"`` .. ``"layer4"``, then with a head ``"head"``.
        Returns the view ``[n * n_off, *row]`` the network is to be called on -- with a head the network's output ``[n * n_off, O]``
        itself; the next ``run`` overwrites it."""
        part = part or (lambda name, call: call())
        part("input", lambda: self._launch_fill(hist, hcount, B, H, items, n))
        for st in self.stages:
            part(st.name, lambda st=st: self._launch_stage(st, n * self.n_off))
        if not self.stages:
            x = self._fill_out(n)                                  # (a view: ``fill="f16"`` needs layer1, so it is never decoded here)
        else:
            x = self._stage_out(self.stages[-1], n * self.n_off)   # (float32 always: its reader is the head or the caller's network)
        if self._head_args is not None:
            x = part("head", lambda: self.run_head(n * self.n_off))
        return x
