"""``MmpInterface``: the multi-hypothesis motion predictor behind the reference's interface.

Mirror of the reference class ``interfaces/mmp_interface.py:14-70`` (the same ``get_motion_prediction`` signature and return
value), so that ``MainBase.run_wta_prediction`` (main_base.py:175-208) can drive it unchanged. THE DIFFERENCE: the
reference's constructor takes a configuration file name and loads the trained network (``pre_load.load_net``); this one is
constructed from the network itself -- any callable that maps the float32 device tensor ``[M, 7, Hm, Wm]`` to ``[M, K * 2]``
or ``[M, K, 2]`` pixel hypotheses, e.g. a ``ConvMultiHypoNet`` the caller has built and put into ``eval()`` mode. It loads no
weights and holds no configuration.

What the reference does on the host around the network runs on the device: the input stack (``pre_load.traj_to_input`` and
the copy per time offset) through ``nmpc_mmp_input_f64`` with one item (with ``stem=``, a :class:`.mmp_stem.StemSpec`, the
stack and the network's first layer in one kernel, ``nmpc_mmp_stem_f64``, and ``network`` = the trunk; with ``blocks=`` as well, the
first residual stage behind it, one ``nmpc_mmp_block_f32`` per block; with ``blocks2=`` on top, the second, strided one,
one ``nmpc_mmp_block2_f32`` per block; with ``blocks3=`` on top, the third, one ``nmpc_mmp_block3_f32`` per block; with
``blocks4=`` the fourth, one ``nmpc_mmp_block4_f32`` per block; with ``head=`` the pool and the linear layers,
``nmpc_mmp_head_f32``, and ``network=None``),
``get_closest_edge_point(...) / rescale`` through
``nmpc_snap_hypotheses_f64`` with the identity transform. There is no host implementation of either in this package. The kernels
in front of the network are driven through :class:`.mmp_front.MmpFrontEnd`, the same object the evaluator uses, with
``B = H = 1``, one item and float64 positions.

For whole batches of scenarios use ``evaluate.BatchEvaluator(predictor="mmp")``, which keeps the pedestrians' histories on
the device and goes on to the obstacle rows; this class uploads its arguments at every call.
"""
from __future__ import annotations

from typing import Callable, List, Optional

import numpy as np

from . import _capi
from .mmp_front import SPEC_NAMES, MmpFrontEnd
from .snap import WorldTransform

SIGMA = 20.0        # pre_load.py:128
OBSV_LEN = 5        # config.obsv_len of the reference's network configurations


class MmpInterface:
    def __init__(self, network: Optional[Callable] = None, stem=None, blocks=None, blocks2=None, blocks3=None, blocks4=None, head=None, half=(),
                 operands=None, activations=None, precision=None, fill=None):
        """``stem``: a :class:`.mmp_stem.StemSpec` = the network's first layer, computed on the device without the input stack
        (``nmpc_mmp_stem_f64``); ``network`` is then the trunk behind it, a callable on ``[M, C, Hp, Wp]``. ``blocks`` (needs
        ``stem``): the :class:`.mmp_stem.BlockSpec` s of the residual stage behind the stem (``mmp_stem.split_network_layer1``),
        one fused kernel each (``nmpc_mmp_block_f32``); ``network`` is then called on ``[M, 16, Hp, Wp]``. ``blocks2``
        (needs ``blocks``): the :class:`.mmp_stem.Block2Spec` s of the second residual stage (``mmp_stem.split_network_layer2``), one
        fused kernel each (``nmpc_mmp_block2_f32``); ``network`` is then the trunk from ``layer3`` on, called on ``[M, 32, H2, W2]``.
        ``blocks3`` (needs ``blocks2``): the :class:`.mmp_stem.Block3Spec` s of the third residual stage
        (``mmp_stem.split_network_layer3``), one fused kernel each (``nmpc_mmp_block3_f32``); ``network`` is then the trunk from
        ``layer4`` on, called on ``[M, 64, H3, W3]``. ``blocks4`` (needs ``blocks3``): the :class:`.mmp_stem.Block4Spec` s of the fourth
        (``mmp_stem.split_network_layer4``, ``nmpc_mmp_block4_f32``); ``network`` is then the trunk from ``apool`` on, called on
        ``[M, 128, H4, W4]``. ``head`` (needs ``blocks4``): the :class:`.mmp_stem.HeadSpec` of the network's end
        (``mmp_stem.split_network_whole``, ``nmpc_mmp_head_f32``); ``network`` must then be ``None``, and ``batch_size`` no longer
        splits anything. ``half``: ``"layer3"`` (needs ``blocks3``) and ``"layer4"`` (with ``blocks4``), alone or together, run
        that stage's blocks on binary16 MFMA operands with float32 accumulation (``nmpc_mmp_block3_f16``, ``nmpc_mmp_block4_f16``;
        the rounding rule: csrc/nmpc_mmp_block3_f16.h); ``()`` changes nothing; any other stage name is a ``ValueError``: only
        layer3 has an f16 kernel, and layer4 where ``blocks4`` is given. ``operands``: a mapping stage name -> ``"f32"`` or ``"f16"``, the
        general form of ``half``: ``"f16"`` for ``"layer2"`` (needs ``blocks2``; ``nmpc_mmp_block2_f16``, csrc/nmpc_mmp_block2_f16.h,
        the same rule), ``"layer3"`` and ``"layer4"``, ``"f32"`` for any stage; ``None``, ``{}`` or all ``"f32"`` changes no bit
        (``MmpFrontEnd.check_operands``). ``activations``: ``None`` or ``"f32"`` changes no bit; ``"f16"`` (needs a stage on f16
        operands) keeps every tensor between two blocks on f16 operands in memory as binary16 (``MmpFrontEnd``,
        ``MmpFrontEnd.check_activations``). ``precision``: ``None`` or ``"f32"`` changes no bit; ``"f16"`` (needs ``blocks``) runs every
        stage given on f16 operands, layer1 included (``nmpc_mmp_block_f16``), with binary16 activations between all blocks
        (``MmpFrontEnd.check_precision``). ``fill``: ``None`` or ``"f32"`` changes no bit; ``"f16"`` (needs ``stem`` and
        ``precision="f16"``) makes the fused first layer write binary16 too (``nmpc_mmp_stem_io_*``), which layer1's first block then
        reads as such (``MmpFrontEnd.check_fill``)."""
        if head is not None and network is not None:
            raise TypeError("head is the network's end: network must be None with it")
        if head is None and not callable(network):
            raise TypeError(f"network must be a callable, got {type(network)}")
        self._prt_name = "MMPInterface"
        self.network = network
        self._specs = MmpFrontEnd.check_specs(stem, blocks, blocks2=blocks2, blocks3=blocks3, blocks4=blocks4, head=head)
        self._operands = MmpFrontEnd.check_operands(operands, half, self._specs)
        self._half = MmpFrontEnd.check_half(half, self._specs)
        self._operands, self._activations = MmpFrontEnd.check_precision(precision, operands, half, activations, self._specs)
        self._fill = MmpFrontEnd.check_fill(fill, precision, self._specs)
        # (the front ends take the caller's own values: the checked operands name layer1, which ``operands`` refuses)
        self._switches = dict(operands=None if operands is None else dict(operands), activations=activations, precision=precision, fill=fill)
        for name, spec in zip(SPEC_NAMES, self._specs):
            setattr(self, name, spec)
        self._handles = {}        # pred_offset -> device handle (the snap stage takes its N_hor from the handle)
        self._map_of = {}         # pred_offset -> the ref_image its map was set from
        self._fronts = {}         # (pred_offset, Hm, Wm, rescale) -> device front end: the weights are uploaded once, the buffers reused

    def _handle(self, pred_offset: int, ref_image, img: np.ndarray) -> _capi.Handle:
        h = self._handles.get(pred_offset)
        if h is None:
            cfg = _capi.default_config_struct()
            cfg.N_hor = pred_offset
            h = self._handles[pred_offset] = _capi.Handle(cfg)
        if self._map_of.get(pred_offset) is not ref_image:
            h.set_map(255.0 - img.astype(np.float64))          # mmp_interface.py:60: the occupancy is 255 - ref_image
            self._map_of[pred_offset] = ref_image
        return h

    def get_motion_prediction(self, input_traj: List[tuple], ref_image, pred_offset: int, rescale: float = 1.0,
                              batch_size: int = 1) -> Optional[List[np.ndarray]]:
        """``input_traj``: the past positions (x, y) in map pixels before ``rescale``, oldest first; ``ref_image``: a tensor
        [Hm, Wm]; ``pred_offset``: the number of time offsets; ``batch_size``: time offsets per network call. Returns a list
        of ``pred_offset`` float64 arrays [K, 2]: the hypotheses, those inside an obstacle moved to the closest edge pixel
        and put first, ``/ rescale``."""
        if input_traj is None:
            return None
        import torch
        if not isinstance(ref_image, torch.Tensor):
            raise TypeError(f"The reference image should be a tensor, got {type(ref_image)}.")
        if ref_image.dim() != 2:
            raise ValueError(f"ref_image must be [Hm, Wm], got {tuple(ref_image.shape)}")
        traj = np.asarray(input_traj, dtype=np.float64).reshape(-1, 2)
        N, bs = int(pred_offset), int(batch_size)
        if traj.shape[0] < 1 or N < 1 or bs < 1 or not float(rescale) != 0.0:
            raise ValueError(f"{traj.shape[0]} positions, pred_offset = {pred_offset}, batch_size = {batch_size}, rescale = {rescale}")
        img = np.ascontiguousarray(ref_image.detach().cpu().numpy(), dtype=np.float32)
        Hm, Wm = img.shape
        h = self._handle(N, ref_image, img)
        h.set_stream(torch.cuda.current_stream().cuda_stream)
        # hist as the evaluator keeps it: the last <= 5 positions, newest last (the rows in front of them are not read)
        last = traj[-OBSV_LEN:]
        hist = np.repeat(last[:1], OBSV_LEN, axis=0)
        hist[OBSV_LEN - len(last):] = last
        d_hist = torch.from_numpy(hist.reshape(1, 1, OBSV_LEN, 2)).cuda()
        d_count = torch.full((1, 1), traj.shape[0], dtype=torch.long, device="cuda")
        ident = WorldTransform()
        key = (N, Hm, Wm, float(rescale))
        if key not in self._fronts:
            d_ref = torch.empty(Hm, Wm, dtype=torch.float32, device=d_hist.device)
            self._fronts[key] = MmpFrontEnd(h, np.float64, d_hist.device, Hm, Wm, N, ident, rescale, SIGMA, d_ref, *self._specs, half=self._half, **self._switches)
            self._fronts[key].allocate(1)
        fe = self._fronts[key]
        fe.ref.copy_(torch.from_numpy(img))
        stack = fe.run(d_hist.data_ptr(), d_count.data_ptr(), 1, 1, None, 1)
        if self.head is not None:
            outs = [stack]                                      # (the head was the front end's last launch: [N, O])
        else:
            with torch.no_grad():
                outs = [self.network(stack[i:i + bs]) for i in range(0, N, bs)]
        raw = torch.cat([o.reshape(o.shape[0], -1, 2) for o in outs], dim=0).to(torch.float64)
        if raw.shape[0] != N or raw.shape[1] < 1 or raw.shape[1] > 256:
            raise ValueError(f"the network returned {tuple(raw.shape)} for {N} inputs")
        K = int(raw.shape[1])
        raw = raw.reshape(1, N, K, 2).contiguous()
        h.snap_hypotheses(np.float64, raw, raw, 1, K, ident, rescale)
        return list(raw[0].cpu().numpy())

    def close(self):
        for h in self._handles.values():
            h.close()
        self._handles, self._map_of, self._fronts = {}, {}, {}
