"""Batched closed-loop evaluator ("next" row f3): B independent warehouse scenarios advanced in lock-step on the device.

Trackers: ``"mpc"`` (below) and ``"dwa"``, the reference's dynamic-window baseline (pkg_dwa_tracker/trajectory_tracker.py:304-355
as main_base.py:303-321 drives it): ``nmpc_dwa_step_*`` (csrc/nmpc_dwa.h) takes the place of f1 + solve between the same
``loop_pre`` / ``loop_post`` kernels, with the predictors ``None``, ``cvmp`` and ``kfmp``; with ``mmp`` the per-offset lists variant
``nmpc_dwa_step_lists_*`` on f2's rows and counts (the reference hands the tracker ``mu_list_list`` whatever the predictor,
main_base.py:303-304).

Semantics of the reference's evaluation loop for the MPC tracker with the constant-velocity predictor (``cvmp``) or the
Kalman-filter predictor (``kfmp``), the two predictor configurations of ``main_eva.py`` that need no network weights
(the reference's ``src/``):

* ``MainBase.run_once`` / ``run_one_step``                      main_base.py:267-346, 348-425
* ``MainBase.run_cv_prediction`` + ``CvmpInterface``            main_base.py:238-264, interfaces/cvmp_interface.py:24-57
  (mean step of the last <= 5 positions, extrapolated; std 1.0 for predicted offsets, HUMAN_SIZE at offset 0)
* ``MainBase.run_kf_prediction`` + ``KfmpInterface`` + ``zfilter`` main_base.py:210-236, interfaces/kfmp_interface.py:26-56,
  zfilter.py:45-78 (``predictor="kfmp"``: the filter re-run over every pedestrian's whole past trajectory at every step,
  ONE covariance per run carried through the pedestrians and the steps; rows ``[mu, P00, P11, 0, 1]``)
* obstacle rows ``[mu_x, mu_y, std_x, std_y, 0, 1]``            main_base.py:293-302
* ``MpcInterface.run_step`` -> ``TrajectoryTracker.run_step``   interfaces/mpc_interface.py:52-71, trajectory_tracker.py:273-337
  (reference-state window, speed-reference rule, previous action; multipliers carried between solves)
* no-backward clip, robot / pedestrian motion                  main_base.py:320-324, basic_agent.py:52-82
* metrics                                                       main_pre.py:20-53, main_base.py:326-335, 427-435

One time step = prediction -> obstacle rows -> reference windows -> ``nmpc_assemble_params`` (f1) ->
``nmpc_solve_batch`` -> first action -> agent motion -> metrics, for all scenarios at once; nothing leaves HBM
between steps. ``BatchEvaluator._run_fused`` composes it from stages, each a HIP kernel launch on the compact buffers of the
scenarios still running:

1. ``nmpc_loop_pre_*`` (``csrc/nmpc_step.h``): constant-velocity obstacle rows, reference windows, speed reference;
2. predictor stage, with ``predictor="kfmp"`` only: ``nmpc_kf_predict_*`` (``csrc/nmpc_kf.h``) overwrites the obstacle rows
   (fused path only -- its independent check is tests/kf_reference.py);
   with ``predictor="mmp"``: ``_mmp_predict`` = the device front end (``mmp_front.MmpFrontEnd.run``: ``nmpc_mmp_input_*``,
   ``csrc/nmpc_mmp.h``, or with ``mmp_stem`` the fused first layer ``nmpc_mmp_stem_*``, then with ``mmp_blocks`` the fused blocks
   of layer1, ``nmpc_mmp_block_f32``, then with ``mmp_blocks2`` those of layer2, ``nmpc_mmp_block2_f32``, then with ``mmp_blocks3`` those of layer3, ``nmpc_mmp_block3_f32``, then with ``mmp_blocks4`` those of layer4, ``nmpc_mmp_block4_f32``; its structs, weights and buffers are stated there, once) -> the caller's network
   (or, with ``mmp_head``, ``nmpc_mmp_head_f32`` in the front end and no network at all) ->
   ``nmpc_snap_hypotheses_*`` -> ``nmpc_hypotheses_to_ellipses_*`` (row f2), whose ``Ndynobs`` rows per scenario replace
   ``loop_pre``'s as the input of f1 (``MainBase.run_wta_prediction``, main_base.py:175-208, ``MmpInterface``,
   interfaces/mmp_interface.py:20-70; its independent check is tests/mmp_reference.py);
3. tracker stage: ``_mpc_step`` = f1, the ``on_params`` hook, ``_solve_step`` (warm start, handle by batch size, dispatch
   order, status counts, ``_solve``); or ``_dwa_step`` = ``nmpc_dwa_step_*`` (behind ``_mmp_predict``: ``nmpc_dwa_step_lists_*``);
4. ``nmpc_loop_post_*``: first action, agent motion, metrics, flags.

With ``fleet=R`` the scenarios form groups of R consecutive robots in one world (``csrc/nmpc_fleet.h``): between
stages 2 and 3 ``nmpc_fleet_exchange_*`` writes every running robot's other-robot block from its group's peers (their current
states and their previous solutions rolled out), which f1 copies into the parameter vector, and after stage 4
``nmpc_fleet_post_*`` adds robot-robot clearance and collision on the same run list.

A run starts in ``_start_run`` (flags and metrics, one namespace with the ``_loop_args`` / ``_kf_args`` / ``_mmp_args`` / ``_dwa_args`` buffers)
and ends in ``_finish_run``. ``_run_torch`` (``fused=False``) is stages 1 and 4 written out op by op in torch around the same
``_mpc_step`` -- the implementation of rounds 1-2, kept as the independent check of the kernels. Where the reference runs
``max_num_run`` scenarios one after another (main_base.py:448-464), this runs them side by side. Pedestrian stagger
(``_draw_stagger``) uses a seeded torch generator (the reference's ``random`` is unseeded).
"""
from __future__ import annotations

from dataclasses import dataclass
from types import SimpleNamespace
from typing import List, Optional, Sequence

import numpy as np

from . import _capi
from .mmp_front import SPEC_NAMES, MmpFrontEnd
from .trajectory_tracker import TrajectoryTracker

HUMAN_SIZE = 0.2   # main_base.py:75, main_pre.py:18
HUMAN_VMAX = 1.5   # main_base.py:76
MMP_SIGMA = 20.0   # pre_load.py:128 (sigmas=[20, 20], pixels)
MMP_INPUT_BYTES = 1 << 30   # default bound on the network's input tensor of one chunk


@dataclass
class EvaluationResult:
    collision: np.ndarray        # [B] bool   (main_base.py:366-371; a time-out counts as a collision, :407-410)
    complete: np.ndarray         # [B] bool
    steps: np.ndarray            # [B] int    time steps executed
    smoothness: np.ndarray       # [B, 2]     mean |2nd difference| of (v, w)        (main_pre.calc_action_smoothness)
    clearance: np.ndarray        # [B]        min distance to the static polygons     (calc_minimal_obstacle_distance)
    clearance_dyn: np.ndarray    # [B]        min distance to a pedestrian            (calc_minimal_dynamic_obstacle_distance)
    deviation: np.ndarray        # [B, 2]     mean / max distance to the reference trajectory (calc_deviation_distance)
    trajectory: np.ndarray       # [B, T+1, 3] robot states (rows after the end repeat the last state)
    actions: np.ndarray          # [B, T, 2]  raw solver actions
    solve_ms: List[float]        # kernel time of every batched solve
    n_obs: Optional[np.ndarray] = None       # [T, B] int32, predictor "mmp": clusters found per step (> Ndynobs: the obstacle
    #                                          list was truncated), -1 where the scenario was not running
    n_outside: Optional[np.ndarray] = None   # [T, B] int32, predictor "mmp": hypotheses the network put outside the map
    clearance_fleet: Optional[np.ndarray] = None   # [B], ``fleet=R``: min distance to another member of the robot's group (inf for R = 1)
    collision_fleet: Optional[np.ndarray] = None   # [B] bool, ``fleet=R``: the run ended in a robot-robot collision (``collision`` counts it too)


def action_smoothness(A):
    """``main_pre.calc_action_smoothness`` (main_pre.py:34-37) for a batch: mean |second difference| of (v, w) over the
    actions taken; ``A`` [B, T, 2] torch tensor, NaN rows = steps after the run ended. Returns [B, 2] (NaN for T < 3)."""
    import torch
    B = A.shape[0]
    smooth = torch.full((B, 2), float("nan"), dtype=A.dtype, device=A.device)
    if A.shape[1] >= 3:
        d2 = (A[:, 2:] - 2 * A[:, 1:-1] + A[:, :-2]).abs()
        valid = ~torch.isnan(d2[..., 0])
        smooth = torch.nan_to_num(d2, nan=0.0).sum(dim=1) / valid.sum(dim=1).clamp(min=1)[:, None].to(A.dtype)
    return smooth


def min_dynamic_distance(robot_xy, humans):
    """``main_pre.calc_minimal_dynamic_obstacle_distance`` (main_pre.py:45-47): [B] distance from the robot to its
    closest pedestrian; ``robot_xy`` [B, 2], ``humans`` [B, H, 2]."""
    import torch
    return torch.linalg.norm(robot_xy[:, None, :] - humans, dim=-1).min(dim=1).values


def deviation_to_reference(robot_xy, ref_traj, ref_len):
    """One term of ``main_pre.calc_deviation_distance`` (main_pre.py:49-53): [B] distance from the robot position to
    the closest point of its reference trajectory (``ref_traj`` [B, L, 2+], first ``ref_len[b]`` rows valid)."""
    import torch
    d = torch.cdist(robot_xy[:, None, :], ref_traj[:, :, :2])[:, 0]
    inf = torch.full_like(d, float("inf"))
    return torch.where(torch.arange(d.shape[1], device=d.device)[None] < ref_len[:, None], d, inf).min(dim=1).values


def unicycle_rk4_step(robot, act, ts):
    """``basic_agent.Robot.one_step`` = ``UnicycleModel(ts, rk4=True)`` (basic_motion_model/motion_model.py:141-163) in
    closed form for a batch: ``robot`` [B, 3], ``act`` [B, 2] -> [B, 3]."""
    import torch
    th, v, w = robot[:, 2], act[:, 0], act[:, 1]
    hh = 0.5 * ts * w
    cc = (torch.cos(th) + 4 * torch.cos(th + hh) + torch.cos(th + 2 * hh)) / 6
    ss = (torch.sin(th) + 4 * torch.sin(th + hh) + torch.sin(th + 2 * hh)) / 6
    return torch.stack([robot[:, 0] + ts * v * cc, robot[:, 1] + ts * v * ss, th + ts * w], dim=1)


class BatchEvaluator:
    def __init__(self, config: _capi.NmpcConfigStruct, robot_starts: np.ndarray, robot_paths: Sequence[Sequence[tuple]],
                 human_starts: np.ndarray, human_paths: np.ndarray, map_polygons: np.ndarray, dtype=np.float64,
                 human_stagger: float = 0.0, seed: int = 0, mode: str = "work",
                 tuning: Optional[Sequence[float]] = None, lin_vel_max: float = 1.5, warm_start: bool = False,
                 compact: Optional[bool] = None, fused: bool = True, n_hyp: int = 1, hyp_fan: float = 0.15,
                 hyp_radius_growth: float = 0.05, predictor: Optional[str] = "cvmp", kf_Q=None, kf_R=None, kf_P0=None,
                 tracker: str = "mpc", dwa_config=None, network=None, mmp_hyp: int = 20, mmp_chunk: Optional[int] = None,
                 ref_image=None, transform=None, rescale: float = 1.0, mmp_stem=None, mmp_blocks=None, mmp_blocks2=None, mmp_blocks3=None,
                 mmp_blocks4=None, mmp_head=None, mmp_half=(), mmp_operands=None, mmp_activations=None, mmp_precision=None,
                 mmp_fill=None, fleet: Optional[int] = None, fleet_coupling: bool = True):
        """``fleet``: ``None`` (default) launches nothing new and changes no bit. ``R`` (1 .. 64, ``B % R == 0``): scenarios
        ``g R .. g R + R - 1`` are the robots of one group, which share the static map and the pedestrians -- every member gets the
        pedestrian starts and paths of the group's member 0 and the same stagger draw per step ([G, H] drawn, expanded to [B, H]).
        Per time step ``nmpc_fleet_exchange_*`` (csrc/nmpc_fleet.h) fills the other-robot blocks ``[c_0 | c]`` of the running robots
        from their peers -- current state in ``c_0``, the previous solution's N controls rolled out from the current state in ``c``
        (at rest on the first step and for robots that have stopped), the nearest ``Nother - 1`` peers nearest first from slot 1, slot 0
        and unused slots zero -- into ``other_c`` (allocated once), which ``assemble_params(..., other_robots=)`` copies into ``P``; after
        ``loop_step(post=True)`` ``nmpc_fleet_post_*`` keeps ``clearance_fleet`` and turns a centre distance ``<= vehicle_width`` into a
        collision (``collision_fleet``; it beats a completion of the same step; a parked robot's outcome is never changed).
        ``fleet_coupling=False`` runs that epilogue only, the blocks stay zeros: the uncoupled arm of a comparison. ``fleet=1`` computes
        the same ``P``, bit for bit, as ``fleet=None``. Needs ``tracker="mpc"`` and ``fused=True`` (the torch path does not have it); works
        with every predictor. Not modelled: priorities, deadlock resolution, any negotiation between robots.

        ``tracker``: ``"mpc"`` = the NMPC solver (f1 + solve), ``"dwa"`` = the reference's dynamic-window baseline
        (``pkg_dwa_tracker``; one kernel, ``nmpc_dwa_step_*``, csrc/nmpc_dwa.h, in place of f1 + solve; ``dwa_config``: a
        :class:`.configs.DwaConfiguration`, default = the reference's ``dwa_test.yaml`` values; its ``ts`` / ``N_hor`` must be the
        configuration's). It runs with ``predictor`` ``None`` (the pedestrians' current positions, as the reference without a
        predictor), ``"cvmp"`` or ``"kfmp"`` (their mean positions per offset) or ``"mmp"`` (the cluster means of f2, whose number
        differs from offset to offset: ``nmpc_dwa_step_lists_*`` with ``R = Ndynobs`` rows and f2's per-offset counts; every ``mmp_*``
        option below applies; ``record=`` entries carry ``dyn``, ``dyn_count``, ``n_obs``, ``n_outside`` and the tracker's outputs), on
        the fused path with ``n_hyp == 1``, and
        creates no parameter vectors, multipliers or solver handles. Metrics, goal and collision rules are the shared ones.

        ``predictor``: ``"cvmp"`` = the constant-velocity predictor; ``"kfmp"`` = the Kalman-filter predictor
        (constant-velocity model at the configuration's ``ts``; ``kf_Q`` [4,4], ``kf_R`` [2,2], ``kf_P0`` [4,4] default to
        the identities main_base.py:165 and ``KfmpInterface`` use). It needs ``n_hyp == 1`` and ``fused=True``. The filter
        runs over the whole past trajectory of every pedestrian at every step, so ``run(max_steps)`` keeps all of them on the
        device: ``B * H * (max_steps + 1) * 2`` reals -- 254 MB in fp32 at B = 65 536, H = 4, 120 steps.

        ``predictor="mmp"``: the reference's multi-hypothesis predictor (``main('mpc', 'mmp')``). ``network``: any callable that
        takes the float32 device tensor ``[M, 7, Hm, Wm]`` (five Gaussian maps of the past positions, the label image, the
        time offset) and returns ``mmp_hyp`` hypotheses per row in network pixels, ``[M, mmp_hyp * 2]`` or ``[M, mmp_hyp, 2]``,
        as the reference's ``ConvMultiHypoNet`` does; it is called under ``torch.no_grad()`` in whatever mode the caller left
        it (no weights are loaded here). ``ref_image`` [Hm, Wm]: the grey label image (255 = free), also the map the
        hypotheses are snapped on (``255 - ref_image`` is the occupancy, ``Handle.set_map`` once, here). ``transform``: the
        :class:`.snap.WorldTransform` between map pixels and the world, ``rescale``: ``scale2nn``. ``mmp_chunk``: pedestrians
        per network call (default: as many as keep the input tensor at or below 1 GiB -- 19 for the warehouse map at
        N_hor = 20). It needs ``fused=True``, ``n_hyp == 1`` and ``H * mmp_hyp <= 256``. ``mmp_stem``: a
        :class:`.mmp_stem.StemSpec` (``mmp_stem.split_network`` / ``fold_stem``) = the network's first layer, computed by the
        device stage itself (``nmpc_mmp_stem_*``, csrc/nmpc_mmp_stem.h) without the input stack ever being written; ``network``
        is then the trunk behind it, called on ``[M, C, Hp, Wp]``, and the chunk is sized from that tensor (34 pedestrians for
        the warehouse map at N_hor = 20 and C = 64). ``None`` (default): the stage as described above. ``mmp_blocks`` (needs
        ``mmp_stem``): the :class:`.mmp_stem.BlockSpec` s of the network's first residual stage (``mmp_stem.split_network_layer1``:
        three for the reference's ``resnet34.layer1``; the first takes the stem's C channels, each later one 16), run by the device
        stage as one fused kernel per block (``nmpc_mmp_block_f32``, csrc/nmpc_mmp_block.h) between two 16-channel buffers;
        ``network`` is then the trunk from ``layer2`` on, called on ``[M, 16, Hp, Wp]``, and the chunk keeps the stem's output plus
        both buffers at or below 1 GiB (22 pedestrians for the warehouse map at N_hor = 20 and C = 64). Measured on an MI355X at
        B = 256, 4 pedestrians, K = 20 (``profiles/mmp_layer1_evaluate.json``): the stage takes 524 ms per
        lock-step against 685 ms with ``mmp_stem`` alone; the three block launches 88 ms where torch's own layer1 took 232.
        ``mmp_blocks2`` (needs ``mmp_blocks``): the :class:`.mmp_stem.Block2Spec` s of the second residual stage
        (``mmp_stem.split_network_layer2``: four for the reference's ``resnet34.layer2``, the first 16 -> 32 at stride 2), one fused
        kernel per block (``nmpc_mmp_block2_f32``, csrc/nmpc_mmp_block2.h) between two 32-channel buffers that lie inside the stem's
        output where they fit (the chunk stays at 22 pedestrians); ``network`` is then the trunk from ``layer3`` on, called on
        ``[M, 32, H2, W2]`` (37 x 42 for the warehouse map). Measured in the same setting (``profiles/mmp_layer2_evaluate.json``,
        DESIGN.md section 7): the stage takes 467 ms per lock-step against 521 ms without; the four launches 72 ms where torch's own
        layer2 took 129.
        ``mmp_blocks3`` (needs ``mmp_blocks2``): the :class:`.mmp_stem.Block3Spec` s of the third residual stage
        (``mmp_stem.split_network_layer3``: six for the reference's ``resnet34.layer3``, the first 32 -> 64 at stride 2), one fused
        kernel per block (``nmpc_mmp_block3_f32``, csrc/nmpc_mmp_block3.h) between two 64-channel buffers that lie inside the stem's
        output behind layer2's where everything fits (the chunk stays at 22 pedestrians); ``network`` is then the trunk from
        ``layer4`` on, called on ``[M, 64, H3, W3]`` (19 x 21 for the warehouse map). Measured in the same setting
        (``profiles/mmp_layer3_evaluate.json``): the stage takes 420 ms per lock-step against 467 ms without;
        the six launches 122 ms where torch's own layer3 took 170.
        ``mmp_blocks4`` (needs ``mmp_blocks3``): the :class:`.mmp_stem.Block4Spec` s of the fourth residual stage
        (``mmp_stem.split_network_layer4``: three for the reference's ``resnet34.layer4``, the first 64 -> 128 at stride 2), one fused
        kernel per block (``nmpc_mmp_block4_f32``, csrc/nmpc_mmp_block4.h) between two 128-channel buffers that lie inside the stem's
        output behind layer3's where everything fits (the chunk stays at 22 pedestrians); ``network`` is then the trunk from
        ``apool`` on, called on ``[M, 128, H4, W4]`` (10 x 11 for the warehouse map). ``mmp_head`` (needs ``mmp_blocks4``): the
        :class:`.mmp_stem.HeadSpec` of the network's end (``mmp_stem.split_network_whole``), one launch (``nmpc_mmp_head_f32``,
        csrc/nmpc_mmp_head.h); ``network`` must then be ``None`` -- nothing of the stage is a torch module any more -- and
        ``mmp_hyp`` must be half the head's outputs. Measured in the same setting (``profiles/mmp_layer4_evaluate.json``, DESIGN.md
        section 7): the stage takes 389 ms per lock-step against 420 ms without; the three launches 58 ms where torch's own layer4
        took 95, the head 4.4 ms where torch's pool and linear layers took 3.0.
        ``mmp_half``: the stages to run on binary16 MFMA operands with float32 accumulation: ``"layer3"`` (needs ``mmp_blocks3``;
        ``nmpc_mmp_block3_f16``, csrc/nmpc_mmp_block3_f16.h), ``"layer4"`` (with ``mmp_blocks4``; ``nmpc_mmp_block4_f16``,
        csrc/nmpc_mmp_block4_f16.h), both, or ``()``, the default, which changes nothing. The rule: whatever an
        MFMA reads -- the weights, rounded once on the host; ``x`` as it is staged; the first convolution's activated output as it
        goes to LDS -- is binary16, rounded to nearest even and saturated at +-65504; nothing else is: the activations in memory, the
        accumulation, the affines, the LeakyReLUs and the identity stay float32. What that costs and gains, measured: DESIGN.md
        section 7, ``profiles/mmp_layer3_f16_evaluate.json`` and ``profiles/mmp_layer4_f16_evaluate.json``. Any other stage name is a
        ``ValueError``: only layer3 has an f16 kernel, and layer4 where ``mmp_blocks4`` is given.
        ``mmp_operands``: a mapping stage name -> ``"f32"`` or ``"f16"``, the general form of ``mmp_half``
        (``mmp_half=("layer3",)`` means ``mmp_operands={"layer3": "f16"}``): ``"f16"`` for ``"layer2"`` (needs ``mmp_blocks2``;
        ``nmpc_mmp_block2_f16``, csrc/nmpc_mmp_block2_f16.h, the same rule; ``mmp_half`` keeps refusing it), ``"layer3"`` and
        ``"layer4"``; ``"f32"`` for any stage. ``None``, the default, ``{}`` or all ``"f32"`` changes no bit. Checked by
        ``MmpFrontEnd.check_operands``, one ``ValueError`` sentence per refusal. Measured (DESIGN.md section 7,
        ``profiles/mmp_layer2_f16_evaluate.json``): the four launches of layer2 take 0.33 x the float32 ones, the stage 198 ms per
        lock-step against 246 with layer3 and layer4 on binary16 in both.
        ``mmp_activations``: ``None``, the default, or ``"f32"`` changes no bit and no launch; ``"f16"`` (needs a stage on f16 operands)
        keeps every tensor that a block on f16 operands writes and a block on f16 operands reads in memory as binary16
        (``MmpFrontEnd``; checked by ``MmpFrontEnd.check_activations``). Measured: DESIGN.md section 7,
        ``profiles/mmp_f16_activations_evaluate.json``.
        ``mmp_precision``: the switch for the whole network. ``None``, the default, or ``"f32"`` changes no bit and no launch; ``"f16"``
        (needs ``mmp_blocks``) runs EVERY stage given on f16 operands, layer1 included (``nmpc_mmp_block_f16``,
        csrc/nmpc_mmp_block1_f16.h, the same rule; ``mmp_operands`` and ``mmp_half`` keep refusing layer1), with binary16 activations
        between all blocks. Refused beside an ``mmp_operands`` entry ``"f32"`` of a stage given or ``mmp_activations="f32"``; checked
        by ``MmpFrontEnd.check_precision``.
        ``mmp_fill``: the form of the fused first layer's output in memory. ``None``, the default, or ``"f32"`` changes no bit, no
        launch and no buffer; ``"f16"`` (needs ``mmp_stem`` and ``mmp_precision="f16"``) makes that layer write binary16 in the octet
        form (``nmpc_mmp_stem_io_*``, csrc/nmpc_mmp_stem.h), which layer1's first block reads as such: the same bits behind a first
        block with a projection, half the fill's bytes per pedestrian, which the chunking sees. Checked by
        ``MmpFrontEnd.check_fill``. Measured: DESIGN.md section 7, ``profiles/mmp_fill_f16_evaluate.json``.

        ``n_hyp`` > 1: every pedestrian enters the solver as ``n_hyp`` obstacle rows fanned around its constant-velocity
        prediction by ``(j - (n_hyp - 1) / 2) * hyp_fan`` rad, radii ``HUMAN_SIZE + hyp_radius_growth * t`` -- the
        multi-hypothesis obstacle tensor SURVEY.md 8(d) prescribes for BASELINE configs[2] (4 pedestrians x 10
        hypotheses), here produced closed-loop from the scenarios' own pedestrian motion instead of one-shot. ``n_hyp``
        = 1 is the reference's constant-velocity predictor (one row per pedestrian, std 1.0)."""
        import torch
        self.torch = torch
        self.fused = fused
        self.n_hyp, self.hyp_fan, self.hyp_grow = max(1, int(n_hyp)), float(hyp_fan), float(hyp_radius_growth)
        if tracker not in ("mpc", "dwa"):
            raise ValueError(f"tracker = {tracker!r} (mpc or dwa)")
        if tracker == "mpc" and predictor is None:
            raise ValueError("tracker = 'mpc' needs a predictor (cvmp, kfmp or mmp)")
        if predictor not in ("cvmp", "kfmp", "mmp") and not (tracker == "dwa" and predictor is None):
            raise ValueError(f"predictor = {predictor!r} (cvmp, kfmp or mmp; None with tracker = 'dwa')")
        if mmp_stem is not None and predictor != "mmp":
            raise ValueError("mmp_stem needs predictor = 'mmp'")
        mmp_specs = MmpFrontEnd.check_specs(mmp_stem, mmp_blocks, prefix="mmp_", blocks2=mmp_blocks2, blocks3=mmp_blocks3, blocks4=mmp_blocks4,
                                            head=mmp_head)
        mmp_head = mmp_specs[-1]
        if mmp_half and predictor != "mmp":
            raise ValueError("mmp_half needs predictor = 'mmp'")
        if mmp_operands and predictor != "mmp":
            raise ValueError("mmp_operands needs predictor = 'mmp'")
        mmp_switches = dict(operands=None if mmp_operands is None else dict(mmp_operands), activations=mmp_activations, precision=mmp_precision,
                            fill=mmp_fill)
        mmp_operands = MmpFrontEnd.check_operands(mmp_operands, mmp_half, mmp_specs, prefix="mmp_")
        mmp_half = MmpFrontEnd.check_half(mmp_half, mmp_specs, prefix="mmp_")
        if mmp_activations and predictor != "mmp":
            raise ValueError("mmp_activations needs predictor = 'mmp'")
        if mmp_precision and predictor != "mmp":
            raise ValueError("mmp_precision needs predictor = 'mmp'")
        # (checks the activations too, in front of its own refusals; the front end takes the caller's own values: the checked
        # operands name layer1, which ``mmp_operands`` refuses)
        MmpFrontEnd.check_precision(mmp_precision, mmp_switches["operands"], mmp_half, mmp_activations, mmp_specs, prefix="mmp_")
        if mmp_fill and predictor != "mmp":
            raise ValueError("mmp_fill needs predictor = 'mmp'")
        MmpFrontEnd.check_fill(mmp_fill, mmp_precision, mmp_specs, prefix="mmp_")
        if predictor == "mmp":
            if self.n_hyp != 1 or not fused:
                raise ValueError("predictor = 'mmp' needs n_hyp = 1 and fused = True")
            if mmp_head is not None:
                if network is not None:
                    raise ValueError("mmp_head is the network's end: network must be None with it")
                if ref_image is None or transform is None:
                    raise ValueError("predictor = 'mmp' needs ref_image and transform")
                if 2 * int(mmp_hyp) != mmp_head.w2.shape[0]:
                    raise ValueError(f"mmp_hyp = {mmp_hyp}, but mmp_head gives {mmp_head.w2.shape[0]} outputs = {mmp_head.w2.shape[0] // 2} hypotheses (x, y)")
            elif not callable(network) or ref_image is None or transform is None:
                raise ValueError("predictor = 'mmp' needs network (a callable), ref_image and transform")
            if int(mmp_hyp) < 1 or (mmp_chunk is not None and int(mmp_chunk) < 1) or not float(rescale) != 0.0:
                raise ValueError(f"mmp_hyp = {mmp_hyp}, mmp_chunk = {mmp_chunk}, rescale = {rescale}")
        if tracker == "dwa" and (self.n_hyp != 1 or not fused):
            raise ValueError("tracker = 'dwa' needs n_hyp = 1 and fused = True")
        if config is None:
            raise ValueError("config is None: an NmpcConfigStruct is needed (default_config_struct())")
        self.fleet, self.fleet_coupling = None, bool(fleet_coupling)
        if fleet is not None:
            if not fused:
                raise ValueError("fleet needs fused = True: the torch path does not have the fleet kernels")
            if tracker != "mpc":
                raise ValueError("fleet needs tracker = 'mpc': the dynamic-window tracker has no other-robot terms")
            if int(fleet) != fleet or not 1 <= int(fleet) <= 64:
                raise ValueError(f"fleet = {fleet!r}: a group has 1 .. 64 robots")
            if robot_starts.shape[0] % int(fleet) != 0:
                raise ValueError(f"fleet = {fleet}: B = {robot_starts.shape[0]} scenarios are not a whole number of groups")
            self.fleet = int(fleet)
            if self.fleet > 1:      # one pedestrian set per group: member 0's
                R, G = self.fleet, robot_starts.shape[0] // self.fleet
                human_starts = np.repeat(np.asarray(human_starts).reshape((G, R) + np.shape(human_starts)[1:])[:, 0], R, axis=0)
                human_paths = np.repeat(np.asarray(human_paths).reshape((G, R) + np.shape(human_paths)[1:])[:, 0], R, axis=0)
        self.tracker, self.predictor = tracker, predictor
        self.dwa_config = None
        if tracker == "dwa":
            from .configs import DwaConfiguration
            self.dwa_config = dwa_config if dwa_config is not None else DwaConfiguration()
            if int(self.dwa_config.N_hor) != int(config.N_hor) or float(self.dwa_config.ts) != float(config.ts):
                raise ValueError(f"dwa_config has N_hor = {self.dwa_config.N_hor}, ts = {self.dwa_config.ts}; the configuration "
                                 f"{config.N_hor}, {config.ts}")
            lin_vel_max = float(self.dwa_config.lin_vel_max)
        if predictor == "kfmp" and (self.n_hyp != 1 or not fused):
            raise ValueError("predictor = 'kfmp' needs n_hyp = 1 and fused = True")
        eye = lambda m, n: np.eye(n) if m is None else np.asarray(m, dtype=np.float64).reshape(n, n)
        self.kf_Q, self.kf_R, self.kf_P0 = eye(kf_Q, 4), eye(kf_R, 2), eye(kf_P0, 4)
        # time_predictor / time_tracker: HIP events around every nmpc_kf_predict / nmpc_dwa_step call; run() leaves the
        # times (ms) in predictor_ms / tracker_ms
        # (predictor "mmp": time_predictor_parts adds events around its four parts -- five with mmp_blocks: "layer1", six with mmp_blocks2: "layer2", seven with mmp_blocks3: "layer3", eight with mmp_blocks4: "layer4"; with mmp_head "head" in place of "network" --;
        # predictor_part_ms: name -> ms per step)
        self.time_predictor, self.time_tracker, self.time_predictor_parts = False, False, False
        self.predictor_ms, self.tracker_ms, self.predictor_part_ms = [], [], {}
        # time_fleet: HIP events around every nmpc_fleet_exchange / nmpc_fleet_post call; run() leaves fleet_ms: name -> ms per step
        self.time_fleet, self.fleet_ms = False, {}
        self.time_solves = True     # record the HIP-event time of every batched solve (one event wait per time step)
        self.dt = np.dtype(dtype)
        self.tdt = torch.float32 if self.dt == np.float32 else torch.float64
        self.dev = torch.device("cuda", config.device_id)
        B = self.B = robot_starts.shape[0]
        self.compact = (B > 1024) if compact is None else bool(compact)
        self.cfg = config = self._mpc_config(config) if tracker == "mpc" else config
        self.h = _capi.Handle(config)
        self.h.set_stream(torch.cuda.current_stream(self.dev).cuda_stream)
        self._h_by_waves = {}
        # ---- the scenarios' state, common to both trackers
        self.N, self.ts = config.N_hor, config.ts
        T = self._tensor
        self.robot = T(robot_starts)                               # [B,3]
        self.goal = T(np.array([p[-1] for p in robot_paths], dtype=float))   # [B,2]
        self.humans = T(human_starts)                              # [B,H,2]
        self.H = self.humans.shape[1]
        if self.H * self.n_hyp > config.Ndynobs:
            raise ValueError(f"{self.H} pedestrians x {self.n_hyp} hypotheses exceed Ndynobs = {config.Ndynobs}")
        self.hpath = T(human_paths)                                # [B,H,W,2]
        self.hidx = torch.zeros(B, self.H, dtype=torch.long, device=self.dev)
        self.hist = self.humans[:, :, None, :].repeat(1, 1, 5, 1)  # last <= 5 positions, newest last
        self.hcount = torch.ones(B, self.H, dtype=torch.long, device=self.dev)
        self.polys = T(map_polygons)                               # [M,4,2]
        self.stagger = float(human_stagger)
        self.warm_start = warm_start       # row f4 (extension): shifted previous solution as the initial guess
        self.gen = torch.Generator(device=self.dev).manual_seed(seed)
        # replay hook for tests: a list of [B, H] tensors, one per pedestrian step, used instead of the generator
        # (the reference draws the stagger with python's `random`, basic_agent.py:64; a recording can be replayed)
        self.stagger_replay: Optional[list] = None
        scale = {"safe": 0.2, "work": 0.8, "super": 1.0}[mode]
        self.base_speed = lin_vel_max * scale
        self.speed_scale = scale
        self.lin_vel_max = lin_vel_max
        # global reference trajectories: TrajectoryTracker.get_ref_traj per scenario (host, once), padded
        # (the Monte-Carlo runs of one scenario share start and path: make_reference_scenarios has three distinct pairs
        #  for any B -- one host call per distinct pair)
        cache = {}

        def ref_traj(p, s):
            key = (tuple(map(tuple, p)), tuple(float(v) for v in s))
            if key not in cache:
                cache[key] = np.array(TrajectoryTracker.get_ref_traj(self.ts, list(p), tuple(s), self.base_speed))
            return cache[key]
        trajs = [ref_traj(p, s) for p, s in zip(robot_paths, robot_starts)]
        self.ref_len = torch.as_tensor([len(t) for t in trajs], device=self.dev)
        Lmax = max(len(t) for t in trajs)
        pad = np.stack([np.concatenate([t, np.repeat(t[-1:], Lmax - len(t), axis=0)]) for t in trajs])
        self.ref_traj = T(pad)                                     # [B,Lmax,3]
        self.idx_ref = torch.zeros(B, dtype=torch.long, device=self.dev)
        # the controls and multipliers of all scenarios and of the compacted batch of the running ones (the loop kernels
        # want the arrays; the dynamic-window tracker never reads y)
        self.U = torch.empty(B, 2 * self.N, dtype=self.tdt, device=self.dev)
        self._Ua = torch.empty(B, 2 * self.N, dtype=self.tdt, device=self.dev)
        self.y = torch.zeros(B, 2 * self.N, dtype=self.tdt, device=self.dev)
        # hook for harvesting (scenarios.harvest_closed_loop), MPC only: called as on_params(kt, idx, Pa) after the parameter
        # vectors of time step kt have been assembled (idx = running scenarios of the compact batch, None = all)
        self.on_params = None
        # dispatch order of a time step's solves from the evaluation counts of the previous one (nmpc_set_dispatch_order)
        self.dispatch_by_history, self.dispatch_min_batch = tracker == "mpc", 32768   # (measured: -4 % at 16 384 scenarios, +10 % at 65 536)
        # count_status: the exit statuses of every time step's solves are counted on the device (status_counts: one [4]
        # tensor per step -- Converged / NotConvergedIterations / NotConvergedOutOfTime / anything else) -- how often the
        # evaluation budget (nmpc_config.max_evaluations) cuts a solve off, and how often the loop runs on a converged answer
        self.count_status = False
        self.status_counts: list = []
        if tracker == "mpc":
            self._init_mpc(tuning)
        else:
            self._init_dwa(robot_paths)
        if predictor == "mmp":
            self._init_mmp(network, mmp_hyp, mmp_chunk, ref_image, transform, rescale, mmp_specs, mmp_half, **mmp_switches)
        if self.fleet is not None and self.fleet_coupling:
            self.other_c = torch.empty(B, 3 * (self.N + 1) * int(config.Nother), dtype=self.tdt, device=self.dev)

    def _tensor(self, x):
        return self.torch.as_tensor(np.ascontiguousarray(x), dtype=self.tdt, device=self.dev)

    def _full(self, *shape, dtype=None, fill=0.0):
        return self.torch.full(shape, fill, dtype=dtype or self.tdt, device=self.dev)

    def _mpc_config(self, config):
        """The configuration the MPC handles are made from: the caller's, with the choices fixed that must not follow the batch."""
        import copy
        if config.axis_aligned == 0:
            # the pedestrians' obstacle rows are written here with angle = 0 (main_base.py:302), so the promise can be
            # made once instead of leaving the code path to the per-call scan of the batch (nmpc_hip.h, axis_aligned:
            # with 0 the path -- and with it the last bits of every result -- depends on the batch composition)
            config = copy.copy(config)
            config.axis_aligned = 1
        li = _capi.layout_info(config)
        streamed = bool(li.global_table_f32 if self.dt == np.float32 else li.global_table_f64)
        # (obstacle table streamed from global memory -- e.g. N = 40, 160 rows: the library's automatic choice there is
        #  the cooperative kernel, whatever the batch size; pinning latency_waves would switch it off)
        if config.latency_waves == 0 and not streamed and self.compact:
            # The batch shrinks as scenarios finish (compaction) and the library's automatic choice between its kernel
            # families follows the batch size. A scenario's closed-loop trajectory must not depend on who else is still
            # running, so either every plan computes the same bits -- fp32 with the obstacle table in registers:
            # nmpc_config.batch_invariant, and the library goes on choosing the fastest plan for what is left (latency
            # kernels for the last few hundred scenarios) -- or, where the families agree to rounding only (fp64, LDS
            # table), the family is fixed here from the initial batch.
            config = copy.copy(config)
            if self.dt == np.float32 and li.reg_slots_f32 > 0:
                config.batch_invariant = 1
            else:
                n_simd = 4 * self.torch.cuda.get_device_properties(self.dev).multi_processor_count
                config.latency_waves = 1 if self.B > 4 * n_simd else 2
        return config

    def _init_mpc(self, tuning):
        """Solver state: parameter vectors, weights, evaluation counts, statuses, one handle per latency-kernel width."""
        import copy
        torch, B, config = self.torch, self.B, self.cfg
        # Within the latency-kernel family the number of wavefronts per instance does not change the result (the W
        # candidates of a round are evaluated with the same arithmetic as one after the other; bit-identical for W = 2,
        # 3, 4 -- tests/test_gpu_options.py), so W follows the number of scenarios still running: as many wavefronts per
        # instance as stay resident together. One handle per W.
        if config.latency_waves >= 2:
            self._n_simd = 4 * torch.cuda.get_device_properties(self.dev).multi_processor_count
            for w in (2, 3, 4):
                if w == config.latency_waves:
                    self._h_by_waves[w] = self.h
                else:
                    c = copy.copy(config)
                    c.latency_waves = w
                    self._h_by_waves[w] = _capi.Handle(c)
                    self._h_by_waves[w].set_stream(torch.cuda.current_stream(self.dev).cuda_stream)
        self.tuning = self._tensor(np.asarray(tuning if tuning is not None else
                                              (0.0, 10.0, 0.0, 0.0, 0.0, 0.0, 0.0, 100.0, 10.0, 20.0), dtype=float))
        self.stcw, self.dynw = self._full(self.N, fill=10.0), self._full(self.N, fill=10.0)   # set_obstacle_weights(10, 10)
        self.P = torch.empty(B, self.h.np_, dtype=self.tdt, device=self.dev)
        self._info, self._evals = self._full(B, 8), self._full(B)
        self.status = torch.empty(B, dtype=torch.int32, device=self.dev)

    def _init_mmp(self, network, mmp_hyp, mmp_chunk, ref_image, transform, rescale, specs, half=(), operands=None, activations=None, precision=None,
                  fill=None):
        """The multi-hypothesis predictor's constants: the label image on the device, the map of the snap stage, the device front
        end (``mmp_front``: its kernels, weights and buffers) and from it the shape of one row of the network's input -- the stack's
        [7, Hm, Wm] or, with a fused first layer, its output [C, Hp, Wp], or behind the last fused stage its [channels, H, W], or with a
        head the network's output [O] -- and the chunk. ``specs``: the six checked specs (``mmp_front.SPEC_NAMES``); they are kept as
        ``mmp_stem``, ``mmp_blocks`` .. ``mmp_head`` with their arrays on the device."""
        img = np.ascontiguousarray(ref_image, dtype=np.float32)
        if img.ndim != 2:
            raise ValueError(f"ref_image must be [Hm, Wm], got {img.shape}")
        self.network, self.mmp_hyp, self.mmp_tf, self.mmp_rescale = network, int(mmp_hyp), transform, float(rescale)
        if self.H * self.mmp_hyp > 256:
            raise ValueError(f"{self.H} pedestrians x {self.mmp_hyp} hypotheses exceed the 256 points per time offset of the snap and f2 kernels")
        self.mmp_Hm, self.mmp_Wm = int(img.shape[0]), int(img.shape[1])
        self.mmp_ref = self.torch.as_tensor(img, device=self.dev)
        # mmp_interface.py:60 snaps on 255 - ref_image; its grey levels decide the edges (Handle.set_map)
        self.h.set_map(255.0 - img.astype(np.float64))
        fe = self.mmp_front = MmpFrontEnd(self.h, self.dt, self.dev, self.mmp_Hm, self.mmp_Wm, self.N, transform, self.mmp_rescale, MMP_SIGMA,
                                          self.mmp_ref, *specs, half=half, operands=operands, activations=activations, precision=precision,
                                          fill=fill)
        self.mmp_row = fe.row
        for name in SPEC_NAMES:
            setattr(self, "mmp_" + name, getattr(fe, name))
        self.mmp_chunk = int(mmp_chunk) if mmp_chunk is not None else max(1, MMP_INPUT_BYTES // fe.bytes_per_item)

    def _init_dwa(self, robot_paths):
        """The node paths the deviation term measures against, padded with their last node; no solver state."""
        pmax = max(2, max(len(p) for p in robot_paths))
        nodes = np.stack([np.array([tuple(q)[:2] for q in p] + [tuple(p[-1])[:2]] * (pmax - len(p)), dtype=float) for p in robot_paths])
        self.node_path = self._tensor(nodes)                                  # [B,Pmax,2]
        self.node_len = self.torch.as_tensor([len(p) for p in robot_paths], dtype=self.torch.long, device=self.dev)
        self.dwa_cap = self._dwa_capacity()

    def _dwa_capacity(self) -> int:
        """Candidates per scenario the limits and resolutions can give (the bound nmpc_dwa_step checks ``cap`` against)."""
        c = self.dwa_config

        def axis(rng, acc, res):
            w = min(rng, 2.0 * acc * float(self.ts))
            return int(w / res * (1.0 + 1e-9)) + 1 if w > 0 else 1
        return axis(c.lin_vel_max - c.lin_vel_min, c.lin_acc_max, c.vel_resolution) * axis(2.0 * c.ang_vel_max, c.ang_acc_max, c.ang_resolution)

    # ---------------------------------------------------------------------------------------------------------
    def _predict_cv(self):
        """[B,H,N+1,6] obstacle rows from the constant-velocity extrapolation of the last <= 5 positions."""
        torch = self.torch
        B, H, N = self.B, self.H, self.N
        diffs = self.hist[:, :, 1:, :] - self.hist[:, :, :-1, :]                 # [B,H,4,2], newest last
        nd = (self.hcount - 1).clamp(min=0, max=4)                               # usable differences
        k = torch.arange(4, device=self.dev)[None, None, :]
        mask = (k >= (4 - nd[..., None])).to(self.tdt)[..., None]
        vel = (diffs * mask).sum(dim=2) / nd.clamp(min=1)[..., None].to(self.tdt)
        off = torch.arange(0, N + 1, device=self.dev, dtype=self.tdt)[None, None, :, None]
        if self.n_hyp > 1:       # hypothesis fan around the constant-velocity step (nmpc_hip.h, nmpc_loop_args::n_hyp)
            nh = self.n_hyp
            ang = (torch.arange(nh, device=self.dev, dtype=self.tdt) - 0.5 * (nh - 1)) * self.hyp_fan
            ca, sa = torch.cos(ang)[None, None, :], torch.sin(ang)[None, None, :]
            wx = ca * vel[:, :, None, 0] - sa * vel[:, :, None, 1]                 # [B,H,nh]
            wy = sa * vel[:, :, None, 0] + ca * vel[:, :, None, 1]
            w = torch.stack([wx, wy], dim=-1).reshape(B, H * nh, 2)
            cur = self.humans[:, :, None, :].expand(-1, -1, nh, -1).reshape(B, H * nh, 2)
            rows = torch.zeros(B, H * nh, N + 1, 6, dtype=self.tdt, device=self.dev)
            rows[..., 0:2] = cur[:, :, None, :] + w[:, :, None, :] * off
            rows[..., 2:4] = (HUMAN_SIZE + self.hyp_grow * off)
            rows[..., 5] = 1.0
            return rows
        rows = torch.zeros(B, H, N + 1, 6, dtype=self.tdt, device=self.dev)
        rows[..., 0:2] = self.humans[:, :, None, :] + vel[:, :, None, :] * off
        rows[..., 2:4] = 1.0
        rows[:, :, 0, 2:4] = HUMAN_SIZE
        rows[..., 5] = 1.0
        return rows

    def _ref_states(self):
        """TrajectoryTracker.get_ref_states for all scenarios (note the reference passes N_hor as ``action_steps``,
        trajectory_tracker.py:186-187, so the search window is [idx - N, idx + 5N); N rows are taken -- the
        reference's default ``horizon=20`` equals N_hor in both shipped yaml files)."""
        torch = self.torch
        N, hor = self.N, self.N
        Lmax = self.ref_traj.shape[1]
        j = torch.arange(Lmax, device=self.dev)[None, :]
        lo = (self.idx_ref - N).clamp(min=0)[:, None]
        hi = torch.minimum(self.ref_len, self.idx_ref + 5 * N)[:, None]
        d = torch.hypot(self.robot[:, None, 0] - self.ref_traj[:, :, 0], self.robot[:, None, 1] - self.ref_traj[:, :, 1])
        d = torch.where((j >= lo) & (j < hi), d, torch.full_like(d, float("inf")))
        self.idx_ref = torch.argmin(d, dim=1)               # first minimum, like list.index(min(...))
        rows = self.idx_ref[:, None] + torch.arange(hor, device=self.dev)[None, :]
        rows = torch.minimum(rows, (self.ref_len - 1)[:, None])
        return torch.gather(self.ref_traj, 1, rows[..., None].expand(-1, -1, 3)).contiguous()[:, :N]

    def _in_polygon(self, pts):
        """[B] strictly inside any convex quadrilateral (shapely Polygon.contains)."""
        a = self.polys[None]                                                     # [1,M,4,2]
        b = self.torch.roll(self.polys, -1, dims=1)[None]
        p = pts[:, None, None, :]
        cross = (b[..., 0] - a[..., 0]) * (p[..., 1] - a[..., 1]) - (b[..., 1] - a[..., 1]) * (p[..., 0] - a[..., 0])
        inside = (cross > 0).all(dim=2) | (cross < 0).all(dim=2)
        return inside.any(dim=1)

    def _polygon_distance(self, pts):
        """[B] distance to the closest polygon (0 inside), shapely Polygon.distance(Point)."""
        torch = self.torch
        a = self.polys[None]
        b = torch.roll(self.polys, -1, dims=1)[None]
        p = pts[:, None, None, :]
        ab = b - a
        t = (((p - a) * ab).sum(-1) / (ab * ab).sum(-1)).clamp(0, 1)
        d = torch.linalg.norm(a + t[..., None] * ab - p, dim=-1).min(dim=2).values     # [B,M]
        cross = ab[..., 0] * (p[..., 1] - a[..., 1]) - ab[..., 1] * (p[..., 0] - a[..., 0])
        inside = (cross > 0).all(dim=2) | (cross < 0).all(dim=2)
        return torch.where(inside, torch.zeros_like(d), d).min(dim=1).values

    def _draw_stagger(self):
        """The [B, H] stagger of one pedestrian step, or None without one: the next recorded draw of ``stagger_replay``, else
        sign x magnitude from the seeded generator (two calls, in this order: a seed fixes the run)."""
        torch = self.torch
        if self.stagger_replay is not None:
            return self.stagger_replay.pop(0).to(self.tdt).contiguous()
        if self.stagger > 0:
            R = self.fleet or 1     # one draw per group: its members see the same pedestrians
            sign = torch.randint(0, 2, (self.B // R, self.H), generator=self.gen, device=self.dev) * 2 - 1
            mag = torch.randint(0, 11, (self.B // R, self.H), generator=self.gen, device=self.dev).to(self.tdt) / 10
            st = sign.to(self.tdt) * mag * self.stagger
            return (st if R == 1 else st.repeat_interleave(R, dim=0)).contiguous()
        return None

    def _step_humans(self):
        torch = self.torch
        W = self.hpath.shape[2]
        tgt = torch.gather(self.hpath, 2, self.hidx.clamp(max=W - 1)[..., None, None].expand(-1, -1, 1, 2))[:, :, 0]
        dist = torch.linalg.norm(tgt - self.humans, dim=-1)
        adv = (dist < HUMAN_VMAX * self.ts) & (self.hidx < W)                    # basic_agent.py:57-59
        self.hidx = self.hidx + adv.long()
        moving = self.hidx < W
        tgt = torch.gather(self.hpath, 2, self.hidx.clamp(max=W - 1)[..., None, None].expand(-1, -1, 1, 2))[:, :, 0]
        dist = torch.linalg.norm(tgt - self.humans, dim=-1).clamp(min=1e-12)
        dire = (tgt - self.humans) / dist[..., None]
        st = self._draw_stagger()
        st = 0.0 if st is None else st[..., None]
        new = self.humans + self.ts * (dire * HUMAN_VMAX + st)                   # omnidirectional model
        self.humans = torch.where(moving[..., None], new, self.humans)
        # past_traj grows only while the pedestrian moves (basic_agent.py:72-82)
        shifted = torch.cat([self.hist[:, :, 1:], self.humans[:, :, None, :]], dim=2)
        self.hist = torch.where(moving[..., None, None], shifted, self.hist)
        self.hcount = self.hcount + moving.long()

    # ---------------------------------------------------------------------------------------------------------
    def _solve(self, hs, Pa, nA, Ua, u0, ya, y_is_input, info, status=None):
        """The MPC solves of one time step: parameters ``Pa[nA, np]`` -> controls ``Ua[nA, 2N]``, multipliers ``ya`` in / out
        (device tensors; main_base.py:308-311 per scenario), optionally the exit statuses. One overridable call, so that a
        checker can drive the same closed loop with another solver (tests/test_gpu_closed_loop.py puts the CPU oracle here)."""
        hs.solve_raw(self.dt, Pa, nA, Ua, status=status, u0=u0, y=ya, y_is_input=y_is_input, info=info, sync=False)

    def run(self, max_steps: int = 120, record: Optional[list] = None) -> EvaluationResult:
        """``record``: if a list, one dict per time step is appended with host copies of what the step saw and
        produced (robot, humans, P, y_in, U) -- for step-by-step checks against the sequential API; costs a
        device->host copy per step."""
        return self._run_fused(max_steps, record) if self.fused else self._run_torch(max_steps, record)

    # ---- one run: its buffers, the argument structs of the stage kernels, its result ---------------------------
    def _start_run(self, flag_dtype):
        """Flags, counters and metrics of a run that starts now (``flag_dtype``: uint8 for the kernels, bool for torch)."""
        torch, B, z = self.torch, self.B, self._full
        d0 = torch.cdist(self.robot[:, None, :2], self.ref_traj[:, :, :2])[:, 0]
        dev_sum = d0.min(dim=1).values.clone()      # trajectory metrics include the start state (robot.past_traj[0])
        return SimpleNamespace(
            alive=z(B, dtype=flag_dtype, fill=1), collision=z(B, dtype=flag_dtype, fill=0), complete=z(B, dtype=flag_dtype, fill=0),
            steps=z(B, dtype=torch.long, fill=0), last_u=z(B, 2), clr_dyn=z(B, fill=float("inf")),
            clr_stc=self._polygon_distance(self.robot[:, :2]).contiguous(), dev_sum=dev_sum, dev_max=dev_sum.clone(), n_traj=z(B, fill=1.0))

    def _finish_run(self, r, traj, acts, solve_ms) -> EvaluationResult:
        """``traj`` [B, T+1, 3] and ``acts`` [B, T, 2] of the T lock-steps run -> the result on the host."""
        torch = self.torch
        T_run = acts.shape[1]
        collision = r.collision.bool() | r.alive.bool()                          # time-out, main_base.py:407-410
        # rows after a scenario's end repeat its last state
        t_idx = torch.minimum(torch.arange(T_run + 1, device=self.dev)[None, :], r.steps.clamp(max=T_run)[:, None])
        traj = torch.gather(traj, 1, t_idx[..., None].expand(-1, -1, 3))
        return EvaluationResult(
            collision=collision.cpu().numpy(), complete=r.complete.bool().cpu().numpy(), steps=r.steps.cpu().numpy(),
            smoothness=action_smoothness(acts).cpu().numpy(), clearance=r.clr_stc.cpu().numpy(), clearance_dyn=r.clr_dyn.cpu().numpy(),
            deviation=torch.stack([r.dev_sum / r.n_traj, r.dev_max], dim=1).cpu().numpy(),
            trajectory=traj.cpu().numpy(), actions=acts.cpu().numpy(), solve_ms=solve_ms,
            clearance_fleet=r.clr_fleet.cpu().numpy() if hasattr(r, "clr_fleet") else None,
            collision_fleet=r.collision_fleet.bool().cpu().numpy() if hasattr(r, "collision_fleet") else None)

    def _loop_args(self, r, max_steps):
        """``NmpcLoopArgs`` of a run: the evaluator's state (made contiguous: the kernels update it in place), the run's
        flags and metrics, and the compact buffers of the running scenarios that the stages between pre and post read."""
        torch, B, N, H, z = self.torch, self.B, self.N, self.H, self._full
        r.traj = torch.empty(B, max_steps + 1, 3, dtype=self.tdt, device=self.dev)
        r.traj[:, 0] = self.robot
        r.acts = z(B, max(max_steps, 1), 2, fill=float("nan"))
        r.state_c, r.last_u_c, r.refs_c, r.speed_c = z(B, 3), z(B, 2), z(B, N, 3), z(B)
        r.dyn_c = z(B, H * self.n_hyp, N + 1, 6)
        r.ya_buf = z(B, 2 * N)
        r.ref_len = self.ref_len.to(torch.long).contiguous()
        for name in ("hidx", "hcount", "idx_ref", "hist", "humans", "robot"):
            setattr(self, name, getattr(self, name).contiguous())
        a = _capi.NmpcLoopArgs()
        a.B, a.H, a.W, a.Lmax, a.M, a.max_steps = B, H, int(self.hpath.shape[2]), int(self.ref_traj.shape[1]), int(self.polys.shape[0]), max(max_steps, 1)
        a.base_speed, a.lin_vel_max, a.human_size, a.human_vmax = self.base_speed, self.lin_vel_max, HUMAN_SIZE, HUMAN_VMAX
        a.n_hyp, a.hyp_fan_rad, a.hyp_radius0, a.hyp_radius_growth = self.n_hyp, self.hyp_fan, HUMAN_SIZE, self.hyp_grow
        for src, names in ((self, ("robot", "humans", "hist", "hcount", "hidx", "hpath", "ref_traj", "idx_ref", "goal", "polys", "U", "y")),
                           (r, ("last_u", "ref_len", "alive", "collision", "complete", "steps", "clr_dyn", "clr_stc", "dev_sum", "dev_max",
                                "n_traj", "traj", "acts", "state_c", "last_u_c", "refs_c", "speed_c", "dyn_c"))):
            for name in names:
                assert getattr(src, name).is_contiguous(), name
                setattr(a, name, getattr(src, name).data_ptr())
        return a

    def _kf_args(self, r, max_steps):
        """``NmpcKfArgs`` of a run: past_traj of every pedestrian (nmpc_kf_predict appends the current position while hcount
        grows) and the run's covariance: main_base.py:158-172 makes a new interface object, i.e. P = P0, per run."""
        B, H, ts, z = self.B, self.H, float(self.ts), self._full
        cap = max(max_steps, 1) + 1
        r.kf_traj, r.kf_len = z(B, H, cap, 2), z(B, H, dtype=self.torch.long, fill=0)
        r.kf_P = self.torch.as_tensor(self.kf_P0, dtype=self.tdt, device=self.dev).repeat(B, 1, 1).contiguous()
        kf = _capi.NmpcKfArgs().set_matrices([[1, 0, ts, 0], [0, 1, 0, ts], [0, 0, 1, 0], [0, 0, 0, 1]],
                                             [[1, 0, 0, 0], [0, 1, 0, 0]], self.kf_Q, self.kf_R)      # zfilter.model_CV(ts)
        kf.B, kf.H, kf.cap, kf.human_size = B, H, cap, HUMAN_SIZE
        kf.humans, kf.hcount, kf.dyn_c = self.humans.data_ptr(), self.hcount.data_ptr(), r.dyn_c.data_ptr()
        kf.kf_traj, kf.kf_len, kf.kf_P = r.kf_traj.data_ptr(), r.kf_len.data_ptr(), r.kf_P.data_ptr()
        return kf

    def _fleet_args(self, r):
        """``NmpcFleetArgs`` of a run: the full robot / U / flag arrays, the run's fleet clearance and flag, the blocks."""
        r.clr_fleet, r.collision_fleet = self._full(self.B, fill=float("inf")), self._full(self.B, dtype=self.torch.uint8, fill=0)
        r.other_in = None
        fa = _capi.NmpcFleetArgs()
        fa.B, fa.R, fa.ts, fa.width = self.B, self.fleet, float(self.ts), float(self.cfg.vehicle_width)
        fa.robot, fa.alive, fa.collision, fa.complete = self.robot.data_ptr(), r.alive.data_ptr(), r.collision.data_ptr(), r.complete.data_ptr()
        fa.clr_fleet, fa.collision_fleet = r.clr_fleet.data_ptr(), r.collision_fleet.data_ptr()
        fa.other_c = self.other_c.data_ptr() if self.fleet_coupling else None
        return fa

    def _mmp_args(self, r, max_steps):
        """The stage's buffers of a run: the hypotheses (pedestrian major as the network returns them, then per scenario as snap
        and f2 take them), f2's obstacle rows -- which f1 reads instead of ``loop_pre``'s -- and the per-step counts. Returns the
        front end with its own buffers (the network's input tensor of one chunk) in place."""
        torch, B, N, H, K, z = self.torch, self.B, self.N, self.H, self.mmp_hyp, self._full
        self.mmp_front.allocate(min(self.mmp_chunk, B * H))
        r.mmp_raw_p, r.mmp_hyp = z(B * H, N, K, 2), z(B, N, H * K, 2)
        r.mmp_dyn = z(B, self.cfg.Ndynobs, N + 1, 6)
        r.mmp_n_obs, r.mmp_n_out = z(B, dtype=torch.int32, fill=0), z(B, dtype=torch.int32, fill=0)
        r.mmp_counts = z(B, N + 1, dtype=torch.int32, fill=0)      # rows of mmp_dyn per offset that are clusters (the lists DWA step reads them)
        r.mmp_obs_steps = z(max(max_steps, 1), B, dtype=torch.int32, fill=-1)
        r.mmp_out_steps = z(max(max_steps, 1), B, dtype=torch.int32, fill=-1)
        r.mmp_all = torch.arange(B * H, dtype=torch.long, device=self.dev)
        r.mmp_events = []
        r.dyn_in = r.mmp_dyn
        return self.mmp_front

    def _mmp_predict(self, r, fe, kt, idx, nA):
        """The multi-hypothesis predictor for the ``nA`` running scenarios (``idx``, None = all), MainBase.run_wta_prediction
        (main_base.py:175-208): per chunk of pedestrians the device front end (``MmpFrontEnd.run``: input stack, or the fused first
        layer's output, then the fused blocks of layer1 to layer4) -> network (with ``mmp_head`` the front end's last launch instead); then, per scenario with its pedestrians' segments concatenated
        in order (:192-195), snap -> f2 with ``cur`` = the current positions. Writes ``r.mmp_dyn[:nA]`` and ``r.mmp_counts[:nA]``."""
        torch, N, H, K = self.torch, self.N, self.H, self.mmp_hyp

        def part(name, call):
            if not self.time_predictor_parts:
                return call()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = call()
            e1.record()
            r.mmp_events.append((kt, name, e0, e1))
            return out
        items = r.mmp_all if idx is None else (idx[:, None] * H + r.mmp_all[None, :H]).reshape(-1).contiguous()
        n_ped = nA * H
        for c0 in range(0, n_ped, self.mmp_chunk):
            n = min(self.mmp_chunk, n_ped - c0)
            x = fe.run(self.hist.data_ptr(), self.hcount.data_ptr(), self.B, H, items[c0:].data_ptr(), n, part)
            if self.mmp_head is not None:
                out = x                                             # (the head was the front end's last launch)
            else:
                with torch.no_grad():
                    out = part("network", lambda: self.network(x))
            if out.numel() != n * N * K * 2:
                raise ValueError(f"the network returned {tuple(out.shape)} for {n * N} inputs; expected {K} hypotheses (x, y) each")
            r.mmp_raw_p[c0:c0 + n] = out.reshape(n, N, K, 2)
        # [pedestrian][offset][K] -> [scenario][offset][H * K]: the pedestrians' segments side by side
        raw = r.mmp_raw_p[:n_ped].view(nA, H, N, K, 2).permute(0, 2, 1, 3, 4).reshape(nA, N, H * K, 2)
        hyp = r.mmp_hyp[:nA]
        part("snap", lambda: self.h.snap_hypotheses(self.dt, raw, hyp, H, K, self.mmp_tf, self.mmp_rescale, n_outside=r.mmp_n_out[:nA]))
        cur = self.humans if idx is None else self.humans.index_select(0, idx)
        part("f2", lambda: self.h.hypotheses_to_ellipses(self.dt, hyp, cur, r.mmp_dyn[:nA], r.mmp_n_obs[:nA], human_size=HUMAN_SIZE,
                                                         eps=1.0, enlarge=2.0, extra_margin=0.0, counts=r.mmp_counts[:nA]))
        for steps, now in ((r.mmp_obs_steps, r.mmp_n_obs), (r.mmp_out_steps, r.mmp_n_out)):
            if idx is None:
                steps[kt].copy_(now)
            else:
                steps[kt].index_copy_(0, idx, now[:nA])

    def _dwa_args(self, r):
        """``NmpcDwaArgs`` of a run: the compact buffers ``loop_pre`` fills in, the node paths, the outputs per scenario. With the
        predictor ``mmp`` (after ``_mmp_args``): ``NmpcDwaListsArgs`` on the stage's ``mmp_dyn`` / ``mmp_counts``."""
        B, z, i32 = self.B, self._full, self.torch.int32
        r.dwa_cost, r.dwa_choice, r.dwa_counts = z(B), z(B, dtype=i32, fill=0), z(B, 2, dtype=i32, fill=0)
        lists = self.predictor == "mmp"        # f2's rows with their per-offset counts: nmpc_dwa_step_lists_*, R = Ndynobs
        dw = (_capi.NmpcDwaListsArgs() if lists else _capi.NmpcDwaArgs()).set_config(self.dwa_config, self.speed_scale)
        dw.B, dw.H, dw.M, dw.Pmax, dw.cap = B, self.H, int(self.polys.shape[0]), int(self.node_path.shape[1]), self.dwa_cap
        dw.dyn_mode = 1 if self.predictor is None else 2
        dw.state_c, dw.last_u_c, dw.dyn_c = r.state_c.data_ptr(), r.last_u_c.data_ptr(), r.dyn_c.data_ptr()
        if lists:
            dw.R, dw.dyn_c, dw.dyn_count = int(self.cfg.Ndynobs), r.mmp_dyn.data_ptr(), r.mmp_counts.data_ptr()
        dw.goal, dw.path, dw.path_len = self.goal.data_ptr(), self.node_path.data_ptr(), self.node_len.data_ptr()
        dw.polys = self.polys.data_ptr() if self.polys.numel() else None
        dw.min_cost, dw.choice, dw.counts = r.dwa_cost.data_ptr(), r.dwa_choice.data_ptr(), r.dwa_counts.data_ptr()
        return dw

    def _timed(self, call, flag):
        """A stage call and the list of its HIP event pairs: ``call`` itself and None, or, with the stage's timing flag set,
        ``call`` between two events that are appended to the list."""
        if not flag:
            return call, None
        Event, events = self.torch.cuda.Event, []

        def timed(*args):
            events.append((Event(enable_timing=True), Event(enable_timing=True)))
            events[-1][0].record()
            call(*args)
            events[-1][1].record()
        return timed, events

    def _record_entry(self, alive):
        """What a time step saw, on the host; the tracker stage adds what it produced."""
        return dict(robot=self.robot.cpu().numpy(), humans=self.humans.cpu().numpy(), alive=alive.bool().cpu().numpy())

    # ---- the tracker stage ----------------------------------------------------------------------------------------
    def _solve_step(self, kt, idx, nA, Pa, Ua, ya, rec):
        """The solves of time step ``kt`` for the ``nA`` running scenarios (``idx``, None = all): ``Pa`` -> ``Ua``, ``ya``
        in / out. Returns the handle that ran them (its ``last_kernel_ms()`` is the step's solve time)."""
        torch = self.torch
        full = nA == self.B
        if rec is not None:
            rec["y_in"] = self.y.cpu().numpy()
        u0 = None
        if self.warm_start and kt > 0:
            shifted = torch.cat([self.U[:, 2:], self.U[:, -2:]], dim=1)
            u0 = shifted.contiguous() if full else shifted.index_select(0, idx).contiguous()
        hs = self.h
        if self._h_by_waves:      # latency-kernel family: W by the size of the running batch (results unchanged)
            cap = 3 * self._n_simd if self.dt == np.float32 else 2 * self._n_simd     # resident wavefronts
            hs = self._h_by_waves[min(4, max(2, cap // max(nA, 1)))]
        # longest first: the evaluation counts of the previous time step rank this step's solves (a scenario that
        # was hard a moment ago still is); pure scheduling -- the results do not depend on the order
        info = None
        if self.dispatch_by_history and nA >= self.dispatch_min_batch:
            if kt > 0:
                prev = self._evals if full else self._evals.index_select(0, idx)
                hs.set_dispatch_order(torch.argsort(prev, descending=True, stable=True).to(torch.int32))
            info = self._info[:nA]
        # (-2: a solver put into _solve that does not report statuses leaves them uncounted)
        st_buf = self.status[:nA].fill_(-2) if self.count_status else None
        self._solve(hs, Pa, nA, Ua, u0, ya, kt > 0, info, status=st_buf)
        if st_buf is not None:
            self.status_counts.append(torch.bincount(st_buf.clamp(min=-1, max=3) + 1, minlength=5)[1:])
        if info is not None:
            if full:
                self._evals.copy_(info[:, 4])
            else:
                self._evals.index_copy_(0, idx, info[:, 4].contiguous())
        if rec is not None:
            rec["P"] = (self.P if full else torch.zeros_like(self.P).index_copy_(0, idx, Pa)).cpu().numpy()
        return hs

    def _mpc_step(self, r, kt, idx, nA, Ua, ya, rec):
        """The MPC tracker on the compact buffers of the running scenarios (``loop_pre``'s, or the torch path's): f1, the
        harvesting hook, the solves."""
        Pa = self.P if nA == self.B else self.P[:nA]
        self.h.assemble_params(self.dt, nA, Pa, r.last_u_c, r.state_c, r.refs_c, r.speed_c, self.tuning, self.stcw, self.dynw,
                               self.polys, getattr(r, "dyn_in", r.dyn_c)[:nA], other_robots=getattr(r, "other_in", None))
        if self.on_params is not None:
            self.on_params(kt, idx, Pa)
        return self._solve_step(kt, idx, nA, Pa, Ua, ya, rec)

    def _dwa_step(self, r, dw, dwa_step, idx, nA, Ua, rec):
        """The dynamic-window tracker in place of f1 + solve: U_c = the chosen control, N times (nmpc_dwa.h). There is no
        solve, so no handle is returned."""
        dwa_step(self.dt, dw)
        if rec is not None:
            rec.update(run=None if idx is None else idx.cpu().numpy(), state_c=r.state_c[:nA].cpu().numpy(), last_u_c=r.last_u_c[:nA].cpu().numpy(),
                       U_c=Ua.cpu().numpy(), min_cost=r.dwa_cost[:nA].cpu().numpy(),
                       choice=r.dwa_choice[:nA].cpu().numpy(), counts=r.dwa_counts[:nA].cpu().numpy())

    # ---- the time step --------------------------------------------------------------------------------------------
    def _run_fused(self, max_steps, record):
        """The time step as HIP kernels (csrc/nmpc_step.h): ``loop_pre`` -> predictor stage -> tracker stage -> ``loop_post``."""
        torch, B = self.torch, self.B
        r = self._start_run(torch.uint8)
        a = self._loop_args(r, max_steps)
        kf = self._kf_args(r, max_steps) if self.predictor == "kfmp" else None
        mm = self._mmp_args(r, max_steps) if self.predictor == "mmp" else None
        dw = self._dwa_args(r) if self.tracker == "dwa" else None
        fa = self._fleet_args(r) if self.fleet is not None else None       # (after _loop_args: self.robot is the contiguous array)
        fleet_exchange, exchange_events = self._timed(self.h.fleet_exchange, self.time_fleet)
        fleet_post, post_events = self._timed(self.h.fleet_post, self.time_fleet)
        kf_predict, kf_events = self._timed(self.h.kf_predict, self.time_predictor)
        mmp_predict, mmp_events = self._timed(self._mmp_predict, self.time_predictor)
        dwa_step, dwa_events = self._timed(self.h.dwa_step_lists if self.tracker == "dwa" and mm is not None else self.h.dwa_step, self.time_tracker)
        solve_ms, n_steps_run = [], 0
        for kt in range(max_steps):
            if not bool(r.alive.any()):
                break
            n_steps_run = kt + 1
            idx = torch.nonzero(r.alive, as_tuple=False).squeeze(1).contiguous() if self.compact else None
            nA = int(idx.numel()) if idx is not None else B
            full = nA == B
            # the robots that run this step, for the fleet epilogue: without compaction loop_post takes all B and skips the stopped
            # ones by their flag, which it has just cleared for those that stop now
            ran = idx if (fa is None or self.compact) else torch.nonzero(r.alive, as_tuple=False).squeeze(1).contiguous()
            Ua = self.U if full else self._Ua[:nA]
            ya = self.y if full else r.ya_buf[:nA]
            st = self._draw_stagger()
            a.n_run, a.step = nA, kt
            a.run = None if full else idx.data_ptr()
            a.stagger = None if st is None else st.data_ptr()
            a.U_c, a.y_c, a.gather_y = Ua.data_ptr(), ya.data_ptr(), int(not full)
            self.h.loop_step(self.dt, a, post=False)
            if kf is not None:
                kf.n_run, kf.run = nA, a.run
                kf_predict(self.dt, kf)
            if mm is not None:
                mmp_predict(r, mm, kt, idx, nA)
            rec = None if record is None else self._record_entry(r.alive)
            if rec is not None and mm is not None:
                rec.update(dyn=(r.mmp_dyn if full else torch.zeros_like(r.mmp_dyn).index_copy_(0, idx, r.mmp_dyn[:nA])).cpu().numpy(),
                           dyn_count=(r.mmp_counts if full else torch.zeros_like(r.mmp_counts).index_copy_(0, idx, r.mmp_counts[:nA])).cpu().numpy(),
                           n_obs=r.mmp_obs_steps[kt].cpu().numpy(), n_outside=r.mmp_out_steps[kt].cpu().numpy())
            if fa is not None and self.fleet_coupling:
                fa.n_run, fa.run, fa.U_prev = nA, a.run, (self.U.data_ptr() if kt > 0 else None)
                fleet_exchange(self.dt, fa)
                r.other_in = self.other_c[:nA]
            if dw is not None:
                dw.n_run, dw.run, dw.U_c = nA, a.run, Ua.data_ptr()
                hs = self._dwa_step(r, dw, dwa_step, idx, nA, Ua, rec)
            else:
                hs = self._mpc_step(r, kt, idx, nA, Ua, ya, rec)
            self.h.loop_step(self.dt, a, post=True)
            if fa is not None:
                fa.n_run = int(ran.numel())
                fa.run = None if fa.n_run == B else ran.data_ptr()
                fleet_post(self.dt, fa)
            if rec is not None:
                if hs is not None:
                    rec["U"] = self.U.cpu().numpy()
                record.append(rec)
            if hs is not None and self.time_solves:
                solve_ms.append(hs.last_kernel_ms())
        for name, events in (("predictor_ms", kf_events if kf is not None else mmp_events), ("tracker_ms", dwa_events)):
            if events:
                torch.cuda.synchronize(self.dev)
                setattr(self, name, [e0.elapsed_time(e1) for e0, e1 in events])
        if exchange_events or post_events:
            torch.cuda.synchronize(self.dev)
            self.fleet_ms = {name: [e0.elapsed_time(e1) for e0, e1 in ev] for name, ev in (("exchange", exchange_events), ("post", post_events)) if ev}
        res = self._finish_run(r, r.traj[:, :n_steps_run + 1], r.acts[:, :n_steps_run], solve_ms)
        if mm is not None:
            res.n_obs, res.n_outside = r.mmp_obs_steps[:n_steps_run].cpu().numpy(), r.mmp_out_steps[:n_steps_run].cpu().numpy()
            self.predictor_part_ms = {}
            for kt, name, e0, e1 in r.mmp_events:       # (the copy above has waited for the stream)
                ms = self.predictor_part_ms.setdefault(name, [0.0] * n_steps_run)
                ms[kt] += e0.elapsed_time(e1)
        return res

    def _run_torch(self, max_steps: int = 120, record: Optional[list] = None) -> EvaluationResult:
        """The same time step written out as torch expressions (rounds 1-2): the independent check of the kernels."""
        torch = self.torch
        B, N, ts = self.B, self.N, self.ts
        r = self._start_run(torch.bool)
        traj = [self.robot.clone()]
        acts, solve_ms = [], []
        for kt in range(max_steps):
            alive = r.alive
            if not bool(alive.any()):
                break
            dyn = self._predict_cv()
            refs = self._ref_states()
            dist_goal = torch.hypot(self.robot[:, 0] - self.goal[:, 0], self.robot[:, 1] - self.goal[:, 1])
            near = dist_goal < self.base_speed * N * ts
            speed = torch.where(near, torch.clamp(dist_goal / N / ts, min=self.lin_vel_max),
                                torch.full_like(dist_goal, self.base_speed))     # sic: max(), trajectory_tracker.py:308-309
            # large batches: only the scenarios still running are assembled and solved (the finished ones keep their
            # last row of U). Small batches end with their slowest instance anyway, compaction would only add host work.
            idx = torch.nonzero(alive, as_tuple=False).squeeze(1) if self.compact else None
            nA = int(idx.numel()) if idx is not None else B
            full = nA == B
            sel = (lambda x: x.contiguous()) if full else (lambda x: x.index_select(0, idx).contiguous())
            Ua = self.U if full else self._Ua[:nA]
            ya = self.y if full else self.y.index_select(0, idx).contiguous()
            r.last_u_c, r.state_c, r.refs_c, r.speed_c, r.dyn_c = sel(r.last_u), sel(self.robot), sel(refs), sel(speed), sel(dyn)
            rec = None if record is None else self._record_entry(alive)
            hs = self._mpc_step(r, kt, idx, nA, Ua, ya, rec)
            if not full:
                self.U.index_copy_(0, idx, Ua)
                self.y.index_copy_(0, idx, ya)
            if rec is not None:
                rec["U"] = self.U.cpu().numpy()
                record.append(rec)
            solve_ms.append(hs.last_kernel_ms())
            raw = self.U[:, :2].clone()
            act = torch.where((raw[:, 0:1] < 0), torch.zeros_like(raw), raw)     # no-backward, main_base.py:320-321
            new_robot = unicycle_rk4_step(self.robot, act, ts)
            self.robot = torch.where(alive[:, None], new_robot, self.robot)
            r.last_u = torch.where(alive[:, None], raw, r.last_u)
            self._step_humans()
            r.steps = r.steps + alive.long()
            traj.append(self.robot.clone())
            acts.append(torch.where(alive[:, None], raw, torch.full_like(raw, float("nan"))))
            # metrics and flags (main_base.py:326-335)
            dd = min_dynamic_distance(self.robot[:, :2], self.humans)
            r.clr_dyn = torch.where(alive, torch.minimum(r.clr_dyn, dd), r.clr_dyn)
            r.clr_stc = torch.where(alive, torch.minimum(r.clr_stc, self._polygon_distance(self.robot[:, :2])), r.clr_stc)
            dref = deviation_to_reference(self.robot[:, :2], self.ref_traj, self.ref_len)
            r.dev_sum = r.dev_sum + torch.where(alive, dref, torch.zeros_like(dref))
            r.dev_max = torch.where(alive, torch.maximum(r.dev_max, dref), r.dev_max)
            r.n_traj = r.n_traj + alive.to(self.tdt)
            col = alive & (self._in_polygon(self.robot[:, :2]) | (dd <= HUMAN_SIZE))
            done = alive & ~col & ((self.robot[:, 0] - self.goal[:, 0]).abs() <= 0.5) & \
                ((self.robot[:, 1] - self.goal[:, 1]).abs() <= 0.5) & (act[:, 0].abs() < 0.4)
            r.collision |= col
            r.complete |= done
            r.alive = alive & ~col & ~done
        A = torch.stack(acts, dim=1) if acts else torch.zeros(B, 0, 2, dtype=self.tdt, device=self.dev)
        return self._finish_run(r, torch.stack(traj, dim=1), A, solve_ms)

    def close(self):
        for h in set(self._h_by_waves.values()) | {self.h}:
            h.close()
