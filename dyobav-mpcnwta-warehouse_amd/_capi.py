"""ctypes binding of ``libnmpc_hip.so`` (C ABI declared in ``include/nmpc_hip.h``).

This is the only place the Python host code touches native code. There is deliberately no fallback: if the
library is missing or no HIP device is visible every entry point raises -- results never come from a CPU path.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from . import build as _build

EXIT_STATUS_NAMES = ("Converged", "NotConvergedIterations", "NotConvergedOutOfTime", "NotFiniteComputation",
                     "CapacityExceeded", "NotAxisAligned")
ABI_VERSION = 5


class NmpcError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libnmpc_hip error {code}: {msg}")
        self.code = code


class NmpcConfigStruct(C.Structure):
    """Mirror of ``struct nmpc_config``."""
    _fields_ = [
        ("abi_version", C.c_int32), ("device_id", C.c_int32),
        ("N_hor", C.c_int32), ("Nother", C.c_int32), ("Nstcobs", C.c_int32), ("Ndynobs", C.c_int32),
        ("ts", C.c_double),
        ("lin_vel_min", C.c_double), ("lin_vel_max", C.c_double), ("ang_vel_max", C.c_double),
        ("lin_acc_min", C.c_double), ("lin_acc_max", C.c_double), ("ang_acc_max", C.c_double),
        ("vehicle_width", C.c_double), ("vehicle_margin", C.c_double), ("social_margin", C.c_double),
        ("tolerance", C.c_double), ("initial_tolerance", C.c_double), ("delta_tolerance", C.c_double),
        ("max_outer_iterations", C.c_int32), ("max_inner_iterations", C.c_int32),
        ("lbfgs_memory", C.c_int32), ("max_active_dynobs", C.c_int32),
        ("initial_penalty", C.c_double), ("penalty_update_factor", C.c_double),
        ("inner_tolerance_update_factor", C.c_double), ("sufficient_decrease_coeff", C.c_double),
        ("lip_eps_f64", C.c_double), ("lip_delta_f64", C.c_double),
        ("lip_eps_f32", C.c_double), ("lip_delta_f32", C.c_double),
        ("cbfgs_alpha", C.c_double), ("cbfgs_epsilon", C.c_double), ("sy_epsilon", C.c_double),
        ("latency_waves", C.c_int32), ("akkt_form", C.c_int32),
        ("max_solver_time_us", C.c_double),
        ("coop_waves", C.c_int32), ("axis_aligned", C.c_int32), ("reg_table", C.c_int32), ("staged", C.c_int32),
        ("polish", C.c_int32), ("polish_max_outer_iterations", C.c_int32), ("polish_max_inner_iterations", C.c_int32),
        ("staged_evals", C.c_int32),
        ("polish_tolerance", C.c_double), ("polish_delta_tolerance", C.c_double),
        ("max_evaluations", C.c_int32), ("tail_latency", C.c_int32), ("batch_invariant", C.c_int32),
    ]


class NmpcLayoutInfo(C.Structure):
    """Mirror of ``struct nmpc_layout_info``."""
    _fields_ = [("np", C.c_int32), ("lds_bytes_f32", C.c_int32), ("lds_bytes_f64", C.c_int32),
                ("reg_slots_f32", C.c_int32), ("global_table_f32", C.c_int32), ("global_table_f64", C.c_int32),
                ("ws_elems_f32", C.c_int64), ("ws_elems_f64", C.c_int64),
                ("table_entries_f32", C.c_int32), ("table_entries_f64", C.c_int32),
                ("dyn_cap", C.c_int32), ("reserved", C.c_int32)]


class NmpcAssembleArgs(C.Structure):
    """Mirror of ``struct nmpc_assemble_args`` (device pointers)."""
    _fields_ = [("last_u", C.c_void_p), ("state", C.c_void_p), ("ref_states", C.c_void_p), ("speed_ref", C.c_void_p),
                ("tuning", C.c_void_p), ("other_robots", C.c_void_p), ("map_polygons", C.c_void_p),
                ("n_map_polygons", C.c_int32), ("n_dyn", C.c_int32), ("dyn_obstacles", C.c_void_p),
                ("stc_weights", C.c_void_p), ("dyn_weights", C.c_void_p), ("selected", C.c_void_p)]


class NmpcLoopArgs(C.Structure):
    """Mirror of ``struct nmpc_loop_args`` (device pointers)."""
    _fields_ = ([(n, C.c_int32) for n in ("B", "n_run", "H", "W", "Lmax", "M", "step", "max_steps")] + [("run", C.c_void_p)] +
                [(n, C.c_double) for n in ("base_speed", "lin_vel_max", "human_size", "human_vmax")] +
                [(n, C.c_void_p) for n in ("robot", "last_u", "humans", "hist", "hcount", "hidx", "hpath", "ref_traj", "ref_len",
                                           "idx_ref", "goal", "polys", "stagger", "alive", "collision", "complete", "steps",
                                           "clr_dyn", "clr_stc", "dev_sum", "dev_max", "n_traj", "traj", "acts", "state_c",
                                           "last_u_c", "refs_c", "speed_c", "dyn_c", "U_c", "y_c", "U", "y")] +
                [("gather_y", C.c_int32), ("n_hyp", C.c_int32)] +
                [(n, C.c_double) for n in ("hyp_fan_rad", "hyp_radius0", "hyp_radius_growth")])


class NmpcKfArgs(C.Structure):
    """Mirror of ``struct nmpc_kf_args`` (device pointers; ``A`` [4,4], ``C`` [2,4], ``Q`` [4,4], ``R`` [2,2] row-major)."""
    _fields_ = ([(n, C.c_int32) for n in ("B", "n_run", "H", "cap")] +
                [(n, C.c_void_p) for n in ("run", "humans", "hcount", "kf_traj", "kf_len", "kf_P")] +
                [("A", C.c_double * 16), ("C", C.c_double * 8), ("Q", C.c_double * 16), ("R", C.c_double * 4),
                 ("human_size", C.c_double), ("dyn_c", C.c_void_p)])

    def set_matrices(self, A, Cm, Q, R):
        for name, m, shape in (("A", A, (4, 4)), ("C", Cm, (2, 4)), ("Q", Q, (4, 4)), ("R", R, (2, 2))):
            m = np.asarray(m, dtype=np.float64)
            if m.shape != shape:
                raise ValueError(f"{name} must be {shape}, got {m.shape}")
            getattr(self, name)[:] = m.ravel().tolist()
        return self


class NmpcFleetArgs(C.Structure):
    """Mirror of ``struct nmpc_fleet_args`` (device pointers; ``ts`` / ``width`` <= 0: the handle's ``ts`` / ``vehicle_width``)."""
    _fields_ = ([(n, C.c_int32) for n in ("B", "R", "n_run", "reserved")] + [("run", C.c_void_p), ("ts", C.c_double), ("width", C.c_double)] +
                [(n, C.c_void_p) for n in ("robot", "U_prev", "alive", "other_c", "clr_fleet", "collision", "complete", "collision_fleet")])


class NmpcDwaArgs(C.Structure):
    """Mirror of ``struct nmpc_dwa_args`` (device pointers)."""
    _fields_ = ([(n, C.c_int32) for n in ("B", "n_run", "H", "M", "Pmax", "cap", "dyn_mode", "reserved")] +
                [(n, C.c_void_p) for n in ("run", "state_c", "last_u_c", "dyn_c", "goal", "path", "path_len", "polys")] +
                [(n, C.c_double) for n in ("lin_vel_min", "lin_vel_max", "lin_acc_max", "ang_vel_max", "ang_acc_max",
                                           "base_speed_factor", "vel_resolution", "ang_resolution", "stuck_threshold",
                                           "q_speed", "q_goal_dir", "q_ref_deviation", "q_stc_obstacle", "q_dyn_obstacle")] +
                [(n, C.c_void_p) for n in ("U_c", "min_cost", "choice", "counts", "cost_all", "cand_all")])

    def set_config(self, cfg, base_speed_factor: float = 0.8):
        """Limits, resolutions and weights from a :class:`.configs.DwaConfiguration` ('work' mode: 0.8 lin_vel_max)."""
        for n in ("lin_vel_min", "lin_vel_max", "lin_acc_max", "ang_vel_max", "ang_acc_max", "vel_resolution", "ang_resolution",
                  "stuck_threshold", "q_speed", "q_goal_dir", "q_ref_deviation", "q_stc_obstacle", "q_dyn_obstacle"):
            setattr(self, n, float(getattr(cfg, n)))
        self.base_speed_factor = float(base_speed_factor)
        return self


class NmpcDwaListsArgs(C.Structure):
    """Mirror of ``struct nmpc_dwa_lists_args`` (device pointers): the fields of ``NmpcDwaArgs`` with ``R`` (rows per scenario) in the
    place of ``reserved``, then ``dyn_count`` [n_run, N+1] int32; ``H`` and ``dyn_mode`` are not read."""
    _fields_ = [(("R" if n == "reserved" else n), t) for n, t in NmpcDwaArgs._fields_] + [("dyn_count", C.c_void_p)]
    set_config = NmpcDwaArgs.set_config


def set_world_transform(args, transform, rescale: float = 1.0):
    """The constants of a :class:`.snap.WorldTransform` and ``rescale`` into ``args`` (any struct with these field names), returned."""
    args.x_reverse, args.y_reverse = int(bool(transform.x_reverse)), int(bool(transform.y_reverse))
    args.scale, args.offset_x, args.offset_y = float(transform.scale), float(transform.offsetx_after), float(transform.offsety_after)
    args.x_max, args.y_max = float(transform.x_max_before), float(transform.y_max_before)
    args.rescale = float(rescale)
    return args


class NmpcSnapArgs(C.Structure):
    """Mirror of ``struct nmpc_snap_args`` (device pointers)."""
    _fields_ = ([(n, C.c_int32) for n in ("n_ped", "n_hyp", "x_reverse", "y_reverse")] +
                [(n, C.c_double) for n in ("rescale", "scale", "offset_x", "offset_y", "x_max", "y_max")] +
                [("n_snapped", C.c_void_p), ("n_outside", C.c_void_p)])


class NmpcMmpArgs(C.Structure):
    """Mirror of ``struct nmpc_mmp_args`` (device pointers)."""
    _fields_ = ([(n, C.c_int32) for n in ("B", "H", "n_item", "n_off", "Hm", "Wm", "x_reverse", "y_reverse")] +
                [(n, C.c_void_p) for n in ("items", "hist", "hcount")] +
                [(n, C.c_double) for n in ("scale", "offset_x", "offset_y", "x_max", "y_max", "rescale", "sigma")] +
                [("ref_image", C.c_void_p), ("out", C.c_void_p)])

    def set_transform(self, transform, rescale: float = 1.0, sigma: float = 20.0):
        """The constants of a :class:`.snap.WorldTransform` (applied backwards: world -> map pixels), ``rescale``, ``sigma``."""
        set_world_transform(self, transform, rescale).sigma = float(sigma)
        return self


class NmpcMmpStemArgs(C.Structure):
    """Mirror of ``struct nmpc_mmp_stem_args`` (device pointers): the fields of ``nmpc_mmp_args`` down to ``ref_image``, then the
    first layer's ``C``, ``slope``, ``weight`` [C, 7, 7, 7], ``bn_scale`` / ``bn_shift`` [C] and ``out`` [n_item, n_off, C, Hp, Wp]."""
    _fields_ = (NmpcMmpArgs._fields_[:-1] + [("C", C.c_int32), ("slope", C.c_float)] +
                [(n, C.c_void_p) for n in ("weight", "bn_scale", "bn_shift", "out")])
    set_transform = NmpcMmpArgs.set_transform


class NmpcMmpBlockArgs(C.Structure):
    """Mirror of ``struct nmpc_mmp_block_args`` (device pointers): one residual block of the network's layer1, ``x`` [M, Cin, H, W]
    -> ``out`` [M, 16, H, W]; ``wd = None`` for the block without a projection (``Cin == 16``)."""
    _fields_ = ([(n, C.c_int32) for n in ("M", "Cin", "H", "W")] +
                [(n, C.c_void_p) for n in ("x", "w1", "s1", "b1", "w2", "s2", "b2", "wd", "sd", "bd")] +
                [("slope_mid", C.c_float), ("slope_out", C.c_float), ("out", C.c_void_p)])


class NmpcMmpBlockF16Args(C.Structure):
    """Mirror of ``struct nmpc_mmp_block_f16_args`` (device pointers): the fields of ``NmpcMmpBlockArgs`` (no stride), with ``w1``,
    ``w2`` and ``wd`` the packed binary16 fragments of ``mmp_stem.pack_block1_f16`` (aligned to 16 bytes)."""
    _fields_ = NmpcMmpBlockArgs._fields_


class NmpcMmpBlock2Args(C.Structure):
    """Mirror of ``struct nmpc_mmp_block2_args`` (device pointers): one residual block of the network's layer2, ``x`` [M, Cin, H, W]
    -> ``out`` [M, 32, H2, W2] with ``H2 = (H - 1) // stride + 1``; the fields of ``NmpcMmpBlockArgs``, then ``stride`` (1 or 2, of
    the first convolution and the projection); ``wd = None`` for the block without a projection (``Cin == 32``, stride 1)."""
    _fields_ = NmpcMmpBlockArgs._fields_ + [("stride", C.c_int32)]


class NmpcMmpBlock2F16Args(C.Structure):
    """Mirror of ``struct nmpc_mmp_block2_f16_args`` (device pointers): the fields of ``NmpcMmpBlock2Args``, with ``w1``, ``w2`` and
    ``wd`` the packed binary16 fragments of ``mmp_stem.pack_block2_f16`` (aligned to 16 bytes)."""
    _fields_ = NmpcMmpBlock2Args._fields_


class NmpcMmpBlock3Args(C.Structure):
    """Mirror of ``struct nmpc_mmp_block3_args`` (device pointers): one residual block of the network's layer3, ``x`` [M, Cin, H, W]
    -> ``out`` [M, 64, H2, W2]; the fields of ``NmpcMmpBlock2Args``; ``wd = None`` for the block without a projection (``Cin == 64``,
    stride 1)."""
    _fields_ = NmpcMmpBlock2Args._fields_


class NmpcMmpBlock3F16Args(C.Structure):
    """Mirror of ``struct nmpc_mmp_block3_f16_args`` (device pointers): the fields of ``NmpcMmpBlock3Args``, with ``w1``, ``w2`` and
    ``wd`` the packed binary16 fragments of ``mmp_stem.pack_block3_f16`` (aligned to 16 bytes)."""
    _fields_ = NmpcMmpBlock3Args._fields_


class NmpcMmpBlock4Args(C.Structure):
    """Mirror of ``struct nmpc_mmp_block4_args`` (device pointers): one residual block of the network's layer4, ``x`` [M, Cin, H, W]
    -> ``out`` [M, 128, H2, W2]; the fields of ``NmpcMmpBlock3Args``; ``wd = None`` for the block without a projection (``Cin == 128``,
    stride 1)."""
    _fields_ = NmpcMmpBlock3Args._fields_


class NmpcMmpBlock4F16Args(C.Structure):
    """Mirror of ``struct nmpc_mmp_block4_f16_args`` (device pointers): the fields of ``NmpcMmpBlock4Args``, with ``w1``, ``w2`` and
    ``wd`` the packed binary16 fragments of ``mmp_stem.pack_block4_f16`` (aligned to 16 bytes)."""
    _fields_ = NmpcMmpBlock4Args._fields_


class NmpcMmpHeadArgs(C.Structure):
    """Mirror of ``struct nmpc_mmp_head_args`` (device pointers): the network's end, ``x`` [M, C, H, W] -> ``out`` [M, O] through the
    2 x 2 average pool, ``w1`` [128, F], ``c1`` [128], the slope, ``w2`` [O, 128] and ``c2`` [O]."""
    _fields_ = [("M", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("O", C.c_int32),
                ("x", C.c_void_p), ("w1", C.c_void_p), ("c1", C.c_void_p), ("w2", C.c_void_p), ("c2", C.c_void_p),
                ("slope", C.c_float), ("out", C.c_void_p)]

MMP_HEAD_ROWS = 16                  # rows of the batch per workgroup of nmpc_mmp_head_f32 (kHeadRows, csrc/nmpc_mmp_head.h)

# every symbol include/nmpc_hip.h declares (checked by the CPU test-suite against the built library)
EXPORTED_SYMBOLS = (
    "nmpc_default_config", "nmpc_layout", "nmpc_create", "nmpc_destroy", "nmpc_param_len", "nmpc_set_stream", "nmpc_use_own_stream", "nmpc_set_pointer_mode",
    "nmpc_set_dispatch_order",
    "nmpc_solve_batch_f32", "nmpc_solve_batch_f64", "nmpc_solve_trace_f64", "nmpc_eval_batch_f32", "nmpc_eval_batch_f64",
    "nmpc_assemble_params_f32", "nmpc_assemble_params_f64",
    "nmpc_hypotheses_to_ellipses_f32", "nmpc_hypotheses_to_ellipses_f64",
    "nmpc_hypotheses_to_ellipses_counts_f32", "nmpc_hypotheses_to_ellipses_counts_f64",
    "nmpc_set_map", "nmpc_snap_hypotheses_f32", "nmpc_snap_hypotheses_f64",
    "nmpc_loop_pre_f32", "nmpc_loop_pre_f64", "nmpc_loop_post_f32", "nmpc_loop_post_f64",
    "nmpc_kf_predict_f32", "nmpc_kf_predict_f64", "nmpc_dwa_step_f32", "nmpc_dwa_step_f64",
    "nmpc_dwa_step_lists_f32", "nmpc_dwa_step_lists_f64",
    "nmpc_fleet_exchange_f32", "nmpc_fleet_exchange_f64", "nmpc_fleet_post_f32", "nmpc_fleet_post_f64",
    "nmpc_mmp_input_f32", "nmpc_mmp_input_f64", "nmpc_mmp_stem_f32", "nmpc_mmp_stem_f64", "nmpc_mmp_stem_shape", "nmpc_mmp_block_f32",
    "nmpc_mmp_block2_f32", "nmpc_mmp_block2_f16", "nmpc_mmp_block3_f32", "nmpc_mmp_block3_f16", "nmpc_mmp_block4_f32", "nmpc_mmp_block4_f16", "nmpc_mmp_head_f32",
    "nmpc_mmp_block2_f16_io", "nmpc_mmp_block3_f16_io", "nmpc_mmp_block4_f16_io", "nmpc_mmp_block_f16", "nmpc_mmp_block_f16_io",
    "nmpc_mmp_stem_io_f32", "nmpc_mmp_stem_io_f64",
    "nmpc_last_kernel_ms", "nmpc_last_launch_info", "nmpc_kernel_info", "nmpc_selftest", "nmpc_probe_f32", "nmpc_probe_f64",
    "nmpc_last_error",
)

# nmpc_probe_*: op name -> (number = ``nmpc_probe_op`` of include/nmpc_hip.h, the functions of csrc/wave_ops.h /
# csrc/nmpc_device.h the op runs, operands read from ``in``, rows of ``out`` it produces, float only). The CPU suite checks
# that every ``__device__`` function of wave_ops.h (but dpp_mov and the ref_* loops) is run by some op.
PROBE_OPS = {
    "wave_sum": (0, ("wave_sum", "read_lane"), 1, 1, False),
    "wave_sum2": (1, ("wave_sum2",), 2, 2, False),
    "wave_sum3": (2, ("wave_sum3",), 3, 3, False),
    "wave_scan_incl": (3, ("wave_scan_incl",), 1, 1, False),
    "wave_scan_incl2": (4, ("wave_scan_incl2",), 2, 2, False),
    "wave_scan_suffix_incl": (5, ("wave_scan_suffix_incl", "wave_suffix_fix_rows"), 1, 1, False),
    "wave_scan_suffix_incl2": (6, ("wave_scan_suffix_incl2", "wave_suffix_fix_rows"), 2, 2, False),
    "wave_suffix_fix_rows": (7, ("wave_suffix_fix_rows",), 1, 1, False),
    "class3_sum2": (8, ("class3_sum2", "class3_addresses", "bperm"), 2, 2, False),
    "class3_sum1": (9, ("class3_sum1", "class3_addresses", "bperm"), 1, 1, False),
    "class3_issue1_finish1": (10, ("class3_issue1", "class3_finish1", "class3_addresses", "bperm"), 1, 1, False),
    "class3_addresses": (11, ("class3_addresses",), 0, 4, False),
    "wave_reverse": (12, ("wave_reverse",), 1, 1, False),
    "read_lane": (13, ("read_lane",), 1, 6, False),
    "bperm": (14, ("bperm",), 2, 1, False),
    "wave_shift_up_1": (15, ("wave_shift_up",), 1, 1, False),
    "wave_shift_up_3": (16, ("wave_shift_up",), 1, 1, False),
    "wave_shift_down_1": (17, ("wave_shift_down",), 1, 1, False),
    "wave_shift_down_2": (18, ("wave_shift_down",), 1, 1, False),
    "wave_shift_down_3": (19, ("wave_shift_down",), 1, 1, False),
    "rollout_prefix": (20, ("wave_scan_incl", "wave_shift_up"), 1, 2, False),
    "adjoint_suffix": (21, ("wave_shift_up", "wave_scan_suffix_incl2", "wave_scan_suffix_incl", "wave_shift_down"), 2, 4, False),
    "class_sums_by_wave_sum3": (22, ("wave_sum3",), 1, 3, False),
    "sincos_medium": (23, ("sincos_medium",), 1, 4, True),
    "sincos_small": (24, ("sincos_small",), 1, 4, True),
    "fast_rcp": (25, ("fast_rcp",), 1, 2, False),
    "ls_point": (26, ("ls_point",), 4, 1, False),
    "wave_scan_suffix_incl_masked": (27, ("wave_scan_suffix_incl_masked", "wave_suffix_fix_rows_masked"), 1, 1, True),
    "wave_scan_suffix_incl2_masked": (28, ("wave_scan_suffix_incl2_masked",), 2, 2, True),
    "wave_suffix_fix_rows_masked": (29, ("wave_suffix_fix_rows_masked",), 1, 1, True),
}

_lib: Optional[C.CDLL] = None


def library_path() -> str:
    return _build.LIB_PATH


def load_library(build_if_missing: bool = True) -> C.CDLL:
    """dlopen the in-tree ``libnmpc_hip.so`` (building it with hipcc first if it is missing)."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64/libhsa-runtime64. If this library
    # pulled in /opt/rocm's copies first, a later `import torch` would find "No HIP GPUs". Loading torch first
    # makes the dynamic linker resolve our NEEDED libamdhip64.so.* to the copy that is already mapped.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    path = library_path()
    if not os.path.exists(path):
        if not build_if_missing:
            raise FileNotFoundError(f"{path} not built; run dyobav-mpcnwta-warehouse_amd/build.py")
        _build.build()
    lib = C.CDLL(path)
    vp, i32 = C.c_void_p, C.c_int32
    lib.nmpc_last_error.restype = C.c_char_p
    lib.nmpc_last_error.argtypes = []
    lib.nmpc_default_config.argtypes = [C.POINTER(NmpcConfigStruct)]
    lib.nmpc_layout.argtypes = [C.POINTER(NmpcConfigStruct), C.POINTER(NmpcLayoutInfo)]
    lib.nmpc_create.argtypes = [C.POINTER(NmpcConfigStruct), C.POINTER(vp)]
    lib.nmpc_destroy.argtypes = [vp]
    lib.nmpc_param_len.argtypes = [vp]
    lib.nmpc_set_stream.argtypes = [vp, vp]
    lib.nmpc_use_own_stream.argtypes = [vp]
    lib.nmpc_set_pointer_mode.argtypes = [vp, i32]
    lib.nmpc_set_dispatch_order.argtypes = [vp, vp, i32]
    lib.nmpc_set_map.argtypes = [vp, vp, vp, i32, i32]
    for sfx in ("f32", "f64"):
        getattr(lib, "nmpc_solve_batch_" + sfx).argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, i32]
        getattr(lib, "nmpc_eval_batch_" + sfx).argtypes = [vp, vp, vp, vp, vp, i32, vp, vp, vp]
        getattr(lib, "nmpc_assemble_params_" + sfx).argtypes = [vp, C.POINTER(NmpcAssembleArgs), i32, vp]
        getattr(lib, "nmpc_hypotheses_to_ellipses_" + sfx).argtypes = [vp, vp, i32, vp, i32, C.c_double, C.c_double,
                                                                       C.c_double, C.c_double, i32, vp, vp]
        getattr(lib, "nmpc_hypotheses_to_ellipses_counts_" + sfx).argtypes = [vp, vp, i32, vp, i32, C.c_double, C.c_double,
                                                                              C.c_double, C.c_double, i32, vp, vp, vp]
        getattr(lib, "nmpc_snap_hypotheses_" + sfx).argtypes = [vp, vp, C.POINTER(NmpcSnapArgs), i32, vp]
        getattr(lib, "nmpc_loop_pre_" + sfx).argtypes = [vp, C.POINTER(NmpcLoopArgs)]
        getattr(lib, "nmpc_loop_post_" + sfx).argtypes = [vp, C.POINTER(NmpcLoopArgs)]
        getattr(lib, "nmpc_kf_predict_" + sfx).argtypes = [vp, C.POINTER(NmpcKfArgs)]
        getattr(lib, "nmpc_dwa_step_" + sfx).argtypes = [vp, C.POINTER(NmpcDwaArgs)]
        getattr(lib, "nmpc_dwa_step_lists_" + sfx).argtypes = [vp, C.POINTER(NmpcDwaListsArgs)]
        getattr(lib, "nmpc_fleet_exchange_" + sfx).argtypes = [vp, C.POINTER(NmpcFleetArgs)]
        getattr(lib, "nmpc_fleet_post_" + sfx).argtypes = [vp, C.POINTER(NmpcFleetArgs)]
        getattr(lib, "nmpc_mmp_input_" + sfx).argtypes = [vp, C.POINTER(NmpcMmpArgs)]
        getattr(lib, "nmpc_mmp_stem_" + sfx).argtypes = [vp, C.POINTER(NmpcMmpStemArgs)]
        getattr(lib, "nmpc_mmp_stem_io_" + sfx).argtypes = [vp, C.POINTER(NmpcMmpStemArgs), i32]
    lib.nmpc_mmp_stem_shape.argtypes = [i32, i32, C.POINTER(i32), C.POINTER(i32)]
    lib.nmpc_mmp_block_f32.argtypes = [vp, C.POINTER(NmpcMmpBlockArgs)]
    lib.nmpc_mmp_block2_f32.argtypes = [vp, C.POINTER(NmpcMmpBlock2Args)]
    lib.nmpc_mmp_block2_f16.argtypes = [vp, C.POINTER(NmpcMmpBlock2F16Args)]
    lib.nmpc_mmp_block3_f32.argtypes = [vp, C.POINTER(NmpcMmpBlock3Args)]
    lib.nmpc_mmp_block3_f16.argtypes = [vp, C.POINTER(NmpcMmpBlock3F16Args)]
    lib.nmpc_mmp_block4_f32.argtypes = [vp, C.POINTER(NmpcMmpBlock4Args)]
    lib.nmpc_mmp_block4_f16.argtypes = [vp, C.POINTER(NmpcMmpBlock4F16Args)]
    lib.nmpc_mmp_block_f16.argtypes = [vp, C.POINTER(NmpcMmpBlockF16Args)]
    lib.nmpc_mmp_block_f16_io.argtypes = [vp, C.POINTER(NmpcMmpBlockF16Args), i32, i32]
    lib.nmpc_mmp_block2_f16_io.argtypes = [vp, C.POINTER(NmpcMmpBlock2F16Args), i32, i32]
    lib.nmpc_mmp_block3_f16_io.argtypes = [vp, C.POINTER(NmpcMmpBlock3F16Args), i32, i32]
    lib.nmpc_mmp_block4_f16_io.argtypes = [vp, C.POINTER(NmpcMmpBlock4F16Args), i32, i32]
    lib.nmpc_mmp_head_f32.argtypes = [vp, C.POINTER(NmpcMmpHeadArgs)]
    lib.nmpc_solve_trace_f64.argtypes = [vp, vp, vp, vp, C.c_double, vp, vp, vp, vp, vp, vp, i32, C.POINTER(i32)]
    lib.nmpc_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
    lib.nmpc_kernel_info.argtypes = [vp] + [C.POINTER(i32)] * 5
    lib.nmpc_last_launch_info.argtypes = [vp, C.POINTER(i32 * 8)]
    lib.nmpc_selftest.argtypes = [vp]
    lib.nmpc_probe_f32.argtypes = lib.nmpc_probe_f64.argtypes = [vp, i32, i32, i32, vp, vp]
    for name in EXPORTED_SYMBOLS:
        if name != "nmpc_last_error":
            getattr(lib, name).restype = C.c_int
    _lib = lib
    return lib


def _check(rc: int) -> int:
    if rc < 0:
        raise NmpcError(rc, load_library().nmpc_last_error().decode(errors="replace"))
    return rc


def default_config_struct() -> NmpcConfigStruct:
    cfg = NmpcConfigStruct()
    _check(load_library().nmpc_default_config(C.byref(cfg)))
    return cfg


def mmp_stem_shape(Hm: int, Wm: int):
    """``nmpc_mmp_stem_shape``: ``(Hp, Wp)`` of the fused first layer's output for an ``Hm x Wm`` map (no device needed)."""
    hp, wp = C.c_int32(), C.c_int32()
    _check(load_library().nmpc_mmp_stem_shape(int(Hm), int(Wm), C.byref(hp), C.byref(wp)))
    return hp.value, wp.value


def layout_info(cfg: NmpcConfigStruct) -> NmpcLayoutInfo:
    """``nmpc_layout``: the dimension bookkeeping of a configuration (no device needed)."""
    out = NmpcLayoutInfo()
    _check(load_library().nmpc_layout(C.byref(cfg), C.byref(out)))
    return out


def _suffix(dtype) -> str:
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return "f32"
    if dtype == np.float64:
        return "f64"
    raise TypeError(f"unsupported dtype {dtype}; the kernels compute in float32 or float64")


class _Arg:
    """A host numpy array or a raw device pointer (``int``) to hand to the C ABI."""

    @staticmethod
    def ptr(x) -> Optional[int]:
        if x is None:
            return None
        if isinstance(x, np.ndarray):
            assert x.flags.c_contiguous
            return x.ctypes.data
        if isinstance(x, int):
            return x
        if hasattr(x, "data_ptr"):   # torch tensor (host or device); must be contiguous
            assert x.is_contiguous()
            return x.data_ptr()
        raise TypeError(type(x))


class Handle:
    """RAII wrapper of ``nmpc_handle``: one HIP device + stream + workspace."""

    def __init__(self, cfg: NmpcConfigStruct):
        self._lib = load_library()
        self._h = C.c_void_p()
        self.cfg = cfg
        _check(self._lib.nmpc_create(C.byref(cfg), C.byref(self._h)))
        self.np_ = _check(self._lib.nmpc_param_len(self._h))
        self.n = 2 * cfg.N_hor

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.nmpc_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ------------------------------------------------------------------------------------------------
    def set_stream(self, stream_ptr: Optional[int]):
        """``stream_ptr``: a ``hipStream_t`` as an int (0 = the null stream = torch's default stream); ``None`` = the
        handle's own non-blocking stream."""
        if stream_ptr is None:
            _check(self._lib.nmpc_use_own_stream(self._h))
        else:
            _check(self._lib.nmpc_set_stream(self._h, C.c_void_p(int(stream_ptr))))

    def set_pointer_mode(self, mode: int):
        """0 = classify every array argument per call (default), 1 = all host pointers, 2 = all device pointers."""
        _check(self._lib.nmpc_set_pointer_mode(self._h, int(mode)))

    def set_dispatch_order(self, order=None):
        """Workgroup b of the following solves of ``len(order)`` instances takes instance ``order[b]`` (a permutation:
        numpy int32 array, or an int32 device tensor on the handle's stream; e.g. ``np.argsort(-previous_evals)`` =
        longest first). The library copies it: a host array before the call returns, a device tensor asynchronously on
        the handle's stream -- so a tensor produced on another stream must be kept alive (and that stream synchronised)
        by the caller; with ``set_stream(torch's current stream)`` the copy is ordered like any other torch operation.
        ``None`` clears it."""
        if order is None:
            _check(self._lib.nmpc_set_dispatch_order(self._h, None, 0))
        elif isinstance(order, np.ndarray) or not hasattr(order, "data_ptr"):
            a = np.ascontiguousarray(order, dtype=np.int32)
            _check(self._lib.nmpc_set_dispatch_order(self._h, C.c_void_p(a.ctypes.data), int(a.size)))
        else:
            assert str(order.dtype) == "torch.int32" and order.is_contiguous()
            _check(self._lib.nmpc_set_dispatch_order(self._h, C.c_void_p(order.data_ptr()), int(order.numel())))

    def selftest(self) -> int:
        return _check(self._lib.nmpc_selftest(self._h))

    def probe_raw(self, dtype, op: int, block_threads: int, n_waves: int, x, out):
        """Thin call of ``nmpc_probe_*``: ``x`` [n_waves, 4, 64] and ``out`` [n_waves, 6, 64] may be numpy, torch or raw pointers."""
        fn = getattr(self._lib, "nmpc_probe_" + _suffix(dtype))
        _check(fn(self._h, int(op), int(block_threads), int(n_waves), _Arg.ptr(x), _Arg.ptr(out)))

    def probe(self, op: str, x, dtype, block_threads: int = 64):
        """``nmpc_probe_*``: one wavefront primitive or scalar function of the product headers (``PROBE_OPS``) run by itself.
        ``x``: one array [n_waves, 64] per operand of the op (a single array for a one-operand op). Returns the op's output
        rows as numpy arrays [n_waves, 64] (a single array if it has one)."""
        num, _, n_in, n_out, _ = PROBE_OPS[op]
        dtype = np.dtype(dtype)
        xs = [x] if isinstance(x, np.ndarray) else list(x)
        assert len(xs) == n_in or (n_in == 0 and len(xs) == 1), (op, len(xs))
        n_waves = xs[0].shape[0]
        buf = np.zeros((n_waves, 4, 64), dtype)
        for i, a in enumerate(xs[:n_in]):
            assert a.shape == (n_waves, 64), a.shape
            buf[:, i, :] = a
        out = np.full((n_waves, 6, 64), np.nan, dtype)
        self.probe_raw(dtype, num, block_threads, n_waves, buf, out)
        rows = [np.ascontiguousarray(out[:, i, :]) for i in range(n_out)]
        return rows[0] if n_out == 1 else rows

    def last_kernel_ms(self) -> float:
        ms = C.c_float()
        _check(self._lib.nmpc_last_kernel_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def last_launch_info(self) -> dict:
        """Which kernel family / variant the last solve or eval call launched (``nmpc_last_launch_info``). ``order_source``:
        0 index order, 1 the caller's (``set_dispatch_order``), 2 one evaluation, 3 a pilot launch."""
        v = (C.c_int32 * 8)()
        _check(self._lib.nmpc_last_launch_info(self._h, C.byref(v)))
        return {"family": ("throughput", "latency", "cooperative")[v[0]], "axis_aligned": int(v[1]),
                "staged_outer_iterations": int(v[2]), "polish_selected": int(v[3]), "tail_handed_off": int(v[4]),
                "deep_parked": int(v[5]), "order_source": int(v[6])}

    def kernel_info(self) -> dict:
        v = [C.c_int32() for _ in range(5)]
        _check(self._lib.nmpc_kernel_info(self._h, *[C.byref(x) for x in v]))
        keys = ("lds_bytes_f32", "lds_bytes_f64", "lanes_per_step", "waves_per_cu_f32", "waves_per_cu_f64")
        return dict(zip(keys, (int(x.value) for x in v)))

    def solve_raw(self, dtype, P, B, U, cost=None, status=None, iters=None, u0=None, y=None, y_is_input=False,
                  c0=None, info=None, sync=True):
        """Thin call of ``nmpc_solve_batch_*``; every array argument may be numpy, torch or a raw pointer."""
        fn = getattr(self._lib, "nmpc_solve_batch_" + _suffix(dtype))
        p = _Arg.ptr
        _check(fn(self._h, p(P), int(B), p(U), p(cost), p(status), p(iters), p(u0), p(y), int(bool(y_is_input)),
                  p(c0), p(info), int(bool(sync))))

    def assemble_params(self, dtype, B, P_out, last_u, state, ref_states, speed_ref, tuning, stc_weights, dyn_weights,
                        map_polygons=None, dyn_obstacles=None, other_robots=None, selected=None):
        """``nmpc_assemble_params_*``: device tensors in (torch / raw pointers), ``P_out[B, np]`` written on the
        handle's stream. ``map_polygons`` [M,4,2]; ``dyn_obstacles`` [B,n_dyn,N+1,6]."""
        a = NmpcAssembleArgs()
        p = _Arg.ptr
        a.last_u, a.state, a.ref_states, a.speed_ref = p(last_u), p(state), p(ref_states), p(speed_ref)
        a.tuning, a.stc_weights, a.dyn_weights = p(tuning), p(stc_weights), p(dyn_weights)
        a.other_robots = p(other_robots)
        a.map_polygons = p(map_polygons)
        a.n_map_polygons = 0 if map_polygons is None else int(map_polygons.shape[0])
        a.dyn_obstacles = p(dyn_obstacles)
        a.n_dyn = 0 if dyn_obstacles is None else int(dyn_obstacles.shape[1])
        a.selected = p(selected)
        fn = getattr(self._lib, "nmpc_assemble_params_" + _suffix(dtype))
        _check(fn(self._h, C.byref(a), int(B), p(P_out)))

    def loop_step(self, dtype, args: "NmpcLoopArgs", post: bool):
        """``nmpc_loop_pre_*`` / ``nmpc_loop_post_*``: one half of a closed-loop time step (row f3), enqueued on the
        handle's stream."""
        fn = getattr(self._lib, ("nmpc_loop_post_" if post else "nmpc_loop_pre_") + _suffix(dtype))
        _check(fn(self._h, C.byref(args)))

    def kf_predict(self, dtype, args: "NmpcKfArgs"):
        """``nmpc_kf_predict_*``: the Kalman-filter pedestrian predictor for the running scenarios (append the new position,
        filter the stored trajectories with the carried covariance, write the obstacle rows), enqueued on the handle's
        stream."""
        fn = getattr(self._lib, "nmpc_kf_predict_" + _suffix(dtype))
        _check(fn(self._h, C.byref(args)))

    def dwa_step(self, dtype, args: "NmpcDwaArgs"):
        """``nmpc_dwa_step_*``: the dynamic-window tracker for the running scenarios (window, grid, rollouts, costs, ordered
        arg-min; ``U_c`` = the chosen control repeated ``N_hor`` times), one launch enqueued on the handle's stream."""
        fn = getattr(self._lib, "nmpc_dwa_step_" + _suffix(dtype))
        _check(fn(self._h, C.byref(args) if args is not None else None))

    def dwa_step_lists(self, dtype, args: "NmpcDwaListsArgs"):
        """``nmpc_dwa_step_lists_*``: the dynamic-window tracker over per-offset lists -- ``dyn_c[n_run, R, N+1, 6]`` with
        ``dyn_count[n_run, N+1]`` (int32), as ``hypotheses_to_ellipses(..., counts=)`` writes them; everything else as ``dwa_step``
        with ``dyn_mode`` 2. One launch enqueued on the handle's stream."""
        fn = getattr(self._lib, "nmpc_dwa_step_lists_" + _suffix(dtype))
        _check(fn(self._h, C.byref(args) if args is not None else None))

    def fleet_exchange(self, dtype, args: "NmpcFleetArgs"):
        """``nmpc_fleet_exchange_*``: the other-robot blocks ``other_c[n_run, 3 (N + 1) Nother]`` of the running robots from their
        group's peers (current states, previous solutions rolled out; nearest ``Nother - 1``, slot 0 zero), one launch enqueued on
        the handle's stream. The block is what ``assemble_params(..., other_robots=)`` takes."""
        fn = getattr(self._lib, "nmpc_fleet_exchange_" + _suffix(dtype))
        _check(fn(self._h, C.byref(args) if args is not None else None))

    def fleet_post(self, dtype, args: "NmpcFleetArgs"):
        """``nmpc_fleet_post_*``: robot-robot clearance and collision of the robots that ran this step, after ``loop_step(post=True)``
        on the same run list; one launch enqueued on the handle's stream."""
        fn = getattr(self._lib, "nmpc_fleet_post_" + _suffix(dtype))
        _check(fn(self._h, C.byref(args) if args is not None else None))

    def mmp_input(self, dtype, args: "NmpcMmpArgs"):
        """``nmpc_mmp_input_*``: the float32 input stack ``out[n_item, n_off, 7, Hm, Wm]`` of the multi-hypothesis predictor's
        network from the pedestrians' ``hist`` / ``hcount`` rows (``dtype``: the element type of ``hist``), one launch enqueued
        on the handle's stream."""
        fn = getattr(self._lib, "nmpc_mmp_input_" + _suffix(dtype))
        _check(fn(self._h, C.byref(args) if args is not None else None))

    def mmp_stem(self, dtype, args: "NmpcMmpStemArgs"):
        """``nmpc_mmp_stem_*``: the pooled output ``out[n_item, n_off, C, Hp, Wp]`` of the network's first layer (convolution,
        folded norm, LeakyReLU, max-pool) straight from the pedestrians' ``hist`` / ``hcount`` rows, the input stack never
        written (``dtype``: the element type of ``hist``), one launch enqueued on the handle's stream."""
        fn = getattr(self._lib, "nmpc_mmp_stem_" + _suffix(dtype))
        _check(fn(self._h, C.byref(args) if args is not None else None))

    def mmp_stem_io(self, dtype, args: "NmpcMmpStemArgs", out_f16: int):
        """``nmpc_mmp_stem_io_*``: ``mmp_stem`` with the form of ``out`` in memory beside the struct. ``out_f16 = 0``: ``mmp_stem``
        itself; ``1``: ``out`` is binary16 in the octet form of the blocks' activations, ``[n_item * n_off][C / 8][Hp][Wp][8]``
        (include/nmpc_hip.h; ``mmp_stem.pack_activations_f16``), aligned to 16 bytes."""
        fn = getattr(self._lib, "nmpc_mmp_stem_io_" + _suffix(dtype))
        _check(fn(self._h, C.byref(args) if args is not None else None, out_f16))

    def mmp_block(self, args: "NmpcMmpBlockArgs"):
        """``nmpc_mmp_block_f32``: one fused residual block of the network's layer1 (two 3 x 3 convolutions with their folded
        norms, the identity or its 1 x 1 projection, both activations), ``out[M, 16, H, W]`` from ``x[M, Cin, H, W]``, float32 under
        both dtypes, one launch enqueued on the handle's stream."""
        _check(self._lib.nmpc_mmp_block_f32(self._h, C.byref(args) if args is not None else None))

    def mmp_block2(self, args: "NmpcMmpBlock2Args"):
        """``nmpc_mmp_block2_f32``: one fused residual block of the network's layer2 (as ``mmp_block``, at 32 output channels and
        with ``args.stride`` = 1 or 2 on the first convolution and the projection), ``out[M, 32, H2, W2]`` from ``x[M, Cin, H, W]``,
        float32 under both dtypes, one launch enqueued on the handle's stream."""
        _check(self._lib.nmpc_mmp_block2_f32(self._h, C.byref(args) if args is not None else None))

    def mmp_block3(self, args: "NmpcMmpBlock3Args"):
        """``nmpc_mmp_block3_f32``: one fused residual block of the network's layer3 (as ``mmp_block2``, at 64 output channels),
        ``out[M, 64, H2, W2]`` from ``x[M, Cin, H, W]``, float32 under both dtypes, one launch enqueued on the handle's stream."""
        _check(self._lib.nmpc_mmp_block3_f32(self._h, C.byref(args) if args is not None else None))

    def mmp_block_f16(self, args: "NmpcMmpBlockF16Args"):
        """``nmpc_mmp_block_f16``: the block of ``mmp_block`` (layer1) with binary16 MFMA operands and float32 accumulation (the rounding
        rule: include/nmpc_hip.h), on the packed weights of ``mmp_stem.pack_block1_f16``; ``x`` and ``out`` stay float32."""
        _check(self._lib.nmpc_mmp_block_f16(self._h, C.byref(args) if args is not None else None))

    def mmp_block_f16_io(self, args: "NmpcMmpBlockF16Args", x_f16: int, out_f16: int):
        """``nmpc_mmp_block_f16_io``: as ``mmp_block2_f16_io``, for ``mmp_block_f16``."""
        _check(self._lib.nmpc_mmp_block_f16_io(self._h, C.byref(args) if args is not None else None, x_f16, out_f16))

    def mmp_block2_f16(self, args: "NmpcMmpBlock2F16Args"):
        """``nmpc_mmp_block2_f16``: the block of ``mmp_block2`` with binary16 MFMA operands and float32 accumulation (the rounding
        rule: include/nmpc_hip.h), on the packed weights of ``mmp_stem.pack_block2_f16``; ``x`` and ``out`` stay float32."""
        _check(self._lib.nmpc_mmp_block2_f16(self._h, C.byref(args) if args is not None else None))

    def mmp_block3_f16(self, args: "NmpcMmpBlock3F16Args"):
        """``nmpc_mmp_block3_f16``: the block of ``mmp_block3`` with binary16 MFMA operands and float32 accumulation (the rounding
        rule: include/nmpc_hip.h), on the packed weights of ``mmp_stem.pack_block3_f16``; ``x`` and ``out`` stay float32."""
        _check(self._lib.nmpc_mmp_block3_f16(self._h, C.byref(args) if args is not None else None))

    def mmp_block4_f16(self, args: "NmpcMmpBlock4F16Args"):
        """``nmpc_mmp_block4_f16``: the block of ``mmp_block4`` with binary16 MFMA operands and float32 accumulation (the rounding
        rule: include/nmpc_hip.h), on the packed weights of ``mmp_stem.pack_block4_f16``; ``x`` and ``out`` stay float32."""
        _check(self._lib.nmpc_mmp_block4_f16(self._h, C.byref(args) if args is not None else None))

    def mmp_block2_f16_io(self, args: "NmpcMmpBlock2F16Args", x_f16: int, out_f16: int):
        """``nmpc_mmp_block2_f16_io``: ``mmp_block2_f16`` with ``args.x`` (``x_f16 = 1``) and / or ``args.out`` (``out_f16 = 1``) in the
        octet form of binary16 activations, ``[M][C / 8][H][W][8]`` (include/nmpc_hip.h; ``mmp_stem.pack_activations_f16``), aligned to
        16 bytes; ``(0, 0)`` is ``mmp_block2_f16``."""
        _check(self._lib.nmpc_mmp_block2_f16_io(self._h, C.byref(args) if args is not None else None, x_f16, out_f16))

    def mmp_block3_f16_io(self, args: "NmpcMmpBlock3F16Args", x_f16: int, out_f16: int):
        """``nmpc_mmp_block3_f16_io``: as ``mmp_block2_f16_io``, for ``mmp_block3_f16``."""
        _check(self._lib.nmpc_mmp_block3_f16_io(self._h, C.byref(args) if args is not None else None, x_f16, out_f16))

    def mmp_block4_f16_io(self, args: "NmpcMmpBlock4F16Args", x_f16: int, out_f16: int):
        """``nmpc_mmp_block4_f16_io``: as ``mmp_block2_f16_io``, for ``mmp_block4_f16``."""
        _check(self._lib.nmpc_mmp_block4_f16_io(self._h, C.byref(args) if args is not None else None, x_f16, out_f16))

    def mmp_block4(self, args: "NmpcMmpBlock4Args"):
        """``nmpc_mmp_block4_f32``: one fused residual block of the network's layer4 (as ``mmp_block3``, at 128 output channels),
        ``out[M, 128, H2, W2]`` from ``x[M, Cin, H, W]``, float32 under both dtypes, one launch enqueued on the handle's stream."""
        _check(self._lib.nmpc_mmp_block4_f32(self._h, C.byref(args) if args is not None else None))

    def mmp_head(self, args: "NmpcMmpHeadArgs"):
        """``nmpc_mmp_head_f32``: the network's end -- 2 x 2 average pool, flatten, ``Linear(F, 128)``, the slope, ``Linear(128, O)`` --
        ``out[M, O]`` from ``x[M, C, H, W]``, float32 under both dtypes, one launch enqueued on the handle's stream."""
        _check(self._lib.nmpc_mmp_head_f32(self._h, C.byref(args) if args is not None else None))

    def hypotheses_to_ellipses(self, dtype, hypos, cur, dyn_out, n_obs_out=None, human_size=0.2, eps=1.0, enlarge=2.0,
                               extra_margin=0.0, counts=None):
        """``nmpc_hypotheses_to_ellipses_*``: device tensors ``hypos[B,N,P,2]``, ``cur[B,H,2]`` ->
        ``dyn_out[B,Ndynobs,N+1,6]`` (+ ``n_obs_out[B]`` int32). ``counts``: an int32 device tensor ``[B,N+1]`` for the rows per
        offset that are clusters (``nmpc_hypotheses_to_ellipses_counts_*``; ``dyn_out`` and ``n_obs_out`` are the same bits)."""
        B, P, H = int(hypos.shape[0]), int(hypos.shape[2]), int(cur.shape[1])
        p = _Arg.ptr
        args = (self._h, p(hypos), P, p(cur), H, float(human_size), float(eps), float(enlarge), float(extra_margin), B, p(dyn_out),
                p(n_obs_out))
        if counts is None:
            _check(getattr(self._lib, "nmpc_hypotheses_to_ellipses_" + _suffix(dtype))(*args))
        else:
            _check(getattr(self._lib, "nmpc_hypotheses_to_ellipses_counts_" + _suffix(dtype))(*args, p(counts)))

    def set_map(self, occupied, edge=None):
        """``nmpc_set_map``: host arrays ``occupied[H, W]`` (non-zero = occupied; for the reference: ``255 - label > 0``)
        and ``edge[H, W]``; ``edge=None`` computes it with :func:`.snap.edge_map` from ``occupied`` (pass the grey-level
        occupancy itself then if it has more than one level: the edges between levels count). ``occupied=None`` clears
        the map."""
        if occupied is None:
            _check(self._lib.nmpc_set_map(self._h, None, None, 0, 0))
            return
        occ = np.asarray(occupied)
        if occ.ndim != 2:
            raise ValueError(f"occupied must be [H, W], got {occ.shape}")
        if edge is None:
            from .snap import edge_map
            edge = edge_map(occ)
        edge = np.asarray(edge)
        if edge.shape != occ.shape:
            raise ValueError(f"edge {edge.shape} and occupied {occ.shape} differ in shape")
        occ8 = np.ascontiguousarray(occ != 0, dtype=np.uint8)
        edge8 = np.ascontiguousarray(edge != 0, dtype=np.uint8)
        _check(self._lib.nmpc_set_map(self._h, occ8.ctypes.data, edge8.ctypes.data, int(occ.shape[0]), int(occ.shape[1])))

    def snap_hypotheses(self, dtype, raw, out, n_ped, n_hyp, transform, rescale=1.0, n_snapped=None, n_outside=None):
        """``nmpc_snap_hypotheses_*``: device tensors ``raw[B, N_hor, n_ped * n_hyp, 2]`` (network pixel coordinates) ->
        ``out`` of the same shape (world coordinates, snapped points first in every segment; ``out`` may be ``raw``),
        enqueued on the handle's stream. ``transform``: a :class:`.snap.WorldTransform`. Optional int32 device outputs
        ``n_snapped[B, N_hor, n_ped]`` and ``n_outside[B]``."""
        B, N, P = int(raw.shape[0]), int(raw.shape[1]), int(raw.shape[2])
        if N != self.cfg.N_hor or P != int(n_ped) * int(n_hyp) or int(raw.shape[3]) != 2:
            raise ValueError(f"raw must be [B, {self.cfg.N_hor}, {int(n_ped) * int(n_hyp)}, 2], got {tuple(raw.shape)}")
        if tuple(out.shape) != tuple(raw.shape):
            raise ValueError(f"out {tuple(out.shape)} and raw {tuple(raw.shape)} differ in shape")
        a = set_world_transform(NmpcSnapArgs(), transform, rescale)
        a.n_ped, a.n_hyp = int(n_ped), int(n_hyp)
        p = _Arg.ptr
        a.n_snapped, a.n_outside = p(n_snapped), p(n_outside)
        fn = getattr(self._lib, "nmpc_snap_hypotheses_" + _suffix(dtype))
        _check(fn(self._h, p(raw), C.byref(a), B, p(out)))

    def solve(self, P: np.ndarray, u0=None, y0=None, c0=None, dtype=None, want_info=True) -> dict:
        """Solve a batch held in host memory; returns numpy arrays."""
        dtype = np.dtype(dtype or P.dtype)
        P = np.ascontiguousarray(P, dtype=dtype)
        if P.ndim != 2 or P.shape[1] != self.np_:
            raise ValueError(f"P must be [B, {self.np_}], got {P.shape}")
        B = P.shape[0]
        U = np.empty((B, self.n), dtype=dtype)
        cost = np.empty(B, dtype=dtype)
        status = np.empty(B, dtype=np.int32)
        iters = np.empty((B, 2), dtype=np.int32)
        y = np.zeros((B, self.n), dtype=dtype) if y0 is None else np.ascontiguousarray(y0, dtype=dtype).copy()
        u0 = None if u0 is None else np.ascontiguousarray(u0, dtype=dtype)
        c0 = None if c0 is None else np.ascontiguousarray(c0, dtype=dtype)
        info = np.empty((B, 8), dtype=dtype) if want_info else None
        self.solve_raw(dtype, P, B, U, cost, status, iters, u0, y, y0 is not None, c0, info, True)
        return dict(U=U, cost=cost, status=status, iters=iters, y=y, info=info)

    def solve_trace(self, p, u0=None, y0=None, c0=None, max_records=None) -> dict:
        """``nmpc_solve_trace_f64``: one instance through the one-wavefront fp64 kernel with its iteration trace --
        ``head[n_rec, 16]`` (fields as in ``include/nmpc_hip.h``) and ``Ut[n_rec, 2N]``, the iterate after each inner
        iteration. Diagnostic (first-divergence audit against the oracle's trace)."""
        p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1)
        if p.size != self.np_:
            raise ValueError(f"p must have {self.np_} entries, got {p.size}")
        n = self.n
        max_records = int(max_records or self.cfg.max_outer_iterations * (self.cfg.max_inner_iterations + 1))
        u0 = None if u0 is None else np.ascontiguousarray(u0, dtype=np.float64).reshape(n)
        y0 = None if y0 is None else np.ascontiguousarray(y0, dtype=np.float64).reshape(n)
        U, y = np.empty(n), np.empty(n)
        status, iters, info = np.empty(1, np.int32), np.empty(2, np.int32), np.empty(8)
        tr = np.zeros((max_records, 16 + n))
        nrec = C.c_int32(0)
        q = _Arg.ptr
        _check(self._lib.nmpc_solve_trace_f64(self._h, q(p), q(u0), q(y0), float(c0 or 0.0), q(U), q(y), q(status), q(iters),
                                              q(info), q(tr), max_records, C.byref(nrec)))
        tr = tr[:nrec.value]
        return dict(U=U, y=y, status=int(status[0]), iters=iters, info=info, head=tr[:, :16].copy(), Ut=tr[:, 16:].copy())

    def eval(self, P: np.ndarray, U: np.ndarray, Y: np.ndarray, Cpen: np.ndarray, grad=True, dtype=None) -> dict:
        dtype = np.dtype(dtype or P.dtype)
        P = np.ascontiguousarray(P, dtype=dtype)
        U = np.ascontiguousarray(U, dtype=dtype)
        Y = np.ascontiguousarray(Y, dtype=dtype)
        Cpen = np.ascontiguousarray(Cpen, dtype=dtype)
        B = P.shape[0]
        assert P.shape == (B, self.np_) and U.shape == (B, self.n) and Y.shape == (B, self.n) and Cpen.shape == (B,)
        psi = np.empty(B, dtype=dtype)
        g = np.empty((B, self.n), dtype=dtype) if grad else None
        f2 = np.empty(B, dtype=dtype)
        fn = getattr(self._lib, "nmpc_eval_batch_" + _suffix(dtype))
        p = _Arg.ptr
        _check(fn(self._h, p(P), p(U), p(Y), p(Cpen), B, p(psi), p(g), p(f2)))
        return dict(psi=psi, grad=g, f2sq=f2)
