"""yaml -> typed configuration objects, with the attribute names of the reference's ``src/configs.py``
(``Configurator`` :10-42, ``CircularRobotSpecification`` :86-103, ``MpcConfiguration`` :140-176) so that code
written against the reference (``TrajectoryTracker``, ``MpcInterface``) can consume them unchanged.
Only the two classes the solve path reads are provided.
"""
from __future__ import annotations

import yaml

ROBOT_KEYS = ("ts", "vehicle_width", "vehicle_margin", "social_margin", "lin_vel_min", "lin_vel_max",
              "lin_acc_min", "lin_acc_max", "ang_vel_max", "ang_acc_max")
MPC_KEYS = ("ts", "N_hor", "action_steps", "ns", "nu", "nq", "Nother", "nstcobs", "Nstcobs", "ndynobs", "Ndynobs",
            "max_solver_time", "build_directory", "build_type", "bad_exit_codes", "optimizer_name",
            "lin_vel_penalty", "lin_acc_penalty", "ang_vel_penalty", "ang_acc_penalty", "qrpd", "qpos", "qvel",
            "qtheta", "qpN", "qthetaN")


class Configurator:
    """Every top-level yaml key becomes an attribute (reference: configs.py:10-22)."""

    def __init__(self, yaml_fp: str, with_partition: bool = False) -> None:
        with open(yaml_fp, "r") as stream:
            if with_partition:
                data = {}
                for doc in yaml.safe_load_all(stream):
                    data.update(doc or {})
            else:
                data = yaml.safe_load(stream)
        self.yaml_path = yaml_fp
        for key, value in data.items():
            setattr(self, key, value)


class _Section:
    KEYS: tuple = ()

    def __init__(self, config: Configurator) -> None:
        self._config = config
        missing = [k for k in self.KEYS if not hasattr(config, k)]
        if missing:
            raise AttributeError(f"{getattr(config, 'yaml_path', 'config')}: missing keys {missing}")
        for k in self.KEYS:
            setattr(self, k, getattr(config, k))

    @classmethod
    def from_yaml(cls, yaml_fp: str, with_partition: bool = False):
        return cls(Configurator(yaml_fp, with_partition))


class CircularRobotSpecification(_Section):
    """ts, vehicle_width/margin, social_margin and the velocity / acceleration limits."""
    KEYS = ROBOT_KEYS


class MpcConfiguration(_Section):
    """Horizon, dimensions, weights and solver build options."""
    KEYS = MPC_KEYS


DWA_KEYS = ("ts", "N_hor", "ns", "nu", "vel_resolution", "ang_resolution", "stuck_threshold", "q_goal_dir",
            "q_ref_deviation", "q_speed", "q_stc_obstacle", "q_dyn_obstacle", "q_social")
DWA_ROBOT_KEYS = ("lin_vel_min", "lin_vel_max", "lin_acc_min", "lin_acc_max", "ang_vel_max", "ang_acc_max")
# the values of the reference's config/dwa_test.yaml (its "{Test}" resolutions; the commented "{Real}" pair is 0.05 / 0.04)
DWA_DEFAULTS = dict(ts=0.2, N_hor=20, ns=3, nu=2, vel_resolution=0.1, ang_resolution=0.1, stuck_threshold=0.001,
                    q_goal_dir=0.05, q_ref_deviation=0.1, q_speed=1.0, q_stc_obstacle=2.0, q_dyn_obstacle=2.0, q_social=0.1,
                    lin_vel_min=-0.5, lin_vel_max=1.5, lin_acc_min=-1.0, lin_acc_max=1.0, ang_vel_max=0.5, ang_acc_max=3.0)


class DwaConfiguration:
    """The dynamic-window tracker's settings (reference: configs.py:179-199) together with the kinematic limits the
    reference reads from the same yaml file through ``CircularRobotSpecification`` (dwa_interface.py:25-26). Without
    arguments: the values of the reference's ``dwa_test.yaml``; keyword arguments override single values."""

    def __init__(self, config: Configurator = None, **overrides) -> None:
        values = dict(DWA_DEFAULTS)
        if config is not None:
            missing = [k for k in DWA_KEYS + DWA_ROBOT_KEYS if not hasattr(config, k)]
            if missing:
                raise AttributeError(f"{getattr(config, 'yaml_path', 'config')}: missing keys {missing}")
            values.update({k: getattr(config, k) for k in DWA_KEYS + DWA_ROBOT_KEYS})
        unknown = [k for k in overrides if k not in values]
        if unknown:
            raise TypeError(f"unknown DWA settings {unknown}")
        values.update(overrides)
        self._config = config
        for k, v in values.items():
            setattr(self, k, v)

    @classmethod
    def from_yaml(cls, yaml_fp: str, with_partition: bool = False, **overrides):
        return cls(Configurator(yaml_fp, with_partition), **overrides)
