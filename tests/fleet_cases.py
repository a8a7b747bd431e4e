"""Inputs and device plumbing shared by the fleet kernel tests (tests/test_gpu_fleet_kernels.py, tests/test_gpu_fleet_read_bounds.py):
seeded groups of robots, the run lists, and single ``nmpc_fleet_exchange_*`` / ``nmpc_fleet_post_*`` calls through the C ABI."""
import numpy as np

TS = 0.2
WIDTH = 0.5         # nmpc_config.vehicle_width of the default configuration
COORD = 20.0        # robots live in [-COORD, COORD]^2: the coordinate scale of the tolerances
G = 3               # groups per case: a first, a middle and a last one

_handles = {}


def handle(N, Nother):
    """One handle per (N_hor, Nother), on torch's current stream."""
    import torch
    import dyobav_mpcnwta_warehouse_amd as nm
    if (N, Nother) not in _handles:
        cfg = nm.default_config_struct()
        cfg.N_hor, cfg.ts, cfg.Nother, cfg.Nstcobs, cfg.Ndynobs = N, TS, Nother, 2, 4
        h = nm.Handle(cfg)
        h.set_stream(torch.cuda.current_stream().cuda_stream)
        _handles[(N, Nother)] = h
    return _handles[(N, Nother)]


def close_handles():
    for h in _handles.values():
        h.close()
    _handles.clear()


def group_sizes(Nother):
    """R in {1, 2, 3, Nother - 1, Nother, Nother + 1}, those that are group sizes."""
    return sorted({r for r in (1, 2, 3, Nother - 1, Nother, Nother + 1) if r >= 1})


def make_case(seed, R, N, dtype, spread=3.0):
    """G groups of R robots: every group within ``spread`` of a centre somewhere in the world (so that distances within a group
    are a few metres and the ranking has something to decide), controls inside the solver's box, a quarter of the robots stopped.
    Values are rounded to ``dtype`` and returned as float64 arrays holding exactly those values, plus flags."""
    rng = np.random.default_rng([seed, R, N])
    B = G * R
    centre = rng.uniform(-(COORD - spread), COORD - spread, size=(G, 1, 2))
    xy = (centre + rng.uniform(-spread, spread, size=(G, R, 2))).reshape(B, 2)
    robot = np.concatenate([xy, rng.uniform(-4.0, 4.0, size=(B, 1))], axis=1)
    U = np.stack([rng.uniform(-0.5, 1.5, size=(B, N)), rng.uniform(-0.5, 0.5, size=(B, N))], axis=-1).reshape(B, 2 * N)
    alive = (rng.random(B) < 0.75).astype(np.uint8)
    rnd = lambda a: np.asarray(a, dtype=dtype).astype(np.float64)
    return dict(robot=rnd(robot), U=rnd(U), alive=alive, R=R, N=N, B=B)


def run_lists(R):
    """None (all), and a compact list that drops members of the middle group and the whole last group."""
    B = G * R
    keep = [b for b in range(B) if b // R == 0 or (b // R == 1 and (b % R) % 2 == 0)]
    return [None, np.array(keep, dtype=np.int64)]


def call_exchange(h, dtype, robot, U, alive, R, run=None, prefill=float("nan"), tensors=None):
    """One ``nmpc_fleet_exchange`` call. ``tensors``: device tensors to use for the inputs (name -> tensor or None) instead of fresh
    uploads. Returns ``other_c`` [n_run, 3 (N + 1) Nother] (numpy) -- it starts filled with ``prefill`` -- and the input tensors."""
    import torch
    from dyobav_mpcnwta_warehouse_amd import _capi
    dt = np.dtype(dtype)
    tdt = torch.float32 if dt == np.float32 else torch.float64
    up = lambda x, d: None if x is None else torch.as_tensor(np.ascontiguousarray(x, dtype=d)).cuda()
    t = tensors if tensors is not None else dict(robot=up(robot, dt), U=up(U, dt), alive=up(alive, np.uint8), run=up(run, np.int64))
    B = int(t["robot"].shape[0])
    n_run = B if t["run"] is None else int(t["run"].numel())
    L = 3 * (h.cfg.N_hor + 1) * h.cfg.Nother
    out = torch.full((max(n_run, 1), L), prefill, dtype=tdt, device="cuda")
    a = _capi.NmpcFleetArgs()
    a.B, a.R, a.n_run = B, R, n_run
    a.run = None if t["run"] is None else t["run"].data_ptr()
    a.robot, a.U_prev = t["robot"].data_ptr(), (None if t["U"] is None else t["U"].data_ptr())
    a.alive = None if t["alive"] is None else t["alive"].data_ptr()
    a.other_c = out.data_ptr()
    h.fleet_exchange(dt, a)
    torch.cuda.synchronize()
    return out[:n_run].cpu().numpy(), t


POST_KEYS = ("clr_fleet", "collision", "complete", "alive", "collision_fleet")


def call_post(h, dtype, robot, R, state, run=None, width=0.0, tensors=None):
    """One ``nmpc_fleet_post`` call on ``state`` (the five arrays of POST_KEYS). Returns the five arrays after the call (numpy)."""
    import torch
    from dyobav_mpcnwta_warehouse_amd import _capi
    dt = np.dtype(dtype)
    up = lambda x, d: None if x is None else torch.as_tensor(np.ascontiguousarray(x, dtype=d)).cuda()
    t = tensors if tensors is not None else dict(robot=up(robot, dt), run=up(run, np.int64), clr_fleet=up(state["clr_fleet"], dt),
                                                   **{k: up(state[k], np.uint8) for k in POST_KEYS[1:]})
    B = int(t["robot"].shape[0])
    a = _capi.NmpcFleetArgs()
    a.B, a.R, a.n_run, a.width = B, R, (B if t["run"] is None else int(t["run"].numel())), float(width)
    a.run = None if t["run"] is None else t["run"].data_ptr()
    a.robot = t["robot"].data_ptr()
    for k in POST_KEYS:
        setattr(a, k, None if t[k] is None else t[k].data_ptr())
    h.fleet_post(dt, a)
    torch.cuda.synchronize()
    return {k: t[k].cpu().numpy() for k in POST_KEYS if t[k] is not None}, t
