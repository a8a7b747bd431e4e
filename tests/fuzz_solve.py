#!/usr/bin/env python3
"""Randomised differential check of short SOLVES (by hand on the GPU box for long runs; a reduced run with fixed seeds is
part of the -m gpu suite through tests/test_gpu_fuzz.py): one outer x four inner iterations, every solver kernel
(throughput, latency with 2..4 wavefronts, cooperative with 2..4, automatic) against the sequential oracle on the cases of
tests/fuzz_eval.py -- iteration counts, exit status and controls.
    python tests/fuzz_solve.py [cases] [seed] [outer] [inner] [32|64]
With more iterations (e.g. 3 x 15: penalty / multiplier updates, L-BFGS ring wrap-around) rounding differences are amplified
along the path; instances whose iteration counts differ from the oracle's are counted, not compared.

fp64 (default): Lipschitz step 1e-4 on both sides; short runs match to 1e-5 on every instance with the oracle's counts.
fp32: the fp32 oracle at a Lipschitz step of 1e-2 on both sides (tests/test_gpu_fp32_paths.py: at the fp32 default step the
finite difference is itself noisy to ~1e-3), plus the fp32-only kernels -- the register table (automatic reg_table; the
plain "throughput" mode runs the LDS / global table there), its axis-aligned (axis_aligned = 1, axis-aligned cases only) and
general members (-1), the on-chip cooperative kernel. Instances whose path the oracle's re-associated fp32 twin does not
reproduce are at the noise floor and only counted. Short runs, on the rest: per mode du q90 below 1e-4, or below twice the
twin's q90 on the same instances where that is larger, max < 1e-2 on the instances with the oracle's counts, and no instance
with other counts: the instances at a decision margin are the ones the twin does not reproduce, so a decision the kernel takes
differently on the rest is a slip, not rounding (the issue's allowance of 1 % let a Lipschitz-test constant changed in one
fp32 member pass with 3 of 783). Measured (seeds 24, 25): q90 8.2e-5..1.1e-4, the twin's on the same instances
7.4e-5..1.1e-4 -- the same in every mode, i.e. the oracle's own spread --, worst 3.2e-3, no count differences; 17 / 22
instances per mode at the twin's noise floor."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dyobav_mpcnwta_warehouse_amd as nm   # noqa: E402
import oracle                               # noqa: E402
from fuzz_eval import make_case             # noqa: E402


def _modes(ci, f32, axis_aligned):
    lw, cw = 2 + ci % 3, 2 + ci % 3
    modes = [("throughput", dict(latency_waves=1, coop_waves=1, reg_table=-1 if f32 else 0)),
             ("latency%d" % lw, dict(latency_waves=lw, coop_waves=1)),
             ("coop%d" % cw, dict(latency_waves=1, coop_waves=cw, reg_table=-1)), ("automatic", dict())]
    if not f32:
        modes.insert(1, ("throughput/reg64", dict(latency_waves=1, coop_waves=1, reg_table=1)))
        return modes
    modes += [("regtable", dict(latency_waves=1, coop_waves=1, reg_table=0)),
              ("axis-general", dict(latency_waves=1, coop_waves=1, reg_table=0, axis_aligned=-1)),
              ("onchip", dict(latency_waves=1, coop_waves=4, reg_table=0))]
    if axis_aligned:
        modes.append(("axis-aligned", dict(latency_waves=1, coop_waves=1, reg_table=0, axis_aligned=1)))
    return modes


def run(cases=100, seed=0, n_outer=1, n_inner=4, out=print, dtype=np.float64):
    f32 = np.dtype(dtype) == np.float32
    lip = 1e-2 if f32 else 1e-4
    rng = np.random.default_rng(seed)
    short = n_outer * n_inner <= 4   # longer runs: rounding differences grow ~4x per iteration on these instances
    worst, flips, total, dus, dus_t, seen, floor = {}, {}, 0, {}, {}, {}, {}
    for ci in range(cases):
        lay, rows, P, _, _, _ = make_case(rng)
        P = P.astype(dtype)
        axis_aligned = not P[:, lay.od:lay.od + 6 * (lay.N + 1) * lay.Ndyn].reshape(-1, 6)[:, 4].any()
        pr = oracle.Problem(lay.N, lay.Nother, lay.Nstc, lay.Ndyn)
        op = oracle.Options(max_outer=n_outer, max_inner=n_inner, lip_delta=lip, lip_eps=lip)
        Uo, ro = oracle.solve_batch(pr, op, P, nthreads=4, dtype=dtype)
        if f32:
            # the noise floor: an instance whose path the oracle's re-associated twin does not reproduce (other counts, or a
            # decision at its margin that moves u by more than 1e-3 -- e.g. a line search that runs out of halvings) is counted
            # as such, not compared
            Ut, rt = oracle.solve_batch(pr, op, P, nthreads=4, dtype=dtype, reassoc=True)
            du_t = np.abs(Ut.astype(np.float64) - Uo).max(axis=1)
            noisy = (rt["inner_iters"] != ro["inner_iters"]) | (rt["n_points"] != ro["n_points"]) | (du_t > 1e-3)
        for name, ov in _modes(ci, f32, axis_aligned):
            cfg = nm.default_config_struct()
            cfg.N_hor, cfg.Nother, cfg.Nstcobs, cfg.Ndynobs = lay.N, lay.Nother, lay.Nstc, lay.Ndyn
            cfg.max_outer_iterations, cfg.max_inner_iterations = n_outer, n_inner
            cfg.lip_eps_f64 = cfg.lip_delta_f64 = 1e-4
            cfg.lip_eps_f32 = cfg.lip_delta_f32 = lip
            for k, v in ov.items():
                setattr(cfg, k, v)
            with nm.Handle(cfg) as h:
                r = h.solve(P, dtype=dtype)
            key = name.rstrip("234") if "reg64" not in name else name
            for i in range(P.shape[0]):
                if f32 and noisy[i]:
                    floor[key] = floor.get(key, 0) + 1
                    continue
                total += 1
                seen[key] = seen.get(key, 0) + 1
                same = r["iters"][i, 1] == ro["inner_iters"][i]
                if f32:
                    same = same and r["iters"][i, 0] == ro["outer_iters"][i] and r["status"][i] == ro["status"][i] and \
                        int(r["info"][i, 4]) == ro["n_points"][i]
                if not same:
                    flips[key] = flips.get(key, 0) + 1    # a line-search / exit decision flipped by rounding
                    continue
                du = np.abs(r["U"][i].astype(np.float64) - Uo[i]).max()
                worst[key] = max(worst.get(key, 0.0), du)
                dus.setdefault(key, []).append(du)
                if f32:
                    dus_t.setdefault(key, []).append(du_t[i])     # the twin's distance on the same instances
                if not np.isfinite(r["U"][i]).all() or (short and not du < (1e-2 if f32 else 1e-5)):
                    out(f"MISMATCH case {ci} N={lay.N} Nother={lay.Nother} Nstc={lay.Nstc} Ndyn={lay.Ndyn} rows={rows} mode={name} "
                          f"instance {i}: max|du| = {du:.3e}")
                    return 1
    prec = "fp32, Lipschitz step 1e-2" if f32 else "fp64"
    out(f"{cases} cases, {total} solves checked against the oracle ({prec}, {n_outer} x {n_inner} iterations)")
    rc = 0
    for k in sorted(seen):
        d = dus.get(k, [np.nan])
        out(f"  {k:16s} max|u - u_oracle|: median {np.median(d):.2e}, q90 {np.quantile(d, 0.9):.2e}, worst {worst.get(k, np.nan):.2e}"
            f"   iteration-count differences {flips.get(k, 0)} of {seen[k]}" + (f" (+ {floor.get(k, 0)} at the twin's noise floor)" if f32 else ""))
        if f32 and short:
            bar = max(1e-4, 2 * np.quantile(dus_t.get(k, [0.0]), 0.9))
            out(f"  {'':16s} the twin on the same instances: q90 {np.quantile(dus_t.get(k, [np.nan]), 0.9):.2e}")
            if not (np.quantile(d, 0.9) < bar and flips.get(k, 0) == 0):
                out(f"MISMATCH mode {k}: q90 {np.quantile(d, 0.9):.2e} (bar {bar:.2e}), count differences {flips.get(k, 0)} of "
                    f"{seen[k]} (bar: none outside the twin's noise floor)")
                rc = 1
    return rc


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:]]
    dt = np.float32 if len(a) > 4 and a[4] == 32 else np.float64
    sys.exit(run(*a[:4], dtype=dt))
