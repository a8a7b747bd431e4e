#!/usr/bin/env python3
"""Randomised differential check of the f2 kernels (nmpc_hypotheses_to_ellipses_*; by hand on the GPU box for long runs, a
reduced run with a fixed seed is part of the -m gpu suite through tests/test_gpu_fuzz.py): random horizon, obstacle slots,
pedestrians, points per time offset (the boundaries of the five kernels and of the groups per pass over-represented), batch
size, clustering parameters and input family (tests/hypotheses_cases.py), fp64 and fp32, against oracle/hypotheses.py --
every element of the output (prefilled with NaN, with a guard region behind it) and n_obs.
    python tests/fuzz_hypotheses.py [cases] [seed]
Also holds what tests/test_gpu_hypotheses_sweep.py uses to run and compare one case."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dyobav_mpcnwta_warehouse_amd as nm   # noqa: E402
import hypotheses_cases as hc               # noqa: E402
from oracle import hypotheses as oh         # noqa: E402

WORST = {}      # kernel type -> worst observed float32 error / a-priori bound


def handle(N, Ndyn):
    cfg = nm.default_config_struct()
    cfg.N_hor, cfg.Ndynobs = int(N), int(Ndyn)
    return nm.Handle(cfg)


def call(h, dt, hypos, P, cur, H, par, B, dyn, n_obs):
    """The C entry point itself; arrays are torch tensors, raw pointers or None. Returns the status code."""
    fn = getattr(h._lib, "nmpc_hypotheses_to_ellipses_" + ("f32" if np.dtype(dt) == np.float32 else "f64"))
    p = lambda x: x if x is None or isinstance(x, int) else x.data_ptr()
    return fn(h._h, p(hypos), int(P), p(cur), int(H), float(par["human_size"]), float(par["eps"]), float(par["enlarge"]),
              float(par["extra_margin"]), int(B), p(dyn), p(n_obs))


def run_gpu(h, dt, hypos, cur, par, N, Ndyn):
    """hypos[B,N,P,2], cur[B,H,2] (numpy) -> (dyn[B,Ndyn,N+1,6] as float64, n_obs[B]). The output is prefilled with NaN and
    followed by one instance of slack, which must stay NaN (as must the element behind n_obs)."""
    tdt = torch.float32 if np.dtype(dt) == np.float32 else torch.float64
    B, P, H = hypos.shape[0], hypos.shape[2], cur.shape[1]
    assert hypos.shape[1] == N
    per = Ndyn * (N + 1) * 6
    buf = torch.full(((B + 1) * per,), float("nan"), dtype=tdt, device="cuda")
    nobs = torch.full((B + 1,), -7, dtype=torch.int32, device="cuda")
    d_h = torch.from_numpy(np.ascontiguousarray(hypos, dtype=dt)).cuda()
    d_c = torch.from_numpy(np.ascontiguousarray(cur if H else np.zeros((B, 1, 2)), dtype=dt)).cuda()   # H = 0: never read
    torch.cuda.synchronize()          # the handle works on a stream of its own: the fills above must have finished
    rc = call(h, dt, d_h, P, d_c, H, par, B, buf, nobs)
    torch.cuda.synchronize()
    if rc < 0:
        raise nm.NmpcError(rc, h._lib.nmpc_last_error().decode(errors="replace"))
    assert torch.isnan(buf[B * per:]).all(), "the kernel wrote behind dyn"
    assert int(nobs[B]) == -7, "the kernel wrote behind n_obs"
    return buf[:B * per].view(B, Ndyn, N + 1, 6).cpu().numpy().astype(np.float64), nobs[:B].cpu().numpy(), buf


def reference(hypos, cur, par, Ndyn):
    want = [oh.hypotheses_to_obstacles(cur[b], hypos[b], par["human_size"], par["eps"], par["enlarge"], par["extra_margin"], Ndyn)
            for b in range(hypos.shape[0])]
    return np.stack([w[0] for w in want]), np.array([w[1] for w in want])


def compare(dt, dyn, nobs, hypos, cur, par, Ndyn, want, want_n):
    """None if every element agrees (fp64: atol 1e-11 max(1, max|coordinate|); fp32: the a-priori bound of
    hypotheses_cases.f32_bounds per element, the rows the kernel copies bit for bit), else a one-line report. Records the
    worst fp32 error / bound ratio per kernel type in WORST."""
    B, P = hypos.shape[0], hypos.shape[2]
    scale = max(1.0, float(np.abs(hypos).max()) if hypos.size else 1.0, float(np.abs(cur).max()) if cur.size else 1.0)
    atol64 = 1e-11 * scale
    if not np.array_equal(nobs, want_n):
        b = int(np.nonzero(nobs != want_n)[0][0])
        return f"n_obs of instance {b}: {nobs[b]} vs {want_n[b]}"
    if np.isnan(dyn).any():
        return f"element {tuple(int(v) for v in np.argwhere(np.isnan(dyn))[0])} was not written"
    if np.dtype(dt) == np.float32:
        want = want.copy()
        H = cur.shape[1]
        want[:, :min(H, Ndyn), 0, 2:4] = float(np.float32(par["human_size"]))       # the kernel holds human_size in fp32
        bound = np.stack([hc.f32_bounds(hypos[b], par, Ndyn, atol64) for b in range(B)])
        exact = bound <= atol64
        err = np.abs(dyn - want)
        if (err[exact] != 0).any():
            k = tuple(int(v) for v in np.argwhere(exact & (err != 0))[0])
            return f"element {k} (copied / constant, must be exact): {dyn[k]!r} vs {want[k]!r}"
        ratio = float((err / bound)[~exact].max()) if (~exact).any() else 0.0
        kern = hc.kernel_of(P)
        WORST[kern] = max(WORST.get(kern, 0.0), ratio)
        if ratio > 1.0:
            k = tuple(int(v) for v in np.argwhere((err > bound) & ~exact)[0])
            return f"element {k}: {dyn[k]!r} vs {want[k]!r}, error {err[k]:.3e} > a-priori bound {bound[k]:.3e}"
    else:
        err = np.abs(dyn - want)
        if not (err <= atol64).all():
            k = tuple(int(v) for v in np.unravel_index(int(np.argmax(err)), err.shape))
            return f"element {k}: {dyn[k]!r} vs {want[k]!r}, error {err[k]:.3e} > {atol64:.1e}"
    return None


def check_case(h, dt, hypos, cur, par, N, Ndyn):
    """Run one batch and compare it in full; returns (report or None, dyn, n_obs, want)."""
    dyn, nobs, _ = run_gpu(h, dt, hypos, cur, par, N, Ndyn)
    want, want_n = reference(hypos, cur, par, Ndyn)
    return compare(dt, dyn, nobs, hypos, cur, par, Ndyn, want, want_n), dyn, nobs, want


def run(cases=100, seed=0, out=print):
    rng = np.random.default_rng(seed)
    checked, resampled, offsets = 0, 0, 0
    edges_P = [1, 2, 3, 20, 21, 22, 31, 32, 33, 63, 64, 65, 128, 129, 192, 193, 255, 256]
    for ci in range(cases):
        N = int(rng.choice([2, 3, 20, 21, 63, 64, rng.integers(2, 65)]))
        P = int(rng.choice(edges_P)) if rng.random() < 0.5 else int(rng.integers(1, 257))
        P = P if rng.random() < 0.7 else int(rng.integers(1, 65))             # the narrow kernels see the most traffic
        Ndyn = int(rng.choice([1, 2, 15, 40, rng.integers(1, 60)]))
        H = int(rng.choice([0, Ndyn, rng.integers(0, Ndyn + 1)]))
        budget = max(1, 1200 // (N * max(P, 16) // 16))                        # keeps the Python reference at ~0.1 s a case
        B = int(max(min(rng.choice([1, 2, 5, 16]), budget), -(-50 // N)))       # at least 50 time offsets (the guard's 2 % cap)
        par = dict(hc.DEFAULT if rng.random() < 0.3 else hc.PARAM_SETS[int(rng.integers(0, 3))])
        family = str(rng.choice(hc.FAMILIES))
        if family == "lattice":
            par["eps"] = float(rng.choice([1.0, 5.0, 0.5]))
        cseed = int(rng.integers(0, 2 ** 31))
        with handle(N, Ndyn) as h:
            for dt in (np.float64, np.float32):
                hypos, cur = hc.generate(family, B, N, P, H, par["eps"], cseed, dt, Ndyn=Ndyn)
                resampled, offsets = resampled + hc.STATS["resampled"], offsets + hc.STATS["offsets"]
                msg, _, _, _ = check_case(h, dt, hypos, cur, par, N, Ndyn)
                checked += B
                if msg:
                    out(f"MISMATCH case {ci}: family={family} N={N} Ndyn={Ndyn} H={H} P={P} B={B} par={par} seed={cseed} "
                        f"dtype={np.dtype(dt).name} kernel={hc.kernel_of(P)}: {msg}")
                    return 1
    worst = ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items()))
    out(f"{cases} cases, {checked} instances checked element by element in fp64 and fp32; {resampled} of {offsets} time offsets "
        f"redrawn by the near-tie guard; worst fp32 error / a-priori bound: {worst}")
    return 0


if __name__ == "__main__":
    sys.exit(run(*[int(x) for x in sys.argv[1:3]]))
