"""The numpy restatement of the Kalman-filter predictor stage (tests/kf_reference.py) is a reference and not a third
opinion: it reproduces the recordings of the reference project's own ``KfmpInterface`` / ``zfilter.KalmanFilter``
(tests/golden/kf_cases.json, written by tests/golden/make_kf_golden.py) to 1e-12. Also established here, on the CPU, for the
inputs tests/test_gpu_kf_predict.py uses: what the fuzz set covers, the restatement's own float32 rounding per output array
(the yardstick of the fp32 kernel), the chain values the data-independent checks use, and the new part of the C ABI (struct
layout against the C compiler)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import kf_cases as kc
import kf_reference as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_reproduces_every_recording():
    """Call by call on one carried covariance per sequence: positions, the returned (P00, P11) and the whole P."""
    seqs = kc.golden_sequences()
    assert sorted(s["H"] for s in seqs if s["kind"] == "interface") == [1, 3, 4] and sum(s["kind"] == "general" for s in seqs) >= 2
    worst = 0.0
    for i, s in enumerate(seqs):
        A, C, Q, R, P = (np.array(s[k]) for k in ("A", "C", "Q", "R", "P0"))
        if s["kind"] == "interface":
            assert all(len(c["traj"]) == 1 for c in s["steps"][0])                      # the first step: every L == 1
            assert s["H"] == 1 or any(len(s["steps"][-1][h]["traj"]) < len(s["steps"]) for h in range(s["H"]))     # one stops
            assert np.array_equal(P, np.eye(4))
        else:
            assert np.abs(Q - np.diag(np.diag(Q))).max() > 0.05 and np.linalg.eigvalsh(R).min() >= 0.5 and not np.array_equal(P, np.eye(4))
        for k, calls in enumerate(s["steps"]):
            assert len(calls) == s["H"]
            for h, c in enumerate(calls):
                pos, P = kr.filter_traj(c["traj"], P, A, C, Q, R, s["N"])
                for got, want in ((pos, c["positions"]), (P, c["P"]), ([P[0, 0], P[1, 1]], c["std"])):
                    err = float(np.abs(np.asarray(got) - np.array(want)).max())
                    worst = max(worst, err)
                    assert err <= 1e-12, (i, k, h, err)
    print(f"restatement against {sum(len(c) for s in seqs for c in s['steps'])} recorded calls: worst absolute error {worst:.2e}")


def test_chain_values_are_the_ones_the_reference_returns():
    """Calls with L = 1, 2, 3 on one object return P00 = 1, 0.671..., 0.6457...: the chain after 0, 1 and 3 one-steps."""
    ch = kr.chain_values(130)
    assert ch[0] == 1.0 and abs(ch[1] - 0.6710526315789469) < 1e-15 and abs(ch[2] - 0.6398786959818044) < 1e-15
    assert abs(ch[3] - 0.6457643460068592) < 1e-15 and abs(ch[-1] - 0.68256212) < 1e-8
    seq = next(s for s in kc.golden_sequences() if s["kind"] == "interface" and s["H"] == 3)
    n = 0
    for calls in seq["steps"][:4]:
        for c in calls:
            n += len(c["traj"]) - 1
            assert abs(c["std"][0] - ch[n]) < 1e-14 and c["std"][0] == c["std"][1]


def test_recording_regenerates_byte_for_byte(tmp_path):
    """tests/golden/make_kf_golden.py run on the reference's own classes writes kf_cases.json exactly as committed (where the
    reference tree exists; the recording itself is what every other test reads)."""
    recipe = os.path.join(kc.GOLDEN, "make_kf_golden.py")
    ref = next(l.split('"')[1] for l in open(recipe) if l.startswith("REF = "))
    if not os.path.exists(os.path.join(ref, "src", "zfilter.py")):
        pytest.skip("the reference tree is not on this machine")
    subprocess.run([sys.executable, recipe, str(tmp_path)], check=True, capture_output=True, timeout=300)
    committed = open(os.path.join(kc.GOLDEN, "kf_cases.json"), "rb").read()
    assert open(os.path.join(str(tmp_path), "kf_cases.json"), "rb").read() == committed
    assert len(committed) < 200 * 1024


def test_fuzz_inputs_cover_every_length_and_append_case():
    counts, longest = kc.fuzz_population()
    print("pedestrians of running scenarios per (kf_len, hcount - kf_len): " + ", ".join(f"{k}: {v}" for k, v in sorted(counts.items())))
    for kind in ("0", "1", "2", "3", "cap-1", "cap"):
        for extra in (0, 1, 2):
            assert counts.get((kind, extra), 0) > 0, (kind, extra)
    assert longest > 130
    assert {g["B"] for g in kc.FUZZ_GROUPS} == {1, 3, 70} and {g["H"] for g in kc.FUZZ_GROUPS} == {1, 4, 5}
    assert {g["cap"] for g in kc.FUZZ_GROUPS} == {2, 41} and {g["run"] for g in kc.FUZZ_GROUPS} == {"all", "first", "last", "alternate"}
    # the long chain starts at the fixed point: a one-step returns the covariance it was given, bit for bit
    c = kc.fuzz_group(len(kc.FUZZ_GROUPS) - 1)
    A, C, Q, R = c["mats"]
    P = c["state"]["kf_P"][0]
    assert np.array_equal(kr.one_step(np.zeros((4, 1)), P, np.zeros((2, 1)), A, C, Q, R)[1], P)


ARRAYS = ("dyn_c", "kf_traj", "kf_P")


def fuzz_twin_errors(verbose=True):
    """The fuzz set evaluated by the restatement in float32 against itself in fp64 on the same (float32-rounded) inputs:
    {array: worst absolute error} over the written elements."""
    worst = {}
    for g in range(len(kc.FUZZ_GROUPS)):
        case = kc.round_inputs(kc.fuzz_group(g), np.float32)
        o64, o32 = kc.reference(case), kc.reference(case, np.float32)
        assert np.array_equal(o64["kf_len"], o32["kf_len"])
        for k in ARRAYS:
            err = float(np.abs(o32[k].astype(np.float64) - o64[k]).max())
            worst[k] = max(worst.get(k, 0.0), err)
    if verbose:
        print("float32 twin of the restatement, worst absolute error per array over the fuzz set:")
        print("    " + ", ".join(f'"{k}": {v:.3e}' for k, v in worst.items()))
    return worst


def test_twin_errors_match_the_committed_bounds():
    """The float32 twin errors are the constants committed in tests/test_gpu_kf_predict.py (to the printed digits) and the
    fp32 bounds there are four times them. Figures: end of this file."""
    import test_gpu_kf_predict as g
    worst = fuzz_twin_errors()
    assert set(worst) == set(g.TWIN_ERROR_F32)
    for k, v in worst.items():
        assert float(f"{v:.3e}") == g.TWIN_ERROR_F32[k], (k, v, g.TWIN_ERROR_F32[k])
        assert g.BOUND_F32[k] == 4 * g.TWIN_ERROR_F32[k]
    assert worst["kf_traj"] == 0.0            # a copy: bit-identical


def test_sixty_step_inputs_end_scenarios_and_walks():
    s0, kf0, seq, recs = kc.sixty_reference()
    fin = recs[-1]["post"]
    W = s0["hpath"].shape[2]
    stopped = int((fin["hidx"] == W).sum())
    partial = sum(r["run"] is not None for r in recs)
    print(f"{len(recs)} steps, {partial} with a run list, survivors {int(fin['alive'].sum())} of {kc.SIXTY_B}, pedestrians at the end of "
          f"their path {stopped} of {fin['hidx'].size}, longest stored trajectory {int(recs[-1]['kf']['kf_len'].max())}")
    assert len(recs) == kc.SIXTY_STEPS and partial > 10 and 0 < fin["alive"].sum() < kc.SIXTY_B
    assert 0 < stopped < fin["hidx"].size
    # the stored trajectory is past_traj: it grows with hcount and stops with the pedestrian
    live = fin["alive"] != 0
    assert np.array_equal(recs[-1]["kf"]["kf_len"][live], recs[-2]["post"]["hcount"][live])


def test_kf_args_struct_matches_the_header(tmp_path):
    from dyobav_mpcnwta_warehouse_amd._capi import NmpcKfArgs, NmpcLoopArgs
    src = os.path.join(str(tmp_path), "sz.c")
    open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "nmpc_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %d", '
                         'sizeof(nmpc_kf_args), offsetof(nmpc_kf_args, run), offsetof(nmpc_kf_args, kf_P), offsetof(nmpc_kf_args, A), '
                         'offsetof(nmpc_kf_args, human_size), offsetof(nmpc_kf_args, dyn_c), NMPC_ABI_VERSION);return 0;}\n')
    exe = os.path.join(str(tmp_path), "sz")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
    size, off_run, off_p, off_a, off_hs, off_dyn, abi = map(int, subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split())
    assert ctypes.sizeof(NmpcKfArgs) == size and NmpcKfArgs.run.offset == off_run and NmpcKfArgs.kf_P.offset == off_p
    assert NmpcKfArgs.A.offset == off_a and NmpcKfArgs.human_size.offset == off_hs and NmpcKfArgs.dyn_c.offset == off_dyn
    assert abi == 5                               # additive: the version and nmpc_loop_args are what they were
    a = NmpcKfArgs().set_matrices(np.arange(16.0).reshape(4, 4), np.arange(8.0).reshape(2, 4), np.eye(4), np.eye(2))
    assert list(a.A) == list(range(16)) and list(a.C) == list(range(8)) and a.Q[5] == 1.0 and a.R[3] == 1.0
    with pytest.raises(ValueError):
        NmpcKfArgs().set_matrices(np.eye(3), np.eye(2), np.eye(4), np.eye(2))


# Output of `pytest -s -m "not gpu" tests/test_kf_reference_cpu.py` (numpy 2.2, x86-64), the figures the GPU module relies on:
#
# restatement against 105 recorded calls: worst absolute error 5.68e-14
# float32 twin of the restatement, worst absolute error per array over the fuzz set:
#     dyn_c 3.164e-05, kf_traj 0, kf_P 1.288e-05
#     (per group: the default-matrix groups give 4e-6 .. 2e-5 on dyn_c at coordinates up to 30 -- a position's float32 rounding
#      times the twenty offsets -- and 6e-8 .. 9e-7 on kf_P; the dense groups 5e-6 .. 3e-5 and 5e-7 .. 1.3e-5: with a perturbed A
#      of spectral radius ~1.05 the update P - K (S K') loses digits to cancellation)
# pedestrians of running scenarios per (kf_len, hcount - kf_len): between 9 and 41 in each of the 18 classes; the longest call
#     performs 160 one-steps
# sixty steps: 41 of 60 with a run list, survivors 5 of 12, pedestrians at the end of their path 9 of 48, longest stored
#     trajectory 60
