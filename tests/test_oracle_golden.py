"""CPU tests: the oracle (oracle/nmpc_oracle*.{c,h}) against everything the reference pins for this path.

* known answers of the reference's own unit tests (src/tests/test_mpc_builder.py:16-253), via fixtures produced
  by running the reference's functions (tests/golden/known_answers.json);
* f, F1, F2 of the reference's MpcModule.build() (mpc_builder.py:28-201) on random (u, p) (problem_*.npz);
* unicycle RK4 (motion_model.py:141-163);
* the hand-written adjoint against central differences of the REFERENCE's f;
* the same at OFF-NOMINAL robot constants (problem_offnominal.npz: default dimensions, every constant of the robot block
  and ts changed, recorded from the reference on a derived yaml), with the sets U and C the reference built there.
"""
import json
import os

import numpy as np
import pytest

import oracle
from conftest import load_problem_fixture


@pytest.fixture(scope="module")
def problem_offnominal():
    return load_problem_fixture("problem_offnominal.npz")


def test_known_answers_primitives(golden_dir):
    ka = json.load(open(os.path.join(golden_dir, "known_answers.json")))
    # every stored reference output equals the value the reference's test asserts
    for name, case in ka.items():
        assert np.allclose(np.ravel(case["got"]), np.ravel(case["expected"]), atol=1e-3), name
    # the oracle's primitives reproduce them (inputs as in test_mpc_builder.py)
    assert oracle.dist2_to_lineseg(1, 2, 3, 2, 3, 0) == pytest.approx(2.0 ** 2)           # :28-43
    assert oracle.dist2_to_lineseg(1, 2, 3, 1, 3, 0) == pytest.approx(5.0)
    assert oracle.inside_ellipse(1, 2, 1, 2, 1, 1, 0) == pytest.approx(1.0)               # :45-60
    assert oracle.inside_ellipse(1, 2, 1, 4, 1, 1, 0) == pytest.approx(-3.0, abs=1e-3)
    b1, a0, a1 = [0, 2, 1, 3], [-1, 1, 0, 0], [0, 0, -1, 1]
    assert oracle.inside_cvx_polygon(1, 2, b1, a0, a1) == pytest.approx(3.0)              # :62-83
    assert oracle.inside_cvx_polygon(1, 2, [0, 1, 0, 1], a0, a1) == pytest.approx(0.0)
    # cost_inside_cvx_polygon weight 2 -> 18 (:123-138); cost_inside_ellipses -> [1, 0] (:140-156)
    assert 2 * oracle.inside_cvx_polygon(1, 2, b1, a0, a1) ** 2 == pytest.approx(18.0)
    assert max(0.0, oracle.inside_ellipse(1, 2, 1, 2, 1, 1, 0)) ** 2 == pytest.approx(1.0)
    assert max(0.0, oracle.inside_ellipse(1, 2, 1, 4, 1, 1, 0)) ** 2 == 0.0
    # cost_refpath_deviation: point (1,2), polyline (0,0)-(1,0)-(3,2), w 0.5 -> 1.0 (:228-240)
    d = min(oracle.dist2_to_lineseg(1, 2, 0, 0, 1, 0), oracle.dist2_to_lineseg(1, 2, 1, 0, 3, 2))
    assert 0.5 * d == pytest.approx(1.0, abs=1e-3)


def test_unicycle_rk4_matches_reference(golden_dir):
    fx = np.load(os.path.join(golden_dir, "motion_model.npz"))
    for s, a, sn in zip(fx["S"], fx["A"], fx["S_next"]):
        assert np.allclose(oracle.unicycle_rk4(float(fx["ts"]), s, a), sn, rtol=0, atol=1e-14)


@pytest.mark.parametrize("fixture", ["problem_n20", "problem_small", "problem_offnominal"])
def test_problem_functions_match_reference(fixture, request):
    fx, pr = request.getfixturevalue(fixture)
    assert pr.np_ == fx["P"].shape[1]
    for i in range(fx["P"].shape[0]):
        f, F1, F2 = oracle.eval_problem(pr, fx["U"][i], fx["P"][i])
        assert f == pytest.approx(fx["f"][i], rel=1e-12)
        np.testing.assert_allclose(F1, fx["F1"][i], rtol=0, atol=1e-12)
        np.testing.assert_allclose(F2, fx["F2"][i], rtol=1e-12, atol=1e-12)
    # the fixtures exercise the penalty constraints (robot inside obstacles)
    assert (fx["F2"] > 0).any()


@pytest.mark.parametrize("fixture", ["problem_n20", "problem_small", "problem_offnominal"])
def test_adjoint_gradient_matches_reference_fd(fixture, request):
    fx, pr = request.getfixturevalue(fixture)
    n = 2 * pr.N
    for i in range(fx["P"].shape[0]):
        val, g = oracle.psi(pr, fx["U"][i], 0.0, np.zeros(n), fx["P"][i])
        assert val == pytest.approx(fx["f"][i], rel=1e-12)
        scale = np.abs(fx["grad_f_fd"][i]).max()
        np.testing.assert_allclose(g, fx["grad_f_fd"][i], rtol=0, atol=2e-7 * scale)


def test_psi_gradient_finite_differences_with_penalty(problem_small):
    fx, pr = problem_small
    rng = np.random.default_rng(0)
    n = 2 * pr.N
    for i in range(4):
        u, p = fx["U"][i], fx["P"][i]
        y, c = rng.normal(size=n), 37.0
        _, g = oracle.psi(pr, u, c, y, p)
        gfd = np.zeros(n)
        for j in range(n):
            h = 1e-6
            up, um = u.copy(), u.copy()
            up[j] += h
            um[j] -= h
            gfd[j] = (oracle.psi(pr, up, c, y, p, grad=False)[0] - oracle.psi(pr, um, c, y, p, grad=False)[0]) / (2 * h)
        np.testing.assert_allclose(g, gfd, rtol=0, atol=5e-7 * np.abs(gfd).max())


def test_psi_is_f_plus_penalties(problem_n20):
    fx, pr = problem_n20
    rng = np.random.default_rng(1)
    n = 2 * pr.N
    lo = np.r_[np.full(pr.N, pr.lin_acc_min), np.full(pr.N, -pr.ang_acc_max)]
    hi = np.r_[np.full(pr.N, pr.lin_acc_max), np.full(pr.N, pr.ang_acc_max)]
    for i in range(6):
        y, c = rng.normal(size=n) * 5, float(rng.uniform(0.5, 200))
        val, _ = oracle.psi(pr, fx["U"][i], c, y, fx["P"][i])
        z = fx["F1"][i] + y / max(c, 1.0)
        d2 = np.sum((z - np.clip(z, lo, hi)) ** 2)
        expect = fx["f"][i] + 0.5 * c * (d2 + np.sum(fx["F2"][i] ** 2))
        assert val == pytest.approx(expect, rel=1e-12)



def test_offnominal_fixture_changes_every_constant_and_the_oracle_builds_the_recorded_sets(golden_dir, problem_offnominal):
    """problem_offnominal.npz: K = 8 instances at the default dimensions, no larger than problem_n20.npz; every robot
    constant differs from mpc_fast.yaml's, no two magnitudes coincide, the acceleration bounds are asymmetric; the constants
    in the npz are the ones recorded in problem_meta.json. The sets the oracle works with are the ones the reference built
    (captured `bounds` / `set_c` of MpcModule.build): C through psi -- the penalty on F1 is the distance to the RECORDED
    box [cmin, cmax] -- and U through the solver's projection: a solve started far outside U is brought back to the recorded faces."""
    fx, pr = problem_offnominal
    meta = json.load(open(os.path.join(golden_dir, "problem_meta.json")))["offnominal"]
    assert os.path.getsize(os.path.join(golden_dir, "problem_offnominal.npz")) <= os.path.getsize(os.path.join(golden_dir, "problem_n20.npz"))
    assert fx["P"].shape == (8, 2778) and [int(v) for v in fx["dims"]] == [20, 10, 10, 15] and (fx["F2"] > 0).any()
    names = ("ts", "lin_vel_min", "lin_vel_max", "ang_vel_max", "lin_acc_min", "lin_acc_max", "ang_acc_max", "vehicle_width",
             "vehicle_margin", "social_margin")
    assert [meta["robot"][k] for k in names] == [float(v) for v in fx["robot"]] == [getattr(pr, k) for k in names]
    nominal = oracle.Problem()
    assert all(getattr(pr, k) != getattr(nominal, k) for k in names)
    assert len({abs(getattr(pr, k)) for k in names}) == len(names) and pr.lin_acc_min != -pr.lin_acc_max
    N, n = pr.N, 2 * pr.N
    umin, umax, cmin, cmax = (np.array(meta[k], dtype=float) for k in ("umin", "umax", "cmin", "cmax"))
    for k in ("umin", "umax", "cmin", "cmax"):
        assert np.array_equal(fx[k], np.array(meta[k], dtype=float))
    # the sets implied by the oracle's constants, in the layouts the reference uses (u interleaved, F1 blocked)
    assert np.array_equal(umin, np.tile([pr.lin_vel_min, -pr.ang_vel_max], N)) and np.array_equal(umax, np.tile([pr.lin_vel_max, pr.ang_vel_max], N))
    assert np.array_equal(cmin, np.r_[np.full(N, pr.lin_acc_min), np.full(N, -pr.ang_acc_max)])
    assert np.array_equal(cmax, np.r_[np.full(N, pr.lin_acc_max), np.full(N, pr.ang_acc_max)])
    rng = np.random.default_rng(2)
    used = np.zeros(2, dtype=bool)
    for i in range(8):
        y, c = rng.normal(size=n) * 5, float(rng.uniform(0.5, 200))
        val, _ = oracle.psi(pr, fx["U"][i], c, y, fx["P"][i])
        z = fx["F1"][i] + y / max(c, 1.0)
        used |= [(z[:N] < cmin[:N]).any(), (z[:N] > cmax[:N]).any()]
        expect = fx["f"][i] + 0.5 * c * (np.sum((z - np.clip(z, cmin, cmax)) ** 2) + np.sum(fx["F2"][i] ** 2))
        assert val == pytest.approx(expect, rel=1e-12)
        wrong = fx["f"][i] + 0.5 * c * (np.sum((z - np.clip(z, -cmax, -cmin)) ** 2) + np.sum(fx["F2"][i] ** 2))
        assert abs(val - wrong) > 1e-6 * abs(val)                 # (the asymmetry is felt: bounds swapped give another psi)
    assert used.all()
    op = oracle.Options(max_outer=1, max_inner=1, lip_delta=1e-4, lip_eps=1e-4)
    for sign, face in ((1.0, umax), (-1.0, umin)):
        u, _, _ = oracle.solve(pr, op, fx["P"][0], u0=np.full(n, sign * 1e3))
        # (the start is projected on U, then one PANOC step is taken from the face: the speeds stay on it, the turn rates
        #  move a little way inside)
        assert (u >= umin).all() and (u <= umax).all()
        assert np.array_equal(u[0::2], face[0::2]) and np.abs(u[1::2] - face[1::2]).max() < 0.01


def test_offnominal_recording_regenerates(golden_dir, tmp_path):
    """tests/golden/make_golden.py run on the reference reproduces problem_offnominal.npz and its entry of problem_meta.json
    (where the reference tree exists; the recording itself is what every other test reads). Arrays are compared, not
    bytes: an npz carries the time it was written."""
    import subprocess
    import sys
    recipe = os.path.join(golden_dir, "make_golden.py")
    ref = next(l.split('"')[1] for l in open(recipe) if l.startswith("REF = "))
    if not os.path.exists(os.path.join(ref, "src", "pkg_mpc_tracker", "solver_build", "mpc_builder.py")):
        pytest.skip("the reference tree is not on this machine")
    subprocess.run([sys.executable, recipe, str(tmp_path), "offnominal"], check=True, capture_output=True, timeout=900)
    new, old = np.load(os.path.join(str(tmp_path), "problem_offnominal.npz")), np.load(os.path.join(golden_dir, "problem_offnominal.npz"))
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        assert np.array_equal(new[k], old[k]), k
    assert not os.path.exists(os.path.join(str(tmp_path), "problem_meta.json"))
    assert json.load(open(os.path.join(str(tmp_path), "problem_meta_offnominal.json"))) == \
        json.load(open(os.path.join(golden_dir, "problem_meta.json")))["offnominal"]
