"""CPU tests of the f2 oracle (oracle/hypotheses.py) against the recordings of the reference's clustering functions and,
where sklearn is installed, against the reference's two functions restated, on the inputs of the GPU sweep."""
import json
import os

import numpy as np
import pytest

import hypotheses_cases as hcs
from oracle import hypotheses as oh


def test_matches_reference_recording(golden_dir):
    cases = json.load(open(os.path.join(golden_dir, "hypotheses_cases.json")))
    assert any(c["n_obs"] > len(c["cur"]) for c in cases)          # multi-modal splits occur
    for c in cases:
        dyn, n_obs = oh.hypotheses_to_obstacles(np.array(c["cur"]), np.array(c["hypos"]))
        assert n_obs == c["n_obs"]
        want = np.array(c["dyn_obs_list"], dtype=float)             # [n_obs][N+1][6]
        np.testing.assert_allclose(dyn[:n_obs], want, rtol=0, atol=1e-12)
        assert (dyn[n_obs:] == 0).all()


def test_dbscan_min2_semantics():
    pts = np.array([[0, 0], [0.9, 0], [1.8, 0], [5, 5], [9, 9], [9.5, 9]], dtype=float)
    assert oh.dbscan_min2(pts, 1.0).tolist() == [0, 0, 0, -1, 1, 1]     # chain, isolated noise, second cluster
    assert oh.dbscan_min2(np.array([[0.0, 0], [1.0, 0]]), 1.0).tolist() == [0, 0]   # distance == eps is a neighbour


# ---- the oracle at the shapes, edges and parameters of the GPU sweep, against sklearn ------------------------------------
def _reference(x, eps, enlarge, extra_margin):
    """The reference's fit_DBSCAN / fit_cluster2gaussian (utils_test.py:133-151) restated: clusters in label order."""
    DBSCAN = pytest.importorskip("sklearn.cluster").DBSCAN
    lab = DBSCAN(eps=eps, min_samples=2).fit(x).labels_
    cl = [x[lab == i] for i in range(len(set(lab)) - (1 if -1 in lab else 0))]
    return lab, [np.r_[c.mean(axis=0), c.std(axis=0) * enlarge + extra_margin] for c in cl]


def _against_sklearn(hypos, cur, par, Ndyn):
    """oracle.hypotheses on a batch == the restated reference + the list assembly of main_base.py:293-302, truncated to
    Ndyn slots: labels and n_obs equal, rows to 1e-12 of the coordinate scale."""
    scale = max(1.0, float(np.abs(hypos).max()))
    for b in range(hypos.shape[0]):
        rows = [[np.r_[c, par["human_size"], par["human_size"]] for c in cur[b]]]
        for t in range(hypos.shape[1]):
            lab, cl = _reference(hypos[b, t], par["eps"], par["enlarge"], par["extra_margin"])
            assert np.array_equal(lab, oh.dbscan_min2(hypos[b, t], par["eps"])), (b, t)
            assert [i.tolist() for i in hcs.components(hypos[b, t], par["eps"])] == [np.nonzero(lab == k)[0].tolist() for k in range(len(cl))]
            rows.append(cl)
        n_obs = max(len(r) for r in rows)
        want = np.zeros((Ndyn, hypos.shape[1] + 1, 6))
        want[:min(n_obs, Ndyn), :, 5] = 1.0
        for t, r in enumerate(rows):
            for c, v in enumerate(r[:Ndyn]):
                want[c, t, :4] = v
        dyn, n = oh.hypotheses_to_obstacles(cur[b], hypos[b], par["human_size"], par["eps"], par["enlarge"], par["extra_margin"], Ndyn)
        assert n == n_obs
        np.testing.assert_allclose(dyn, want, rtol=0, atol=1e-12 * scale)


@pytest.mark.parametrize("case", hcs.family_cases(), ids=lambda c: f"{c['family']}-{c['kernel']}")
def test_oracle_matches_sklearn_on_every_family(case):
    """Every generator family of tests/hypotheses_cases.py at the point counts of all five kernels and with the
    non-default parameter sets -- the inputs of the GPU sweep, as float64 and as float32 see them."""
    pytest.importorskip("sklearn")
    for dt in (np.float64, np.float32):
        hypos, cur = hcs.case_inputs(case, dt)
        assert hcs.STATS["share"] <= 0.02
        _against_sklearn(hypos, cur, case["par"], case["Ndyn"])


@pytest.mark.parametrize("N,Ndyn,H,P", [(20, 40, 4, 40), (40, 160, 8, 160), (64, 15, 2, 256), (2, 7, 2, 1), (3, 7, 2, 33),
                                       (63, 7, 2, 64), (21, 1, 1, 22), (7, 15, 15, 129), (7, 15, 0, 193)])
def test_oracle_matches_sklearn_at_sweep_shapes(N, Ndyn, H, P):
    """Blobs and chains at the quoted configurations (BASELINE configs[2] and [4]) and at the extremes of the sweep."""
    pytest.importorskip("sklearn")
    for k, (gen, par) in enumerate(((hcs.blobs, hcs.DEFAULT), (hcs.chains, hcs.PARAM_SETS[(N + P) % 3]))):
        hypos, cur = gen(1, N, P, H, par["eps"], 77 + k, np.float32 if k else np.float64)
        _against_sklearn(hypos, cur, par, Ndyn)


def test_lattice_ties_are_exact_and_frequent():
    """The lattice family does what it is for: every squared distance is exact in float32, and a good share of the
    neighbour pairs sit at exactly d^2 == eps^2 (3-4-5 pairs at eps = 5 among them)."""
    for eps, s in ((1.0, 1.0), (5.0, 1.0), (0.5, 0.25)):
        hypos, _ = hcs.lattice(2, 4, 60, 1, eps, 3, np.float32, s=s)
        d = hypos[:, :, :, None, :] - hypos[:, :, None, :, :]
        d2 = (d * d).sum(axis=-1)
        d32 = d.astype(np.float32)
        assert np.array_equal((d32 * d32).sum(axis=-1, dtype=np.float32).astype(np.float64), d2)
        assert (d2 == eps * eps).sum() >= 40
        if eps == 5.0:
            assert ((d2 == 25.0) & (np.abs(d[..., 0]) == 3.0)).any()


def test_matches_edge_recording(golden_dir):
    """tests/golden/hypotheses_edge_cases.json (the reference's own functions on exact ties, duplicates, all-noise offsets,
    overflow, non-default parameters): the oracle reproduces the first Ndyn rows and the untruncated n_obs."""
    cases = json.load(open(os.path.join(golden_dir, "hypotheses_edge_cases.json")))
    assert len(cases) >= 12 and os.path.getsize(os.path.join(golden_dir, "hypotheses_edge_cases.json")) < 64 * 1024
    assert any(c["n_obs"] > c["Ndyn"] for c in cases) and any(len(c["hypos"][0]) > 64 for c in cases)
    for c in cases:
        p = c["params"]
        dyn, n_obs = oh.hypotheses_to_obstacles(np.array(c["cur"]).reshape(-1, 2), np.array(c["hypos"]), p["human_size"], p["eps"],
                                                p["enlarge"], p["extra_margin"], c["Ndyn"])
        assert n_obs == c["n_obs"], c["name"]
        want = np.array(c["dyn_obs_list"], dtype=float).reshape(c["n_obs"], c["N"] + 1, 6)
        k = min(n_obs, c["Ndyn"])
        np.testing.assert_allclose(dyn[:k], want[:k], rtol=0, atol=1e-12, err_msg=c["name"])
        assert (dyn[k:] == 0).all()


def test_recordings_regenerate_byte_for_byte(golden_dir, tmp_path):
    """tests/golden/make_golden.py run on the reference's own utils_test.py writes both f2 recordings exactly as committed
    (where the reference tree and sklearn exist; the recordings themselves are what every other test reads)."""
    import subprocess
    import sys
    recipe = os.path.join(golden_dir, "make_golden.py")
    ref = next(l.split('"')[1] for l in open(recipe) if l.startswith("REF = "))
    if not os.path.exists(os.path.join(ref, "src", "utils_test.py")):
        pytest.skip("the reference tree is not on this machine")
    pytest.importorskip("sklearn")
    subprocess.run([sys.executable, recipe, str(tmp_path), "hypotheses"], check=True, capture_output=True, timeout=600)
    for name in ("hypotheses_cases.json", "hypotheses_edge_cases.json"):
        assert open(os.path.join(str(tmp_path), name), "rb").read() == open(os.path.join(golden_dir, name), "rb").read(), name
