"""Seeded inputs of the Kalman-filter predictor tests (tests/test_gpu_kf_predict.py on the device,
tests/test_kf_reference_cpu.py for the figures that depend only on inputs and reference): the recordings of
tests/golden/kf_cases.json as call sequences, the fuzz set of single calls, and a sixty-step closed loop with prescribed
controls."""
import json
import os

import numpy as np

import kf_reference as kr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TS, HUMAN_SIZE = 0.2, 0.2
SENTINEL = -777.25
FUZZ_SEED = 20262

# B, H, cap, N_hor, matrices, run list. Together: B 1 / 3 / 70, H 1 / 4 / 5, cap 2 / 41, every scenario running, only the
# first, only the last, every other one; the constant-velocity defaults (P never couples x and y there) and dense matrices.
FUZZ_GROUPS = (
    dict(B=1, H=1, cap=2, N=20, mats="default", run="all"),
    dict(B=3, H=4, cap=41, N=20, mats="default", run="first"),
    dict(B=3, H=5, cap=41, N=20, mats="dense", run="last"),
    dict(B=70, H=4, cap=2, N=5, mats="dense", run="alternate"),
    dict(B=70, H=1, cap=41, N=20, mats="default", run="all"),
    dict(B=70, H=5, cap=41, N=20, mats="dense", run="alternate"),
    dict(B=3, H=4, cap=41, N=5, mats="dense", run="alternate"),
    # 4 x 40 = 160 one-steps in one call from a covariance that already sits at the chain's fixed point
    dict(B=1, H=4, cap=41, N=20, mats="default", run="all", long_chain=True),
)


def golden_sequences():
    with open(os.path.join(GOLDEN, "kf_cases.json")) as fh:
        return json.load(fh)["sequences"]


def spd(rng, n, floor):
    m = rng.normal(size=(n, n))
    w, v = np.linalg.eigh(m @ m.T)
    return (v * (floor + w / w.max())) @ v.T


def fixed_point(ts=TS, steps=400):
    """The default chain's covariance after ``steps`` one-steps (stationary long before)."""
    A, C, Q, R, P = kr.default_matrices(ts)
    for _ in range(steps):
        _, P = kr.one_step(np.zeros((4, 1)), P, np.zeros((2, 1)), A, C, Q, R)
    return P


def matrices(kind, rng):
    """(A, C, Q, R): ``default`` = main_base.py:165 on model_CV(0.2); ``dense`` = a perturbed model with SPD noise
    covariances that couple every state (eigenvalues of R >= 0.5, so that S stays well conditioned)."""
    A, C, Q, R, _ = kr.default_matrices(TS)
    if kind == "dense":
        A = A + rng.normal(0, 0.01, (4, 4))
        C = C + rng.normal(0, 0.05, (2, 4))
        Q, R = spd(rng, 4, 0.3), spd(rng, 2, 0.5)
    return A, C, Q, R


def fuzz_group(g):
    """-> dict(dims, mats (A, C, Q, R), state, run): one call; ``g`` is an index into FUZZ_GROUPS, or a group of the same form
    with a ``seed`` of its own (what other test modules use for shapes the fuzz set does not hold). Per pedestrian kf_len is
    drawn from {0, 1, 2, 3, cap - 1, cap} (what fits into cap) and hcount = kf_len + {0, 1, 2}; the rows of kf_traj beyond
    kf_len hold SENTINEL."""
    d = dict(g) if isinstance(g, dict) else dict(FUZZ_GROUPS[g])
    rng = np.random.default_rng([FUZZ_SEED, d.pop("seed") if isinstance(g, dict) else g])
    B, H, cap = d["B"], d["H"], d["cap"]
    A, C, Q, R = matrices(d["mats"], rng)
    lens = sorted({n for n in (0, 1, 2, 3, cap - 1, cap) if n <= cap})
    k = np.arange(B * H).reshape(B, H)
    kf_len = np.array(lens, dtype=np.int64)[(k + rng.integers(0, len(lens))) % len(lens)]      # every value occurs where B H allows
    hcount = kf_len + (k // len(lens) + rng.integers(0, 3, (B, H))) % 3
    start = rng.uniform(-15, 15, (B, H, 1, 2))
    vel = rng.uniform(-0.3, 0.3, (B, H, 1, 2))
    walk = start + vel * np.arange(cap + 1)[None, None, :, None] + np.cumsum(rng.normal(0, 0.03, (B, H, cap + 1, 2)), axis=2)
    kf_traj = np.full((B, H, cap, 2), SENTINEL)
    humans = np.zeros((B, H, 2))
    for b in range(B):
        for h in range(H):
            n = int(kf_len[b, h])
            kf_traj[b, h, :n] = walk[b, h, :n]
            humans[b, h] = walk[b, h, n] if hcount[b, h] > n else walk[b, h, max(n - 1, 0)]
    if d.get("long_chain"):
        kf_len[:] = cap
        hcount[:] = cap
        kf_traj = walk[:, :, :cap].copy()
        humans = walk[:, :, cap - 1].copy()
        kf_P = np.tile(fixed_point(), (B, 1, 1))
    elif d["mats"] == "default":
        # a covariance of the default chain itself (block structure kept) for every other scenario, a dense one for the rest
        chain = [kr.default_matrices(TS)[4]]
        for _ in range(3):
            chain.append(kr.one_step(np.zeros((4, 1)), chain[-1], np.zeros((2, 1)), A, C, Q, R)[1])
        kf_P = np.stack([chain[b % 4] if b % 2 == 0 else spd(rng, 4, 0.2) for b in range(B)])
    else:
        kf_P = np.stack([spd(rng, 4, 0.2) for _ in range(B)])
    run = {"all": None, "first": np.array([0]), "last": np.array([B - 1]), "alternate": np.arange(0, B, 2)}[d["run"]]
    state = dict(humans=humans, hcount=hcount.astype(np.int64), kf_traj=kf_traj, kf_len=kf_len, kf_P=kf_P)
    return dict(dims=d, mats=(A, C, Q, R), state=state, run=None if run is None else run.astype(np.int64), human_size=HUMAN_SIZE)


def round_inputs(case, dtype):
    """The case with its real arrays rounded to ``dtype`` (and stored as fp64 again): what both sides of an fp32 comparison see.
    The matrices stay as they are: both sides convert them themselves."""
    T = np.dtype(dtype).type
    st = {k: (np.asarray(v, dtype=T).astype(np.float64) if k in kr.REAL_KEYS else v.copy()) for k, v in case["state"].items()}
    return dict(case, state=st)


def reference(case, dtype=np.float64):
    A, C, Q, R = case["mats"]
    return kr.predict(case["state"], case["dims"]["N"], case["human_size"], A, C, Q, R, run=case["run"], dtype=dtype)


def coord_max(state):
    """[B] largest coordinate of a scenario: pedestrians and the stored rows of their trajectories."""
    B, H, cap = state["kf_traj"].shape[:3]
    valid = np.arange(cap)[None, None, :] < state["kf_len"][:, :, None]
    tr = np.where(valid[..., None], np.abs(state["kf_traj"]), 0.0).reshape(B, -1).max(axis=1)
    return np.maximum(tr, np.abs(state["humans"]).reshape(B, -1).max(axis=1))


def fuzz_population():
    """What the fuzz set covers: {(kf_len kind, hcount - kf_len): pedestrians of running scenarios}, one-steps of the longest call."""
    counts, longest = {}, 0
    for g in range(len(FUZZ_GROUPS)):
        c = fuzz_group(g)
        s, cap = c["state"], c["dims"]["cap"]
        rows = np.arange(c["dims"]["B"]) if c["run"] is None else c["run"]
        for b in rows:
            steps = 0
            for h in range(c["dims"]["H"]):
                n, extra = int(s["kf_len"][b, h]), int(s["hcount"][b, h] - s["kf_len"][b, h])
                kind = "cap" if n == cap else "cap-1" if n == cap - 1 else str(n)
                counts[(kind, extra)] = counts.get((kind, extra), 0) + 1
                steps += max(min(n + (extra > 0), cap) - 1, 0)
            longest = max(longest, steps)
    return counts, longest


# ---- sixty steps: pre -> kf -> post with prescribed controls -------------------------------------------------------------
SIXTY_B, SIXTY_STEPS = 12, 60


def sixty_setup():
    """The first twelve of the reference scenarios of tests/step_cases.py (four pedestrians each, the 55-rectangle map) with a
    seeded smooth control sequence per robot and stagger draws: -> (loop state, kf state, list of dict(stagger, U, y))."""
    import step_cases as sc
    B, N = SIXTY_B, sc.SIXTY["N"]
    s256, _ = sc.sixty_initial("reference")
    s0 = {k: (v.copy() if k == "polys" else v[:B].copy()) for k, v in s256.items()}
    H = s0["humans"].shape[1]
    rng = np.random.default_rng([sc.SIXTY["seed"], 7])
    ph, om = rng.uniform(0, 2 * np.pi, (2, B)), rng.uniform(0.05, 0.4, (2, B))
    seq = []
    for t in range(SIXTY_STEPS):
        U = rng.uniform(-0.5, 0.5, (B, 2 * N))
        U[:, 0] = np.clip(0.65 + 0.95 * np.sin(ph[0] + om[0] * t), -0.2, 1.5)
        U[:, 1] = 0.5 * np.sin(ph[1] + om[1] * t)
        st = rng.choice([1.0, -1.0], (B, H)) * rng.integers(0, 11, (B, H)) / 10 * 0.5
        seq.append(dict(stagger=st, U=U, y=rng.uniform(-1, 1, (B, 2 * N))))
    cap = SIXTY_STEPS + 1
    kf0 = dict(kf_traj=np.full((B, H, cap, 2), SENTINEL), kf_len=np.zeros((B, H), np.int64), kf_P=np.tile(np.eye(4), (B, 1, 1)))
    return s0, kf0, seq


def sixty_reference():
    """The free-running fp64 reference loop, compaction on. -> (s0, kf0, seq, records): per step dict(run, dyn_c, kf (the three
    arrays after the call), post (loop state after the step))."""
    import step_cases as sc
    import step_reference as sr
    N, ts = sc.SIXTY["N"], sc.SIXTY["ts"]
    A, C, Q, R, _ = kr.default_matrices(ts)
    s0, kf0, seq = sixty_setup()
    s = {k: v.copy() for k, v in s0.items()}
    kf = {k: v.copy() for k, v in kf0.items()}
    B = s["robot"].shape[0]
    recs = []
    for t, c in enumerate(seq):
        alive = np.nonzero(s["alive"])[0].astype(np.int64)
        if alive.size == 0:
            break
        run = None if alive.size == B else alive
        op, _ = sr.pre(s, N, ts, sc.SIXTY["base_speed"], sc.SIXTY["lin_vel_max"], HUMAN_SIZE, run=run, gather_y=run is not None)
        s["idx_ref"] = op["idx_ref"]
        ok = kr.predict(dict(kf, humans=s["humans"], hcount=s["hcount"]), N, HUMAN_SIZE, A, C, Q, R, run=run)
        kf = {k: ok[k] for k in ("kf_traj", "kf_len", "kf_P")}
        oq, _ = sr.post(s, c["U"][alive], c["y"][alive], ts, HUMAN_SIZE, sc.HUMAN_VMAX, t, run=run, stagger=c["stagger"])
        s.update(oq)
        recs.append(dict(run=run, dyn_c=ok["dyn_c"], kf={k: v.copy() for k, v in kf.items()}, post={k: v.copy() for k, v in s.items()}))
    return s0, kf0, seq, recs
