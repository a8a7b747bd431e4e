"""Inputs of the hypothesis-clustering tests (tests/test_hypotheses_cpu.py, tests/test_gpu_hypotheses_sweep.py and
tests/fuzz_hypotheses.py share them, so that what the CPU test establishes about oracle/hypotheses.py against sklearn
holds for the very inputs the GPU tests use). numpy only; deterministic given the seed.

Every generator is called as ``gen(B, N, P, H, eps=..., seed=..., dtype=...)`` and returns ``(hypos[B,N,P,2], cur[B,H,2])``
as float64 arrays whose values are exactly representable in ``dtype`` (the type the kernel under test will read them
in), so the reference and the kernel see the same numbers.

Near-tie guard of the random families: the kernels evaluate ``dx*dx + dy*dy <= eps*eps`` in ``dtype`` with contraction
allowed, so their squared distance may differ from numpy's in the last places. A pair within rounding of ``eps**2`` is a
case where the reference itself is not stable; a time offset with a pair at ``|d2 - eps2| <= 16 u eps2`` (u = unit
roundoff of ``dtype``) is drawn again -- replaced, not skipped or masked. At most 2 % of the offsets of a case may be
redrawn (asserted); ``STATS`` records the share of the last call. The lattice family is exempt: its coordinates are
integers times a power of two, so differences, squares and their sums are exact in float32 and float64 with or without
fused multiply-add, and its many pairs at exactly ``d2 == eps2`` are the point."""
import numpy as np

FAR = 1.0e3                       # clusters "far from the origin"
STATS = {"resampled": 0, "offsets": 0, "share": 0.0}
FAMILIES = ("blobs", "chains", "lattice", "duplicates", "slots", "holes")


def unit_roundoff(dtype):
    return 2.0 ** -24 if np.dtype(dtype) == np.float32 else 2.0 ** -53


def as_seen(x, dtype):
    """x as ``dtype`` holds it, back in float64."""
    return np.asarray(x, dtype=np.float64).astype(dtype).astype(np.float64)


def near_tie(pts, eps, dtype):
    """Any pair of pts[P,2] whose squared distance lies within 16 u eps^2 of eps^2."""
    d = pts[:, None, :] - pts[None, :, :]
    d2 = (d * d).sum(axis=2)
    e2 = eps * eps
    return bool((np.abs(d2 - e2) <= 16.0 * unit_roundoff(dtype) * e2).any())


def _assemble(B, N, P, H, eps, seed, dtype, offset_fn, guard=True, cur_scale=4.0):
    """offset_fn(rng, b, t) -> pts[P,2]; rounds to dtype, redraws near-tie offsets, draws the current positions."""
    rng = np.random.default_rng(seed)
    hypos = np.empty((B, N, P, 2))
    resampled = 0
    for b in range(B):
        for t in range(N):
            for _ in range(50):
                pts = as_seen(offset_fn(rng, b, t), dtype)
                assert pts.shape == (P, 2), pts.shape
                if not guard or not near_tie(pts, eps, dtype):
                    break
                resampled += 1
            else:
                raise AssertionError("no offset without a near-tie in 50 draws")
            hypos[b, t] = pts
    STATS.update(resampled=resampled, offsets=B * N, share=resampled / float(B * N))
    assert resampled <= 0.02 * B * N, f"{resampled} of {B * N} time offsets redrawn by the near-tie guard (> 2 %)"
    cur = as_seen(rng.uniform(-cur_scale, cur_scale, (B, H, 2)), dtype)
    return hypos, cur


# ---- blobs and chains (the two families of test_point_counts_and_chain_clusters) --------------------------------------
def blobs(B, N, P, H, eps=1.0, seed=0, dtype=np.float64):
    """Points around three centres (sigma 0.3 eps): a few large clusters, occasionally a stray noise point."""
    def off(rng, b, t):
        ctr = rng.uniform(-6, 6, (3, 2)) * eps
        pts = ctr[rng.integers(0, 3, P)] + rng.normal(0, 0.3 * eps, (P, 2))
        return pts[rng.permutation(P)]
    return _assemble(B, N, P, H, eps, seed, dtype, off)


def chains(B, N, P, H, eps=1.0, seed=0, dtype=np.float64):
    """A chain of 1..P points 0.9 eps apart in shuffled order (the component is only found through paths as long as the
    chain), the rest scattered."""
    def off(rng, b, t):
        n1 = int(rng.integers(1, P + 1))
        chain = np.c_[np.arange(n1) * 0.9 * eps, np.zeros(n1)] + rng.uniform(-3, 3, 2) * eps
        rest = rng.uniform(20, 60, (P - n1, 2)) * eps
        return np.r_[chain, rest][rng.permutation(P)]
    return _assemble(B, N, P, H, eps, seed, dtype, off)


# ---- exact ties ------------------------------------------------------------------------------------------------------
def lattice(B, N, P, H, eps=1.0, seed=0, dtype=np.float64, s=1.0, span=12):
    """Integer lattice points times the power of two ``s``: every squared distance is exact, many are exactly eps^2
    (eps = 1 with s = 1, eps = 0.5 with s = 0.25, and the 3-4-5 pairs at eps = 5)."""
    assert s in (1.0, 0.5, 0.25, 0.125)
    def off(rng, b, t):
        return rng.integers(-span, span + 1, (P, 2)) * s
    hypos, cur = _assemble(B, N, P, H, eps, seed, dtype, off, guard=False)
    assert (hypos.astype(np.float32).astype(np.float64) == hypos).all()        # float32(x) == x for every coordinate
    return hypos, cur


# ---- duplicates ------------------------------------------------------------------------------------------------------
def _cells(rng, k, eps, pitch=5.0):
    """k distinct cell centres of a grid with pitch 5 eps (groups below stay within 1.2 eps of their centre, so that
    points of different groups are at least 2.6 eps apart)."""
    side = max(4, int(np.ceil(np.sqrt(2.0 * k))))
    idx = rng.permutation(side * side)[:k]
    return np.stack([idx % side - side // 2, idx // side - side // 2], axis=1) * (pitch * eps)


def _group(rng, kind, n, ctr, eps):
    """n points of one group around ctr: 0 identical points, 1 same x (std_x == 0), 2 same y, 3 an ordinary cluster,
    4 a single noise point (n == 1)."""
    if kind == 0 or n == 1:
        return np.tile(ctr + rng.uniform(-0.5, 0.5, 2) * eps, (n, 1))
    if kind in (1, 2):
        # neighbours at most 0.4 eps apart, the whole line at most 2 eps long, no multiple of the spacing equal to eps
        line = (rng.permutation(n) - (n - 1) / 2.0) * min(0.4, 2.0 / (n + 0.37)) * eps
        pts = np.tile(ctr, (n, 1)).astype(float)
        pts[:, 2 - kind] += line
        return pts
    return ctr + np.clip(rng.normal(0, 0.25 * eps, (n, 2)), -0.45 * eps, 0.45 * eps)


def duplicates(B, N, P, H, eps=1.0, seed=0, dtype=np.float64):
    """Clusters of 2..P identical points (population std exactly 0 in both coordinates), clusters whose points differ in
    one coordinate only (one std exactly 0), ordinary clusters and single noise points; about a third of the groups sit
    near (+-1e3, +-1e3). Points in shuffled order."""
    def off(rng, b, t):
        sizes, left = [], P
        while left > 0:
            if not sizes and rng.random() < 0.1:
                n = P
            else:
                n = int(min(left, rng.choice([1, 2, 2, 3, 4, rng.integers(2, P // 3 + 3)])))
            sizes.append(n)
            left -= n
        ctrs = _cells(rng, len(sizes), eps)
        out = []
        for n, c in zip(sizes, ctrs):
            if rng.random() < 0.35:
                c = c + FAR * rng.choice([-1.0, 1.0], 2)
            out.append(_group(rng, int(rng.integers(0, 4)), n, c, eps))
        return np.concatenate(out)[rng.permutation(P)]
    return _assemble(B, N, P, H, eps, seed, dtype, off)


# ---- register slots of the wide kernels --------------------------------------------------------------------------------
def slots(B, N, P, H, eps=1.0, seed=0, dtype=np.float64, n_noise=64, first=None, n_clusters=None):
    """The first ``n_noise`` points are isolated noise (on a grid with pitch 3.5 eps, at least 3 eps apart, far from
    everything else); the clusters sit among the later points, so their first points lie in later register slots of the wide kernels. With ``first`` and
    ``n_clusters`` set, the first points of ``n_clusters`` clusters are the consecutive points first, first + 1, ...
    (choose them to straddle a multiple of 64 and n_clusters > Ndynobs: truncation then happens in the middle of a
    register slot); the clusters' other points follow, everything before ``first`` is noise. The point order is the case
    and is not shuffled."""
    if first is not None:
        n_noise = first
    def off(rng, b, t):
        k = np.arange(n_noise)
        noise = np.stack([200.0 + 3.5 * (k % 16), 200.0 + 3.5 * (k // 16)], axis=1) * eps + rng.uniform(-0.2, 0.2, (n_noise, 2)) * eps
        room = P - n_noise
        if first is not None:
            nc = n_clusters
            assert room >= 2 * nc, (P, first, nc)
        else:
            nc = int(rng.integers(1, max(2, min(room // 2, 12)) + 1)) if room >= 2 else 0
        ctrs = _cells(rng, nc + 1, eps)
        lead = ctrs[:nc] + rng.uniform(-0.3, 0.3, (nc, 2)) * eps
        extra = room - nc                                   # points after the clusters' first points
        owner = np.r_[np.arange(nc), rng.integers(0, max(nc, 1), max(extra - nc, 0))][:extra] if nc else np.zeros(0, int)
        rest = lead[owner] + rng.uniform(-0.3, 0.3, (len(owner), 2)) * eps if nc else np.zeros((0, 2))
        if nc == 0 and room:                                # one point left over: one more isolated point
            rest = ctrs[:1] + np.zeros((room, 2))
            rest[:, 0] += 3.5 * eps * np.arange(room)
        return np.concatenate([noise, lead, rest])
    return _assemble(B, N, P, H, eps, seed, dtype, off)


# ---- empty and full --------------------------------------------------------------------------------------------------
def holes(B, N, P, H, eps=1.0, seed=0, dtype=np.float64, max_clusters=4, p_empty=0.4):
    """At some time offsets every point is noise (pitch 3.5 eps), at the others there are 1..max_clusters clusters (never
    more), exactly max_clusters at one offset of every instance: used obstacle slots then have [0,0,0,0,0,1] holes, and with
    H > max_clusters every cluster count stays below H."""
    peak = np.random.default_rng(seed + 1).integers(0, N, B)
    def off(rng, b, t):
        nc = max_clusters if t == peak[b] else (0 if rng.random() < p_empty else int(rng.integers(1, max_clusters + 1)))
        nc = min(nc, P // 2)
        if nc == 0:
            k = rng.permutation(P)
            return np.stack([3.5 * (k % 16), 3.5 * (k // 16)], axis=1) * eps + rng.uniform(-0.2, 0.2, (P, 2)) * eps
        ctrs = _cells(rng, nc, eps)
        owner = np.r_[np.arange(nc), np.arange(nc), rng.integers(0, nc, P - 2 * nc)]
        pts = ctrs[owner] + rng.uniform(-0.3, 0.3, (P, 2)) * eps
        return pts[rng.permutation(P)]
    return _assemble(B, N, P, H, eps, seed, dtype, off)


def generate(family, B, N, P, H, eps=1.0, seed=0, dtype=np.float64, Ndyn=None):
    """One case of ``family`` at any shape (the fuzz driver and the CPU cross-check call this): family-specific arguments
    are chosen from the shape."""
    if family == "lattice":
        s = {1.0: 1.0, 5.0: 1.0, 0.5: 0.25}.get(eps)
        assert s is not None, "lattice ties need eps in {1, 5, 0.5}"
        return lattice(B, N, P, H, eps, seed, dtype, s=s, span=12 if P <= 80 else 40)
    if family == "slots":
        if P < 4:
            return blobs(B, N, P, H, eps, seed, dtype)
        n_noise = 64 * ((P - 2) // 64) if P > 66 else (P - 2) // 2
        if Ndyn is not None and P - n_noise >= 2 * (Ndyn + 2) + 3 and n_noise >= 3:
            return slots(B, N, P, H, eps, seed, dtype, first=n_noise - min(3, Ndyn), n_clusters=Ndyn + 2)
        return slots(B, N, P, H, eps, seed, dtype, n_noise=n_noise)
    if family == "holes":
        return holes(B, N, P, H, eps, seed, dtype, max_clusters=max(1, min(4, P // 2)))
    return {"blobs": blobs, "chains": chains, "duplicates": duplicates}[family](B, N, P, H, eps, seed, dtype)


# ---- parameters and the case lists shared by the CPU cross-check and the GPU sweep ---------------------------------------
DEFAULT = dict(human_size=0.2, eps=1.0, enlarge=2.0, extra_margin=0.0)
# non-default (eps, enlarge, extra_margin, human_size); enlarge and extra_margin are exact in float32, so that the float32
# kernel and the float64 reference work with the same factors
PARAM_SETS = (dict(human_size=0.3, eps=1.0, enlarge=1.5, extra_margin=0.25),
              dict(human_size=0.2, eps=2.0, enlarge=1.0, extra_margin=0.0),
              dict(human_size=0.5, eps=0.5, enlarge=2.5, extra_margin=0.125))
# one point count per kernel: hypotheses_kernel<T, unsigned>, <T, unsigned long long>, hypotheses_wide_kernel<T, 2 | 3 | 4>
KERNEL_P = {"narrow32": 24, "narrow64": 50, "wide2": 100, "wide3": 180, "wide4": 250}


def kernel_of(P):
    return "narrow32" if P <= 32 else "narrow64" if P <= 64 else "wide2" if P <= 128 else "wide3" if P <= 192 else "wide4"


def family_cases():
    """Every generator family on a kernel of every type, the parameter sets cycled through: dicts with family, N, Ndyn,
    H, P, B, par, seed."""
    out, k = [], 0
    for fi, fam in enumerate(FAMILIES):
        for ki, (kern, P) in enumerate(KERNEL_P.items()):
            par = dict(((DEFAULT,) + PARAM_SETS)[(fi + ki) % 4])
            if fam == "lattice":
                par["eps"] = (1.0, 5.0, 0.5)[ki % 3]
            N = (3, 5, 4, 7, 6)[ki]
            Ndyn = 6 if fam in ("slots", "duplicates") else 9
            out.append(dict(family=fam, kernel=kern, N=N, Ndyn=Ndyn, H=(2, 0, 5, 1, 3)[(fi + ki) % 5], P=P, B=4, par=par,
                            seed=1000 + k))
            k += 1
    return out


def case_inputs(c, dtype):
    return generate(c["family"], c["B"], c["N"], c["P"], c["H"], c["par"]["eps"], c["seed"], dtype, Ndyn=c["Ndyn"])


# ---- clusters without the reference's search, and the a-priori float32 bound ----------------------------------------------
def components(pts, eps):
    """Clusters of DBSCAN(eps, min_samples = 2) as a list of index arrays, in the order of their smallest index: boolean
    closure of the ``d2 <= eps2`` graph by repeated squaring (independent of oracle.hypotheses.dbscan_min2's search)."""
    d = pts[:, None, :] - pts[None, :, :]
    adj = ((d) ** 2).sum(axis=2) <= eps * eps
    reach = adj
    while True:
        f = reach.astype(np.float32)
        nxt = (f @ f) > 0
        if (nxt == reach).all():
            break
        reach = nxt
    first = reach.argmax(axis=1)
    clustered = adj.sum(axis=1) >= 2
    return [np.nonzero(clustered & (first == l))[0] for l in np.unique(first[clustered])]


def f32_bounds(hypos, par, Ndyn, atol_ref):
    """A-priori bound on |kernel - reference| for every element of one instance's float32 output, [Ndyn][N+1][6], from the
    inputs alone (the values in ``hypos`` are exact float32 numbers). Zero where the kernel must be exact (it copies or
    writes constants there), except for the reference's own rounding ``atol_ref``, which is added everywhere.

    Notation: u = 2^-24 (round to nearest: every float32 operation, division and square root included, has relative
    error at most u); a cluster has n points; d_j = x_j - x_first, |d_j| <= R (per coordinate), d_first = 0.
    The kernel computes dx_j = fl(x_j - x_first) (relative error u), sums them in point order (exact zeros for the
    points outside the cluster and for the first point: n - 1 terms, n - 2 inexact additions, so the sum is off by at most
    (n - 2) u sum|d_j| + u sum|d_j|), multiplies by fl(1 / n) (2 u more) and adds x_first (u |mean|):
        |d mean| <= ((n - 2) + 1 + 2) u (n - 1) R / n + u |mean|  <=  (n + 2) u R + u |mean|.
    Variance: fl(dx_j^2) carries 3 u (two from dx_j, one from the product or the fused sum), the sum of n - 1 non-negative
    terms (n - 2) u, the product with fl(1 / n) 2 u: (n + 3) u S2 with S2 = sum d_j^2 / n <= R^2 (n - 1) / n. The mean of
    the d_j is off by at most (n + 1) u R (n - 1) / n and is at most R (n - 1) / n in size, so its square is off by at most
    (2 (n + 1) + 1) u R^2 ((n - 1) / n)^2; the subtraction adds u var <= u R^2. Together less than (3 n + 3) u R^2; the square
    root and the product with ``enlarge`` add 2 u std <= 2 u R^2 / std, i.e. two more units in the same constant when the
    error is carried through the square root, and the terms of second order in u are below 3 n u < 5e-5 of the whole:
        |d var| <= (3 n + 6) u R^2   (square root and enlarge roundings included)
        |d radius| <= enlarge min(sqrt(d var), d var / std_ref) + u |radius|      (the last addition)
    (|sqrt(a) - sqrt(b)| <= sqrt|a - b| and = |a - b| / (sqrt(a) + sqrt(b)); the clamp of a negative variance to zero only
    moves the value towards the non-negative truth.)"""
    u = 2.0 ** -24
    N, P = hypos.shape[0], hypos.shape[1]
    bound = np.full((Ndyn, N + 1, 6), float(atol_ref))
    for t in range(N):
        for c, idx in enumerate(components(hypos[t], par["eps"])[:Ndyn]):
            pts = hypos[t][idx]
            n = len(idx)
            R = np.abs(pts - pts[0]).max(axis=0)
            mean, std = pts.mean(axis=0), pts.std(axis=0)
            dvar = (3 * n + 6) * u * R * R
            with np.errstate(divide="ignore", invalid="ignore"):
                dsd = np.minimum(np.sqrt(dvar), np.where(std > 0, dvar / std, np.inf))
            radius = std * par["enlarge"] + par["extra_margin"]
            bound[c, t + 1, 0:2] += (n + 2) * u * R + u * np.abs(mean)
            bound[c, t + 1, 2:4] += par["enlarge"] * dsd + u * np.abs(radius)
    return bound


def degenerate_rows(hypos, par, Ndyn):
    """[(slot, t + 1, point, zero_x, zero_y)] for the clusters of one instance whose points agree in x, in y or in both:
    the kernel must return exactly ``extra_margin`` as that radius, and for identical points the point itself as the mean."""
    out = []
    for t in range(hypos.shape[0]):
        for c, idx in enumerate(components(hypos[t], par["eps"])[:Ndyn]):
            same = (hypos[t][idx] == hypos[t][idx[0]]).all(axis=0)
            if same.any():
                out.append((c, t + 1, hypos[t][idx[0]], bool(same[0]), bool(same[1])))
    return out
