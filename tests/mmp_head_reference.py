"""float64 restatement (test infrastructure) of the end of the multi-hypothesis predictor's network as ``nmpc_mmp_head_f32``
(csrc/nmpc_mmp_head.h) fuses it:

    p[c][i][j] = 0.25 ((x[c][2i][2j] + x[c][2i][2j+1]) + (x[c][2i+1][2j] + x[c][2i+1][2j+1])),  i < H // 2, j < W // 2
    f          = leaky(W1 flat(p) + c1, slope)            F = C (H // 2) (W // 2) -> 128, flat index (c (H // 2) + i) (W // 2) + j
    out        = W2 f + c2                                128 -> O

``head`` returns ``(out, bound)``. The bound is a running first-order error analysis in the manner of
tests/mmp_block_reference.py (u = 2^-24; a float32 sum of K products in any order, with its added constant and slope, errs by
at most c(K) u times the sum of the magnitudes, c(K) = K + 8), derived and not tuned:

    e_p   = 3 u pool(|x|)                                 three additions; the factor 0.25 is exact
    e_f   = |W1| e_p                                      the inherited error of p, through a linear map
            + c(F) u (|W1| (|p| + e_p) + |c1|)            the first sum's own; the slope (|slope| <= 1) does not enlarge it
    e_out = |W2| e_f + c(128) u (|W2| (|f| + e_f) + |c2|)

Four wrong variants serve as controls (``head(..., wrong=...)``): ``"ceil"`` pools an odd last row or column in as a partial
window (what ``ceil_mode`` gives; applies where H or W is odd); ``"order"`` flattens ``[h][w][c]`` (applies where the pooled plane
has more than one pixel); ``"sum"`` leaves the 0.25 out; ``"slope"`` leaves the activation out."""
from __future__ import annotations

import functools

import numpy as np

U = 2.0 ** -24            # unit roundoff of float32
FEATURES = 128            # outputs of the first linear layer
ROWS = 16                 # rows of the batch per workgroup of the kernel (kHeadRows)


def _c(K):
    return K + 8


def _spec(*a):
    from dyobav_mpcnwta_warehouse_amd.mmp_stem import HeadSpec
    return HeadSpec(*a)


def features(C, H, W):
    return C * (H // 2) * (W // 2)


def random_head(C, H, W, O, seed):
    """Seeded weights of both signs, non-zero constants, the reference's slope 0.01."""
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    Fn = features(C, H, W)
    w1 = f32(rng.standard_normal((FEATURES, Fn)) / np.sqrt(Fn))
    w2 = f32(rng.standard_normal((O, FEATURES)) / np.sqrt(FEATURES))
    c1 = f32(rng.uniform(0.25, 1.0, FEATURES) * np.where(np.arange(FEATURES) % 3 == 1, -1.0, 1.0))
    c2 = f32(rng.uniform(0.25, 1.0, O) * np.where(np.arange(O) % 2 == 1, -1.0, 1.0))
    return _spec(w1, c1, 0.01, w2, c2)


def integer_head(C, H, W, O, seed):
    """W1 in {-1, 0, 1} (an eighth non-zero), W2 and the constants small integers, slope 1/4: on x in multiples of 4 nothing
    rounds as long as the sums stay small (``integer_units``)."""
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    Fn = features(C, H, W)
    w1 = f32(rng.choice([-1.0, 1.0] + [0.0] * 14, (FEATURES, Fn)))
    w2 = f32(rng.integers(-2, 3, (O, FEATURES)))
    return _spec(w1, f32(rng.integers(-3, 4, FEATURES)), 0.25, w2, f32(rng.integers(-3, 4, O)))


def random_x(M, C, H, W, seed):
    return np.random.default_rng(seed).standard_normal((M, C, H, W)).astype(np.float32)


def integer_x(M, C, H, W, seed):
    """Multiples of 4 in [-8, 8] as float32: every 2 x 2 mean is an integer."""
    return (4 * np.random.default_rng(seed).integers(-2, 3, (M, C, H, W))).astype(np.float32)


def pool(x, wrong=None):
    """[M, C, H, W] float64 -> [M, C, H // 2, W // 2]; ``"ceil"``: the last window along an odd side takes the odd last row /
    column in as well (mean over its own size); ``"sum"``: no division."""
    M, C, H, W = x.shape
    Hp, Wp = H // 2, W // 2
    if wrong == "ceil":
        out = np.empty((M, C, Hp, Wp))
        for i in range(Hp):
            for j in range(Wp):
                out[:, :, i, j] = x[:, :, 2 * i:(H if i == Hp - 1 else 2 * i + 2), 2 * j:(W if j == Wp - 1 else 2 * j + 2)].mean(axis=(2, 3))
        return out
    v = x[:, :, :2 * Hp, :2 * Wp]
    s = (v[..., 0::2, 0::2] + v[..., 0::2, 1::2]) + (v[..., 1::2, 0::2] + v[..., 1::2, 1::2])
    return s if wrong == "sum" else 0.25 * s


def applies(wrong, C, H, W):
    """Whether the wrong variant differs from the definition on a [C, H, W] plane at all."""
    if wrong == "ceil":
        return H % 2 == 1 or W % 2 == 1
    if wrong == "order":
        return C > 1 and (H // 2) * (W // 2) > 1
    return True


def _forward(x, w1, c1, w2, c2, slope, wrong):
    M = x.shape[0]
    p = pool(x, wrong if wrong in ("ceil", "sum") else None)
    flat = p.transpose(0, 2, 3, 1).reshape(M, -1) if wrong == "order" else p.reshape(M, -1)
    v = flat @ w1.T + c1
    f = v if wrong == "slope" else np.where(v > 0, v, slope * v)
    return flat, f, f @ w2.T + c2


def head(x, spec, wrong=None):
    """x [M, C, H, W], spec a HeadSpec (any float type, used as float64) -> (out, bound) [M, O] float64; the bound is always the
    definition's, whatever ``wrong`` computes."""
    x = np.asarray(x, dtype=np.float64)
    w1, c1, w2, c2 = (np.asarray(a, dtype=np.float64) for a in (spec.w1, spec.c1, spec.w2, spec.c2))
    flat, f, out = _forward(x, w1, c1, w2, c2, float(spec.slope), None)
    e_p = 3 * U * pool(np.abs(x)).reshape(x.shape[0], -1)
    e_f = e_p @ np.abs(w1).T + _c(w1.shape[1]) * U * ((np.abs(flat) + e_p) @ np.abs(w1).T + np.abs(c1))
    bound = e_f @ np.abs(w2).T + _c(FEATURES) * U * ((np.abs(f) + e_f) @ np.abs(w2).T + np.abs(c2))
    if wrong is not None:
        out = _forward(x, w1, c1, w2, c2, float(spec.slope), wrong)[2]
    return out, bound


def integer_units(x, spec):
    """For ``integer_head`` on ``integer_x``: the largest magnitude any partial sum or intermediate value can take, in units of its
    own last place (from the absolute values, so for every order of summation). x is in units of 4 and the window sums in
    units of 4 too; p is an integer; f in units of 1/4 (the slope); out in units of 1/4. Below 2^24 float32 holds all of them."""
    xa = np.abs(np.asarray(x, dtype=np.float64))
    w1, c1, w2, c2 = (np.abs(np.asarray(a, dtype=np.float64)) for a in (spec.w1, spec.c1, spec.w2, spec.c2))
    M = xa.shape[0]
    S0 = pool(xa, "sum")                                     # the window sums, multiples of 4
    P = 0.25 * S0
    A1 = P.reshape(M, -1) @ w1.T + c1                        # integers
    A2 = A1 @ w2.T + c2                                      # in units of 1/4
    return float(max(S0.max() / 4, A1.max() * 4, A2.max() * 4))


def torch_float32(x, spec):
    """torch's own float32 AvgPool2d, Linear and LeakyReLU on the CPU: a correct fp32 implementation, as a control."""
    import torch
    import torch.nn.functional as F
    t = lambda a: torch.as_tensor(np.array(a, dtype=np.float32))
    p = F.avg_pool2d(t(x), 2, 2)
    f = F.leaky_relu(F.linear(p.reshape(p.shape[0], -1), t(spec.w1), t(spec.c1)), float(spec.slope))
    return F.linear(f, t(spec.w2), t(spec.c2)).numpy()


# (C, H, W): the smallest plane; a row and a column dropped; a wide odd plane; the warehouse plane of layer4
PLANES = ((8, 2, 2), (8, 3, 3), (16, 4, 7), (128, 10, 11))
OUTPUTS = (2, 40, 512)
ROWS_M = (1, 3, 2 * ROWS + 1)                               # one more than two of the kernel's row groups
M_MAX = max(ROWS_M)
CASES = tuple(p + (O,) for p in PLANES for O in OUTPUTS)
case_id = lambda c: f"c{c[0]}-{c[1]}x{c[2]}-o{c[3]}"


@functools.lru_cache(maxsize=None)
def case(kind, C, H, W, O, M=M_MAX):
    """(x, spec, out, bound) of a seeded case, computed once and shared (read-only). A call with fewer rows takes the first rows."""
    seed = 100000 * C + 1000 * H + 10 * W + O
    if kind == "random":
        x, spec = random_x(M, C, H, W, seed), random_head(C, H, W, O, seed + 1)
    else:
        x, spec = integer_x(M, C, H, W, seed), integer_head(C, H, W, O, seed + 1)
    out, bound = head(x, spec)
    for a in (x, out, bound):
        a.setflags(write=False)
    return x, spec, out, bound
