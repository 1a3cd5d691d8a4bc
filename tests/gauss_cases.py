"""Shared case tables, inputs, float64 references and error bars of
tests/test_gpu_gauss.py (GPU) and tests/test_gauss_cases.py (CPU): the Gaussian
likelihood and LayerNorm kernels of csrc/latent_kernels.hip (gauss_stats_kernel,
gauss_loglik_kernel, gauss_backward_kernel, ln_backward_kernel).  Plain helper
module: no test is collected from it.

Inputs are seeded from the case alone, rounded to f32 and widened back, so the
device sees exactly what the float64 reference sees.  The references are the
reference's own form ((x - mu)^2 per frame, no frame sums), never the kernel's.

Bars.  Every bar is  2^-23 |ref|  (one f32 rounding of the result, doubled, as
mmb2_cases.sum_bar doubles)  plus the accumulated rounding of the kernel's own
arithmetic, doubled as well, u64 = 2^-53, u32 = 2^-24:

  stats    2 T u64 sum_t |term|            (f64 results: no f32 part; T - 1
                                           additions and the rounding of m x x)
  lp       2 (T + F_k) u64 S               S = sum_{t,f} |m| (|log|s| + log(2 pi)/2|
                                           + (x^2 + 2 |mu x| + mu^2) / (2 s^2))
  dmu      2 (T + 5) u64 |up| (sum_t |m x| + |mu| M0) / s^2
  dsigma   2 (T + 11) u64 |up| (M0 / |s| + (M2 + 2 |mu| sum_t |m x| + mu^2 M0) / |s|^3)
  LN dx    2 (chain + 12) u32 rstd (|g| + (sum |g| + |xhat| sum |g xhat|) / d),
           g = dy gamma, chain = ceil(d / 64) + 6 (a lane's sum, the shuffle tree)
  dgamma   2 (ceil(n / 4) + 5) u32 sum_r |dy xhat|
  dbeta    2 (ceil(n / 4) + 2) u32 sum_r |dy|

The counts are read off the kernels.  After the T-term frame sums, dmu takes 5
roundings (mu M0, the subtraction, s s, the product with dlp, the division) and
dsigma 11 (mu M1, mu mu and its product with M0, the two additions of q, s s
and s s s, q / s^3, M0 / s, their sum, the product with dlp).
The worst term of a dx element, rstd xhat b / d, carries one chain and 12
roundings: xhat (2), a term of b (g, xhat (2), their product), xhat b, the
addition to a, 1 / d and the product with it, the subtraction, the product
with rstd; the bar gives every term that many.  A dgamma term is three
roundings and the four row groups meet in two more additions; dbeta's terms
are exact.  The sums of
magnitudes (sum_t |m x| where the kernel holds M1, sum |g| where it holds
sum g) are what a running sum's rounding is bounded by, so the bars use them.
Where losses.get_normal_log_prob returns the 0-d sum over the batch (the
.squeeze() of losses.py:33) torch adds B f32 rows: the rows' bars add up, plus
2 (B - 1) u32 sum_b |lp_b|.
"""
from __future__ import annotations

import collections
import copy
import functools
import math

import numpy as np
import torch

import models
from oracle import latent_oracle as LO

U32 = 2.0 ** -24
U64 = 2.0 ** -53
HL2PI = 0.5 * math.log(2.0 * math.pi)
POISON_BITS = 0x7FC0BEEF  # a quiet NaN with a payload: compared as bits
LN_EPS = 1e-5

# the bars tests/test_gpu_latent.py states
LP_RTOL, LP_ATOL, GRAD_TOL = 2e-5, 1e-4, 2e-4


def f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def _freeze(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)


# ---------------------------------------------------------------- references
def _mask_of(mask, shape):
    return np.ones(shape) if mask is None else np.broadcast_to(np.asarray(mask, np.float64), shape)


def normal_reference(mu, sigma, x, mask, up):
    """losses.py:13-33 in float64, per row: lp [B] of mu, sigma [B, F], x
    [B, T, F], mask broadcastable to x (None: ones), and the closed-form dmu,
    dsigma [B, F] of sum_b up_b lp_b."""
    m = _mask_of(mask, x.shape)
    mu3, s3 = mu[:, None, :], sigma[:, None, :]
    d = x - mu3
    var = s3 * s3
    lp = ((-0.5 * np.log(2.0 * math.pi * var) - d * d / (2.0 * var)) * m).sum((1, 2))
    dmu = up[:, None] * (m * d / var).sum(1)
    dsigma = up[:, None] * (m * (-1.0 / s3 + d * d / (var * s3))).sum(1)
    return lp, dmu, dsigma


def normal_bars(mu, sigma, x, mask, up, ref):
    """(lp [B], dmu [B, F], dsigma [B, F]) bars of the module docstring for
    ref = normal_reference(...)."""
    lp, dmu, dsigma = ref
    T, F = x.shape[1], x.shape[2]
    am = np.abs(_mask_of(mask, x.shape))
    a0, a1, a2 = am.sum(1), (am * np.abs(x)).sum(1), (am * x * x).sum(1)
    s1, amu, aup = np.abs(sigma), np.abs(mu), np.abs(up)[:, None]
    q = a2 + 2.0 * amu * a1 + mu * mu * a0
    S = (a0 * np.abs(np.log(s1) + HL2PI) + q / (2.0 * s1 * s1)).sum(1)
    return (2 * U32 * np.abs(lp) + 2 * (T + F) * U64 * S,
            2 * U32 * np.abs(dmu) + 2 * (T + 5) * U64 * aup * (a1 + amu * a0) / (s1 * s1),
            2 * U32 * np.abs(dsigma) + 2 * (T + 11) * U64 * aup * (a0 / s1 + q / s1 ** 3))


def stats_reference(x, mask):
    """(stats [N, 3, F], bar [N, 3, F]): M0 | M1 | M2 = sum_t m, m x, m x^2,
    accumulated in extended precision (the bar is of the order of a float64
    sum's own rounding) and rounded to float64 once."""
    xl = np.asarray(x, np.longdouble)
    ml = np.ones(x.shape, np.longdouble) if mask is None else \
        np.broadcast_to(np.asarray(mask, np.longdouble), x.shape)
    terms = [ml, ml * xl, ml * xl * xl]
    st = np.stack([t.sum(1) for t in terms], 1).astype(np.float64)
    T = x.shape[1]
    bar = np.stack([np.abs(t).sum(1) for t in terms], 1).astype(np.float64) * (2 * T * U64)
    return st, bar


def layer_norm_backward_reference(dy, x, mean32, rstd32, gamma):
    """dx [n, d], dgamma [d], dbeta [d] in float64 from the GIVEN f32 row
    statistics (the kernel's contract: they are the forward's, torch's), and
    their bars."""
    n, d = x.shape
    g = dy * gamma
    xh = (x - mean32[:, None]) * rstd32[:, None]
    a, b = g.sum(1, keepdims=True), (g * xh).sum(1, keepdims=True)
    rs = rstd32[:, None]
    dx = rs * (g - (a + xh * b) / d)
    dgamma, dbeta = (dy * xh).sum(0), dy.sum(0)
    chain = -(-d // 64) + 6
    mag = np.abs(rs) * (np.abs(g) + (np.abs(g).sum(1, keepdims=True) +
                                     np.abs(xh) * np.abs(g * xh).sum(1, keepdims=True)) / d)
    rows = -(-n // 4)
    bars = (2 * U32 * np.abs(dx) + 2 * (chain + 12) * U32 * mag,
            2 * U32 * np.abs(dgamma) + 2 * (rows + 5) * U32 * np.abs(dy * xh).sum(0),
            2 * U32 * np.abs(dbeta) + 2 * (rows + 2) * U32 * np.abs(dy).sum(0))
    return (dx, dgamma, dbeta), bars


# ---------------------------------------------------------------- families A and B
MASKS = ("none", "01", "frac", "bcast")
GaussCase = collections.namedtuple("GaussCase", "B T F mask neg offset spread")


def _a(B, T, F, mask="01", neg=False):
    return GaussCase(B, T, F, mask, neg, 0.0, 1.0)


BASE = (16, 12, 37)
SQUEEZE_SHAPES = [(B, T, F) for B in (1, 5) for T in (1, 12) for F in (1, 37)]
FAMILY_A = (
    [_a(*BASE)] +
    [_a(16, 12, F) for F in (255, 256, 257, 421, 1)] +   # the block's 256 threads; f += blockDim.x
    [_a(5, 1357, 64)] +                                  # POM's length
    [_a(*s) for s in SQUEEZE_SHAPES] +
    [_a(*BASE, mask=m) for m in ("none", "frac", "bcast")] +
    [_a(16, 12, 257, mask=m) for m in ("none", "frac", "bcast")] +
    [_a(*BASE, neg=True), _a(16, 12, 257, mask="frac", neg=True), _a(5, 1, 37, neg=True)])
# features 30 to 1000 spreads away from zero: M2 - 2 mu M1 + mu^2 M0 cancels
OFFSETS = [(0.0, 1.0), (30.0, 0.05), (100.0, 0.05), (1000.0, 0.5)]
FAMILY_B = [GaussCase(9, 20, 300, "01", False, o, s) for o, s in OFFSETS]
EMPTY_SHAPES = [(0, 12, 37), (5, 0, 37)]


def gauss_id(c):
    return (f"B{c.B}-T{c.T}-F{c.F}-{c.mask}" + ("-neg" if c.neg else "") +
            (f"-off{c.offset:g}-spread{c.spread:g}" if c.offset or c.spread != 1.0 else ""))


def squeezed(shape):
    """losses.py:33 sums the last two axes of the SQUEEZED [B, T, F]: with
    fewer than three non-unit axes the batch goes too (a 0-d result)."""
    return sum(1 for s in shape if s != 1) < 3


def make_mask(rng, kind, B, T, F):
    if kind == "none":
        return None
    if kind == "frac":
        return f32(1.0 - rng.random((B, T, F)))  # (0, 1]
    if kind == "bcast":
        return (rng.random((B, T, 1)) > 0.3).astype(np.float64)
    m = (rng.random((B, T, F)) > 0.3).astype(np.float64)
    if B > 1:
        m[1] = 0.0      # an utterance without frames
    if F > 1:
        m[:, :, 0] = 0.0  # a feature never observed
    return m


def make_gauss_inputs(c):
    """x = c_f + spread N(0, 1), mu likewise, sigma = spread U(0.5, 2) (a third
    negative where c.neg), c_f = offset N(0, 1); up [B] N(0, 1)."""
    rng = np.random.default_rng([c.B, c.T, c.F, MASKS.index(c.mask), int(c.neg), int(c.offset),
                                 int(round(100 * c.spread))])
    cf = c.offset * rng.standard_normal(c.F)
    z = {"x": f32(cf + c.spread * rng.standard_normal((c.B, c.T, c.F))),
         "mu": f32(cf + c.spread * rng.standard_normal((c.B, c.F))),
         "sigma": f32(c.spread * rng.uniform(0.5, 2.0, (c.B, c.F))),
         "mask": make_mask(rng, c.mask, c.B, c.T, c.F),
         "up": f32(rng.standard_normal(c.B))}
    if c.neg:
        z["sigma"] = np.where(rng.random((c.B, c.F)) < 1.0 / 3.0, -z["sigma"], z["sigma"])
    return z


@functools.lru_cache(maxsize=None)
def gauss_reference(c):
    """(inputs, ref, bar) of a family A / B case as losses.get_normal_log_prob
    returns it: ref / bar = dict(lp, dmu, dsigma); lp is [B], or the 0-d sum
    where the shape squeezes, the gradients those of lp up (up[0] then)."""
    z = make_gauss_inputs(c)
    sq = squeezed((c.B, c.T, c.F))
    up = np.full(c.B, z["up"][0]) if sq else z["up"]
    ref = normal_reference(z["mu"], z["sigma"], z["x"], z["mask"], up)
    bar = normal_bars(z["mu"], z["sigma"], z["x"], z["mask"], up, ref)
    lp, lp_bar = ref[0], bar[0]
    if sq:
        lp_bar = np.asarray(lp_bar.sum() + 2 * (c.B - 1) * U32 * np.abs(lp).sum())
        lp = np.asarray(lp.sum())
    ref = {"lp": lp, "dmu": ref[1], "dsigma": ref[2], "lp_rows": ref[0]}
    bar = {"lp": lp_bar, "dmu": bar[1], "dsigma": bar[2], "lp_rows": bar[0]}
    _freeze(*z.values(), *ref.values(), *bar.values())
    return z, ref, bar


# what the kernels compute, restated in numpy with chosen accumulators (CPU
# tests only: the condition the bars rest on, and their teeth)
def block_sum_f32(terms):
    """gauss_loglik_kernel's feature sum with an f32 accumulator: thread j adds
    f = j, j + 256, ..; xor butterfly over 64 lanes; the four waves in order."""
    B, F = terms.shape
    n = -(-F // 256)
    pad = np.zeros((B, n * 256), np.float32)
    pad[:, :F] = terms.astype(np.float32)
    acc = np.zeros((B, 256), np.float32)
    for j in range(n):
        acc = acc + pad[:, j * 256:(j + 1) * 256]
    w = acc.reshape(B, 4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, :, np.arange(64) ^ o]
    return (((w[:, 0, 0] + w[:, 1, 0]) + w[:, 2, 0]) + w[:, 3, 0]).astype(np.float64)


def kernel_route_lp(mu, sigma, x, mask, stat_dtype=np.float64, feat_f32=False):
    """lp [B] by the kernels' route: running frame sums M0, M1, M2 kept in
    stat_dtype, q = M2 - 2 mu M1 + mu^2 M0 and the terms in float64, the
    features summed in float64, by block_sum_f32 (feat_f32 = True) or by a plain
    f32 running sum (feat_f32 = "loop")."""
    B, T, F = x.shape
    m = _mask_of(mask, x.shape)
    m0, m1, m2 = (np.zeros((B, F), stat_dtype) for _ in range(3))
    for t in range(T):
        v, mm = x[:, t].astype(stat_dtype), m[:, t].astype(stat_dtype)
        m0 = m0 + mm
        m1 = m1 + mm * v
        m2 = m2 + mm * v * v
    m0, m1, m2 = (a.astype(np.float64) for a in (m0, m1, m2))
    q = m2 - 2.0 * mu * m1 + mu * mu * m0
    terms = m0 * (-np.log(np.abs(sigma)) - HL2PI) - q / (2.0 * sigma * sigma)
    if feat_f32 == "loop":  # one thread per row: a plain running sum
        return np.cumsum(terms.astype(np.float32), axis=1, dtype=np.float32)[:, -1].astype(np.float64)
    return block_sum_f32(terms) if feat_f32 else terms.sum(1)


# ---------------------------------------------------------------- family C: key sets
ALL8 = ("text", "audio", "visual", "audiovisual", "textaudio", "textvisual", "textaudiovisual",
        "textaudio")  # the seven combinations and one repeat: kMaxKeys
MODS = ("text", "audio", "visual")
KEY_T = 6
KeyCase = collections.namedtuple("KeyCase", "D A Vd keys N B idx layout grads")
# idx: none (rows 0..B) | perm (rows of N > B, with repeats) | wrap (B > N)
# layout: rows (contiguous [B, F_k]) | gen (column blocks of one [B, 2 F] / [B, F] buffer)
# grads: all | some (mu of every other key, sigma of every third)
FAMILY_C = [
    KeyCase(300, 76, 48, models.MMB2_KEYS, 40, 17, "perm", "rows", "all"),
    KeyCase(300, 76, 48, models.MMB2_KEYS, 40, 17, "perm", "gen", "all"),
    KeyCase(300, 76, 48, models.MMB2_KEYS, 40, 17, "perm", "rows", "some"),
    KeyCase(300, 76, 48, models.MMB1_KEYS, 17, 17, "none", "rows", "all"),   # no text stats
    KeyCase(50, 1, 3, ALL8, 5, 17, "wrap", "gen", "some"),
    KeyCase(1, 5, 1, ALL8, 40, 17, "perm", "rows", "all"),
    KeyCase(4, 300, 7, ALL8, 17, 17, "none", "gen", "all"),
    KeyCase(4, 300, 7, ALL8, 40, 17, "perm", "rows", "some"),
]
# through mmb_gauss_*_strided directly, rows F_k + 3 apart
FAMILY_C_PADDED = [KeyCase(300, 76, 48, models.MMB2_KEYS, 40, 17, "perm", "pad", "all"),
                   KeyCase(50, 1, 3, ALL8, 5, 17, "wrap", "pad", "some"),
                   KeyCase(4, 300, 7, ALL8, 17, 17, "none", "pad", "some")]
PAD = 3


def key_id(c):
    name = {models.MMB2_KEYS: "mmb2", models.MMB1_KEYS: "mmb1", ALL8: "all8"}[c.keys]
    return f"D{c.D}-A{c.A}-V{c.Vd}-{name}-N{c.N}-B{c.B}-{c.idx}-{c.layout}-{c.grads}"


def key_segments(c, key):
    return models.combo_dims(key, c.D, c.A, c.Vd)


def key_width(c, key):
    return sum(w for _, w in key_segments(c, key))


def wants_grad(c, k):
    """(mu, sigma) of key number k carry requires_grad."""
    return (True, True) if c.grads == "all" else (k % 2 == 0, k % 3 == 0)


def make_key_inputs(c):
    """Frames and 0/1 masks [N, T, F_m] of the modalities some key uses (None
    for the others), idx [B] or None, mu / sigma [B, F_k] and up [B] per key."""
    rng = np.random.default_rng([c.D, c.A, c.Vd, len(c.keys), c.N, c.B, len(c.idx), len(c.layout),
                                 len(c.grads)])
    used = {m for k in c.keys for m, _ in key_segments(c, k)}
    z = {"x": {}, "mask": {}}
    for mod, w in zip(MODS, (c.D, c.A, c.Vd)):
        z["x"][mod] = f32(rng.standard_normal((c.N, KEY_T, w))) if mod in used else None
        z["mask"][mod] = make_mask(rng, "01", c.N, KEY_T, w) if mod in used else None
    if c.idx == "none":
        assert c.B == c.N
        z["idx"] = None
    else:
        z["idx"] = rng.integers(0, c.N, c.B)
        z["idx"][1] = z["idx"][0]  # at least one repeat
    widths = [key_width(c, k) for k in c.keys]
    z["mu"] = [f32(rng.standard_normal((c.B, w))) for w in widths]
    z["sigma"] = [f32(rng.uniform(0.5, 2.0, (c.B, w))) for w in widths]
    z["up"] = f32(rng.standard_normal((len(c.keys), c.B)))
    return z


@functools.lru_cache(maxsize=None)
def key_reference(c):
    """(inputs, refs, bars): per key (lp [B], dmu, dsigma [B, F_k]), a key's
    features concatenated in text, audio, visual order (models.combo_dims)."""
    z = make_key_inputs(c)
    rows = np.arange(c.B) if z["idx"] is None else z["idx"]
    refs, bars = [], []
    for k, key in enumerate(c.keys):
        xk = np.concatenate([z["x"][m][rows] for m, _ in key_segments(c, key)], -1)
        mk = np.concatenate([z["mask"][m][rows] for m, _ in key_segments(c, key)], -1)
        ref = normal_reference(z["mu"][k], z["sigma"][k], xk, mk, z["up"][k])
        refs.append(ref)
        bars.append(normal_bars(z["mu"][k], z["sigma"][k], xk, mk, z["up"][k], ref))
    return z, refs, bars


# ---------------------------------------------------------------- family D: the frame sums
StatsCase = collections.namedtuple("StatsCase", "N T F mask")
# (4097, 2, 257): N F = 1 052 929, 4 353 past the launch's 4096 x 256 threads
FAMILY_D = [StatsCase(N, T, F, m) for (N, T, F), kinds in
            (((3, 7, 5), ("none", "01")), ((40, 20, 300), ("none", "frac")),
             ((4097, 2, 257), ("none", "01"))) for m in kinds]
STATS_THREADS = 4096 * 256


def stats_id(c):
    return f"N{c.N}-T{c.T}-F{c.F}-{c.mask}"


@functools.lru_cache(maxsize=None)
def stats_case(c):
    rng = np.random.default_rng([c.N, c.T, c.F, MASKS.index(c.mask)])
    x = f32(2.0 * rng.standard_normal((c.N, c.T, c.F)) + 0.5)
    mask = make_mask(rng, c.mask, c.N, c.T, c.F)
    st, bar = stats_reference(x, mask)
    _freeze(x, mask, st, bar)
    return x, mask, st, bar


# ---------------------------------------------------------------- family E: LayerNorm backward
LNCase = collections.namedtuple("LNCase", "n d rows")
LN_SHAPES = [(1, 1), (3, 17), (4, 64), (5, 65), (37, 300), (130, 1000)]
FAMILY_E = [LNCase(n, d, "wide") for n, d in LN_SHAPES] + [LNCase(37, 300, "tight")]
LN_OUTS = ("both", "dgamma", "dbeta", "none")  # none: the cb = 0 launch of a frozen generator


def ln_id(c):
    return f"n{c.n}-d{c.d}-{c.rows}"


@functools.lru_cache(maxsize=None)
def ln_case(c):
    """(inputs, (dx, dgamma, dbeta), bars): rows 3 N(0, 1) + 1 (wide) or
    1000 + 0.01 N(0, 1) (tight); mean / rstd the float64 row statistics
    (biased variance, eps 1e-5) rounded to f32."""
    rng = np.random.default_rng([c.n, c.d, len(c.rows)])
    g = rng.standard_normal((c.n, c.d))
    x = f32(3.0 * g + 1.0 if c.rows == "wide" else 1000.0 + 0.01 * g)
    z = {"x": x, "dy": f32(rng.standard_normal((c.n, c.d))),
         "gamma": f32(1.0 + 0.5 * rng.standard_normal(c.d)),
         "mean": f32(x.mean(1)), "rstd": f32(1.0 / np.sqrt(x.var(1) + LN_EPS))}
    ref, bars = layer_norm_backward_reference(z["dy"], x, z["mean"], z["rstd"], z["gamma"])
    _freeze(*z.values(), *ref, *bars)
    return z, ref, bars


# ---------------------------------------------------------------- family F: the whole objective
MatrixCase = collections.namedtuple("MatrixCase", "D A Vd unimodal B T V")
FAMILY_F = [MatrixCase(50, 5, 3, False, 17, 9, 211), MatrixCase(300, 76, 48, True, 17, 9, 211)]
WORD_A = 1e-3
ARGS = {"word_loss_weight": 0.002}


def matrix_id(c):
    return f"D{c.D}-A{c.A}-V{c.Vd}-" + ("mmb1" if c.unimodal else "mmb2")


def make_generator(c):
    torch.manual_seed(c.D + c.A)
    return models.AudioVisualGeneratorMultimodal(c.D, c.A, c.Vd, norm="layer_norm", frozen_weights=False,
                                                 unimodal=c.unimodal)


def make_matrix_inputs(c):
    rng = np.random.default_rng([c.D, c.A, c.Vd, int(c.unimodal), c.B, c.T, c.V])
    common = rng.standard_normal(c.D)
    ids = rng.integers(1, c.V, (c.B, c.T))
    ids[rng.random((c.B, c.T)) < 0.2] = 0  # pads
    ids[:, 0] = 1 + np.arange(c.B) % (c.V - 1)
    z = {"table": f32(0.4 * rng.standard_normal((c.V, c.D)) + 0.3 * common), "ids": ids,
         "weights": f32(rng.uniform(0.05, 1.0, c.V)), "lat": f32(0.5 * rng.standard_normal((c.B, c.D))),
         "audio": f32(rng.standard_normal((c.B, c.T, c.A))), "visual": f32(rng.standard_normal((c.B, c.T, c.Vd))),
         "amask": make_mask(rng, "01", c.B, c.T, c.A), "vmask": make_mask(rng, "01", c.B, c.T, c.Vd)}
    return z


def matrix_data(z, keys, tensor):
    """(data, masks) of losses.get_log_prob_matrix from make_matrix_inputs'
    arrays, every array through `tensor` (the device's f32 or the CPU's f64)."""
    t = {k: tensor(v) for k, v in z.items() if k != "ids"}
    ids = torch.as_tensor(z["ids"])
    text = t["table"][ids.to(t["table"].device)]
    tm = tensor((z["ids"] != 0).astype(np.float64))[:, :, None].expand(*ids.shape, text.shape[-1])
    part = {"text": (text, tm), "audio": (t["audio"], t["amask"]), "visual": (t["visual"], t["vmask"])}
    data = {"text": text, "text_weights": t["weights"][ids.to(t["weights"].device)]}
    masks = {"text": tm}
    for k in keys:
        segs = [m for m in MODS if (k.startswith("text") if m == "text" else m in k)]
        data[k] = torch.cat([part[m][0] for m in segs], -1)
        masks[k] = torch.cat([part[m][1] for m in segs], -1)
    return t, data, masks


@functools.lru_cache(maxsize=None)
def matrix_reference(c):
    """(inputs, total [B], dlat [B, D], {parameter: gradient}) of
    oracle.latent_oracle.log_prob_matrix in float64 on a .double() copy of
    make_generator(c), loss (-total).mean()."""
    z = make_matrix_inputs(c)
    gen = copy.deepcopy(make_generator(c)).double()
    t, data, masks = matrix_data(z, list(gen.embed2out), lambda a: torch.tensor(np.asarray(a, np.float64)))
    x = t["lat"].clone().requires_grad_(True)

    def wfn(latents, word_weights, sent, mask):
        return LO.word_log_prob_angular2(latents, t["table"], word_weights, sent, mask, WORD_A)

    total = LO.log_prob_matrix(ARGS, x, gen(x), data, masks, wfn)
    (-total).mean().backward()
    grads = {n: p.grad.numpy() for n, p in gen.named_parameters()}
    return z, total.detach().numpy(), x.grad.numpy(), grads
