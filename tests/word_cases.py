"""Shared case table, inputs and float64 reference of tests/test_gpu_word_widths.py
(GPU) and tests/test_word_cases.py (CPU): the word log-likelihood kernels
(csrc/latent_kernels.hip) at table widths other than 300; tests/test_gpu_scratch.py
and tests/test_gpu_large.py hold their runs of these kernels to the same bars
(lp_ratio, grad_ratio).  Plain helper module: no test is collected from it.

word_zsum_kernel<NT> is instantiated per 16-column tile count NT = pad16(D) / 16
= 1..20; the table below reaches NT 1, 2, 4, 7, 13, 19 and 20, a pad of 0, 1,
3, 4, 8, 11, 12, 14 and 15 columns, fewer words than one 16-word tile, fewer
tiles than the block's 4 waves, and latent tiles of 1, 16, 17 and 33 rows.

The gradient holds 1 / sqrt(1 - cos^2), so a case means something only while
every cosine of the float64 reference stays away from +-1: MAX_COS over every
(latent, word) and (latent, token) pair, asserted by tests/test_word_cases.py.
The seeds were searched for that when the table was written (search_seed;
never at test time): random directions come that close only in narrow
tables, so the D = 4 and 5 lines keep B V small.
"""
from __future__ import annotations

import collections
import functools

import numpy as np
import torch

from oracle import latent_oracle as LO

MAX_COS = 0.99
A = 1e-3

WordCase = collections.namedtuple("WordCase", "D V B L seed")

# D, V, B, L, seed
WORD_CASES = [
    WordCase(4, 15, 1, 1, 0), WordCase(4, 33, 16, 5, 0),        # NT 1, pad 12; B V kept small
    WordCase(5, 16, 17, 1, 0), WordCase(5, 17, 1, 5, 0),        # pad 11
    WordCase(15, 1, 16, 5, 0), WordCase(15, 517, 33, 1, 0),     # pad 1; one word
    WordCase(16, 16, 16, 1, 0), WordCase(16, 33, 17, 5, 0),     # exactly one tile each way
    WordCase(17, 15, 33, 5, 0), WordCase(17, 517, 1, 1, 0),     # NT 2 with one real column
    WordCase(50, 17, 16, 1, 0), WordCase(50, 517, 33, 5, 0),    # GloVe 50: NT 4, pad 14
    WordCase(100, 1, 1, 1, 0), WordCase(100, 517, 17, 5, 0),    # GloVe 100: NT 7, pad 12
    WordCase(200, 33, 17, 5, 0), WordCase(200, 517, 33, 1, 0),  # GloVe 200: NT 13, pad 8
    WordCase(299, 33, 17, 5, 0), WordCase(299, 517, 16, 1, 0),  # NT 19, pad 5
    WordCase(301, 15, 33, 1, 0), WordCase(301, 517, 1, 5, 0),   # NT 19, pad 3
    WordCase(304, 16, 16, 5, 0), WordCase(304, 517, 33, 1, 0),  # NT 19, pad 0
    WordCase(320, 17, 1, 1, 0), WordCase(320, 517, 33, 5, 0),   # NT 20: the widest
]


def word_id(c):
    return f"D{c.D}-V{c.V}-B{c.B}-L{c.L}"


def f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def make_inputs(c, seed=None):
    """f32-representable float64 inputs: table [V, D] (a common direction on
    noise, like synth.word_table), latents [B, D], ids [B, L], dense tokens
    [B, L, D] (not table rows), weights, 0/1 mask and an upstream gradient."""
    rng = np.random.default_rng([c.D, c.V, c.B, c.L, c.seed if seed is None else seed])
    g = rng.standard_normal(c.D)
    z = {"table": f32(0.4 * rng.standard_normal((c.V, c.D)) + 0.3 * g),
         "lat": f32(0.5 * rng.standard_normal((c.B, c.D))),
         "ids": rng.integers(0, c.V, size=(c.B, c.L)),
         "dense": f32(0.4 * rng.standard_normal((c.B, c.L, c.D)) + 0.3 * g),
         "w": f32(rng.uniform(0.05, 1.0, (c.B, c.L))),
         "mask": (rng.random((c.B, c.L)) > 0.2).astype(np.float64),
         "up": f32(rng.standard_normal(c.B))}
    z["mask"][:, 0] = 1.0
    return z


def _cos(a, b):
    return (a / np.linalg.norm(a, axis=-1, keepdims=True)) @ \
        np.swapaxes(b / np.linalg.norm(b, axis=-1, keepdims=True), -1, -2)


def max_abs_cos(z):
    """Largest |cos| over every (latent, word), (latent, table token) and
    (latent, dense token) pair."""
    lat = z["lat"]
    m = np.abs(_cos(lat, z["table"])).max()
    for tok in (z["table"][z["ids"]], z["dense"]):
        m = max(m, np.abs(_cos(lat[:, None, :], tok)).max())
    return float(m)


def search_seed(c, tries=400):
    for s in range(tries):
        if max_abs_cos(make_inputs(c, s)) <= MAX_COS:
            return s
    return None


@functools.lru_cache(maxsize=None)
def reference(c, dense):
    """(inputs, lp [B], dlat [B, D]) of oracle.latent_oracle.word_log_prob_angular2
    in float64, tokens by id (rows of the table) or dense; computed once."""
    z = make_inputs(c)
    t = {k: torch.tensor(v) for k, v in z.items()}
    x = t["lat"].clone().requires_grad_(True)
    sent = t["dense"] if dense else t["table"][t["ids"]]
    mask3 = t["mask"][:, :, None].expand(c.B, c.L, c.D)
    lp = LO.word_log_prob_angular2(x, t["table"], t["w"], sent, mask3, A)
    (lp * t["up"]).sum().backward()
    out = (z, lp.detach().numpy(), x.grad.numpy())
    for a in list(z.values()) + list(out[1:]):
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------- the bars, as fractions
# (the ones tests/test_gpu_latent.py states: lp |y - y_ref| <= 2e-5 |y_ref| + 1e-4;
#  the gradient, per row, max |g - g_ref| <= 2e-4 max |g_ref|)
def lp_ratio(y, ref, rtol=2e-5, atol=1e-4):
    y, ref = np.asarray(y, np.float64), np.asarray(ref, np.float64)
    assert y.shape == ref.shape
    return float((np.abs(y - ref) / (rtol * np.abs(ref) + atol)).max())


def grad_ratio(g, ref, tol=2e-4):
    g, ref = np.asarray(g, np.float64), np.asarray(ref, np.float64)
    assert g.shape == ref.shape
    return float((np.abs(g - ref).max(1) / (tol * np.abs(ref).max(1))).max())
