"""CPU restatement of the closed-form MMB2 estimate (a7/a8) — TEST INFRASTRUCTURE ONLY.

Follows `/root/reference/sif2.py:103-114` (calc_weights) and `:164-208`
(estimate_embedding_overall_gpu2), restated in numpy so it can run in float64
(the parity target) or float32 (the reference's own arithmetic).
"""
from __future__ import annotations

import numpy as np

KEYS = ("audio", "visual", "audiovisual", "textaudio", "textvisual", "textaudiovisual")


def calc_weights(data, b_mean, b_log_sigma):
    """sif2.py:103-114 — the mask argument is ignored by the reference (pads count)."""
    b_mean = b_mean.reshape((1, 1, -1))
    b_log_sigma = b_log_sigma.reshape((1, 1, -1))
    q_mean = (data - b_mean) / np.exp(2 * b_log_sigma)
    q_sigma = (data - b_mean) ** 2 / np.exp(2 * b_log_sigma) - 1.0
    return q_mean, q_sigma


def concat_inputs(text, audio, visual):
    """The 7 data tensors the callers build (simplesif.py:820-830)."""
    return {"text": text, "audio": audio, "visual": visual,
            "audiovisual": np.concatenate([audio, visual], -1),
            "textaudio": np.concatenate([text, audio], -1),
            "textvisual": np.concatenate([text, visual], -1),
            "textaudiovisual": np.concatenate([text, audio, visual], -1)}


def estimate_embedding_overall_gpu2(data, params, sentence_weights, embeddings, dtype=np.float64):
    """sif2.py:164-208.

    params: {key: (W_mu [F,D], b_mu [F], W_ls [F,D], b_ls [F])} as numpy.
    Keys are visited in the fixed order of :167-174; total weight is the sum of
    sentence weights plus every q_mean and q_sigma element (:186-188); cs is
    the weighted text average plus sum_k sum_t (q/total) @ W_k (:200-205), then
    row-L2-normalised (:207).  No PC removal.
    """
    c = lambda a: np.asarray(a, dtype=dtype)
    qm, qs = {}, {}
    for k in KEYS:
        Wm, bm, Wl, bl = params[k]
        qm[k], qs[k] = calc_weights(c(data[k]), c(bm), c(bl))
    sw = c(sentence_weights)
    total = sw.sum(-1) + sum(qm[k].sum(-1).sum(-1) for k in KEYS)
    total = total + sum(qs[k].sum(-1).sum(-1) for k in KEYS)
    total = total.reshape((-1, 1, 1))
    cs = np.einsum("nt,ntd->nd", sw / total.reshape((-1, 1)), c(embeddings))
    for k in KEYS:
        Wm, bm, Wl, bl = params[k]
        cs = cs + np.matmul(qm[k] / total, c(Wm)).sum(axis=1)
        cs = cs + np.matmul(qs[k] / total, c(Wl)).sum(axis=1)
    cs = cs / np.linalg.norm(cs, axis=1, keepdims=True)
    return cs


def total_weight(data, params, sentence_weights, dtype=np.float64):
    """(total, absolute): the total weight of sif2.py:186-188 per utterance, and
    the sum of |sentence weights| + |q_mean| + |q_sigma| over every key that it
    is the signed sum of (absolute / |total| is its cancellation)."""
    c = lambda a: np.asarray(a, dtype=dtype)
    sw = c(sentence_weights)
    total, absolute = sw.sum(-1), np.abs(sw).sum(-1)
    for k in KEYS:
        Wm, bm, Wl, bl = params[k]
        qm, qs = calc_weights(c(data[k]), c(bm), c(bl))
        total = total + qm.sum(-1).sum(-1) + qs.sum(-1).sum(-1)
        absolute = absolute + np.abs(qm).sum(-1).sum(-1) + np.abs(qs).sum(-1).sum(-1)
    return total, absolute


def _segments(key, D, A, Vd):
    """(modality 0 text / 1 audio / 2 visual, offset in the key's features, width)."""
    segs, off = [], 0
    for m, w in ((0, D if key.startswith("text") else 0), (1, A if "audio" in key else 0),
                 (2, Vd if "visual" in key else 0)):
        if w:
            segs.append((m, off, w))
            off += w
    return segs


def frame_sums(text, audio, visual):
    """(s, s_abs) in f64: the per-utterance sums over the frames [Sx_t | Sxx_t |
    Sx_a | Sxx_a | Sx_v | Sxx_v] ([N, 2 (D + A + Vd)]) that the closed form
    projects, and the sums of the terms' absolute values."""
    parts, absolute = [], []
    for x in (text, audio, visual):
        x = np.asarray(x, np.float64)
        parts += [x.sum(1), (x * x).sum(1)]
        absolute += [np.abs(x).sum(1), (x * x).sum(1)]
    return np.concatenate(parts, -1), np.concatenate(absolute, -1)


def merged_projection(params, D, A, Vd, T):
    """(Wm [K, D + 1], c0 [D + 1], Wm_abs, c0_abs) in f64: the twelve
    projections of sif2.py:200-205 and the total weight (:186-188, column D)
    folded over the frame sums of frame_sums().  With a = exp(-2 b_ls) and
    b = b_mu of feature f of key k (q_mean = a (x - b), q_sigma = a (x - b)^2
    - 1 summed over T frames):
      Sx row   of f: sum_k a (W_mu[f] - 2 b W_ls[f])     | column D: a (1 - 2 b)
      Sxx row  of f: sum_k a W_ls[f]                     | column D: a
      c0           : T sum_k sum_f (-a b W_mu[f] + a b^2 W_ls[f] - W_ls[f])
                                                         | column D: -a b + a b^2 - 1
    The *_abs arrays sum the absolute values of the same terms."""
    w = (D, A, Vd)
    base = (0, 2 * D, 2 * D + 2 * A)
    K = 2 * (D + A + Vd)
    Wm, Wa = np.zeros((K, D + 1)), np.zeros((K, D + 1))
    c0, ca = np.zeros(D + 1), np.zeros(D + 1)
    for k in KEYS:
        Wmu, bmu, Wls, bls = (np.asarray(p, np.float64) for p in params[k])
        for m, off, wid in _segments(k, D, A, Vd):
            sl = slice(off, off + wid)
            a = np.exp(-2.0 * bls[sl])[:, None]
            b = bmu[sl][:, None]
            mu1 = np.concatenate([Wmu[sl], np.ones((wid, 1))], 1)  # column D: weight 1
            ls1 = np.concatenate([Wls[sl], np.ones((wid, 1))], 1)
            rx = slice(base[m], base[m] + w[m])
            rxx = slice(base[m] + w[m], base[m] + 2 * w[m])
            Wm[rx] += a * (mu1 - 2.0 * b * ls1)
            Wa[rx] += np.abs(a * mu1) + np.abs(2.0 * a * b * ls1)
            Wm[rxx] += a * ls1
            Wa[rxx] += np.abs(a * ls1)
            c0 += T * (-a * b * mu1 + a * b * b * ls1 - ls1).sum(0)
            ca += T * (np.abs(a * b * mu1) + np.abs(a * b * b * ls1) + np.abs(ls1)).sum(0)
    return Wm, c0, Wa, ca


def params_from_module(gen):
    """{key: (W_mu, b_mu, W_ls, b_ls)} numpy f32 from an AudioVisualGeneratorMultimodal."""
    out = {}
    for k, m in gen.embed2out.items():
        out[k] = tuple(t.detach().cpu().numpy() for t in (m["mu"].weight, m["mu"].bias,
                                                           m["log_sigma"].weight, m["log_sigma"].bias))
    return out


def row_rel_err(y, yref):
    """SURVEY §8d parity metric: max_j |y - yref| / max_j |yref| per row, max over rows."""
    y = np.asarray(y, np.float64)
    yref = np.asarray(yref, np.float64)
    return float((np.abs(y - yref).max(axis=1) / np.abs(yref).max(axis=1)).max())
