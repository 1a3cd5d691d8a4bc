"""Shared case tables, input family and f64 references of
tests/test_gpu_mmb2_widths.py (GPU) and tests/test_mmb2_cases.py (CPU): the
MMB2 stream and projection kernels at text widths other than 300.  Plain
helper module: no test is collected from it.

A case is (D, A, Vd, T, N, V): text / audio / visual widths, frames, rows,
vocabulary.  Its inputs are synth's numpy family -- word table 0.4 N(0, 1)
plus a common direction with row 0 zero, Zipf ids (ragged, id 0 pads), SIF
weights rounded to f32, U(-1, 1) frames -- seeded by the shape alone, and the
generator is models.AudioVisualGeneratorMultimodal(D, A, Vd, norm=None) under
torch.manual_seed(0) on the CPU.  tests/test_mmb2_cases.py pins, on the CPU,
the three conditions on every case that the GPU bars rest on.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

import models
import synth
from oracle import mmb2_oracle as M

U = 2.0 ** -24  # unit roundoff of f32
TOL = 1e-5      # the end-to-end bar of the suite: MMB2 and SIF rows against the oracle, row-relative

# ---------------------------------------------------------------- the shape table: (D, A, Vd, T)
# 1: wave stream kernel, D <= 256 (widths % 4, T <= 64): launch_wave<true, 1, CA, CV>
WAVE_D256 = [(4, 4, 4, 1), (52, 8, 12, 7), (100, 76, 48, 20), (200, 300, 4, 33), (256, 4, 300, 64),
             (128, 260, 320, 40)]
WAVE_ROWS_SHAPE, WAVE_ROWS = (52, 8, 12, 7), (1, 3, 4, 5)  # the four rows of a workgroup
# 2: wave stream kernel, 320 <= D <= 512, and its narrow-frame route (A, Vd <= 128)
WAVE_D512 = [(320, 20, 36, 21), (400, 300, 260, 40), (512, 4, 4, 64)]
NARROW_ROUTE = [(260, 76, 48, 20), (316, 128, 4, 33), (512, 8, 128, 64)]
# 3: workgroup stream kernel
WG_SCALAR_TEXT = [(50, 76, 48, 20), (50, 5, 3, 9), (17, 8, 3, 70), (63, 4, 4, 3), (301, 300, 300, 12),
                  (319, 4, 4, 3)]
WG_VECTOR_TEXT = [(100, 76, 48, 65), (52, 4, 4, 513), (516, 4, 4, 5), (640, 4, 4, 2)]
WG_CU_EDGE = (52, 4, 4, 70)       # N on either side of the CU count: FU = 16 | the default
WG_UNALIGNED = (100, 76, 48, 20)  # table 4 bytes off alignment: scalar text at a width % 4 == 0
# the eight vector / scalar combinations (text, audio, visual), T = 70
COMBOS = [(D, A, Vd, 70) for D in (52, 50) for A in (8, 5) for Vd in (12, 3)]
# 5: mmb_mm2_prepare
PREPARE_D = [4, 63, 64, 127, 128, 191, 192, 255, 256, 319, 320, 382, 383]  # every ldw, both edges
PREPARE_KP = [(8, 4, 4), (20, 8, 4), (24, 12, 12), (52, 8, 4), (60, 12, 8)]  # Kp 32 .. 160
PREPARE_T = (1, 40, 1357)
# 6 / 7: the projections.  D at every ldw edge (the total-weight column D the last column of
# a tile | the first of an otherwise padded one), the natural short K (nch = 1 .. 4)
PROJECT_D = [63, 64, 127, 128, 191, 192, 255, 256, 319, 320, 382, 383]
PROJECT_X3_D = [63, 64, 127, 128, 191, 192, 255, 256, 257, 299, 319]
PROJECT_KP = [(8, 4, 4, 3), (20, 8, 4, 5), (24, 12, 12, 7), (52, 8, 4, 9)]  # Kp 32, 64, 96, 128
PROJECT_N = (1, 63, 64, 65, 200)
PROJECT_X3_N = (1, 127, 128, 129, 300)
# 9: the narrow fused kernel (D, A, Vd, T, N, V).  (260, 128, 124, 64) is past its
# K limit (kq(A) + kq(Vd) = 512 > 256): the step must fall back to the stream kernel
NARROW_FUSED = [(260, 76, 48, 20, 1, 3016), (260, 76, 48, 20, 31, 3016), (260, 76, 48, 20, 517, 3016),
                (280, 20, 8, 7, 64, 300), (260, 64, 56, 64, 40, 16384), (260, 128, 124, 64, 40, 16384)]
# 10: FusedStep and the drop-in (D, A, Vd, T, N)
STEP = [(50, 76, 48, 20, 97), (100, 300, 300, 40, 97), (200, 76, 48, 20, 700), (100, 76, 48, 20, 700),
        (200, 300, 300, 40, 97), (50, 300, 300, 40, 700)]
STEP_WIDE = [(320, 20, 36, 21, 97), (380, 8, 12, 7, 97)]  # (382 % 4 != 0: past the scalar stream's 320)
DROP_IN = [(50, 76, 48, 20, 12, 20), (50, 76, 48, 130, 16, 130), (100, 76, 48, 20, 12, 9)]  # .., L
DEFAULT_N, DEFAULT_V = 5, 300
ROWS = {(4, 4, 4, 1): 1}  # the smallest of everything


def case_of(shape, n=None, v=DEFAULT_V):
    return tuple(shape) + (ROWS.get(tuple(shape), DEFAULT_N) if n is None else n, v)


def shape_id(s):
    return "-".join(str(x) for x in s)


def project_cases():
    return ([case_of((D, 8, 12, 7), n) for D in PROJECT_D for n in PROJECT_N]
            + [case_of(s, n) for s in PROJECT_KP for n in (1, 65)])


def project_x3_cases():
    return ([case_of((D, 8, 12, 7), n) for D in PROJECT_X3_D for n in PROJECT_X3_N]
            + [case_of(s, n) for s in PROJECT_KP for n in (1, 129)])


def oracle_cases():
    """Every case whose MMB2 rows or total weight a GPU test compares with the
    oracle: the CPU test pins the family's conditions on all of them."""
    out = [case_of(s) for s in WAVE_D256 + WAVE_D512 + NARROW_ROUTE + WG_SCALAR_TEXT + WG_VECTOR_TEXT
           + COMBOS]
    out += project_cases() + project_x3_cases() + [case_of((300, 8, 12, 7), n) for n in (1, 129, 300)]
    out += [tuple(c) for c in NARROW_FUSED]
    out += [case_of(c[:4], c[4]) for c in STEP + STEP_WIDE]
    out += [case_of(c[:4], c[4]) for c in DROP_IN]
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return uniq


# ---------------------------------------------------------------- the input family
def seed_of(case):
    D, A, Vd, T, N, V = case
    return (((((D * 521 + A) * 523 + Vd) * 541 + T) * 547 + N) * 557 + V) % (2 ** 31 - 1)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """The case's host inputs (read-only numpy): table E [V, D] f32, wt32 [V]
    f32, ids [N, T] int64, sw [N, T] f32 (the gathered weights), text E[ids],
    audio, visual, and emb2 (rows of a second table: a weighted sum over
    another tensor than the text)."""
    D, A, Vd, T, N, V = case
    s = seed_of(case)
    E = synth.word_table(V, D, seed=s)
    wt32 = synth.sif_weights(V, w0=1.0).astype(np.float32)
    ids = synth.token_ids(N, T, V, seed=s + 1, ragged=True)
    z = {"E": E, "wt32": wt32, "ids": ids, "sw": wt32[ids], "text": E[ids],
         "audio": synth.frames(N, T, A, seed=s + 2), "visual": synth.frames(N, T, Vd, seed=s + 3),
         "emb2": synth.word_table(V, D, seed=s + 4)[ids]}
    for a in z.values():
        a.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def generator(D, A, Vd):
    torch.manual_seed(0)
    return models.AudioVisualGeneratorMultimodal(D, A, Vd, norm=None)


@functools.lru_cache(maxsize=None)
def params(D, A, Vd):
    return M.params_from_module(generator(D, A, Vd))


def _chunks(n, rows=64):
    return [slice(r, min(n, r + rows)) for r in range(0, n, rows)]


@functools.lru_cache(maxsize=None)
def oracle_rows(case, f32=False, emb2=False):
    """The oracle's estimate_embedding_overall_gpu2 of the case (f64, or the
    reference's own f32 arithmetic), computed once, in row chunks."""
    D, A, Vd, T, N, V = case
    z = inputs(case)
    out = []
    for r in _chunks(N):
        cat = M.concat_inputs(z["text"][r], z["audio"][r], z["visual"][r])
        out.append(M.estimate_embedding_overall_gpu2(cat, params(D, A, Vd), z["sw"][r],
                                                     (z["emb2"] if emb2 else z["text"])[r],
                                                     dtype=np.float32 if f32 else np.float64))
    out = np.concatenate(out)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def total_weight(case, f32=False):
    """(total, sum of |terms|) of the case's total weight, per row."""
    D, A, Vd, T, N, V = case
    z = inputs(case)
    tot, ab = [], []
    for r in _chunks(N):
        cat = M.concat_inputs(z["text"][r], z["audio"][r], z["visual"][r])
        t, a = M.total_weight(cat, params(D, A, Vd), z["sw"][r],
                              dtype=np.float32 if f32 else np.float64)
        tot.append(t)
        ab.append(a)
    return np.concatenate(tot).astype(np.float64), np.concatenate(ab).astype(np.float64)


def family_conditions(case):
    """(f32 error, cancellation, sign flips): the three figures the CPU test
    bounds -- the row-relative distance of the oracle's f32 run from its f64
    run, the largest sum of |terms| / |total| of the total weight, and the
    rows whose total weight changes sign between the two runs."""
    e32 = M.row_rel_err(oracle_rows(case, f32=True), oracle_rows(case))
    t64, a64 = total_weight(case)
    t32, _ = total_weight(case, f32=True)
    return e32, float((a64 / np.abs(t64)).max()), int((np.sign(t32) != np.sign(t64)).sum())


# ---------------------------------------------------------------- f64 references
def stream_reference(text, emb, w, audio, visual):
    """f64 numpy of what the stream kernels write, from the f32 inputs a
    launch sees (text / emb [N, T, D] rows with a dropped token's row zeroed,
    w [N, T] f32): x = (sum_t w emb) / count_nonzero(w), the frame sums s, the
    weight sum -- and for each the sum over t of |term|, which scales its
    bar."""
    w64 = np.asarray(w, np.float64)
    terms = w64[:, :, None] * np.asarray(emb, np.float64)
    cnt = np.count_nonzero(w64, axis=1).astype(np.float64)
    s, s_abs = M.frame_sums(text, audio, visual)
    with np.errstate(invalid="ignore", divide="ignore"):
        x = terms.sum(1) / cnt[:, None]
        x_abs = np.abs(terms).sum(1) / cnt[:, None]
    return {"x": x, "x_abs": x_abs, "cnt": cnt, "s": s, "s_abs": s_abs, "sw": w64.sum(1),
            "sw_abs": np.abs(w64).sum(1)}


def sum_bar(T, absolute):
    """|f32 sum of T terms - exact| <= 2 (T + 1) 2^-24 sum |term|: T roundings
    of the running sum (any order, fused or not: each at most 2^-24 of a partial
    sum, itself at most sum |term|), one of the term or the final division,
    doubled."""
    return 2.0 * (T + 1) * U * absolute


def row_scale_of(smax):
    """The power of two that puts smax into [2^14, 2^15) (1 for 0 / non-finite)."""
    smax = np.asarray(smax, np.float64)
    ok = (smax > 0) & np.isfinite(smax)
    _, ex = np.frexp(np.where(ok, smax, 1.0))
    return np.where(ok, np.ldexp(1.0, 15 - ex), 1.0)


def project_reference(s, x, aux, Wm, c0, D, K, x3=False):
    """The projection in f64 from the device's own operands: y_j = text_j +
    s . Wm_j + c0_j with text_j = x_j * count (j < D) or the weight sum (column
    D, the total weight); the output row is sign(y_D) y / ||y|| (the division by
    the total cancels in the normalisation).  Returns (rows [N, D], bar [N]):
    beta_j = 2 (K + 3) 2^-24 S_j bounds the f32 kernel's error of y_j, S_j =
    sum_k |s_k Wm_kj| + |text_j| + |c0_j| (K products accumulated in f32 in any
    order, the three additions of the epilogue, doubled); the fp16 x3 kernel adds
    3 * 2^-22 S_j (each operand carries 22 bits, the lo * lo product is omitted).
    To first order the normalised row moves by at most 2 ||beta|| / ||y||; its own
    two roundings (the division, the norm) add 2^-22 of an element.  The bar is
    row-relative: divided by max_j |row_j|."""
    s = np.asarray(s, np.float64)[:, :K]
    x = np.asarray(x, np.float64)
    aux = np.asarray(aux, np.float64)
    Wm = np.asarray(Wm, np.float64)[:K, :D + 1]
    c0 = np.asarray(c0, np.float64)[:D + 1]
    cnt = aux[0][:, None]
    text = np.concatenate([np.where(cnt != 0, np.nan_to_num(x) * cnt, 0.0), aux[1][:, None]], 1)
    y = text + s @ Wm + c0
    S = np.abs(s) @ np.abs(Wm) + np.abs(text) + np.abs(c0)
    beta = (2.0 * (K + 3) * U + (3.0 * 2.0 ** -22 if x3 else 0.0)) * S[:, :D]
    nrm = np.linalg.norm(y[:, :D], axis=1)
    rows = np.sign(y[:, D:]) * y[:, :D] / nrm[:, None]
    bar = (2.0 * np.linalg.norm(beta, axis=1) / nrm + 2.0 ** -22) / np.abs(rows).max(1)
    return rows, bar


def prepare_reference(D, A, Vd, T):
    """(Wm, c0, Wm bar, c0 bar) of mmb_mm2_prepare: one f32 rounding of the f64
    value (2^-24 relative, doubled) plus 1e-12 of the sum of |terms| for the
    order of the kernel's own f64 sum."""
    Wm, c0, Wa, ca = M.merged_projection(params(D, A, Vd), D, A, Vd, T)
    return Wm, c0, 2.0 * U * np.abs(Wm) + 1e-12 * Wa, 2.0 * U * np.abs(c0) + 1e-12 * ca
