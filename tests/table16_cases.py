"""Shared inputs and references of tests/test_gpu_table16.py (GPU) and
tests/test_table16_cases.py (CPU): the SIF gather and the MMB2 stream kernels
on a word table kept in 16-bit storage (mmb_sif_wavg_tt, mmb_mm2_stream_tt).
Plain helper module: no test is collected from it.

A case is one of mmb2_cases (D, A, Vd, T, N, V); a kind is "bf16" or "f16"
(pipeline.TABLE_KINDS).  The case's word table is rounded to the kind on the
CPU (round to nearest even, torch's conversion) -- that is the caller's
rounding, the library converts nothing -- and every reference here is taken
on the UPCAST image of that 16-bit table, which is what a 16-bit launch must
reproduce: bit for bit against an f32 launch on the image, to the usual bars
against the oracle on the image.  The frames of a case are its f32 ones or,
with `fkind`, frames16_cases' rounding of them (and then their upcast image).
"""
from __future__ import annotations

import functools

import numpy as np
import torch

import frames16_cases as F
import mmb2_cases as C
import mmb_lib
import width_cases as W
from frames16_cases import BF16, EINVAL, F16, F32, OK, P  # noqa: F401  (the argument tables' vocabulary)
from oracle import mmb2_oracle as M
from oracle import sif_oracle as O

KINDS = F.KINDS
TABLE_TYPES = (("f32", mmb_lib.MMB_TABLE_F32), ("f16", mmb_lib.MMB_TABLE_F16), ("bf16", mmb_lib.MMB_TABLE_BF16))
TABLE_TYPES16 = TABLE_TYPES[1:]

# ---------------------------------------------------------------- argument tables
# (frames16_cases' scaffolding: ARGS, BASE and rows (what, change, want))
SIF_ARGS = "table table_type v d ids n l w wtab32 x_out num_out cnt_out flag stream".split()
SIF_BASE = dict(table=P, table_type=mmb_lib.MMB_TABLE_BF16, v=1000, d=300, ids=P, n=100, l=40, w=None, wtab32=P,
                x_out=P, num_out=None, cnt_out=None, flag=None, stream=None)
STREAM_ARGS = ("ids table table_type v wtab32 w_dense audio visual frame_type n t d a vd num_out s_out s_half "
               "aux_out flag colmax colmax_ws stream").split()
STREAM_BASE = dict(ids=P, table=P, table_type=mmb_lib.MMB_TABLE_BF16, v=1000, wtab32=P, w_dense=None, audio=P,
                   visual=P, frame_type=F32, n=100, t=40, d=300, a=300, vd=300, num_out=P, s_out=P, s_half=1,
                   aux_out=P, flag=None, colmax=None, colmax_ws=None, stream=None)


def table_rows(types, rows):
    """Every (what, change, want) of `rows` once per table type of `types`."""
    return [(f"{name} table, {what}", dict(table_type=tt, **change), want)
            for name, tt in types for what, change, want in rows]


def pair_rows(rows):
    """Every row once per (table type, frame type) pair: all nine."""
    return [(f"{tn} table, {what}", dict(table_type=tt, **change), want)
            for tn, tt in TABLE_TYPES for what, change, want in F.arg_rows(F.ALL_TYPES, rows)]


def _ids(cases):
    return [c[0].replace(" ", "_").replace(",", "") for c in cases]


# the FusedStep keywords a 16-bit table's plan must not depend on: none, every
# f32-frame front kernel asked for, every 16-bit-frame front kernel as well
OVERRIDES = ({}, dict(stream_project=True, narrow_fused=True, split_stream=True),
             dict(stream_project=True, narrow_fused=True, split_stream=True, fused_frames16=True,
                  narrow_frames16=True, split_frames16=True))


# ---------------------------------------------------------------- rounding
@functools.lru_cache(maxsize=None)
def table(case, kind):
    """The case's word table rounded to `kind` (a CPU tensor)."""
    return F.to_kind(C.inputs(case)["E"], kind)


@functools.lru_cache(maxsize=None)
def inputs(case, kind, fkind=None, special=False):
    """mmb2_cases.inputs(case) with E replaced by the upcast image of its
    rounding to `kind` (and text = that image's rows); "E16" holds the 16-bit
    table.  With `fkind` the frames are frames16_cases' (their upcast image,
    and "audio16" / "visual16").  `special`: the table with the special
    values planted (special_table)."""
    E16 = special_table(case, kind) if special else table(case, kind)
    base = F.inputs(case, fkind) if fkind else C.inputs(case)
    E = F.upcast(E16)
    text = E[base["ids"]]
    text.setflags(write=False)
    return dict(base, E=E, text=text, E16=E16)


# ---------------------------------------------------------------- special values
# planted into the rounded table of frames16_cases.SPECIAL_SHAPES: value j of
# the kind's list (frames16_cases.SPECIALS: +-0, the smallest subnormal, the
# largest planted value) at E[0, j] -- mmb2_cases tables have row 0 zero, so
# the workgroup kernel's row-0 shortcut multiplies zeros unless row 0 is
# planted -- and at E[hot, D - 1 - j], `hot` the row the case's ids use most.
SPECIAL_SHAPES = F.SPECIAL_SHAPES
SPECIALS = F.SPECIALS


def hot_row(case):
    """The table row (not row 0) most of the case's tokens name."""
    ids = C.inputs(case)["ids"]
    V = case[5]
    rows = np.where(ids < 0, ids + V, ids).ravel()
    counts = np.bincount(rows[rows > 0], minlength=V)
    return int(counts.argmax())


@functools.lru_cache(maxsize=None)
def special_table(case, kind):
    D, A, Vd, T, N, V = case
    vals = torch.tensor([v for v, _ in SPECIALS[kind]], dtype=torch.float64).to(KINDS[kind])
    assert D >= 2 * len(vals)
    E16 = table(case, kind).clone()
    E16[0, :len(vals)] = vals
    E16[hot_row(case), D - len(vals):] = vals.flip(0)
    return E16


# ---------------------------------------------------------------- the SIF gather's cases: (d, l)
SIF_WAVE = [(d, l) for d in (4, 52, 256, 260, 512) for l in (1, 7, 64)]  # one and two column units
SIF_WG = [(50, 9), (52, 513), (516, 5), (1280, 3)]  # scalar; past a staging chunk; second column; the widest
SIF_UNALIGNED = (52, 7)  # a table 2 bytes off: the scalar workgroup kernel at a width % 4 == 0
SIF_N, SIF_V = 5, 300


@functools.lru_cache(maxsize=None)
def sif_inputs(d, l, kind, n=SIF_N, v=SIF_V):
    """(E16 [v, d], ids [n, l] int64 with some negative ones that wrap, wt32
    [v], w [n, l] the gathered weights) of one SIF gather case; row 0 of the
    table is planted non-zero (the row-0 shortcut)."""
    import synth

    seed = 7919 * d + l
    E = synth.word_table(v, d, seed=seed).copy()
    E[0] = np.linspace(-0.5, 0.75, d, dtype=np.float32)
    ids = synth.token_ids(n, l, v, seed=seed + 1, ragged=True).copy()
    wt32 = synth.sif_weights(v, w0=1.0).astype(np.float32)
    w = wt32[ids]
    if l >= 7:  # negative ids wrap for the row (table[v + id]); their table weight is 0
        ids[1, 2], ids[n - 1, l - 1] = -3, -v
        w[1, 2], w[n - 1, l - 1] = 0.25, 0.5  # (given weights keep theirs)
    for a in (ids, wt32, w):
        a.setflags(write=False)
    return F.to_kind(E, kind), ids, wt32, w


# ---------------------------------------------------------------- the steps: oracle on the upcast inputs
STEP, STEP_NARROW_TWIN, CHUNKED = F.STEP, F.STEP_NARROW_TWIN, F.CHUNKED
FRAME_CHOICES = ("f32", "same")  # the frames of a step: f32, or the table's own kind


def fkind_of(kind, frames):
    return None if frames == "f32" else kind


def oracle_cases():
    return [(F.step_case(d), kind, fr) for d in STEP for kind in KINDS for fr in FRAME_CHOICES]


@functools.lru_cache(maxsize=None)
def oracle_rows(case, kind, fkind=None, f32=False):
    """The oracle's estimate_embedding_overall_gpu2 of the upcast inputs (f64,
    or the reference's own f32 arithmetic)."""
    D, A, Vd, T, N, V = case
    z = inputs(case, kind, fkind)
    out = []
    for r in C._chunks(N):
        cat = M.concat_inputs(z["text"][r], z["audio"][r], z["visual"][r])
        out.append(M.estimate_embedding_overall_gpu2(cat, C.params(D, A, Vd), z["sw"][r], z["text"][r],
                                                     dtype=np.float32 if f32 else np.float64))
    out = np.concatenate(out)
    out.setflags(write=False)
    return out


def total_weight(case, kind, fkind=None, f32=False):
    D, A, Vd, T, N, V = case
    z = inputs(case, kind, fkind)
    tot, ab = [], []
    for r in C._chunks(N):
        cat = M.concat_inputs(z["text"][r], z["audio"][r], z["visual"][r])
        t, a = M.total_weight(cat, C.params(D, A, Vd), z["sw"][r], dtype=np.float32 if f32 else np.float64)
        tot.append(t)
        ab.append(a)
    return np.concatenate(tot).astype(np.float64), np.concatenate(ab).astype(np.float64)


def family_conditions(case, kind, fkind=None):
    """mmb2_cases.family_conditions on the upcast inputs: (f32 error,
    cancellation, sign flips)."""
    e32 = M.row_rel_err(oracle_rows(case, kind, fkind, f32=True), oracle_rows(case, kind, fkind))
    t64, a64 = total_weight(case, kind, fkind)
    t32, _ = total_weight(case, kind, fkind, f32=True)
    return e32, float((a64 / np.abs(t64)).max()), int((np.sign(t32) != np.sign(t64)).sum())


@functools.lru_cache(maxsize=None)
def pc_routes(case, kind):
    """The oracle's two routes to the PC of the step's a2 rows on the rounded
    table: compute_pc on the rows, and the Gram route (pc_from_gram on X^T X
    with the device solver's start block).  The rows are the reference's own
    (get_weighted_average on the upcast table, f32 as the table)."""
    z = inputs(case, kind)
    X = O.get_weighted_average(z["E"], z["ids"], z["sw"])
    z0, tr = W.start_block(X, 1)
    return O.compute_pc(X, 1), O.pc_from_gram(X.T @ X, z0, 1, tr)
