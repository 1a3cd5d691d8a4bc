"""Shared tables of tests/test_gpu_split_table16.py (GPU) and
tests/test_split_table16_cases.py (CPU): the split stream on a word table
kept in fp16 / bf16 storage (mmb_mm2_stream_split_tt,
pipeline.mm2_stream_split_tt, FusedStep(split_table16=True)).  Plain helper
module: no test is collected from it.

The definition under test is table16_cases': a launch on a 16-bit table
writes, bit for bit, what the same launch (the same parts) of
mmb_mm2_stream_split_ft writes on that table upcast to f32 -- x, s in both
s_half formats, the three aux planes, the column bounds and the flag word --
and, with one range, what the one-workgroup launch (mmb_mm2_stream_tt) writes
on the 16-bit table.
"""
from __future__ import annotations

import functools

import numpy as np

import frames16_cases as F
import split_frames16_cases as SF
import synth
import table16_cases as T
from frames16_cases import EINVAL, F32, OK, P
from table16_cases import TABLE_TYPES, TABLE_TYPES16

KINDS = T.KINDS
NT = SF.NT
TOK_CHUNK = 512  # tokens staged per LDS chunk (kTokChunk)
FRAME_CHOICES = T.FRAME_CHOICES  # the frames of a case: f32, or the table's own kind
WS_FILLS = (0x00, 0xFF, 0xA5)  # the scratch rule of include/mmb.h: three byte patterns

# D = 300 on the frame shapes of split_frames16_cases, with their part tuples: (N, T, A, Vd, parts)
FRAME_SHAPE_CASES = [c[:5] for c in SF.KERNEL_CASES[:2]]
D_FRAME_SHAPES = SF.D
# (D, T, parts, table offset in bytes, A = Vd, N): the smallest text shapes that
# reach each way the text workgroups can go wrong.  A text workgroup runs
# D / VT column units x NT // units row slots over the range's kept tokens.
TEXT_CASES = [
    (50, 97, (2,), 0, 8, 6),    # d % 4 != 0: scalar 2-byte loads
    (52, 97, (2,), 2, 8, 6),    # a table 2 bytes off: scalar at a width % 4 == 0
    (664, 70, (3,), 0, 4, 5),   # 166 units x ONE row slot; A = Vd = 4 keeps 3 d + 2 a + 2 vd <= 2240
    (4, 70, (2,), 0, 8, 6),     # one unit, 320 row slots, most of them empty
    (52, 600, (1,), 0, 8, 4),   # one range past a 512-token staging chunk
]
V = 300
# the run with the column bounds on, and the one on split_frames16_cases.BAD_CASE
BOUNDS_CASE = TEXT_CASES[0]
BAD_CASE = SF.BAD_CASE
# the step: (N, T, A, Vd) at D = 300
STEP = SF.STEP


def vector(d: int, off_bytes: int) -> bool:
    """stream_vec's rule for a 16-bit table: whole 4-value units from an 8-byte aligned base."""
    return d % 4 == 0 and off_bytes % 8 == 0


def units(d: int, off_bytes: int) -> tuple[int, int]:
    """(column units, row slots) of a text workgroup."""
    u = d // 4 if vector(d, off_bytes) else d
    return u, NT // u


@functools.lru_cache(maxsize=None)
def text_inputs(d, t, n, kind, v=V):
    """(E16 [v, d], ids [n, t] int64, wt32 [v]) of a text case.  Row 0 is
    planted non-zero and the ids are row-0-heavy (about 70 % id 0, POM's pad /
    OOV share), so the row-0 shortcut of the finish kernel carries most of the
    sums; utterance 0 names row 0 only, and utterance 1 keeps no token in its
    middle third (all row 0 there), whatever the part count cuts."""
    seed = 6007 * d + t
    E = synth.word_table(v, d, seed=seed).copy()
    E[0] = np.linspace(-0.5, 0.75, d, dtype=np.float32)
    rng = np.random.default_rng(seed + 1)
    ids = rng.integers(1, v, size=(n, t))
    ids[rng.random((n, t)) < 0.7] = 0
    ids[0] = 0
    ids[1, t // 3:-(-2 * t // 3)] = 0
    wt32 = synth.sif_weights(v, w0=1.0).astype(np.float32)
    ids[2, 1], ids[n - 1, t - 1] = -3, -v  # negative ids wrap for the row (-v: row 0); their table weight is 0
    for a in (ids, wt32):
        a.setflags(write=False)
    return F.to_kind(E, kind), ids, wt32


def frames_of(a, t, n, d):
    """(audio, visual) f32 [n, t, a] of a text case."""
    return synth.frames(n, t, a, seed=31 * d + t), synth.frames(n, t, a, seed=37 * d + t)


# ---------------------------------------------------------------- the argument table
ARGS = ("ids table table_type v wtab32 w_dense audio visual frame_type n t d a vd num_out s_out s_half aux_out "
        "flag colmax colmax_ws parts ws ws_bytes stream").split()
BASE = dict(SF.BASE, table_type=TABLE_TYPES16[1][1], frame_type=F32)
ONE_SHORT = SF.ONE_SHORT
resolve = SF.resolve

ARG_CASES = [("table_type -1", dict(table_type=-1), EINVAL),
             ("table_type 3", dict(table_type=3), EINVAL),
             ("table_type 3, n 0", dict(table_type=3, n=0, parts=0, ws=None, ws_bytes=0), EINVAL),
             ("table_type -1, n 0", dict(table_type=-1, n=0, parts=0, ws=None, ws_bytes=0), EINVAL),
             ("frame_type 3", dict(frame_type=3), EINVAL)]
# all nine (table type, frame type) pairs: the empty call (before the workspace is looked at), null ids
ARG_CASES += T.pair_rows([("n 0, no workspace", dict(n=0, parts=0, ws=None, ws_bytes=0), OK),
                          ("null ids", dict(ids=None), EINVAL)])
# per table type: what _split_ft rejects
ARG_CASES += T.table_rows(TABLE_TYPES, [("null table", dict(table=None), EINVAL),
                                        ("no weights", dict(wtab32=None), EINVAL),
                                        ("workspace one byte short", dict(ws_bytes=ONE_SHORT), EINVAL),
                                        ("null workspace", dict(ws=None), EINVAL),
                                        ("parts -1", dict(parts=-1), EINVAL),
                                        ("D 512", dict(d=512), EINVAL),  # past the finish kernel's columns
                                        ("bounds with n 8193", dict(colmax=P, colmax_ws=P, n=SF.MAX_BOUND_ROWS + 1),
                                         EINVAL),
                                        ("bounds without workspace", dict(colmax=P), EINVAL),
                                        ("s_half 2", dict(s_half=2), EINVAL)])
# a 16-bit table: never from an odd address; 2 and 4 bytes off are the scalar
# route (d up to 320: D = 300 passes the checks, D = 324 does not), 8 bytes off whole units
ARG_CASES += T.table_rows(TABLE_TYPES16, [("table 1 byte off", dict(table=P + 1), EINVAL),
                                          ("table 1 byte off, n 0", dict(table=P + 1, n=0), EINVAL),
                                          ("table 2 bytes off, n 0", dict(table=P + 2, n=0), OK),
                                          ("table 4 bytes off, n 0", dict(table=P + 4, n=0), OK),
                                          ("table 2 bytes off, D 324", dict(table=P + 2, d=324), EINVAL),
                                          ("table 4 bytes off, D 324", dict(table=P + 4, d=324), EINVAL)])
# the frames' own rule, under a 16-bit table
ARG_CASES += [(f"{tn} table, {what}", dict(table_type=tt, **change), want)
              for tn, tt in TABLE_TYPES16
              for what, change, want in F.arg_rows(F.TYPES16, [("audio at an odd address", dict(audio=P + 1), EINVAL),
                                                               ("visual at an odd address, n 0",
                                                                dict(visual=P + 1, n=0), EINVAL)])]
