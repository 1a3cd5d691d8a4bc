"""Shared tables of tests/test_gpu_narrow_table16.py (GPU) and
tests/test_narrow_table16_cases.py (CPU): the narrow fused kernel and its
text cache on a word table kept in fp16 / bf16 storage
(mmb_mm2_text_cache_tt, mmb_mm2_stream_project_narrow_tt,
pipeline.mm2_stream_project_narrow_tt, MMB2Projection.enable_text_cache(table16=True),
FusedStep(narrow_table16=True)).  Plain helper module: no test is collected
from it.

The definition under test is table16_cases': a launch on a 16-bit table
writes, bit for bit, what the same launch writes on that table upcast to f32
-- here the text cache byte for byte, and every output of the narrow fused
kernel (x, the three aux planes, the MMB2 rows, the column bounds, the flag
word), for frames of f32 or of the table's kind.
"""
from __future__ import annotations

import frames16_cases as F
import narrow_frames16_cases as NF
import table16_cases as T
from frames16_cases import EINVAL, F32, OK, P
from table16_cases import TABLE_TYPES, TABLE_TYPES16

KINDS = T.KINDS
D = NF.D
FRAME_CHOICES = T.FRAME_CHOICES  # the frames of a kernel case: f32, or the table's own kind

# ---------------------------------------------------------------- the text cache
# widths either side of nothing: the cache row is [E (d) | P (d + 1) | 0 pad] of 608 floats
CACHE_D = (260, 300)
# one word; fewer words than the 32 hot slots (the unwritten gap); one more than the slots; MOSI's table
CACHE_V = (1, 20, 33, 3016)
CACHE_ROW, CACHE_HOT = 608, 32  # kTextLdq, kTextHot
CACHE_FRAMES = (76, 48, 20)  # (A, Vd, T) of the merged projection the P half comes from
# the two pre-fills of the compared buffers: what a byte of the gap must still hold
CACHE_FILL16, CACHE_FILL32 = 0xA5, 0x3C
# beside table16_cases.SPECIALS (+-0, a subnormal, a large value): the non-finite values
CACHE_NONFINITE = (float("inf"), float("-inf"), float("nan"))


def cache_gap(v: int) -> tuple[int, int]:
    """The byte range mmb_mm2_text_cache leaves unwritten (include/mmb.h): the
    hot-word id slots v .. 31 of a table of v < 32 words; empty otherwise."""
    if v >= CACHE_HOT:
        return (0, 0)
    return (4 * (CACHE_ROW + 2) * v, 4 * ((CACHE_ROW + 1) * v + CACHE_HOT))


CACHE_ARGS = "table table_type v d wtab32 wm ldw cache stream".split()
# (no empty call: v > 0; an accepted call launches, so the table holds rejections only)
CACHE_BASE = dict(table=P, table_type=TABLE_TYPES16[1][1], v=3016, d=D, wtab32=P, wm=P, ldw=320, cache=P, stream=None)
CACHE_ARG_CASES = [("table_type -1", dict(table_type=-1), EINVAL),
                   ("table_type 3", dict(table_type=3), EINVAL)]
CACHE_ARG_CASES += T.table_rows(TABLE_TYPES, [("null table", dict(table=None), EINVAL),
                                              ("no weights", dict(wtab32=None), EINVAL),
                                              ("null wm", dict(wm=None), EINVAL),
                                              ("null cache", dict(cache=None), EINVAL),
                                              ("cache 8 bytes off", dict(cache=P + 8), EINVAL),
                                              ("V 0", dict(v=0), EINVAL),
                                              ("V 16385", dict(v=16385), EINVAL),
                                              ("D 302", dict(d=302), EINVAL),
                                              ("D 304", dict(d=304), EINVAL),
                                              ("ldw 300", dict(ldw=300), EINVAL)])
CACHE_ARG_CASES += T.table_rows(TABLE_TYPES16, [("table 1 byte off", dict(table=P + 1), EINVAL),
                                                ("table 3 bytes off", dict(table=P + 3), EINVAL)])

# ---------------------------------------------------------------- the kernel
# (A, Vd, T, N, V) of narrow_frames16_cases.KERNEL_CASES: 1 and 4 utterances per
# wave, a ragged last batch, fewer rows than a batch, 2 per wave
KERNEL_CASES = [c for c in NF.KERNEL_CASES if c[:3] == (76, 48, 20) and c[3] in (1, 31, 3000, 8200)]
SPECIAL_CASE = NF.SPECIAL_CASES[0]  # (D, A, Vd, T, N, V): MOSI's widths, table16_cases.special_table
BAD_CASE = NF.BAD_CASES[0]
ALIGN_CASE = (76, 48, 20, 31, 3016)  # the table 2 / 4 / 8 bytes off: not read by the launch

# the step compared with its f32-table twin and the oracle: (D, A, Vd, T, N, V)
STEP = NF.STEP
PLAN_UNCHANGED = NF.PLAN_UNCHANGED

# ---------------------------------------------------------------- the argument table
ARGS = ("ids table table_type v wtab32 text_cache audio visual frame_type n t d a vd wpieces c0 num_out aux_out "
        "mmb2_out flag colmax colmax_ws stream").split()
BASE = dict(NF.BASE, table_type=TABLE_TYPES16[1][1], frame_type=F32)
ARG_CASES = [("table_type -1", dict(table_type=-1), EINVAL),
             ("table_type 3", dict(table_type=3), EINVAL),
             ("table_type 3, n 0", dict(table_type=3, n=0), EINVAL),
             ("table_type -1, n 0", dict(table_type=-1, n=0), EINVAL),
             ("frame_type 3", dict(frame_type=3), EINVAL)]
# all nine (table type, frame type) pairs: the empty call, and null ids
ARG_CASES += T.pair_rows([("n 0", dict(n=0), OK),
                          ("null ids", dict(ids=None), EINVAL)])
# per table type: what _narrow_ft rejects
ARG_CASES += T.table_rows(TABLE_TYPES, [("null table", dict(table=None), EINVAL),
                                        ("no weights", dict(wtab32=None), EINVAL),
                                        ("null text cache", dict(text_cache=None), EINVAL),
                                        ("text cache 8 bytes off", dict(text_cache=P + 8), EINVAL),
                                        ("null wpieces", dict(wpieces=None), EINVAL),
                                        ("A 128 Vd 100", dict(a=128, vd=100), EINVAL),  # kq > 256
                                        ("V 16385", dict(v=16385), EINVAL),
                                        ("D 256", dict(d=256), EINVAL),
                                        ("D 304", dict(d=304), EINVAL),
                                        ("T 65", dict(t=65), EINVAL),
                                        ("f32 audio 8 bytes off", dict(audio=P + 8), EINVAL),
                                        ("bounds without workspace", dict(colmax=P), EINVAL)])
# the table is not read by the launch: a 16-bit one is held to its element (2 bytes)
ARG_CASES += T.table_rows(TABLE_TYPES16, [("table 1 byte off", dict(table=P + 1), EINVAL),
                                          ("table 1 byte off, n 0", dict(table=P + 1, n=0), EINVAL),
                                          ("table 2 bytes off, n 0", dict(table=P + 2, n=0), OK),
                                          ("table 4 bytes off, n 0", dict(table=P + 4, n=0), OK)])
# an f32 table stays _narrow_ft's: whole 16-byte units
ARG_CASES += [("f32 table 8 bytes off", dict(table_type=TABLE_TYPES[0][1], table=P + 8), EINVAL),
              ("f32 table 8 bytes off, n 0", dict(table_type=TABLE_TYPES[0][1], table=P + 8, n=0), EINVAL)]
# the frames' own alignment, under a 16-bit table
ARG_CASES += [(f"{tn} table, {what}", dict(table_type=tt, **change), want)
              for tn, tt in TABLE_TYPES16
              for what, change, want in F.arg_rows(F.TYPES16, [("audio 4 bytes off", dict(audio=P + 4), EINVAL),
                                                               ("visual 2 bytes off", dict(visual=P + 2), EINVAL)])]
