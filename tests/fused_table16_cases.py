"""Shared tables of tests/test_gpu_fused_table16.py (GPU) and
tests/test_fused_table16_cases.py (CPU): the fused stream + projection kernel
on a word table kept in fp16 / bf16 storage (mmb_mm2_stream_project_tt,
pipeline.mm2_stream_project_tt, FusedStep(fused_table16=True)).  Plain helper
module: no test is collected from it.

The definition under test is table16_cases': a launch on a 16-bit table
writes, bit for bit, what the same launch writes on that table upcast to f32
-- here for every output of the fused kernel: x, the three aux planes, the
MMB2 rows, the column bounds and the flag word, for each of the three frame
types.
"""
from __future__ import annotations

import frames16_cases as F
import fused_cases as FT
import fused_frames16_cases as FF
import large_cases as LC
import table16_cases as T
from frames16_cases import EINVAL, F32, OK, P
from table16_cases import TABLE_TYPES, TABLE_TYPES16

KINDS = T.KINDS

# (D, A, Vd, T, N, bad ids): the shapes of tests/fused_cases.py (tests/test_gpu_fused_tail.py), for its
# reasons -- on a 16-bit table the b128 / b32 loads of a text row become a b64
# and a b16 load with their own lane offsets, clamps, row offsets and
# descriptor range, so the text widths (no tail, 4 / 44 / 60 tail lanes), the
# row lengths either side of the fallback | pipelined rule (20 | 21), the
# partial groups, the row counts and the bad ids are the same
KERNEL_CASES = list(FT.CASES)
KERNEL_V = FT.V
# the frames of a kernel case: f32, or the table's own kind
FRAME_CHOICES = T.FRAME_CHOICES
# the case run for all six new (table, frame) pairs: a text tail, both frame
# tails, a negative and an out-of-range id
ALL_PAIRS_CASE = (300, 260, 320, 40, 97, True)

# special values (table16_cases.special_table): one shape of the
# group-at-a-time fallback (T < 21), one of the pipelined streamer with a text
# tail (D = 260: the hot row's planted last columns are the b16 tail's)
SPECIAL_SHAPES = FF.SPECIAL_SHAPES
SPECIAL_N = FF.SPECIAL_N

# the step compared with its f32 fused twin and the oracle (in frames16_cases.STEP:
# tests/test_table16_cases.py pins the family's conditions on its upcast table)
STEP = FF.STEP
# steps whose plan the keyword leaves alone (narrow frames; T > 64)
STEP_UNCHANGED = FF.STEP_UNCHANGED

# the descriptor guard (fused_pipe_ok: V D sizeof(TE) < 2^31): a bf16 table of
# 2^22 rows at D = 256 is 2 GiB, the footprint of large_cases'
# fused_table_refused; V = 2^22 - 1 is the last size the pipelined streamer takes
GUARD_D, GUARD_T, GUARD_V = 256, 21, 2 ** 22
GUARD_LAST = LC.table_case("fused_tt_bf16_last", 5, "mmb_mm2_stream_project_tt", GUARD_D, GUARD_V - 1, tbytes=2,
                           t=GUARD_T)
GUARD_REFUSED = LC.table_case("fused_tt_bf16_refused", 5, "mmb_mm2_stream_project_tt", GUARD_D, GUARD_V, tbytes=2,
                              t=GUARD_T)

# ---------------------------------------------------------------- the argument table
ARGS = ("ids table table_type v wtab32 w_dense audio visual frame_type n t d a vd wpieces c0 num_out aux_out "
        "mmb2_out flag colmax colmax_ws stream").split()
BASE = dict(ids=P, table=P, table_type=TABLE_TYPES16[1][1], v=1000, wtab32=P, w_dense=None, audio=P, visual=P,
            frame_type=F32, n=100, t=40, d=300, a=300, vd=300, wpieces=P, c0=P, num_out=P, aux_out=P, mmb2_out=P,
            flag=None, colmax=None, colmax_ws=None, stream=None)
ARG_CASES = [("table_type -1", dict(table_type=-1), EINVAL),
             ("table_type 3", dict(table_type=3), EINVAL),
             ("table_type 3, n 0", dict(table_type=3, n=0), EINVAL),
             ("frame_type -1", dict(frame_type=-1), EINVAL),
             ("frame_type 3", dict(frame_type=3), EINVAL),
             ("frame_type 3, n 0", dict(frame_type=3, n=0), EINVAL)]
# all nine (table type, frame type) pairs: the empty call, and what _ft rejects for each
ARG_CASES += T.pair_rows([("n 0", dict(n=0), OK),
                          ("null ids", dict(ids=None), EINVAL),
                          ("num_out 8 bytes off", dict(num_out=P + 8), EINVAL)])
# per table type: the shapes and operands _ft rejects
ARG_CASES += T.table_rows(TABLE_TYPES, [("null table", dict(table=None), EINVAL),
                                        ("no weights", dict(wtab32=None), EINVAL),
                                        ("D 252", dict(d=252), EINVAL),
                                        ("D 320", dict(d=320), EINVAL),
                                        ("A 322", dict(a=322), EINVAL),
                                        ("T 65", dict(t=65), EINVAL),
                                        ("missing wpieces", dict(wpieces=None), EINVAL),
                                        ("wpieces 8 bytes off", dict(wpieces=P + 8), EINVAL),
                                        ("bounds without workspace", dict(colmax=P), EINVAL)])
# a 16-bit text column unit is 8 bytes: whole units from an 8-byte aligned base
ARG_CASES += T.table_rows(TABLE_TYPES16, [("table 2 bytes off", dict(table=P + 2), EINVAL),
                                          ("table 4 bytes off", dict(table=P + 4), EINVAL),
                                          ("table 4 bytes off, n 0", dict(table=P + 4, n=0), EINVAL),
                                          ("table 8 bytes off, n 0", dict(table=P + 8, n=0), OK)])
# an f32 text column unit is 16 bytes: half a unit off is whole units for the 16-bit types only
ARG_CASES.append(("f32 table 8 bytes off", dict(table_type=TABLE_TYPES[0][1], table=P + 8), EINVAL))
# the frames' own alignment, under a 16-bit table
ARG_CASES += [(f"{tn} table, {what}", dict(table_type=tt, **change), want)
              for tn, tt in TABLE_TYPES16
              for what, change, want in F.arg_rows(F.TYPES16, [("audio 4 bytes off", dict(audio=P + 4), EINVAL),
                                                               ("visual 2 bytes off", dict(visual=P + 2), EINVAL)])]
ARG_CASES += T.table_rows(TABLE_TYPES16, [("f32 audio 8 bytes off", dict(audio=P + 8), EINVAL)])
