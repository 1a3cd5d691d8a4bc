"""Shared tables of tests/test_gpu_fused_frames16.py (GPU) and
tests/test_fused_frames16_cases.py (CPU): the fused stream + projection kernel
on audio / visual frames kept in fp16 / bf16 storage
(mmb_mm2_stream_project_ft, pipeline.mm2_stream_project_ft,
FusedStep(fused_frames16=True)).  Plain helper module: no test is collected
from it.

The definition under test is frames16_cases': a launch on 16-bit frames
writes, bit for bit, what the same launch writes on those frames upcast to
f32 -- here for every output of the fused kernel: x, the three aux planes, the
MMB2 rows, the column bounds and the flag word.
"""
from __future__ import annotations

import frames16_cases as F
import fused_cases as FT
from frames16_cases import BF16, EINVAL, F32, OK, P

KINDS = F.KINDS

# (D, A, Vd, T, N, bad ids): the shapes of tests/fused_cases.py (tests/test_gpu_fused_tail.py), for its
# reasons -- on 16-bit rows the b128 / b32 loads of a frame become a b64 and a
# b16 load with their own lane offsets, clamps and descriptor ranges, so the
# widths (no tail, 4 / 44 / 60 / 64 tail lanes, 1- and 5-lane pieces), the
# neighbour combinations the prefetch crosses, the row lengths either side of
# the fallback | pipelined rule (20 | 21) and the row counts are the same
KERNEL_CASES = list(FT.CASES)
KERNEL_V = FT.V

# the dynamic batch order (>= 16 rounds of 48-row batches on 256 CUs) with a
# 2-row last unit, and visual rows whose byte offsets pass 2^31 in 16-bit storage
LARGE = (300, 20, 260, 21, 200_018)

# special values (frames16_cases.special_frames): one shape of the
# group-at-a-time fallback (T < 21), one of the pipelined streamer with a text
# tail, both taken by the fused kernel; N >= 3
SPECIAL_SHAPES = [(256, 8, 12, 7), (260, 12, 8, 21)]
SPECIAL_N = 5

# the step compared with its f32 fused twin and the oracle (in frames16_cases.STEP:
# tests/test_frames16_cases.py pins the family's conditions on its upcast inputs)
STEP = (300, 300, 300, 40, 97)
# steps whose plan the keyword leaves alone (narrow frames; T > 64)
STEP_UNCHANGED = [(300, 76, 48, 20, 97), (50, 76, 48, 130, 16)]

# ---------------------------------------------------------------- the argument table
ARGS = ("ids table v wtab32 w_dense audio visual frame_type n t d a vd wpieces c0 num_out aux_out "
        "mmb2_out flag colmax colmax_ws stream").split()
BASE = dict(ids=P, table=P, v=1000, wtab32=P, w_dense=None, audio=P, visual=P, frame_type=BF16, n=100,
            t=40, d=300, a=300, vd=300, wpieces=P, c0=P, num_out=P, aux_out=P, mmb2_out=P, flag=None,
            colmax=None, colmax_ws=None, stream=None)
ARG_CASES = [("frame_type -1", dict(frame_type=-1), EINVAL),
             ("frame_type 3", dict(frame_type=3), EINVAL)]
ARG_CASES += F.arg_rows(F.ALL_TYPES, [("n 0", dict(n=0), OK),
                                      ("audio 4 bytes off", dict(audio=P + 4), EINVAL)])
ARG_CASES += F.arg_rows(F.TYPES16, [("null ids", dict(ids=None), EINVAL),
                                    ("audio 2 bytes off", dict(audio=P + 2), EINVAL),
                                    ("visual 4 bytes off", dict(visual=P + 4), EINVAL),
                                    ("D 252", dict(d=252), EINVAL),
                                    ("D 320", dict(d=320), EINVAL),
                                    ("A 322", dict(a=322), EINVAL),
                                    ("missing wpieces", dict(wpieces=None), EINVAL)])
# an f32 column unit is 16 bytes: half a unit off is whole units for the 16-bit types only
ARG_CASES.append(("f32 audio 8 bytes off", dict(frame_type=F32, audio=P + 8), EINVAL))
