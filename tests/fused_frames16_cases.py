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
import mmb_lib
import test_gpu_fused_tail as FT

KINDS = F.KINDS

# (D, A, Vd, T, N, bad ids): the shapes of tests/test_gpu_fused_tail.py, for its
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
P = 0x7F0000001000  # a stand-in device pointer: 16-byte aligned, never dereferenced
ARGS = ("ids table v wtab32 w_dense audio visual frame_type n t d a vd wpieces c0 num_out aux_out "
        "mmb2_out flag colmax colmax_ws stream").split()
F32, F16, BF16 = mmb_lib.MMB_FRAMES_F32, mmb_lib.MMB_FRAMES_F16, mmb_lib.MMB_FRAMES_BF16
BASE = dict(ids=P, table=P, v=1000, wtab32=P, w_dense=None, audio=P, visual=P, frame_type=BF16, n=100,
            t=40, d=300, a=300, vd=300, wpieces=P, c0=P, num_out=P, aux_out=P, mmb2_out=P, flag=None,
            colmax=None, colmax_ws=None, stream=None)
EINVAL, OK = -1, 0
ARG_CASES = [("frame_type -1", dict(frame_type=-1), EINVAL),
             ("frame_type 3", dict(frame_type=3), EINVAL)]
for _name, _ft in (("f32", F32), ("f16", F16), ("bf16", BF16)):
    ARG_CASES.append((f"{_name} n 0", dict(frame_type=_ft, n=0), OK))
    ARG_CASES.append((f"{_name} audio 4 bytes off", dict(frame_type=_ft, audio=P + 4), EINVAL))
for _name, _ft in (("f16", F16), ("bf16", BF16)):
    ARG_CASES += [(f"{_name} null ids", dict(frame_type=_ft, ids=None), EINVAL),
                  (f"{_name} audio 2 bytes off", dict(frame_type=_ft, audio=P + 2), EINVAL),
                  (f"{_name} visual 4 bytes off", dict(frame_type=_ft, visual=P + 4), EINVAL),
                  (f"{_name} D 252", dict(frame_type=_ft, d=252), EINVAL),
                  (f"{_name} D 320", dict(frame_type=_ft, d=320), EINVAL),
                  (f"{_name} A 322", dict(frame_type=_ft, a=322), EINVAL),
                  (f"{_name} missing wpieces", dict(frame_type=_ft, wpieces=None), EINVAL)]
