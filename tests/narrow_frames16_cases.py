"""Shared tables of tests/test_gpu_narrow_frames16.py (GPU) and
tests/test_narrow_frames16_cases.py (CPU): the narrow fused kernel on audio /
visual frames kept in fp16 / bf16 storage (mmb_mm2_stream_project_narrow_ft,
pipeline.mm2_stream_project_narrow_ft, FusedStep(narrow_frames16=True)).
Plain helper module: no test is collected from it.

The definition under test is frames16_cases': a launch on 16-bit frames
writes, bit for bit, what the same launch writes on those frames upcast to
f32 -- here for every output of the narrow fused kernel: x, the three aux
planes, the MMB2 rows, the column bounds and the flag word.
"""
from __future__ import annotations

import frames16_cases as F
from frames16_cases import BF16, EINVAL, F32, OK, P

KINDS = F.KINDS
D = 300
WAVE = 64

# (A, Vd, T, N, V): the smallest shapes that reach each way the packed frame
# loads can go wrong.  A frame instruction loads P = 64 // (W / 4) rows of a
# W-wide modality, lane = f (W / 4) + c; the first kNFGA = 7 audio / kNFGV = 4
# visual groups are issued with the text loads, later groups in loops; the
# launch runs 1, 2 or 4 utterances per wave and batch by N (256 CUs: below
# ~4k, ~4-8k, above).
KERNEL_CASES = [
    (76, 48, 20, 3000, 3016),    # MOSI: P = 3 / 5, partial last groups, 1 utterance per wave
    (76, 48, 20, 6000, 3016),    # 2 utterances per wave
    (76, 48, 20, 8200, 3016),    # 4 utterances per wave; last batch of 8 rows
    (76, 48, 20, 1, 3016),
    (76, 48, 20, 5, 3016),
    (76, 48, 20, 31, 3016),
    (76, 48, 20, 77, 17),        # fewer words than hot slots
    (76, 48, 64, 517, 5000),     # 22 audio groups: the later-group loops run
    (64, 56, 64, 517, 5000),     # U = 16: all 64 lanes live
    (20, 8, 7, 64, 300),
    (44, 76, 33, 259, 16384),
    (4, 4, 1, 5, 3016),          # U = 1, P = 64, T = 1
    (112, 16, 40, 1001, 3016),   # P = 2; kq = 256, the widest frames the kernel takes
]
MAX_ROWS = 8200
# wrapped negative ids, an id >= V (flagged), an utterance whose weights are all 0 (flagged)
BAD_CASES = [(76, 48, 20, 3000, 3016), (64, 56, 64, 517, 5000)]
LOAD_GROUPS = (7, 4)  # kNFGA, kNFGV


def rows_per_instruction(w: int) -> int:
    return WAVE // (w // 4)


def groups(t: int, w: int) -> int:
    p = rows_per_instruction(w)
    return -(-t // p)


def rows_per_wave(n: int, cus: int = 256) -> int:
    """The launcher's choice: 4 once that fills every CU, fewer for small N."""
    rpw = 4
    while rpw > 1 and -(-n // (8 * rpw)) < cus:
        rpw -= 1
    return rpw


# The 16-bit frame tensors are views into a larger allocation whose other
# elements hold GUARD: a descriptor range or an offset computed in the wrong
# unit then shows at the first and the last utterance too, and a partial last
# group reads non-zero neighbours unless the range is right.  (2^14 is exact
# in both kinds; a single one moves a U(-1, 1) frame sum far past rounding.)
GUARD = 2.0 ** 14


def guard_elements(t: int, w: int) -> int:
    """Guard elements on either side: two whole rows of frames, so that a range
    taken in f32 bytes still lies inside the allocation; a multiple of 8
    elements (16 bytes)."""
    return -(-2 * t * w // 8) * 8


# special values (frames16_cases.special_frames): MOSI's widths and the
# narrowest rows (U = 1: every lane another frame); N >= 3, T >= 4
SPECIAL_CASES = [(D, 76, 48, 20, 5, 3016), (D, 4, 4, 7, 5, 300)]

# the step compared with its f32 narrow fused twin and the oracle: (D, A, Vd, T, N, V)
STEP = (D, 76, 48, 20, 3000, 3016)
# steps whose plan the keyword leaves alone, as (name in frames16_cases._shapes, why)
PLAN_UNCHANGED = {"c3": "wide frames", "pom": "T > 64", "mid": "wide frames"}

# ---------------------------------------------------------------- the argument table
ARGS = ("ids table v wtab32 text_cache audio visual frame_type n t d a vd wpieces c0 num_out aux_out "
        "mmb2_out flag colmax colmax_ws stream").split()
BASE = dict(ids=P, table=P, v=3016, wtab32=P, text_cache=P, audio=P, visual=P, frame_type=BF16, n=100,
            t=20, d=D, a=76, vd=48, wpieces=P, c0=P, num_out=P, aux_out=P, mmb2_out=P, flag=None,
            colmax=None, colmax_ws=None, stream=None)
ARG_CASES = [("frame_type -1", dict(frame_type=-1), EINVAL),
             ("frame_type 3", dict(frame_type=3), EINVAL)]
ARG_CASES += F.arg_rows(F.ALL_TYPES, [("n 0", dict(n=0), OK),
                                      ("audio 4 bytes off", dict(audio=P + 4), EINVAL),
                                      ("visual 4 bytes off", dict(visual=P + 4), EINVAL),
                                      ("null ids", dict(ids=None), EINVAL),
                                      ("null text cache", dict(text_cache=None), EINVAL),
                                      ("null wpieces", dict(wpieces=None), EINVAL),
                                      ("A 128 Vd 100", dict(a=128, vd=100), EINVAL),  # kq > 256
                                      ("V 16385", dict(v=16385), EINVAL),
                                      ("D 256", dict(d=256), EINVAL),
                                      ("D 304", dict(d=304), EINVAL)])
ARG_CASES += F.arg_rows(F.TYPES16, [
    ("audio 2 bytes off", dict(audio=P + 2), EINVAL),
    ("visual 2 bytes off", dict(visual=P + 2), EINVAL),
    # whole 8-byte units: past the checks (the empty call returns before any launch)
    ("n 0 frames 8 bytes off", dict(n=0, audio=P + 8, visual=P + 8), OK)])
# an f32 column unit is 16 bytes: half a unit off is whole units for the 16-bit types only
ARG_CASES.append(("f32 audio 8 bytes off", dict(frame_type=F32, audio=P + 8), EINVAL))
