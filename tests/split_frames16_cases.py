"""Shared tables of tests/test_gpu_split_frames16.py (GPU) and
tests/test_split_frames16_cases.py (CPU): the split stream on audio / visual
frames kept in fp16 / bf16 storage (mmb_mm2_stream_split_ft,
pipeline.mm2_stream_split_ft, FusedStep(split_frames16=True)).
Plain helper module: no test is collected from it.

The definition under test is frames16_cases': a launch on 16-bit frames
writes, bit for bit, what the same launch (the same parts) writes on those
frames upcast to f32 -- x, s, aux, the column bounds and the flag word.
"""
from __future__ import annotations

import frames16_cases as F
import narrow_frames16_cases as NF
from frames16_cases import BF16, EINVAL, OK, P

KINDS = F.KINDS
D, V = 300, 500
NT = 320            # threads of a split workgroup (kNT)
FINISH_COLUMNS = 2240  # kSplitJ * kNT: 3 d + 2 a + 2 vd of the finish kernel
MAX_BOUND_ROWS = 8192  # rows of the column-bound workspace
PLAN_MIN_T = 64     # the plan takes the split for t > 64 (and n <= CUs)
FRAME_UNROLLS = (8, 16)  # frames unrolled per thread group: the product's, and the other candidate

# The 16-bit frame tensors are views into larger allocations whose other
# elements hold GUARD (narrow_frames16_cases): a range or an offset in the
# wrong unit then shows at the first and the last utterance too.
GUARD, guard_elements = NF.GUARD, NF.guard_elements

# (N, T, A, Vd, parts, audio_off, visual_off): the smallest shapes at which
# the frame workgroups can still go wrong; *_off: the 16-bit view that many
# elements past a 16-byte boundary.  A frame workgroup of one modality and one
# range runs width / VF column units x NT // units row slots; slot r sums
# frames r, r + slots, .. of the range, unrolled FRAME_UNROLLS at a time.
KERNEL_CASES = [
    (5, 65, 300, 300, (1, 2, 0), 0, 0),  # T just past the plan's threshold; ranges of 33 / 32 on 4 slots
    (3, 200, 76, 48, (7,), 0, 0),        # 19 / 12 units, 16 / 26 slots, a short last range (26 frames)
    (4, 130, 4, 664, (3,), 0, 0),        # 1 unit x 320 slots, most empty | 166 units x ONE slot; widest a + vd
    (6, 97, 46, 37, (2,), 0, 0),         # widths % 4 != 0: scalar 2-byte loads
    (6, 97, 76, 48, (2,), 1, 4),         # audio 2 bytes off: scalar; visual 8 bytes off: whole units
]
# special values (frames16_cases.special_frames) on the vector and the scalar path: (D, A, Vd, T, N, V), parts
SPECIAL_CASES = [((D, 76, 48, 97, 5, V), 2), ((D, 46, 37, 97, 5, V), 2)]
# wrapped negative ids, an id >= V (flagged), an utterance whose weights are all 0 (flagged)
BAD_CASE = (6, 97, 76, 48, 2)
# the step: (N, T, A, Vd); POM's valid shape comes from the g11_pom_splits fixture
STEP = (12, 130, 300, 300)
POM_VALID = (100, 1089, 300, 300)


def case_of(n, t, a, vd):
    """The mmb2_cases case (D, A, Vd, T, N, V) of a row."""
    return (D, a, vd, t, n, V)


def vector(width: int, off_elements: int = 0, fbytes: int = 2) -> bool:
    """stream_vec's rule: whole 4-value units from a base aligned to one unit."""
    return width % 4 == 0 and (off_elements * fbytes) % (4 * fbytes) == 0


def slots(width: int, vec: bool) -> tuple[int, int]:
    """(column units, row slots) of a frame workgroup."""
    units = width // 4 if vec else width
    return units, NT // units


def ranges(t: int, parts: int) -> list[int]:
    """Frames per range of split_plan_of for an explicit part count."""
    lf = -(-t // min(parts, t))
    return [min(lf, t - s) for s in range(0, t, lf)]


# ---------------------------------------------------------------- the argument table
ARGS = ("ids table v wtab32 w_dense audio visual frame_type n t d a vd num_out s_out s_half aux_out "
        "flag colmax colmax_ws parts ws ws_bytes stream").split()
# parts > 0: parts = 0 asks the device for its CU count
BASE = dict(ids=P, table=P, v=1000, wtab32=P, w_dense=None, audio=P, visual=P, frame_type=BF16, n=100,
            t=1089, d=D, a=300, vd=300, num_out=P, s_out=P, s_half=1, aux_out=P, flag=None,
            colmax=None, colmax_ws=None, parts=2, ws=P, ws_bytes=1 << 40, stream=None)


ONE_SHORT = "one byte short"  # ws_bytes: filled in by resolve() (the size is the library's answer)


def ws_bytes(**kw):
    import mmb_lib

    a = dict(BASE, **kw)
    return mmb_lib.query("mmb_mm2_stream_split_ws_bytes", a["n"], a["t"], a["d"], a["a"], a["vd"], a["parts"])


def resolve(change: dict) -> dict:
    if change.get("ws_bytes") == ONE_SHORT:
        return dict(change, ws_bytes=ws_bytes(**{k: v for k, v in change.items() if k != "ws_bytes"}) - 1)
    return change


ARG_CASES = [("frame_type -1", dict(frame_type=-1), EINVAL),
             ("frame_type 3", dict(frame_type=3), EINVAL)]
ARG_CASES += F.arg_rows(F.ALL_TYPES, [
    ("null ids", dict(ids=None), EINVAL),
    ("workspace one byte short", dict(ws_bytes=ONE_SHORT), EINVAL),
    ("null workspace", dict(ws=None), EINVAL),
    ("parts -1", dict(parts=-1), EINVAL),
    ("D 512", dict(d=512), EINVAL),  # past the finish kernel's columns
    ("bounds with n 8193", dict(colmax=P, colmax_ws=P, n=MAX_BOUND_ROWS + 1), EINVAL),
    ("bounds without workspace", dict(colmax=P), EINVAL),
    ("n 0, no workspace", dict(n=0, parts=0, ws=None, ws_bytes=0), OK)])
ARG_CASES += F.arg_rows(F.TYPES16, [
    ("audio at an odd address", dict(audio=P + 1), EINVAL),
    ("visual at an odd address", dict(visual=P + 3), EINVAL),
    ("visual at an odd address, n 0", dict(visual=P + 1, n=0), EINVAL)])
