"""Byte patterns, the poisoning helper and the case tables of
tests/test_gpu_scratch.py (GPU) and tests/test_scratch_cases.py (CPU): no
kernel's output may depend on what its scratch, its outputs or a derived
weight image held before the launch (the rule at the top of include/mmb.h).
Plain helper module: no test is collected from it.

Three byte patterns, filled over a buffer's uint8 view:

  pattern  byte  f32              f64               fp16  bf16    int32       uint32
  Z        0x00  0                0                 0     0       0           0
  N        0xFF  NaN              NaN               NaN   NaN     -1          4294967295
  H        0x7F  finite, 3.39e38  finite, 1.38e306  NaN   finite  2139062143  2139062143

N alone is not enough: fmaxf drops a NaN, so an unwritten per-wave maximum
filled with N would go unseen.  H is a huge finite positive value that wins
every max and overflows every sum.

Protected regions.  A word that workgroups synchronise on is never poisoned,
whoever zeroes it: a dirty one makes workgroups wait out their ~1 s timeout,
which tests/test_gpu_robustness.py covers on purpose and nothing here adds to:
  * bytes [0, 16) of the mmb_pc_solve_mc workspace (arrival counter, abort
    word, squaring counter: solve_keep);
  * the last 16 bytes of mmb_mm2_colmax_ws_bytes(d) (the batch counter of
    mmb_mm2_stream_project: colmax_ws_keep);
  * the whole mmb_mlp_train workspace (never poisoned: checked to read zero
    after a launch instead).
Every other region poisoned here was checked against its launcher: the Gram
partials (gram_kernels.hip), the split stream's and the split-K projection's
partial rows, the per-wave column maxima below that counter, the word
likelihood's per-wave partials, mmb_mlp_backward's dh_ws and the solve
workspace past byte 16 (tiles, G2, z0) hold data only; the only global words a
kernel spins on are the three regions above (the fused kernels' other waits
are on LDS words).

The shape families are imported, not copied: a case named here is a member of
mmb2_cases / width_cases / word_cases / regressor_cases / frames16_cases, and
tests/test_scratch_cases.py checks each membership and each Gram route.
"""
from __future__ import annotations

import numpy as np

import frames16_cases as F
import mmb2_cases as C
import regressor_cases as R
import width_cases as W
import word_cases as WC

# ---------------------------------------------------------------- patterns
PATTERNS = {"Z": 0x00, "N": 0xFF, "H": 0x7F}
POISONS = ("N", "H")  # compared with the Z run


def _bytes_of(buf):
    """The flat uint8 view of a contiguous torch tensor or numpy array."""
    if isinstance(buf, np.ndarray):
        assert buf.flags.c_contiguous
        return buf.reshape(-1).view(np.uint8)
    import torch

    assert buf.is_contiguous()
    return buf.reshape(-1).view(torch.uint8)


def poison(buf, pattern, keep_zero=()):
    """Fill every byte of `buf` with the pattern's byte, then zero the byte
    ranges [lo, hi) of `keep_zero` (the protected regions).  Returns buf."""
    b = _bytes_of(buf)
    n = b.shape[0]
    if isinstance(b, np.ndarray):
        b[...] = PATTERNS[pattern]
    else:
        b.fill_(PATTERNS[pattern])
    for lo, hi in keep_zero:
        assert 0 <= lo <= hi <= n, (lo, hi, n)
        if isinstance(b, np.ndarray):
            b[lo:hi] = 0
        else:
            b[lo:hi].zero_()
    return buf


def same_bytes(a, b):
    """Equality of the uint8 views: a NaN row equals itself, +0 differs from -0."""
    a, b = _bytes_of(a), _bytes_of(b)
    if a.shape != b.shape:
        return False
    if isinstance(a, np.ndarray):
        return bool(np.array_equal(a, np.asarray(b)))
    import torch

    return bool(torch.equal(a, b))


def solve_keep(d=None):
    """The control words of the mmb_pc_solve_mc workspace."""
    return ((0, 16),)


def colmax_ws_keep(nbytes):
    """The batch counter at the end of mmb_mm2_colmax_ws_bytes(d) = nbytes."""
    return ((nbytes - 16, nbytes),)


# ---------------------------------------------------------------- 1: Gram
def gram_route(n, d, aligned=True):
    """mmb_gram's dispatch (csrc/gram_kernels.hip): one launch without partials
    for small splits, the 16x16-tile row-range kernel for float4 rows, the
    64x64-block kernel for everything else."""
    if n <= 4096 and d <= 320:
        return "small"
    if d % 4 == 0 and d <= 320 and aligned:
        return "tri"
    return "generic"


GRAM_TRI = [(4097, 300), (4100, 4), (5000, 320)]
GRAM_GENERIC = [(4097, 17), (700, 321), (64, 512)]
GRAM_F64 = [(700, 321), (5, 17)]          # mmb_gram_f64: always the generic kernels
GRAM_SMALL = [(7, 300)]                   # no partials: the workspace is never read
GRAM_PARTS = (5000, 300)                  # (n_plan, d) of mmb_gram_part + mmb_gram_finish
GRAM_PART_CHUNKS = [[100], [1, 4999], [0, 5000]]  # [0, 5000]: an empty first chunk at accumulate = 0
GRAM_I8 = [(7, 300), (65, 4), (5000, 304), (40000, 16)]  # the last: past one 32768-row range
GRAM_I8_RANGE_ROWS = 32768
GRAM_CONTROL = (5000, 300)                # mmb_gram_finish on a poisoned workspace, no part before it

# ---------------------------------------------------------------- 2: stream kernels
# (shape (D, A, Vd, T), N or None for the case's default, the mmb2_cases list it belongs to)
STREAM_CASES = [
    (C.WAVE_ROWS_SHAPE, 1, "WAVE_D256"), (C.WAVE_ROWS_SHAPE, 5, "WAVE_D256"),
    ((320, 20, 36, 21), None, "WAVE_D512"),
    ((260, 76, 48, 20), None, "NARROW_ROUTE"),
    ((50, 5, 3, 9), None, "WG_SCALAR_TEXT"), ((52, 4, 4, 513), 3, "WG_VECTOR_TEXT"),
]
STREAM_CU_EDGE = C.WG_CU_EDGE             # at N = CUs and CUs + 1
STREAM_MODES = ("ids+table", "dense+emb2")
STREAM_SPLIT = [(52, 8, 12, 70), (50, 5, 3, 70)]  # of mmb2_cases.COMBOS
STREAM_SPLIT_PARTS = (1, 3, 200, 0)
STREAM_FRAMES16 = [(52, 8, 12, 7), (50, 5, 3, 9)]  # a wave and a workgroup shape (frames16_cases.SPECIAL_SHAPES)

# ---------------------------------------------------------------- 3: split-K projection
PROJECT_D = (256, 300, 316)
PROJECT_FRAMES = ((8, 12), (300, 300))
PROJECT_T = 7
PROJECT_N = (2, 129, 300)
PROJECT_SLICES = (0, 2, 7, 57)            # 57 clamps to the K chunks at the narrow widths
PROJECT_ANCHOR = C.case_of((300, 8, 12, 7), 129)

# ---------------------------------------------------------------- 4: derived images
FUSED_TAIL_ROWS = (0, 2, 5)               # of tests/fused_cases.CASES
NARROW_FUSED = [(260, 76, 48, 20, 31, 3016), (280, 20, 8, 7, 64, 300)]  # of mmb2_cases.NARROW_FUSED
WORD_TABLE_D = (15, 17, 299)
WORD_TABLE_V = 33

# ---------------------------------------------------------------- 5: PC solve
SOLVE_MAX_D = 320


def solve_cases():
    """(n, d, npc) of tests/widths_gpu.SOLVE_CASES on the multi-workgroup solver."""
    return [(n, d, npc) for n, d, npc in W.pc_cases() if npc in (1, 2) and 1 < d <= SOLVE_MAX_D]


SOLVE_XT = [(7, 300), (100, 300), (229, 300), (12, 64)]
SOLVE_ANCHOR = (700, 260, 1)

# ---------------------------------------------------------------- 6: word likelihood
WORD_CASES = [WC.WordCase(4, 15, 1, 1, 0), WC.WordCase(15, 1, 16, 5, 0), WC.WordCase(17, 517, 1, 1, 0),
              WC.WordCase(299, 33, 17, 5, 0), WC.WordCase(320, 517, 33, 5, 0)]

# ---------------------------------------------------------------- 7: regressor
BACKWARD_CASES = [R.FWD_CASES[0], R.FWD_CASES[len(R.FWD_CASES) // 2], R.FWD_CASES[-1]]
BACKWARD_WANTS = ("all", "no_dx", "no_params")
TRAIN_CASES = [R.TRAIN_CASES[0], R.TrainCase(300, 40, 1, 32, 35, 0, 1, 0, 14),
               R.TrainCase(448, 33, 1, 32, 33, 0, 1, 0, 26)]
TRAIN_SMALLER = R.TRAIN_CASES[0]          # relaunched on the workspace a larger case left

# ---------------------------------------------------------------- 9: the whole step
# name -> ((D, A, Vd, T, N, V), FusedStep keywords, the plan fields it must be on)
STEPS = {
    "fused": ((300, 300, 300, 40, 97, C.DEFAULT_V), {}, {"front": "fused"}),
    "narrow_fused": ((300, 76, 48, 20, 97, 3016), {}, {"front": "narrow_fused"}),
    "stream_i8": (C.STEP[2] + (C.DEFAULT_V,), {"gram_kind": "i8"},
                  {"front": "stream", "split": False, "gram": "i8"}),
    "split_fork": (C.DROP_IN[1][:5] + (C.DEFAULT_V,), {},
                   {"front": "stream", "split": True, "project": "fork", "proj_split": True}),
}
# the buffers of a FusedStep that are filled between runs (colmax_ws and
# solve_ws except their protected words); inputs, parameters and flag are not
STEP_BUFFERS = ("x", "s", "G", "pc_buf", "sif", "mmb2", "aux_flat", "colmax_ws", "split", "proj_split",
                "solve_ws")


def frames16_kinds():
    return tuple(F.KINDS)
