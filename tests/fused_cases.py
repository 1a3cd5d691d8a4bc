"""The shape table of the fused stream + projection kernel's row-tail layout:
the cases of tests/test_gpu_fused_tail.py, which tests/fused_frames16_cases.py
and tests/fused_table16_cases.py run again on 16-bit frames and tables and
tests/test_gpu_scratch.py on poisoned scratch.  The module docstring of
tests/test_gpu_fused_tail.py says why these shapes.  Plain helper module: no
test is collected from it.
"""
V = 5000

# (D, A, Vd, T, N, bad ids)
CASES = [
    (256, 300, 4, 40, 49, False),     # text without a tail, next to a tailed and a 1-lane piece
    (256, 20, 260, 7, 13, False),     # one partial group per row: the group-at-a-time fallback
    (260, 256, 320, 33, 97, False),   # 4-float tail | none | all 64 tail lanes; partial last group
    (260, 320, 20, 17, 13, False),    # 3 groups of 8 frames (8 + 8 + 1)
    (300, 260, 256, 16, 49, False),   # 2 groups of 8: below the 8-frame rule
    (300, 4, 320, 64, 97, False),     # T = 64: every lane of the token stage in use
    (300, 320, 260, 40, 1, False),    # a single row
    (316, 300, 20, 21, 49, False),    # 3 groups of 10 frames (10 + 10 + 1)
    (316, 256, 260, 20, 13, False),   # 2 groups of 10: below the 10-frame rule
    (316, 320, 4, 1, 97, False),      # one frame per row
    (300, 256, 300, 40, 2500, False),  # 53 batches, the last of 4 rows
    (300, 260, 320, 40, 97, True),    # a negative and an out-of-range id
]


def _ids(c):
    return "D{}-A{}-V{}-T{}-N{}{}".format(*c[:5], "-bad" if c[5] else "")
