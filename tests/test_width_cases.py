"""CPU: the input family of tests/width_cases.py keeps the GPU bars of
tests/test_gpu_widths.py meaningful.

The GPU tests hold the device PC to 1e-10 (npc 1, 2) / 1e-8 (npc 6) of
oracle.sif_oracle.compute_pc.  That is a statement about the kernels only
while the CPU oracle's own two routes to the PC agree far below those bars
on the same inputs:

  * blocks of full rank (min(n, d) >= npc + 10): pc_from_gram (the device
    solver's algebra on the Gram) against compute_pc (sklearn's randomized
    SVD on X);
  * rank-deficient blocks: compute_pc against the exact top singular vectors
    (the block spans X's whole row space).

Measured over the whole table: 2.4e-15 / 2.6e-15 / 2.0e-13 (npc 1 / 2 / 6)
and 4.8e-15; the bar on both is 1e-12.  Someone who edits the family (or the
shape table) so that a case has no spectral gap fails here, on the CPU,
instead of chasing a GPU failure that no kernel caused.
"""
import numpy as np
import pytest

import width_cases as W
from oracle import sif_oracle as O

BAR = 1e-12


def test_table_is_the_issue_table():
    assert len(W.SHAPES) == len(set(W.SHAPES)) == 39
    assert max(n for n, _ in W.SHAPES) <= 5000 and max(d for _, d in W.SHAPES) == 512
    # every dispatch edge the table exists for is still in it
    ds = {d for _, d in W.SHAPES}
    assert {2, 5, 16, 17, 50, 100, 200, 256, 260, 299, 301, 304, 308, 320, 321, 400, 512} <= ds
    assert any(n > 4096 and d % 4 for n, d in W.SHAPES)      # generic Gram at an odd width
    assert any(320 < n < d for n, d in W.SHAPES)             # generic X^T Omega
    assert any(n < d <= 320 for n, d in W.SHAPES)            # wave X^T Omega


def test_family_is_f32_representable_and_seeded_by_shape():
    X = W.x32(63, 64)
    assert X.dtype == np.float64 and np.array_equal(X.astype(np.float32).astype(np.float64), X)
    assert np.array_equal(X, W.make_x(63, 64, seed=63064))
    assert not np.array_equal(W.make_x(64, 64)[:63], X)
    X64 = W.x64(63, 64)
    assert not np.array_equal(X64.astype(np.float32).astype(np.float64), X64)
    assert np.abs(X64 / X - 1).max() < 1e-5


def test_oracle_routes_agree_over_the_table():
    worst_full = {npc: 0.0 for npc in W.NPCS}
    worst_def = 0.0
    for n, d, npc in W.pc_cases():
        X = W.x32(n, d)
        ref = W.oracle_pc(n, d, npc)
        assert ref.shape == (npc, d)
        if W.full_rank(n, d, npc):
            z0, tr = W.start_block(X, npc)
            e = np.abs(O.pc_from_gram(X.T @ X, z0, npc, tr) - ref).max()
            worst_full[npc] = max(worst_full[npc], e)
        else:
            e = np.abs(ref - O.exact_top_pc(X, npc)).max()
            worst_def = max(worst_def, e)
        assert e < BAR, (n, d, npc, e)
    print("full-rank blocks, pc_from_gram vs compute_pc:",
          {k: f"{v:.1e}" for k, v in worst_full.items()},
          f"; rank-deficient, compute_pc vs exact: {worst_def:.1e} (bar {BAR})")


@pytest.mark.parametrize("npc", W.NPCS)
def test_top_eigvecs_of_the_gram_are_the_exact_pc(npc):
    """The rank-deficient solver cases compare with the Gram's top
    eigenvectors: on this family they are the exact PC far below that bar."""
    for n, d in [(3, 5), (10, 16), (600, 5), (5, 400)]:
        if npc > min(n, d):
            continue
        X = W.x32(n, d)
        assert np.abs(W.top_eigvecs(X.T @ X, npc) - O.exact_top_pc(X, npc)).max() < 1e-10
