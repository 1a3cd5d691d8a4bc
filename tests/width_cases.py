"""Shared case tables and the input family of tests/test_gpu_widths.py (GPU)
and tests/test_width_cases.py (CPU): the SIF / PC kernels at widths other
than 300; and the bars of the SIF / PC path (EMB_TOL, F32_ROW, PC_BAR,
SOLVE_BAR), which every GPU test of that path imports from here or through
tests/common_gpu.py.  Plain helper module: no test is collected from it.

Input family X(n, d): rows with two planted directions (so npc = 2 has a
spectral gap) on 0.4 N(0, 1) noise, rounded to f32 and widened back, seeded
by the shape alone.  The CPU test pins how closely the CPU oracle's own two
routes agree on this family; the GPU bars rest on that.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import sif_oracle as O

N_OVERSAMPLES = 10
NPCS = (1, 2, 6)

# the bars the suite holds the SIF / PC path to, at 300 and at every other width
EMB_TOL = 1e-5        # sentence embeddings, row-relative
F32_ROW = 2.0 ** -23  # one f32 rounding (2^-24 of the element) with 2x margin, of the row's max
PC_BAR = {1: 1e-10, 2: 1e-10, 6: 1e-8}  # per npc: the drop-ins' PCs against the oracle's
SOLVE_BAR = {1: 1e-12, 2: 1e-10}        # per npc: the solvers against pc_from_gram of the same G, z0

# (n, d): what each shape reaches in the dispatch of csrc/gram_kernels.hip,
# csrc/pc_kernels.hip (X^T Omega, the solvers) and csrc/pc_remove_kernels.hip
SHAPES = [
    (2, 2), (40, 2),                        # smallest d; one solver workgroup; block wider than the space
    (3, 5), (600, 5),                       # d < k, transposed and direct
    (10, 11), (11, 11), (12, 12),           # around d = k
    (10, 16), (700, 16),                    # exactly one full tile
    (17, 17), (5000, 17),                   # 1-column last tile; odd d; > 4096 rows on the generic Gram
    (63, 64), (64, 64),                     # either side of n = d; removal PER = 1
    (200, 50), (4097, 100), (300, 200), (199, 200),  # GloVe widths; scalar rows at 50; gram_tri at 100
    (513, 128), (4097, 129),                # gram_small<12>; generic Gram at an odd width
    (255, 255), (256, 256), (700, 260),     # removal PER 1 -> 2; pc_remove1_kernel's edge
    (600, 299), (300, 301), (301, 301),     # odd neighbours of 300
    (4097, 304), (5000, 308),               # last int8-Gram width and the first past it
    (319, 320), (320, 320), (4097, 320),    # last multi-workgroup width, 20 workgroups
    (320, 321), (700, 321),                 # first single-workgroup width
    (330, 400), (4500, 400),                # generic X^T Omega (n > 320); generic Gram at d > 320
    (511, 512), (512, 512),                 # the maximum width
    (1, 300), (1, 512), (5, 400),           # tiny splits
]


def shape_id(s):
    return "n{}-d{}".format(*s)


def npcs_of(n, d):
    return [npc for npc in NPCS if npc <= min(n, d)]


def pc_cases():
    """(n, d, npc) over the table, npc <= min(n, d)."""
    return [(n, d, npc) for n, d in SHAPES for npc in npcs_of(n, d)]


def full_rank(n, d, npc):
    """The randomized-SVD block (k = npc + 10 columns) has full rank."""
    return min(n, d) >= npc + N_OVERSAMPLES


def transposed(n, d):
    """sklearn's transposed branch (fewer rows than features)."""
    return n < d


def make_x(n, d, seed=None):
    """The family's X [n, d]: f32-representable float64."""
    rng = np.random.default_rng(1000 * n + d if seed is None else seed)
    g = rng.standard_normal((2, d))
    c = rng.standard_normal((n, 1))
    X = 0.4 * rng.standard_normal((n, d)) + 0.3 * g[0] + 0.25 * c * g[1]
    return X.astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def x32(n, d):
    X = make_x(n, d)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def x64(n, d):
    """The f64-row input: X perturbed below f32 resolution (not f32-representable)."""
    rng = np.random.default_rng(3)
    X = x32(n, d) * (1.0 + 1e-6 * rng.standard_normal((n, d)))
    X.setflags(write=False)
    return X


def omega(rows, k):
    """RandomState(0).normal(size=(rows, k)): the randomized SVD's start block."""
    return np.random.RandomState(0).normal(size=(rows, k))


def start_block(X, npc):
    """(z0, transposed) of the device solver for X: Omega [d, k] (direct) or
    X^T Omega_n (transposed)."""
    n, d = X.shape
    k = npc + N_OVERSAMPLES
    if transposed(n, d):
        return X.T @ omega(n, k), True
    return omega(d, k), False


@functools.lru_cache(maxsize=None)
def _oracle_pc(n, d, npc, f64):
    pc = O.compute_pc(x64(n, d) if f64 else x32(n, d), npc)
    pc.setflags(write=False)
    return pc


def oracle_pc(n, d, npc, f64=False):
    """O.compute_pc of the family's X, computed once per case."""
    return _oracle_pc(n, d, npc, bool(f64))


def top_eigvecs(G, npc):
    """Top-npc eigenvectors of a Gram, rows, svd_flip'ed (largest |.| entry > 0)."""
    w, v = np.linalg.eigh(np.asarray(G, np.float64))
    v = v[:, ::-1][:, :npc].T
    idx = np.argmax(np.abs(v), axis=1)
    return v * np.sign(v[np.arange(npc), idx])[:, None]


def orthonormal_rows(npc, d, seed):
    """npc orthonormal f64 rows of width d (a given PC for the removal tests)."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((d, npc)))
    return np.ascontiguousarray(q.T)
