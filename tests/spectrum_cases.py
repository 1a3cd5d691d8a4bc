"""Shared input families, case tables and bar rules of
tests/test_gpu_spectrum.py (GPU) and tests/test_spectrum_cases.py (CPU): the
PC solvers, the int8 Gram and the removals on spectra with a dominant
component.  Plain helper module: no test is collected from it.

Every family is seeded by the shape alone, default_rng(1000 n + d), and (but
for `pair`) rounded to f32 and widened back.

Bars.  The reference is O.compute_pc on X itself (sklearn's randomized SVD,
what the drop-ins promise); O.pc_from_gram on X^T X is the second CPU route.
dev(case, c) is the max-abs difference of the two on component c: what ANY
Gram-based route loses against the X-based one (about eps l1 / lc).  The GPU
bar of component c is max(floor_c, 8 dev(case, c)), floor_0 = 1e-12,
floor_c = 1e-10 (c >= 1), capped at 1e-9; the factor 8 is the margin for
another summation order and CholeskyQR in place of the oracle's MGS^2 -- a
multiple of a reference-measured quantity, never of the device's own error.
A (case, component) with 8 dev > 1e-9 is EXEMPT: held finite, of unit norm to
1e-12 and orthogonal to the earlier components to 1e-9 only.  The exemption
may cover only what allowed_exempt() admits; the CPU test pins that.
"""
from __future__ import annotations

import functools

import numpy as np

import width_cases as W
from oracle import sif_oracle as O

# (n, d): the smallest shapes that reach each solver path
SHAPES = [
    (4096, 300),  # direct, 19 workgroups, squared rounds
    (180, 300),   # transposed, mmb_pc_solve_mc and mmb_pc_solve_mc_xt
    (700, 64),    # direct, 4 workgroups
    (40, 64),     # transposed, narrow
    (600, 400),   # direct, pc_solve_kernel
    (330, 400),   # transposed, pc_solve_kernel
]
RS = (1e2, 1e3, 1e4, 1e5, 1e6, 1e8, 1e10)
MEAN_CS = (0.3, 3.0, 30.0, 300.0)
GAPS = (0.5, 1e-2, 1e-4, 1e-6)
NPCS = {"spike": (1, 2), "geom": (1, 2, 6), "mean": (1, 2, 3), "pair": (1, 2)}
PAIR_SHAPES = [(4096, 300), (180, 300), (600, 400)]
I8_SHAPES = [(4096, 300), (2048, 64)]

FLOOR = (1e-12, 1e-10)  # first / later components: width_cases.SOLVE_BAR
CAP = 1e-9              # the project's PC bar everywhere
MARGIN = 8.0
EXEMPT_FROM_R = 1e8


def case_id(case):
    fam, n, d, p = case
    return f"{fam}-n{n}-d{d}-{p:g}"


def family_cases(fam):
    if fam == "pair":
        return [("pair", n, d, g) for n, d in PAIR_SHAPES for g in GAPS]
    ps = MEAN_CS if fam == "mean" else RS
    return [(fam, n, d, p) for n, d in SHAPES for p in ps]


def solver_cases():
    """(case, npc) of GPU group 1."""
    return [(c, npc) for fam in ("spike", "geom", "mean") for c in family_cases(fam)
            for npc in NPCS[fam]]


def pair_cases():
    return [(c, npc) for c in family_cases("pair") for npc in NPCS["pair"]]


# ------------------------------------------------------------------ the families
@functools.lru_cache(maxsize=None)
def _factors(n, d):
    """(U [n, m], V [d, m]) orthonormal, m = min(n, d), and the generator past them."""
    rng = np.random.default_rng(1000 * n + d)
    m = min(n, d)
    U, _ = np.linalg.qr(rng.standard_normal((n, m)))
    V, _ = np.linalg.qr(rng.standard_normal((d, m)))
    return U, V


def _f32(X):
    return X.astype(np.float32).astype(np.float64)


def planted_s(n, d, R, kind):
    s = np.linspace(1.0, 0.5, min(n, d))
    if kind == "spike":   # l1/l2 = R/16, l2/l3 = 4: a dominant common component
        s[:3] = np.sqrt(R), 4.0, 2.0
    elif kind == "geom":  # l1/l11 = R spread evenly: the band the squared rounds square
        s[:11] = np.sqrt(R) ** (1.0 - np.arange(11) / 10.0)
    else:
        raise ValueError(kind)
    return s


def planted(n, d, R, kind):
    U, V = _factors(n, d)
    return _f32((U * planted_s(n, d, R, kind)) @ V.T)


def mean(n, d, c):
    """0.4 N(0, 1) + c g0 + 0.5 a1 g1 + 0.3 a2 g2: SIF rows with a common mean."""
    rng = np.random.default_rng(1000 * n + d)
    g = rng.standard_normal((3, d))
    a = rng.standard_normal((2, n, 1))
    return _f32(0.4 * rng.standard_normal((n, d)) + c * g[0] + 0.5 * a[0] * g[1]
                + 0.3 * a[1] * g[2])


def pair(n, d, gap):
    """A close top pair, l1/l2 = 1 + gap; kept in f64 so the gap survives."""
    U, V = _factors(n, d)
    s = np.linspace(1.0, 0.5, min(n, d))
    s[:2] = 100.0, 100.0 / np.sqrt(1.0 + gap)
    return (U * s) @ V.T


@functools.lru_cache(maxsize=8)
def make(case):
    fam, n, d, p = case
    X = {"spike": lambda: planted(n, d, p, "spike"), "geom": lambda: planted(n, d, p, "geom"),
         "mean": lambda: mean(n, d, p), "pair": lambda: pair(n, d, p)}[fam]()
    X.setflags(write=False)
    return X


def max_npc(case):
    return max(NPCS[case[0]])


# ------------------------------------------------------------------ the two CPU routes
@functools.lru_cache(maxsize=None)
def refs(case, npc):
    """(compute_pc(X), pc_from_gram(X^T X)) for the case, computed once."""
    X = make(case)
    ref = O.compute_pc(X, npc)
    z0, tr = W.start_block(X, npc)
    alt = O.pc_from_gram(X.T @ X, z0, npc, tr)
    for a in (ref, alt):
        a.setflags(write=False)
    return ref, alt


def dev(case, npc):
    """Per-component max-abs difference between the two CPU routes [npc]."""
    ref, alt = refs(case, npc)
    return np.abs(ref - alt).max(axis=1)


def bars_of(devs):
    """Per-component (bar, exempt) from per-component reference deviations."""
    out = []
    for c, dv in enumerate(np.atleast_1d(devs)):
        want = MARGIN * float(dv)
        out.append((min(max(FLOOR[min(c, 1)], want), CAP), want > CAP))
    return out


def bars(case, npc):
    return bars_of(dev(case, npc))


def allowed_exempt(case, c, i8=False):
    """The only (case, component) the exemption may cover: the second
    component of `spike` at R >= 1e8 (l1/l2 >= 6e6: eps l1/l2 is past the cap
    for any Gram-based route); with the int8 Gram, the later components of
    `mean` at c = 300 (the int8 Gram's CPU model is itself 3.1e-10 / 1.4e-9
    (second / third component, (4096, 300)) and 1.8e-9 / 7.1e-9 ((2048, 64))
    from the reference there)."""
    fam, _, _, p = case
    if i8:
        return fam == "mean" and c >= 1 and p == 300.0
    return fam == "spike" and c == 1 and p >= EXEMPT_FROM_R


def check_exempt_component(pc, c):
    """What an exempt component is still held to."""
    assert np.isfinite(pc[c]).all()
    assert abs(np.linalg.norm(pc[c]) - 1.0) < 1e-12, (c, np.linalg.norm(pc[c]))
    if c:
        o = np.abs(pc[:c] @ pc[c]).max()
        assert o < 1e-9, (c, o)


@functools.lru_cache(maxsize=None)
def i8_refs(case, npc):
    """(compute_pc(X), pc_from_gram(sliced_gram(X))): the int8 Gram's model error."""
    X = make(case)
    z0, tr = W.start_block(X, npc)
    return refs(case, npc)[0], O.pc_from_gram(O.sliced_gram(X), z0, npc, tr)


def i8_bars(case, npc):
    ref, alt = i8_refs(case, npc)
    return bars_of(np.abs(ref - alt).max(axis=1))


def i8_cases():
    return [("mean", n, d, c) for n, d in I8_SHAPES for c in MEAN_CS]


def eig_desc(X, k=12):
    w = np.linalg.eigvalsh(X.T @ X)[::-1]
    return w[:k]
