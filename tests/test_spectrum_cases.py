"""CPU: the conditions the GPU bars of tests/test_gpu_spectrum.py rest on.

The GPU tests hold the device PC on spectra with a dominant component to
max(floor, 8 dev) of oracle.sif_oracle.compute_pc, dev being the difference
between the CPU oracle's own two routes (compute_pc on X, pc_from_gram on
X^T X), and exempt a component from that comparison where 8 dev is past the
1e-9 cap.  That is a statement about the kernels only while, on every case of
tests/spectrum_cases.py:

  * the first component's dev is far below its 1e-12 floor (bar here 1e-13;
    measured <= 2.6e-15 on the planted and mean families).  `pair` is the one
    family whose first component is itself ill-conditioned (eps / gap): its
    dev is 1e-11 to 8.2e-11 at gap = 1e-6 and it is held to the cap rule
    instead, with nothing exempt;
  * the exemption covers only what spectrum_cases.allowed_exempt admits: the
    second component of `spike` at R >= 1e8 (measured dev 5e-11 to 1.4e-10
    at R = 1e8, where only the shapes past 1.25e-10 are exempt, and 5e-9 to
    1.9e-8 at R = 1e10, all exempt) and, with the int8 Gram, the later
    components of `mean` at c = 300 (model error 3.1e-10 / 1.4e-9 at
    (4096, 300), 1.8e-9 / 7.1e-9 at (2048, 64));
  * the f32 rounding did not flatten the planted spectrum (realised l1 / l11
    within a factor 2 of the nominal R) and each family's documented gaps hold;
  * pc_from_gram is invariant under a power-of-two scale of X.

Worst dev measured for everything else: geom 2.5e-12 (sixth component,
R = 1e10), spike second component at R <= 1e6 2.1e-12, mean 6.0e-11 (third
component, c = 300), pair 8.2e-11 (gap = 1e-6).  The file takes about 25 s.
"""
import numpy as np
import pytest

import spectrum_cases as S
import width_cases as W
from oracle import sif_oracle as O

FAMILIES = ("spike", "geom", "mean", "pair")


def test_tables_are_the_issue_tables():
    assert S.SHAPES == [(4096, 300), (180, 300), (700, 64), (40, 64), (600, 400), (330, 400)]
    assert S.RS == (1e2, 1e3, 1e4, 1e5, 1e6, 1e8, 1e10)
    assert S.MEAN_CS == (0.3, 3.0, 30.0, 300.0) and S.GAPS == (0.5, 1e-2, 1e-4, 1e-6)
    assert S.NPCS == {"spike": (1, 2), "geom": (1, 2, 6), "mean": (1, 2, 3), "pair": (1, 2)}
    assert (S.FLOOR, S.CAP, S.MARGIN) == ((1e-12, 1e-10), 1e-9, 8.0)
    assert len(S.solver_cases()) == 6 * (7 * 2 + 7 * 3 + 4 * 3) and len(S.pair_cases()) == 24


def test_families_are_seeded_by_shape_and_f32_representable():
    for fam, p in (("spike", 1e6), ("geom", 1e6), ("mean", 30.0)):
        X = S.make((fam, 40, 64, p))
        assert X.dtype == np.float64 and np.array_equal(X.astype(np.float32).astype(np.float64), X)
    X = S.make(("pair", 180, 300, 1e-6))  # kept in f64 so the gap survives
    assert not np.array_equal(X.astype(np.float32).astype(np.float64), X)
    assert np.array_equal(S.mean(40, 64, 3.0), S.make(("mean", 40, 64, 3.0)))
    assert not np.array_equal(S.mean(41, 64, 3.0)[:40], S.mean(40, 64, 3.0))


def test_bar_rule():
    b = S.bars_of([3e-15, 2e-14, 2e-11, 1.2e-10, 1.3e-10])
    assert b == [(1e-12, False), (1e-10, False), (1.6e-10, False), (9.6e-10, False), (1e-9, True)]
    assert S.bars_of([2e-13])[0] == (1.6e-12, False)


@pytest.mark.parametrize("fam", FAMILIES)
def test_reference_routes_and_exempt_list(fam):
    worst = {}
    for case in S.family_cases(fam):
        for npc in S.NPCS[fam]:
            dv = S.dev(case, npc)
            for c, (d_c, (bar, exempt)) in enumerate(zip(dv, S.bars_of(dv))):
                if c == 0 and fam != "pair":
                    assert d_c <= 1e-13, (case, npc, d_c)
                if exempt:
                    assert S.allowed_exempt(case, c), (case, npc, c, d_c)
                else:
                    worst[c] = max(worst.get(c, 0.0), d_c)
                    assert S.FLOOR[min(c, 1)] <= bar <= S.CAP
                if fam == "spike" and c == 1 and case[3] >= 1e10:
                    assert exempt, (case, d_c)  # eps l1/l2 = 1.4e-7 of a unit vector's entries
                if fam == "spike" and c == 1 and case[3] <= 1e6:
                    assert d_c <= 1e-11, (case, d_c)
    print(f"{fam}: worst dev of the compared components",
          {c: f"{v:.1e}" for c, v in sorted(worst.items())})
    lim = {"spike": 1.25e-10, "geom": 1e-11, "mean": 1.25e-10, "pair": 1.25e-10}[fam]
    assert max(worst.values()) <= lim


def test_exempt_list_int8_gram():
    for case in S.i8_cases():
        for npc in S.NPCS["mean"]:
            ref, alt = S.i8_refs(case, npc)
            dv = np.abs(ref - alt).max(axis=1)
            assert dv[0] <= 1e-11, (case, dv)  # measured <= 3.8e-12
            for c, (bar, exempt) in enumerate(S.bars_of(dv)):
                assert not exempt or S.allowed_exempt(case, c, i8=True), (case, npc, c, dv[c])
    dv = np.abs(np.subtract(*S.i8_refs(("mean", 2048, 64, 300.0), 3))).max(axis=1)
    print("int8 model error at (2048, 64), c = 300:", dv)
    assert S.bars_of(dv)[2][1]  # the third component is past the cap: measured 7.1e-9


@pytest.mark.parametrize("fam", FAMILIES)
def test_realised_spectra(fam):
    for case in S.family_cases(fam):
        _, n, d, p = case
        w = S.eig_desc(S.make(case))
        if fam in ("spike", "geom"):
            assert 0.5 * p <= w[0] / w[10] <= 2.0 * p, (case, w[0] / w[10])
        if fam == "spike":   # l1/l2 = R/16, l2/l3 = 4: later components still separated
            assert abs(w[0] / w[1] / (p / 16) - 1) < 1e-3 and abs(w[1] / w[2] / 4 - 1) < 1e-3
            assert w[2] / w[3] > 3.9
        elif fam == "geom":  # evenly spread: l1/l2 = R^(1/10) while the block's condition is R
            r = p ** 0.1
            assert np.abs(w[:10] / w[1:11] / r - 1).max() < 1e-3, case
        elif fam == "mean":  # l1/l2 ~ 4 c^2 from c = 3 on; three separated components
            if p >= 3:
                assert 0.75 < w[0] / w[1] / (4 * p * p) < 1.1, (case, w[0] / w[1])
                assert w[1] / w[2] > 2.5
            else:
                assert 2.5 < w[0] / w[1] < 2.8
            assert w[2] / w[3] > 8, (case, w[2] / w[3])
        else:                # the f64 rows keep the gap: l1/l2 - 1 = gap
            assert abs((w[0] / w[1] - 1) / p - 1) < 1e-3, (case, w[0] / w[1] - 1)
            assert w[1] / w[2] > 5000


@pytest.mark.parametrize("fam", FAMILIES)
def test_pc_from_gram_is_scale_invariant(fam):
    """X -> 2^s X scales G by 2^(2s) and the transposed start block by 2^s,
    exactly; the oracle's second route returns the same PC (measured: bit-equal)."""
    worst = 0.0
    for case in S.family_cases(fam):
        X = S.make(case)
        npc = S.max_npc(case)
        z0, tr = W.start_block(X, npc)
        G = X.T @ X
        base = S.refs(case, npc)[1]
        for s in (-20, 20):
            pc = O.pc_from_gram(np.ldexp(G, 2 * s), np.ldexp(z0, s) if tr else z0, npc, tr)
            worst = max(worst, np.abs(pc - base).max())
    print(f"{fam}: largest change under 2^+-20: {worst:.1e}")
    assert worst <= 1e-15
