"""CPU: the case table of tests/word_cases.py keeps the GPU bars of
tests/test_gpu_word_widths.py meaningful.

The gradient of the angular word model holds 1 / sqrt(1 - cos^2): a cosine
near +-1 amplifies float32 rounding without bound, and then a GPU failure says
nothing about the kernel.  Every line of the table keeps the float64
reference's largest |cos| over every (latent, word) and (latent, token) pair
at or below 0.99.  Narrow tables (D = 4, 5) are where random directions come
that close, so those lines keep B V small.
"""
import numpy as np
import pytest

import word_cases as W


def test_table_is_the_issue_table():
    cs = W.WORD_CASES
    assert 18 <= len(cs) <= 26 and len(set(c[:-1] for c in cs)) == len(cs)
    assert {c.D for c in cs} == {4, 5, 15, 16, 17, 50, 100, 200, 299, 301, 304, 320}
    assert {c.V for c in cs} == {1, 15, 16, 17, 33, 517}
    assert {c.B for c in cs} == {1, 16, 17, 33} and {c.L for c in cs} == {1, 5}
    assert all(c.B * c.V <= 600 for c in cs if c.D <= 5)
    # every tile count the widths reach, and the widest the kernel serves
    assert {-(-c.D // 16) for c in cs} == {1, 2, 4, 7, 13, 19, 20}


@pytest.mark.parametrize("c", W.WORD_CASES, ids=[W.word_id(c) for c in W.WORD_CASES])
def test_case_keeps_clear_of_unit_cosines(c):
    z = W.make_inputs(c)
    for k in ("table", "lat", "dense", "w", "up"):
        assert np.array_equal(W.f32(z[k]), z[k])
    assert z["ids"].min() >= 0 and z["ids"].max() < c.V
    m = W.max_abs_cos(z)
    print(f"{W.word_id(c)}: largest |cos| {m:.3f}")
    assert m <= W.MAX_COS


def test_reference_is_finite_and_read_only():
    c = W.WORD_CASES[1]
    for dense in (False, True):
        z, lp, g = W.reference(c, dense)
        assert lp.shape == (c.B,) and g.shape == (c.B, c.D)
        assert np.isfinite(lp).all() and np.isfinite(g).all() and np.abs(g).max() > 0
        assert not lp.flags.writeable and not z["table"].flags.writeable
    assert not np.array_equal(W.reference(c, False)[1], W.reference(c, True)[1])
