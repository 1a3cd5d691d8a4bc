"""CPU: the input family and the f64 references of tests/mmb2_cases.py keep the
GPU bars of tests/test_gpu_mmb2_widths.py meaningful.

The GPU tests hold every stage of the MMB2 path to a bar derived from the
case's own terms and the end-to-end rows to 1e-5 of the oracle.  Both are
statements about the kernels only while, on the same inputs,

  1. the oracle's own f32 run (the reference's arithmetic) lies within 1e-6
     row-relative of its f64 run,
  2. the total weight does not cancel: the sum of |sentence weights| +
     |q_mean| + |q_sigma| over every key is at most 10 |total|,
  3. no row's total weight changes sign between the two runs (the rows are
     sign(total) y / ||y||).

These are conditions on the inputs, not measurements: a case that does not fit
gets another seed (mmb2_cases.seed_of), never a wider cap.  The closed form restated in f64
(oracle.mmb2_oracle.frame_sums / merged_projection, what the stage tests
compare the kernels with) must also reproduce the oracle's rows.
"""
import numpy as np
import pytest

import mmb2_cases as C
from oracle import mmb2_oracle as M

F32_CAP, CANCEL_CAP = 1e-6, 10.0


def test_table_is_the_issue_table():
    shapes = set(C.WAVE_D256 + C.WAVE_D512 + C.NARROW_ROUTE + C.WG_SCALAR_TEXT + C.WG_VECTOR_TEXT)
    assert {(4, 4, 4, 1), (256, 4, 300, 64), (128, 260, 320, 40), (512, 4, 4, 64), (316, 128, 4, 33),
            (50, 5, 3, 9), (301, 300, 300, 12), (319, 4, 4, 3), (52, 4, 4, 513), (640, 4, 4, 2)} <= shapes
    # the four launch_wave<true, 1, CA, CV> instantiations
    assert {(a > 256, v > 256) for d, a, v, t in C.WAVE_D256} == {(False, False), (True, False),
                                                                   (False, True), (True, True)}
    assert all(d <= 256 and d % 4 == a % 4 == v % 4 == 0 and t <= 64 for d, a, v, t in C.WAVE_D256)
    assert all(256 < d <= 512 and a <= 128 and v <= 128 and t <= 64 for d, a, v, t in C.NARROW_ROUTE)
    assert all(d % 4 for d, a, v, t in C.WG_SCALAR_TEXT) and max(d for d, *_ in C.WG_SCALAR_TEXT) == 319
    # the eight vector / scalar combinations
    assert len({(d % 4 == 0, a % 4 == 0, v % 4 == 0) for d, a, v, t in C.COMBOS}) == 8
    assert [2 * sum(s[:3]) for s in C.PROJECT_KP] == [32, 64, 96, 128]
    assert [(2 * sum(s) + 31) // 32 * 32 for s in C.PREPARE_KP] == [32, 64, 96, 128, 160]
    assert {(d + 64) // 64 * 64 for d in C.PREPARE_D} == {64, 128, 192, 256, 320, 384}
    cases = C.oracle_cases()
    assert len(cases) == len(set(cases))


def test_family_is_seeded_by_shape():
    a, b = C.inputs((52, 8, 12, 7, 5, 300)), C.inputs((52, 8, 12, 7, 4, 300))
    assert a["E"].dtype == np.float32 and a["wt32"].dtype == np.float32
    assert a["audio"].dtype == np.float32 and np.abs(a["audio"]).max() <= 1.0
    assert not a["E"][0].any() and a["ids"].min() >= 0 and a["ids"].max() < 300
    assert not np.array_equal(a["E"], b["E"])
    assert C.seed_of((52, 8, 12, 7, 5, 300)) != C.seed_of((52, 12, 8, 7, 5, 300))
    assert np.array_equal(a["text"], a["E"][a["ids"]]) and np.array_equal(a["sw"], a["wt32"][a["ids"]])


@pytest.mark.parametrize("case", C.oracle_cases(), ids=C.shape_id)
def test_family_conditions(case):
    e32, cancel, flips = C.family_conditions(case)
    print(f"f32 run {e32:.2e} (cap {F32_CAP}); cancellation {cancel:.2f} (cap {CANCEL_CAP}); "
          f"sign flips {flips}")
    assert e32 <= F32_CAP
    assert cancel <= CANCEL_CAP
    assert flips == 0


@pytest.mark.parametrize("case", [C.case_of(s) for s in
                                  [(4, 4, 4, 1), (50, 5, 3, 9), (63, 4, 4, 3), (100, 76, 48, 20)]],
                         ids=C.shape_id)
def test_closed_form_restatement_reproduces_the_oracle(case):
    """frame_sums x merged_projection (+ the weighted text sum and c0),
    normalised, is estimate_embedding_overall_gpu2 -- in f64 to 1e-12."""
    D, A, Vd, T, N, V = case
    z = C.inputs(case)
    ref = C.stream_reference(z["text"], z["text"], z["sw"], z["audio"], z["visual"])
    Wm, c0, Wa, ca = M.merged_projection(C.params(D, A, Vd), D, A, Vd, T)
    assert Wm.shape == (2 * (D + A + Vd), D + 1) and (Wa >= np.abs(Wm) - 1e-15).all()
    aux = np.stack([ref["cnt"], ref["sw"]])
    rows, bar = C.project_reference(ref["s"], ref["x"], aux, Wm, c0, D, 2 * (D + A + Vd))
    assert M.row_rel_err(rows, C.oracle_rows(case)) < 1e-12
    assert (bar > 0).all() and np.isfinite(bar).all()
    print(f"projection bar of the f32 kernel: {bar.min():.2e} .. {bar.max():.2e}")
    tot, _ = C.total_weight(case)
    y_tot = ref["sw"] + ref["s"] @ Wm[:, D] + c0[D]
    assert np.abs(y_tot / tot - 1).max() < 1e-12


def test_row_scale_and_sum_bar():
    assert list(C.row_scale_of([0.0, 1.0, 0.75, 2.0 ** 14, 2.0 ** 15, np.inf])) == \
        [1.0, 2.0 ** 14, 2.0 ** 15, 1.0, 0.5, 1.0]
    assert C.sum_bar(1, 1.0) == 4 * C.U
