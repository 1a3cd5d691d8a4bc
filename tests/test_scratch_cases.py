"""CPU checks of tests/scratch_cases.py: the three byte patterns read as its
table says in every type, poison() keeps exactly the protected ranges zero,
and every case named there is a member of the family it claims (each Gram
shape takes the route named; the stream, word, regressor and solve cases are
rows of the existing case tables).
"""
import numpy as np
import pytest
import torch

import frames16_cases as F
import mmb2_cases as C
import regressor_cases as R
import scratch_cases as S
import width_cases as W
import word_cases as WC


def _filled(pattern, nbytes=16):
    return S.poison(np.empty(nbytes, np.uint8), pattern)


# ------------------------------------------------------------------ the patterns
def test_pattern_z_is_zero_in_every_type():
    b = _filled("Z")
    for dt in (np.float32, np.float64, np.float16, np.int32, np.uint32):
        assert not b.view(dt).any()
    assert not torch.from_numpy(b.copy()).view(torch.bfloat16).float().any()


def test_pattern_n_is_nan_or_minus_one():
    b = _filled("N")
    for dt in (np.float32, np.float64, np.float16):
        assert np.isnan(b.view(dt)).all()
    assert torch.isnan(torch.from_numpy(b.copy()).view(torch.bfloat16).float()).all()
    assert (b.view(np.int32) == -1).all()
    assert (b.view(np.uint32) == 4294967295).all()


def test_pattern_h_is_huge_and_finite_where_the_table_says():
    b = _filled("H")
    f32, f64 = b.view(np.float32), b.view(np.float64)
    assert np.isfinite(f32).all() and (f32 > 3.38e38).all() and (f32 < 3.40e38).all()
    assert np.isfinite(f64).all() and (f64 > 1.37e306).all() and (f64 < 1.39e306).all()
    assert np.isnan(b.view(np.float16)).all()
    bf = torch.from_numpy(b.copy()).view(torch.bfloat16).float()
    assert torch.isfinite(bf).all() and (bf > 3.3e38).all()
    assert (b.view(np.int32) == 2139062143).all()
    assert (b.view(np.uint32) == 2139062143).all()
    # the bits rank above every finite column bound a kernel computes (unsigned order)
    assert b.view(np.uint32)[0] > np.float32(1e30).view(np.uint32)


def test_h_is_seen_by_fmax_where_n_is_not():
    """Why both patterns: a max drops the NaN of N and keeps the value of H."""
    n32, h32 = _filled("N").view(np.float32)[0], _filled("H").view(np.float32)[0]
    assert np.fmax(np.float32(1.0), n32) == 1.0
    assert np.fmax(np.float32(1.0), h32) == h32
    with np.errstate(over="ignore", invalid="ignore"):
        assert np.isnan(np.float32(0.0) * n32) and not np.isfinite(h32 + h32)


# ------------------------------------------------------------------ poison / same_bytes
@pytest.mark.parametrize("pattern", ["N", "H"])
@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_poison_keeps_only_the_protected_ranges_zero(pattern, kind):
    keep = ((0, 16), (40, 44), (1000, 1024))
    buf = np.zeros(256, np.float32) if kind == "numpy" else torch.zeros((16, 16), dtype=torch.float32)
    out = S.poison(buf, pattern, keep_zero=keep)
    assert out is buf
    b = np.asarray(S._bytes_of(buf))
    inside = np.zeros(1024, bool)
    for lo, hi in keep:
        inside[lo:hi] = True
    assert not b[inside].any()
    assert (b[~inside] == S.PATTERNS[pattern]).all()


def test_poison_z_overwrites_what_was_there():
    buf = torch.full((3, 5), 7.0, dtype=torch.float64)
    assert not S.poison(buf, "Z").any()


def test_poison_rejects_a_range_outside_the_buffer():
    with pytest.raises(AssertionError):
        S.poison(np.zeros(4, np.float32), "N", keep_zero=((8, 24),))


def test_protected_regions():
    assert S.solve_keep(300) == ((0, 16),)
    assert S.colmax_ws_keep(4096) == ((4080, 4096),)


def test_same_bytes():
    nan = torch.full((4,), float("nan"))
    assert S.same_bytes(nan, nan.clone()) and not torch.equal(nan, nan.clone())
    assert not S.same_bytes(torch.tensor([0.0]), torch.tensor([-0.0]))
    assert not S.same_bytes(torch.zeros(4), torch.zeros(5))
    a = np.arange(6, dtype=np.float64)
    assert S.same_bytes(a, a.copy()) and not S.same_bytes(a, a[::-1].copy())


# ------------------------------------------------------------------ the tables
def _route(n, d):
    """The route rule of csrc/gram_kernels.hip (mmb_gram), restated: n <= 4096
    and d <= 320 is the small route, d % 4 == 0 and d <= 320 the tri route
    (16-byte aligned rows), anything else the generic route."""
    if n <= 4096 and d <= 320:
        return "small"
    if d % 4 == 0 and d <= 320:
        return "tri"
    return "generic"


def test_gram_cases_take_the_routes_named():
    for n, d in S.GRAM_TRI:
        assert _route(n, d) == S.gram_route(n, d) == "tri", (n, d)
        assert S.gram_route(n, d, aligned=False) == "generic"
    for n, d in S.GRAM_GENERIC:
        assert _route(n, d) == S.gram_route(n, d) == "generic", (n, d)
    for n, d in S.GRAM_SMALL:
        assert _route(n, d) == S.gram_route(n, d) == "small", (n, d)
    n_plan, d = S.GRAM_PARTS
    assert d % 4 == 0 and d <= 320  # mmb_gram_part's own condition
    for chunks in S.GRAM_PART_CHUNKS:
        assert all(0 <= c <= n_plan for c in chunks) and sum(chunks) <= n_plan
    assert S.GRAM_PART_CHUNKS[-1][0] == 0  # the empty first chunk
    for n, d in S.GRAM_I8:
        assert d % 4 == 0 and d <= 304  # mmb_gram_i8's own condition
    assert max(n for n, _ in S.GRAM_I8) > S.GRAM_I8_RANGE_ROWS
    assert S.GRAM_CONTROL == S.GRAM_PARTS


def test_stream_cases_are_members_of_mmb2_cases():
    for shape, n, family in S.STREAM_CASES:
        assert tuple(shape) in getattr(C, family), (shape, family)
        assert n is None or n >= 1
    assert S.STREAM_CASES[0][0] == S.STREAM_CASES[1][0] == C.WAVE_ROWS_SHAPE
    assert {S.STREAM_CASES[0][1], S.STREAM_CASES[1][1]} <= set(C.WAVE_ROWS)
    assert S.STREAM_CU_EDGE == C.WG_CU_EDGE
    for shape in S.STREAM_SPLIT:
        assert shape in C.COMBOS and shape[3] > 64
    assert max(S.STREAM_SPLIT_PARTS) > max(s[3] for s in S.STREAM_SPLIT)  # clipped to T
    for shape in S.STREAM_FRAMES16:
        assert shape in F.SPECIAL_SHAPES
    wave, wg = S.STREAM_FRAMES16
    assert all(w % 4 == 0 for w in wave[:3]) and wave[3] <= 64   # the wave kernel's conditions
    assert any(w % 4 for w in wg[:3])                            # scalar rows: the workgroup kernel
    assert set(S.frames16_kinds()) == {"f16", "bf16"}
    assert set(S.STREAM_MODES) <= {"ids+table", "ids+w", "dense", "dense+emb2"}


def test_projection_cases():
    oracle = set(C.oracle_cases())
    assert S.PROJECT_ANCHOR in oracle
    for D in S.PROJECT_D:
        assert 256 <= D < 320 and (D + 64) // 64 * 64 == 320  # the split-K kernel's widths
    narrow_k = (2 * (min(S.PROJECT_D) + 8 + 12) + 31) // 32   # K chunks at the narrow widths
    assert max(S.PROJECT_SLICES) > narrow_k                   # 57 clamps there
    assert 0 in S.PROJECT_SLICES and 2 in S.PROJECT_SLICES


def test_derived_image_cases():
    for c in S.NARROW_FUSED:
        assert c in C.NARROW_FUSED
    assert all(d % 16 for d in S.WORD_TABLE_D)  # a padded column in every table


def test_solve_cases_are_the_width_tables():
    cases = S.solve_cases()
    assert cases and set(cases) <= set(W.pc_cases())
    assert all(d <= S.SOLVE_MAX_D and npc in (1, 2) for _, d, npc in cases)
    assert S.SOLVE_ANCHOR in cases and W.full_rank(*S.SOLVE_ANCHOR)
    assert {d for _, d, _ in cases} >= {16, 17, 300 - 1, 320}
    for n, d in S.SOLVE_XT:
        assert n < d <= S.SOLVE_MAX_D and n <= 320  # mmb_pc_solve_mc_xt's own conditions


def test_word_and_regressor_cases_are_members():
    for c in S.WORD_CASES:
        assert c in WC.WORD_CASES, c
    for c in S.BACKWARD_CASES:
        assert c in R.FWD_CASES
    assert S.BACKWARD_CASES[0] == R.FWD_CASES[0] and S.BACKWARD_CASES[-1] == R.FWD_CASES[-1]
    for c in S.TRAIN_CASES:
        assert c in R.TRAIN_CASES, c
    assert [c.d for c in S.TRAIN_CASES] == [R.TRAIN_CASES[0].d, 300, 448]
    big = max(S.TRAIN_CASES, key=lambda c: c.d * c.h)
    assert S.TRAIN_SMALLER in R.TRAIN_CASES
    assert S.TRAIN_SMALLER.d < big.d and S.TRAIN_SMALLER.h <= big.h


def test_step_cases():
    assert set(S.STEPS) == {"fused", "narrow_fused", "stream_i8", "split_fork"}
    assert S.STEPS["stream_i8"][0][:5] == C.STEP[2]
    assert S.STEPS["split_fork"][0][:5] == C.DROP_IN[1][:5] and S.STEPS["split_fork"][0][3] == 130
    assert S.STEPS["fused"][0][:5] == (300, 300, 300, 40, 97)
    assert S.STEPS["narrow_fused"][0] == (300, 76, 48, 20, 97, 3016)
    assert "flag" not in S.STEP_BUFFERS and "colmax" not in S.STEP_BUFFERS
