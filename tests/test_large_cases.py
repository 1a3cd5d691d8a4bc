"""CPU: the size facts and references tests/test_gpu_large.py relies on.

For every case of tests/large_cases.py: which operand passes which boundary
and by how little (the smallest row count of its widest row), which rows hold
the boundaries, that the sample (or the hand-set ids, or the planted rows)
holds them, that the case's buffers stay within 16 GiB, and that its f64
reference stays inside the GPU test's bar when it is computed a second way.
For the reductions: a read of a late planted row at its offset modulo 2^31 or
2^32 moves the result by more than 1e3 x the bar.
"""
import numpy as np
import pytest

import gauss_cases as G
import large_cases as LC
import mmb2_cases as C
import synth
import width_cases as W
from oracle import mmb2_oracle as M
from oracle import sif_oracle as O

B31, B32 = LC.B31, LC.B32
ALL = list(LC.CASES)
# at 2^31 by design, not past 2^32: (the last size the guard accepts, the first it refuses)
GUARD_CASES = {"table_narrow_last": 2 ** 20 - 1, "table_narrow_refused": 2 ** 20,
               "fused_table_last": 2 ** 21 - 1, "fused_table_refused": 2 ** 21}
REDUCTIONS = LC.names(family=8) + ["ln_backward_dgamma"]
GATHERS = LC.names(family=4) + ["fused_table_last", "fused_table_refused", "wavg_table", "wavg_tt_bf16",
                                "gauss_loglik_idx", "mlp_gather", "mlp_train"]


def test_table_covers_the_families():
    assert {c.family for c in LC.CASES.values()} == set(range(1, 13))
    assert len(set(ALL)) == len(ALL) and all(LC.CASES[n].name == n for n in ALL)
    entries = {c.entry for c in LC.CASES.values()}
    assert {"mmb_mm2_stream", "mmb_mm2_stream_ft", "mmb_mm2_stream_tt", "mmb_mm2_stream_split",
            "mmb_mm2_stream_split_ft", "mmb_mm2_stream_project", "mmb_mm2_stream_project_ft",
            "mmb_mm2_stream_project_narrow", "mmb_mm2_stream_project_narrow_ft", "mmb_sif_wavg", "mmb_sif_wavg_tt",
            "mmb_gram", "mmb_gram_f64", "mmb_gram_part", "mmb_gram_i8", "mmb_pc_remove", "mmb_pc_remove_f64",
            "mmb_mm2_project", "mmb_mm2_project_x3", "mmb_mlp_forward", "mmb_mlp_forward_train", "mmb_mlp_train",
            "mmb_gauss_stats", "mmb_gauss_loglik", "mmb_layer_norm_backward", "mmb_word_normalize",
            "mmb_word_logprob_forward"} == entries
    # a 16-bit instantiation of every family that has one passes 2^32 too
    for fam in (1, 2, 3, 4, 5, 6, 7):
        assert any(c.dims.get("fbytes", 4) == 2 or c.dims.get("tbytes", 4) == 2
                   for c in LC.CASES.values() if c.family == fam and c.op(c.crossing).past32), fam


@pytest.mark.parametrize("name", ALL)
def test_crossing_operand_is_the_smallest_past_b32(name):
    c = LC.CASES[name]
    op = c.op(c.crossing)
    if name in GUARD_CASES and name.endswith("_last"):  # the last table the guard accepts: one row short of 2^31
        assert op.nbytes < B31 <= op.nbytes + op.row_bytes and op.rows == GUARD_CASES[name]
    elif name in GUARD_CASES:                            # the first it refuses: 2^31 bytes exactly
        assert op.nbytes == B31 and op.rows == GUARD_CASES[name]
    else:
        assert op.nbytes > B32 >= op.nbytes - op.row_bytes, (op.nbytes - B32, op.row_bytes)
        assert op.rows == LC.rows_past(B32, op.row_bytes) and op.past31 and op.past32
        print(f"{name}: {c.crossing} {op.rows} rows x {op.row_bytes} B = 2^32 + {op.nbytes - B32} B")
    assert c.total_bytes <= LC.MAX_CASE_BYTES, c.total_bytes
    # nothing else of the launch is large unless the shape itself makes it so
    others = sorted(o.name for o in c.operands if o.past31 and o.name != c.crossing)
    allowed = {"wave_x_s32": ["s"], "wave_x_s16": ["s"], "word_normalize": ["wn"],
               "ln_backward_dx": ["dx", "dy"], "ln_backward_dgamma": ["dx", "dy"], "gauss_stats_mask": ["mask"],
               "narrow_fused_x": ["mmb2"], "mlp_rows_x": ["dx"], "mlp_rows_hid": ["dh"]}
    if c.family == 9:
        allowed[name] = ["out"]
    assert others == allowed.get(name, []), others


def test_issue_shapes():
    """The row counts the shapes of the issue give."""
    assert LC.CASES["wave_audio"].n == 52_429 and LC.CASES["wave_audio"].op("audio").row_bytes == 81_920
    assert LC.CASES["wave_x_s32"].n == 2 ** 21 + 1 and LC.CASES["wave_x_s32"].op("s").row_bytes == 1056 * 4
    assert LC.CASES["table_past_b32"].dims["v"] == 2 ** 21 + 1
    assert LC.CASES["table_tt_bf16"].dims["v"] == 2 ** 22 + 1
    p = LC.CASES["project_x3"]
    assert p.n == 588_675 and p.op("s").row_bytes == 7_296 and p.dims["kp"] == 1824
    assert LC.CASES["gram_i8"].dims["d"] == 304 and LC.CASES["gram_tri"].dims["d"] == 320


@pytest.mark.parametrize("rb", [1216, 1280, 2044, 2048, 4096, 4224, 7296, 7680, 40_960, 81_920, 82_680, 83_200])
def test_boundary_rows_straddle(rb):
    for b in (B31, B32):
        rows = LC.rows_past(B32, rb)
        below, at, above = LC.boundary_rows(rb, b, rows)
        assert (below + 1) * rb <= b and below * rb < b           # wholly below, and the last such row
        assert at * rb <= b < (at + 1) * rb                        # holds byte `boundary`
        assert at == below + 1
        if b == B31:
            assert above == at + 1 and above * rb > b              # wholly above
        else:  # the smallest row count: the row holding 2^32 is the last row, none lies wholly above
            assert at == rows - 1 and above is None


def test_word_rows_lie_at_the_scratch_boundaries():
    """The word kernels' scratch is indexed by tiles of 16 latents: the checked
    latents are the first and last of the tiles around its boundaries."""
    c = LC.CASES["word_logprob"]
    rows, tiles = LC.word_rows(c), c.dims["tiles"]
    assert len(rows) == c.dims["b"] == 33 and rows[0] == 0 and rows[-1] == c.n - 1 == (tiles - 1) * 16
    for b in (B31, B32):
        for t in LC.boundary_rows(LC.WORD_TILE_BYTES, b, tiles):
            assert t is None or (16 * t in rows and (16 * t + 15 in rows or 16 * t + 15 >= c.n))


@pytest.mark.parametrize("name", [n for n in ALL if n not in REDUCTIONS + GATHERS + ["word_logprob"]])
def test_sample_holds_the_boundary_rows(name):
    c = LC.CASES[name]
    rows = LC.sample_rows(c)
    assert len(rows) == min(LC.MAX_SAMPLE, c.n) and len(set(rows)) == len(rows)
    assert list(rows) == sorted(rows) and rows[0] == 0 and rows[-1] == c.n - 1
    ops = LC.crossing_operands(c, "row")
    assert c.crossing in [o.name for o in ops]
    for o in ops:
        assert o.rows == c.n
        for b in (B31, B32):
            if o.nbytes > b:
                for r in LC.boundary_rows(o.row_bytes, b, o.rows):
                    assert r is None or r in rows, (o.name, b, r)
    assert np.array_equal(rows, LC.sample_rows(c))  # seeded by the case alone


@pytest.mark.parametrize("name", GATHERS)
def test_hand_set_ids_reach_both_sides(name):
    c = LC.CASES[name]
    t = c.op("table")
    l = c.dims.get("t", 1)  # (an index per row: idx / perm)
    for ll in {l, 65} if c.family == 7 else {l}:
        ids = LC.gather_ids(c, c.n, ll)
        assert ids.shape == (c.n, ll) and ids.min() == 0 and ids.max() == t.rows - 1
        have = set(ids.ravel())
        assert {t.rows - 3, t.rows - 2, t.rows - 1} <= have
        for b in (B31, B32):
            if t.nbytes > b:
                below, at, above = LC.boundary_rows(t.row_bytes, b, t.rows)
                assert below in have and at in have and (above is None or above in have)
                assert any(r * t.row_bytes < b for r in have) and any((r + 1) * t.row_bytes > b for r in have)
    if name in GUARD_CASES:  # every gathered row's byte offset fits 2^31; the table's size does, or just does not
        assert ((t.rows - 1) * t.row_bytes < B31) and (t.rows * t.row_bytes < B31) == name.endswith("_last")


# ---------------------------------------------------------------- reductions: planted rows
def _planted_reference(c, vals, rows=None):
    if c.family == 8:
        return LC.gram_reference(vals), {"mmb_gram_i8": 2e-9}.get(c.entry, 1e-13)
    raise AssertionError(c.name)


@pytest.mark.parametrize("name", LC.names(family=8))
def test_planted_rows_and_wrapped_reads(name):
    c = LC.CASES[name]
    op, d, esize = c.op("x"), c.dims["d"], c.dims["esize"]
    rows, vals = LC.planted_values(c, d, np.float64 if esize == 8 else np.float32)
    rb = op.row_bytes
    assert rows[0] == 0 and rows[-1] == op.rows - 1 and len(set(rows)) == len(rows) <= LC.MAX_SAMPLE
    regions = [sum(1 for r in rows if (r + 1) * rb <= B31), sum(1 for r in rows if r * rb >= B31 and (r + 1) * rb <= B32),
               sum(1 for r in rows if (r + 1) * rb > B32)]
    assert regions[0] >= 4 and regions[1] >= 4 and regions[2] >= 1, regions
    for b in (B31, B32):
        assert all(r is None or r in rows for r in LC.boundary_rows(rb, b, op.rows))
    ref, bar = _planted_reference(c, vals)
    # a second way, far inside the bar
    assert np.abs(LC.gram_reference_2(vals) - ref).max() <= 1e-2 * 1e-13 * np.abs(ref).max()
    if c.dims["cnt"]:
        cnt = np.arange(1, len(rows) + 1, dtype=np.float32) % 7 + 1
        assert np.abs(LC.gram_reference_2(vals, cnt) - LC.gram_reference(vals, cnt)).max() <= \
            1e-15 * np.abs(LC.gram_reference(vals, cnt)).max()
    # a late row read at its offset modulo 2^31 / 2^32: zeros or an early row's values
    where = {int(r): i for i, r in enumerate(rows)}
    for b in (B31, B32):
        late = LC.late_rows(rows, rb, b)
        assert late and late[-1] == op.rows - 1
        for r in late:
            w = LC.wrapped_row(rows, vals, r, esize, b)
            v = vals[where[r]]
            moved = np.abs(np.outer(w, w) - np.outer(v, v)).max() / np.abs(ref).max()
            assert moved >= 1e3 * bar, (name, b, r, moved)
    if c.entry == "mmb_gram_i8":  # the column bounds move too
        for b in (B31, B32):
            r = LC.late_rows(rows, rb, b)[-1]
            w = vals.copy()
            w[where[r]] = LC.wrapped_row(rows, vals, r, esize, b)
            assert not np.array_equal(np.abs(w).max(0), np.abs(vals).max(0)) or \
                not np.array_equal(O.sliced_gram(w.astype(np.float32)), O.sliced_gram(vals.astype(np.float32)))
        # the sliced oracle of the planted rows is within the GPU test's second bar of the exact Gram
        sl = O.sliced_gram(vals.astype(np.float32))
        assert np.abs(sl - ref).max() / np.abs(ref).max() <= 2e-9


def test_gram_workspace_bound():
    import mmb_lib

    for name in LC.names(family=8):
        c = LC.CASES[name]
        assert mmb_lib.query("mmb_gram_workspace_bytes", c.n, c.dims["d"]) <= LC.GRAM_WS, name


def test_int8_gram_guard_is_not_reachable():
    """gram_i8l_block requires chunk d 4 < 2^31.  mmb_gram_i8 takes d <= 304 and
    cuts its rows into blocks of 128 ranges of at most 32768 rows, so a range
    never holds more than 32768 x 304 x 4 = 39,845,888 bytes: no size that
    pipeline.gram_i8 can be asked for is refused by the guard."""
    assert 512 * 64 * 304 * 4 == 39_845_888 < B31
    assert LC.CASES["gram_i8"].n <= 128 * 512 * 64  # one block at the case's size


def test_layer_norm_planted_rows_fill_the_four_row_groups():
    c = LC.CASES["ln_backward_dgamma"]
    n, d = c.n, c.dims["d"]
    rows, vals = LC.planted_values(c, d)
    per = [int(np.sum(rows % 4 == g)) for g in range(4)]
    assert min(per) == max(per) and len(rows) <= LC.MAX_SAMPLE
    assert set(LC.required_rows(n, [4 * d])) <= set(rows)
    # the reference of the planted rows alone, a second way (extended precision), inside the bars
    rng = np.random.default_rng(0)
    x = G.f32(1.5 * rng.standard_normal((len(rows), d)) + 0.2)
    mean = G.f32(x.mean(1))
    rstd = G.f32(1.0 / np.sqrt(x.var(1) + G.LN_EPS))
    gamma = G.f32(rng.uniform(0.5, 1.5, d))
    ref, bars = G.layer_norm_backward_reference(vals, x, mean, rstd, gamma)
    ld = np.longdouble
    xh = (x.astype(ld) - mean.astype(ld)[:, None]) * rstd.astype(ld)[:, None]
    g = vals.astype(ld) * gamma.astype(ld)
    dx2 = rstd.astype(ld)[:, None] * (g - (g.sum(1, keepdims=True) + xh * (g * xh).sum(1, keepdims=True)) / d)
    second = (dx2, (vals.astype(ld) * xh).sum(0), vals.astype(ld).sum(0))
    for a, b, bar in zip(ref, second, bars):
        assert (np.abs(a - b.astype(np.float64)) <= 1e-3 * bar).all()
    # a late planted dy row read at its wrapped offset: dgamma and dbeta move by more than 1e3 bars
    where = {int(r): i for i, r in enumerate(rows)}
    for b in (B31, B32):
        for r in LC.late_rows(rows, 4 * d, b):
            w = vals.copy()
            w[where[r]] = LC.wrapped_row(rows, vals, r, 4, b)
            moved, _ = G.layer_norm_backward_reference(w, x, mean, rstd, gamma)
            for k in (1, 2):
                assert (np.abs(moved[k] - ref[k]) / bars[k]).max() >= 1e3, (b, r, k)


# ---------------------------------------------------------------- per-row references a second way
def _stand_in(c, k=8, seed=0):
    """k host rows of the case's input family (the GPU test fills the same
    family on the device): the gathered text, weights, frames."""
    z = c.dims
    rng = np.random.default_rng(seed)
    E = synth.word_table(300, z["d"], seed=seed)
    wt = synth.sif_weights(300, w0=1.0).astype(np.float32)
    ids = rng.integers(0, 300, (k, z["t"]))
    fr = lambda w: rng.uniform(-1, 1, (k, z["t"], w)).astype(np.float32)
    if z.get("fbytes", 4) == 2 or z.get("tbytes", 4) == 2:
        import torch

        t16 = torch.float16 if z.get("frames") == "f16" else torch.bfloat16
        r16 = lambda a: torch.as_tensor(a).to(t16).float().numpy()
    else:
        r16 = lambda a: a
    text = r16(E[ids]) if z.get("tbytes", 4) == 2 else E[ids]
    f16 = r16 if z.get("fbytes", 4) == 2 else (lambda a: a)
    return text, wt[ids], f16(fr(z.get("a", 4))), f16(fr(z.get("vd", 4)))


STREAMS = LC.names(family=1) + LC.names(family=2) + LC.names(family=3) + LC.names(family=4)
FUSED = LC.names(family=5) + LC.names(family=6)


@pytest.mark.parametrize("name", FUSED)
def test_fused_family_conditions(name):
    """The 1e-5 bar of the MMB2 rows rests on the input family: the oracle's own
    f32 run is 30 times closer to its f64 run than the bar, the total weight
    keeps one sign and cancels by less than 2 (as tests/test_mmb2_cases.py pins
    for the small shapes)."""
    c = LC.CASES[name]
    z = c.dims
    text, sw, audio, visual = _stand_in(c, k=128)
    prm = C.params(z["d"], z["a"], z["vd"])
    data = M.concat_inputs(text, audio, visual)
    o64 = M.estimate_embedding_overall_gpu2(data, prm, sw, text)
    o32 = M.estimate_embedding_overall_gpu2(data, prm, sw, text, dtype=np.float32)
    tot, ab = M.total_weight(data, prm, sw)
    e32 = LC.row_err(o32, o64).max()
    print(f"{name}: oracle f32 vs f64 {e32:.2e}, cancellation {(ab / np.abs(tot)).max():.2f}")
    assert e32 < 1e-5 / 30 and (ab / np.abs(tot)).max() < 2.0 and len(set(np.sign(tot))) == 1


@pytest.mark.parametrize("name", STREAMS)
def test_stream_reference_a_second_way(name):
    c = LC.CASES[name]
    text, sw, audio, visual = _stand_in(c)
    ref = C.stream_reference(text, text, sw, audio, visual)
    ld = np.longdouble
    t = c.dims["t"]
    x2 = sum(sw[:, i, None].astype(ld) * text[:, i].astype(ld) for i in range(t)) / np.count_nonzero(sw, axis=1)[:, None]
    s2 = np.concatenate([f(m) for m in (text, audio, visual)
                         for f in (lambda m: sum(m[:, i].astype(ld) for i in range(t)),
                                   lambda m: sum(m[:, i].astype(ld) ** 2 for i in range(t)))], 1)
    assert (np.abs(ref["x"] - x2.astype(np.float64)) <= 1e-3 * C.sum_bar(t, ref["x_abs"]) + 1e-300).all()
    assert (np.abs(ref["s"] - s2.astype(np.float64)) <= 1e-3 * C.sum_bar(t, ref["s_abs"]) + 1e-300).all()
    assert np.isfinite(ref["x"]).all() and (ref["cnt"] > 0).all()


@pytest.mark.parametrize("name", LC.names(family=7))
def test_weighted_average_reference_a_second_way(name):
    c = LC.CASES[name]
    for l in {c.dims["t"], 65} if c.crossing == "table" else {c.dims["t"]}:
        text, sw, _, _ = _stand_in(LC.Case(c.name, 7, c.entry, dict(c.dims, t=l), c.crossing, c.operands))
        a, b = LC.wavg_reference(text, sw), LC.wavg_reference_2(text, sw)
        assert M.row_rel_err(a[0], b[0]) <= 1e-3 * 2e-6 and M.row_rel_err(a[1], b[1]) <= 1e-3 * 2e-6
        assert np.array_equal(a[2], b[2])
        # and the CPU oracle of the same operation
        E = synth.word_table(300, c.dims["d"], seed=0)
        ids = np.random.default_rng(0).integers(0, 300, (8, l))
        wt = synth.sif_weights(300, w0=1.0).astype(np.float32)
        want = O.get_weighted_average(E, ids, wt[ids].astype(np.float64))
        assert M.row_rel_err(LC.wavg_reference(E[ids], wt[ids])[0], want) <= 1e-3 * 2e-6


@pytest.mark.parametrize("name", LC.names(family=9))
def test_remove_reference_a_second_way(name):
    c = LC.CASES[name]
    d, npc = c.dims["d"], c.dims["npc"]
    rng = np.random.default_rng(d + npc)
    x = 0.4 * rng.standard_normal((16, d)) + 0.3
    cnt = None
    if c.dims["in_bytes"] == 4:
        x = G.f32(x)
        cnt = rng.integers(1, 8, 16).astype(np.float32) if c.dims["cnt"] else None
    pc = W.orthonormal_rows(npc, d, seed=d + npc)
    a, b = LC.remove_reference(x, cnt, pc), LC.remove_reference_2(x, cnt, pc)
    bar = 1e-12 if c.dims["out_bytes"] == 8 else LC.F32_ROW
    assert LC.row_err(a, b).max() <= 1e-3 * bar
    assert LC.row_err(a, x).min() > 1e3 * bar  # the removal moves every row by far more than the bar


def test_removal_bar_is_the_suite_s():
    """One definition, with the width tables; large_cases and the GPU tests import it."""
    assert LC.F32_ROW is W.F32_ROW and W.F32_ROW == 2.0 ** -23
    src = open(__file__.replace("test_large_cases.py", "large_cases.py")).read()
    assert "F32_ROW =" not in src


def test_projection_reference_and_family_conditions():
    """project_reference on exact f64 operands is the oracle's row (far inside
    1e-5), and the case's input family (T = 2 tokens of a 300-word table, U(-1,
    1) frames) keeps the total weight away from cancellation."""
    c = LC.CASES["project_x3"]
    z = c.dims
    D, A, Vd, T = z["d"], z["a"], z["vd"], z["t"]
    text, sw, audio, visual = _stand_in(c, k=256)
    prm = C.params(D, A, Vd)
    ref = C.stream_reference(text, text, sw, audio, visual)
    Wm, c0 = M.merged_projection(prm, D, A, Vd, T)[:2]
    rows, bar = C.project_reference(ref["s"], ref["x"], np.stack([ref["cnt"], ref["sw"]]), Wm, c0, D, 2 * (D + A + Vd))
    data = M.concat_inputs(text, audio, visual)
    oracle = M.estimate_embedding_overall_gpu2(data, prm, sw, text)
    e = LC.row_err(rows, oracle)
    assert e.max() <= 1e-3 * 1e-5 and (e <= bar).all()
    tot, ab = M.total_weight(data, prm, sw)
    print(f"largest cancellation of the total weight: {(ab / np.abs(tot)).max():.1f}")
    assert (ab / np.abs(tot)).max() < 50 and (np.sign(tot) == np.sign(tot[0])).all()
    o32 = M.estimate_embedding_overall_gpu2(data, prm, sw, text, dtype=np.float32)
    assert LC.row_err(o32, oracle).max() < 1e-5


def test_gauss_references_a_second_way():
    rng = np.random.default_rng(1)
    c = LC.CASES["gauss_stats_mask"]
    x = G.f32(rng.uniform(-1, 1, (4, c.dims["t"], c.dims["f"])))
    for mask in (None, (rng.random(x.shape) < 0.7).astype(np.float64)):
        st, bar = G.stats_reference(x, mask)
        m = np.ones(x.shape) if mask is None else mask
        plain = np.stack([m.sum(1), (m * x).sum(1), (m * x * x).sum(1)], 1)
        assert (np.abs(plain - st) <= bar).all()
    c = LC.CASES["gauss_loglik_idx"]
    b, f, t = 8, c.dims["f"], 12
    x = G.f32(rng.uniform(-1, 1, (b, t, f)))
    mu, sigma = G.f32(0.5 * rng.standard_normal((b, f))), G.f32(rng.uniform(0.5, 1.5, (b, f)))
    up = G.f32(rng.standard_normal(b))
    ref = G.normal_reference(mu, sigma, x, None, up)
    bars = G.normal_bars(mu, sigma, x, None, up, ref)
    lp2 = G.kernel_route_lp(mu, sigma, x, None)  # the closed form over the frame sums
    assert (np.abs(lp2 - ref[0]) <= bars[0]).all()


def test_normalize_reference_a_second_way():
    c = LC.CASES["word_normalize"]
    d = c.dims["d"]
    w = synth.word_table(32, d, seed=3)
    a, b = LC.normalize_reference(w, LC.pad16(d)), LC.normalize_reference_2(w, LC.pad16(d))
    bar = 2 * ((d + 1) / 2 + 2) * C.U * np.abs(a)
    assert (np.abs(a - b) <= 1e-3 * bar).all() and not a[0].any() and np.abs(a[1:]).max(1).min() > 0


def test_embedded_cases_are_the_suite_s_own():
    """The regressor gathers, the training run and the word likelihood embed a
    case of the small-shape tables, so their float64 references, margins and
    bars are the ones tests/test_regressor_cases.py and tests/test_word_cases.py pin."""
    import regressor_cases as RC
    import word_cases as WC

    z = LC.CASES["mlp_gather"].dims
    assert RC.FwdCase(z["d"], z["h"], z["o"], z["n"]) in RC.FWD_CASES and RC.takes_v4(z["d"], z["h"])
    z = LC.CASES["mlp_train"].dims
    tc = RC.TrainCase(z["d"], z["h"], z["o"], z["batch"], z["n"], 0, 1, 0, z["seed"])
    assert tc in RC.TRAIN_CASES and z["d"] == RC.train_max_d(z["o"]) == 448
    z = LC.CASES["word_logprob"].dims
    assert WC.WordCase(z["d"], z["v"], z["b"], z["t"], 0) in WC.WORD_CASES and z["d"] == 320
    z = LC.CASES["mlp_rows_x"].dims
    assert RC.takes_v4(z["d"], z["h"]) and not RC.takes_v4(z["d"], z["h"] + 1)
    z = LC.CASES["mlp_rows_hid"].dims
    assert 4 * 8 * (z["d"] + z["h"]) <= 64 * 1024 < 4 * 8 * (z["d"] + z["h"] + 8) and not RC.takes_v4(z["d"], z["h"])


def test_guard_table_names_seven_guards():
    assert len(LC.GUARDS) == 7 and all(len(g) == 3 for g in LC.GUARDS)
