"""GPU: the narrow fused kernel and its text cache on a word table kept in
fp16 / bf16 storage (mmb_mm2_text_cache_tt, mmb_mm2_stream_project_narrow_tt,
pipeline.mm2_stream_project_narrow_tt, FusedStep(narrow_table16=True)).

A 16-bit value widens to f32 exactly, so every definition under test is an
equality.  (A) The text cache built from the 16-bit table is, byte for byte,
the cache mmb_mm2_text_cache builds from that table upcast to f32 -- the E
half the widened value, the P half the same f64 fma chain over it -- with the
documented hot-id gap of a table of fewer than 32 words left unwritten in
both.  (B) The narrow fused kernel reads its text from that cache only, never
from the table, so a launch on the 16-bit table writes, bit for bit, what
mmb_mm2_stream_project_narrow_ft writes on the upcast table with a cache built
from it: x, the three aux planes, the MMB2 rows, the column bounds and the flag
word, for frames of f32 and of the table's kind.  (C) The opted-in step gives
the rows of its twin on the upcast table and holds the bars of
tests/test_gpu_table16.py against the oracle on the upcast inputs.
Product library only.
"""
import functools

import numpy as np
import pytest
import torch

import frames16_cases as F
import frames16_gpu as G16
import mmb2_cases as C
import mmb_lib as L
import models
import narrow_table16_cases as NT
import pipeline as P
import table16_cases as T
from common_gpu import F32_ROW, TOL, _dev, _i32, _networks, _off, _untouched
from frames16_gpu import _assert_bit_for_bit, _bufs, _frames_of, _launch, _run
from oracle import mmb2_oracle as M
from oracle import sif_oracle as O

pytestmark = pytest.mark.gpu

KIND_IDS = list(NT.KINDS)
D = NT.D


# ------------------------------------------------------------------ A: the text cache, byte for byte
@functools.lru_cache(maxsize=None)
def _projection(d, gpu):
    A, Vd, T_ = NT.CACHE_FRAMES
    torch.manual_seed(0)
    gen = models.AudioVisualGeneratorMultimodal(d, A, Vd, norm=None).to(gpu)
    return P.MMB2Projection(gen.networks(), d, A, Vd, T_, gpu)


def _cache_table(v, d, kind, gpu, special=False):
    import synth

    E16 = F.to_kind(synth.word_table(v, d, seed=17 * v + d), kind).clone()
    E16[0] = torch.linspace(-0.5, 0.75, d).to(NT.KINDS[kind])  # (word tables have row 0 zero)
    if special:
        vals = [x for x, _ in T.SPECIALS[kind]] + list(NT.CACHE_NONFINITE)
        vals = torch.tensor(vals, dtype=torch.float64).to(NT.KINDS[kind])
        E16[0, :len(vals)] = vals
        E16[v - 1, d - len(vals):] = vals.flip(0)
    wt = synth.sif_weights(v, w0=1.0).astype(np.float32)
    return _dev(E16, gpu), _dev(wt, gpu)


def _build(entry, table, table_type, wtab, proj, fill):
    """The cache `entry` builds into a buffer pre-filled with the byte `fill`."""
    v, d = table.shape
    nbytes = L.query("mmb_mm2_text_cache_bytes", v, d)
    cache = torch.full(((nbytes + 15) // 16 * 16,), fill, dtype=torch.uint8, device=table.device)
    if entry == "mmb_mm2_text_cache_tt":
        L.call(entry, L.ptr(table, L.TABLE), table_type, v, d, L.ptr(wtab, L.F32), L.ptr(proj.wm, L.F32), proj.ldw,
               L.ptr(cache, L.BYTES), L.stream_ptr())
    else:
        L.call(entry, L.ptr(table, L.F32), v, d, L.ptr(wtab, L.F32), L.ptr(proj.wm, L.F32), proj.ldw,
               L.ptr(cache, L.BYTES), L.stream_ptr())
    torch.cuda.synchronize()
    return cache[:nbytes]


def _assert_same_cache(E16, wtab, kind, proj, what):
    v, d = E16.shape
    got = _build("mmb_mm2_text_cache_tt", E16, P.TABLE_KINDS[kind][1], wtab, proj, NT.CACHE_FILL16)
    want = _build("mmb_mm2_text_cache", E16.float(), None, wtab, proj, NT.CACHE_FILL32)
    lo, hi = NT.cache_gap(v)
    # the documented gap keeps each buffer's pre-fill; everything else is written, and the same
    assert bool((got[lo:hi] == NT.CACHE_FILL16).all()) and bool((want[lo:hi] == NT.CACHE_FILL32).all()), what
    assert torch.equal(got[:lo], want[:lo]) and torch.equal(got[hi:], want[hi:]), what
    # (and written: a second build over the other pre-fill gives the same bytes)
    again = _build("mmb_mm2_text_cache_tt", E16, P.TABLE_KINDS[kind][1], wtab, proj, NT.CACHE_FILL32)
    assert torch.equal(again[:lo], got[:lo]) and torch.equal(again[hi:], got[hi:]), what
    # the E half of a row is the widened table
    rows = got[:v * NT.CACHE_ROW * 4].view(torch.float32).view(v, NT.CACHE_ROW)
    assert torch.equal(_i32(rows[:, :d]), _i32(E16.float())), what
    return got


@pytest.mark.parametrize("kind", KIND_IDS)
@pytest.mark.parametrize("v", NT.CACHE_V)
@pytest.mark.parametrize("d", NT.CACHE_D)
def test_text_cache_byte_for_byte(gpu, d, v, kind):
    proj = _projection(d, gpu)
    E16, wtab = _cache_table(v, d, kind, gpu)
    got = _assert_same_cache(E16, wtab, kind, proj, (d, v, kind))
    rows = got[:v * NT.CACHE_ROW * 4].view(torch.float32).view(v, NT.CACHE_ROW)
    assert bool(torch.isfinite(rows).all()) and bool((rows[:, d:2 * d + 1].abs().amax(dim=1) > 0).all())
    # the special values: +-0, a subnormal, a large value, +-inf, NaN
    E16s, _ = _cache_table(v, d, kind, gpu, special=True)
    got = _assert_same_cache(E16s, wtab, kind, proj, (d, v, kind, "special"))
    rows = got[:v * NT.CACHE_ROW * 4].view(torch.float32).view(v, NT.CACHE_ROW)
    assert bool(torch.isnan(rows[0, d:2 * d + 1]).all())  # the NaN reached every P column of its row
    # a table view 2 bytes off: never an 8-byte unit, the same bytes
    _assert_same_cache(_off(E16, 1), wtab, kind, proj, (d, v, kind, "2 bytes off"))


def test_f32_table_through_the_tt_entry_point_is_the_f32_entry_point(gpu):
    proj = _projection(D, gpu)
    E16, wtab = _cache_table(33, D, "bf16", gpu)
    E = E16.float()
    nbytes = L.query("mmb_mm2_text_cache_bytes", 33, D)
    a = torch.zeros(nbytes, dtype=torch.uint8, device=gpu)
    L.call("mmb_mm2_text_cache_tt", L.ptr(E, L.TABLE), L.MMB_TABLE_F32, 33, D, L.ptr(wtab, L.F32),
           L.ptr(proj.wm, L.F32), proj.ldw, L.ptr(a, L.BYTES), L.stream_ptr())
    assert torch.equal(a, _build("mmb_mm2_text_cache", E, None, wtab, proj, 0))


@pytest.mark.parametrize("kind", KIND_IDS)
def test_enable_text_cache_takes_a_16_bit_table_only_opted_in(gpu, kind):
    A, Vd, T_ = NT.CACHE_FRAMES
    torch.manual_seed(0)
    gen = models.AudioVisualGeneratorMultimodal(D, A, Vd, norm=None).to(gpu)
    proj = P.MMB2Projection(gen.networks(), D, A, Vd, T_, gpu)
    E16, wtab = _cache_table(3016, D, kind, gpu)
    with pytest.raises(L.MMBError, match="enable_text_cache.* word table"):
        proj.enable_text_cache(E16, wtab)
    assert getattr(proj, "text_cache", None) is None
    with pytest.raises(L.MMBError, match="enable_text_cache.* word table"):
        proj.enable_text_cache(E16.double(), wtab, table16=True)
    assert getattr(proj, "text_cache", None) is None
    proj.enable_text_cache(E16, wtab, table16=True)
    c16 = proj.text_cache.clone()
    # keyed on identity: the same tensors keep the cache, the upcast table rebuilds it -- to the same bytes
    first = proj.text_cache
    proj.enable_text_cache(E16, wtab, table16=True)
    assert proj.text_cache is first
    proj.enable_text_cache(E16.float(), wtab)
    torch.cuda.synchronize()
    assert torch.equal(proj.text_cache, c16)
    # a re-merge rebuilds it through the entry point of the table it holds
    proj.enable_text_cache(E16, wtab, table16=True)
    proj.text_cache.fill_(0x5A)
    proj.invalidate()
    assert proj.refresh_if_changed() is True
    torch.cuda.synchronize()
    assert torch.equal(proj.text_cache, c16)


# ------------------------------------------------------------------ B: the kernel, bit for bit
def _case(A, Vd, T_, N, V, kind, frames, gpu, bad=False):
    """(text on the 16-bit table, text on its upcast, audio, visual, proj, the zero-weight row)."""
    inp, proj = G16._synth_case(D, A, Vd, T_, N, V, kind, gpu)
    au, vi = (inp["audio"], inp["visual"]) if frames == "same" else (inp["audio"].float(), inp["visual"].float())
    zero_row = None
    if bad:
        # an utterance of rare words whose weights are all 0 (flagged: its x row is 0 / 0)
        zero_row = N - 2
        rare = V - 1 - torch.arange(T_, device=gpu, dtype=torch.int32)
        inp["ids"][zero_row] = rare
        inp["wtab"][rare.long()] = 0.0
        # negative ids wrap (weight 0); an id >= V is flagged and contributes a zero row
        inp["ids"][3, min(5, T_ - 1)] = -7
        inp["ids"][N - 1, 0] = -3
        inp["ids"][N // 2, T_ - 1] = V + 11
    E16 = inp["table"].to(NT.KINDS[kind])  # the caller's rounding
    text = {"ids": inp["ids"], "wtab": inp["wtab"]}
    return dict(text, table=E16), dict(text, table=E16.float()), au, vi, proj, zero_row


def _pair(dims, t16, t32, au, vi, proj, gpu, what, bounds=True, nan_rows=False):
    """The launch on the 16-bit table and its twin on the upcast table (each
    builds the projection's text cache from its own table)."""
    got = _launch(P.mm2_stream_project_narrow_tt, dims, au, vi, proj, t16, gpu, bounds)
    assert proj.text_src[0] is t16["table"]
    twin = _launch(P.mm2_stream_project_narrow_ft, dims, au, vi, proj, t32, gpu, bounds)
    assert proj.text_src[0] is t32["table"]
    _assert_bit_for_bit(got, twin, what, nan_rows)
    return got


@pytest.mark.parametrize("frames", NT.FRAME_CHOICES)
@pytest.mark.parametrize("kind", KIND_IDS)
@pytest.mark.parametrize("A,Vd,T_,N,V", NT.KERNEL_CASES, ids=[C.shape_id(c) for c in NT.KERNEL_CASES])
def test_narrow_fused_kernel_bit_for_bit(gpu, A, Vd, T_, N, V, kind, frames):
    assert P.narrow_fused_supported(T_, D, A, Vd, V)
    t16, t32, au, vi, proj, _ = _case(A, Vd, T_, N, V, kind, frames, gpu)
    dims = (D, A, Vd, T_, N)
    for bounds in (True, False):
        got = _pair(dims, t16, t32, au, vi, proj, gpu, (dims, V, kind, frames, bounds), bounds)
        assert got[4] == 0
        assert bool(torch.isfinite(got[2]).all()) and bool((got[2].abs().amax(dim=1) > 0).all())
        if bounds:  # the bounds are those of the x written
            assert torch.equal(got[3], _i32(got[0].abs().amax(dim=0)))


@pytest.mark.parametrize("frames", NT.FRAME_CHOICES)
@pytest.mark.parametrize("kind", KIND_IDS)
def test_wrapped_out_of_range_and_zero_weight_ids(gpu, kind, frames):
    A, Vd, T_, N, V = NT.BAD_CASE
    t16, t32, au, vi, proj, z = _case(A, Vd, T_, N, V, kind, frames, gpu, bad=True)
    dims = (D, A, Vd, T_, N)
    got = _pair(dims, t16, t32, au, vi, proj, gpu, (dims, V, kind, frames, "bad"), nan_rows=True)
    assert got[4] == L.MMB_FLAG_ID_RANGE | L.MMB_FLAG_ZERO_WEIGHTS
    assert float(got[1][0, z]) == 0.0  # the zero-weight utterance counts no token


@pytest.mark.parametrize("frames", NT.FRAME_CHOICES)
@pytest.mark.parametrize("kind", KIND_IDS)
def test_special_values_in_the_table(gpu, kind, frames):
    """+-0, the smallest subnormal and the largest planted value of the kind
    in row 0 and in the row most tokens name (table16_cases.special_table)."""
    case = NT.SPECIAL_CASE
    dims = case[:5]
    z = C.inputs(case)
    E16 = _dev(T.special_table(case, kind), gpu)
    text = {"ids": _dev(z["ids"], gpu, torch.int32), "wtab": _dev(z["wt32"], gpu)}
    au, vi = _frames_of(case, kind, frames, gpu)
    proj = P.MMB2Projection(_networks(case, gpu), *case[:4], gpu)
    got = _pair(dims, dict(text, table=E16), dict(text, table=E16.float()), au, vi, proj, gpu,
                (dims, kind, frames, "special"))
    assert got[4] == 0
    # the planted values reached the rows: x differs from the plain rounded table's
    P16 = _dev(T.table(case, kind), gpu)
    plain = _pair(dims, dict(text, table=P16), dict(text, table=P16.float()), au, vi, proj, gpu,
                  (dims, kind, frames, "plain"))
    assert bool((got[0] != plain[0]).any())


@pytest.mark.parametrize("kind", KIND_IDS)
def test_table_alignment_is_its_element_s(gpu, kind):
    """The launch does not read the table: 2, 4 and 8 bytes off a 16-byte
    boundary it is accepted and gives the aligned launch's bits."""
    A, Vd, T_, N, V = NT.ALIGN_CASE
    t16, t32, au, vi, proj, _ = _case(A, Vd, T_, N, V, kind, "same", gpu)
    dims = (D, A, Vd, T_, N)
    want = _pair(dims, t16, t32, au, vi, proj, gpu, (dims, kind, "aligned"))
    for elements in (1, 2, 4):
        moved = dict(t16, table=_off(t16["table"], elements))
        got = _launch(P.mm2_stream_project_narrow_tt, dims, au, vi, proj, moved, gpu)
        _assert_bit_for_bit(got, want, (dims, kind, f"{2 * elements} bytes off"))


def test_f32_table_through_the_tt_mirror_is_the_ft_entry_point(gpu):
    A, Vd, T_, N, V = NT.ALIGN_CASE
    t16, t32, au, vi, proj, _ = _case(A, Vd, T_, N, V, "bf16", "same", gpu)
    dims = (D, A, Vd, T_, N)
    got = _launch(P.mm2_stream_project_narrow_tt, dims, au, vi, proj, t32, gpu)
    want = _launch(P.mm2_stream_project_narrow_ft, dims, au, vi, proj, t32, gpu)
    _assert_bit_for_bit(got, want, (dims, "f32 table"))


# ------------------------------------------------------------------ rejections, outputs untouched
@pytest.mark.parametrize("kind", KIND_IDS)
def test_rejections_leave_the_outputs_untouched(gpu, kind):
    A, Vd, T_, N, V = NT.ALIGN_CASE
    t16, t32, au, vi, proj, _ = _case(A, Vd, T_, N, V, kind, "same", gpu)
    ids, table, wtab = t16["ids"], t16["table"], t16["wtab"]
    out, flag, colmax, ws = _bufs(N, D, gpu, fill=-7.0)
    kw = dict(flag=flag, out=out, colmax=colmax, colmax_ws=ws)
    tt = P.mm2_stream_project_narrow_tt
    with pytest.raises(L.MMBError, match="gathered text"):  # dense text: no ids
        tt(N, T_, D, A, Vd, au, vi, proj, None, table, wtab, **kw)
    with pytest.raises(L.MMBError, match="gathered text"):  # a missing table
        tt(N, T_, D, A, Vd, au, vi, proj, ids, None, wtab, **kw)
    with pytest.raises(L.MMBError, match="mm2_stream_project_narrow_tt.* word table"):
        tt(N, T_, D, A, Vd, au, vi, proj, ids, table.double(), wtab, **kw)
    with pytest.raises(L.MMBError, match="one dtype"):
        tt(N, T_, D, A, Vd, au, vi.float(), proj, ids, table, wtab, **kw)
    with pytest.raises(L.MMBError, match="colmax_ws holds"):
        tt(N, T_, D, A, Vd, au, vi, proj, ids, table, wtab, **dict(kw, colmax_ws=ws[:64]))
    assert getattr(proj, "text_cache", None) is None  # nothing was built either
    # the C ABI's own: a table at an odd address, a table type outside 0..2, frames 4 bytes off
    proj.enable_text_cache(table, wtab, table16=True)
    tail = (N, T_, D, A, Vd, L.ptr(proj.wpieces, L.BYTES), L.ptr(proj.c0, L.F32), L.ptr(out[0], L.F32),
            L.ptr(out[1], L.F32), L.ptr(out[2], L.F32), L.ptr(flag, L.I32), L.ptr(colmax, L.I32),
            L.ptr(ws, L.BYTES), L.stream_ptr())
    tk, fk = P.TABLE_KINDS[kind][1], P.FRAME_KINDS[kind][1]
    for dt, tt_, da in ((1, tk, 0), (0, 3, 0), (0, -1, 0), (0, tk, 4)):
        with pytest.raises(L.MMBError, match=r"code -1 \(invalid argument\)"):
            L.call("mmb_mm2_stream_project_narrow_tt", L.ptr(ids, L.I32), L.ptr(table, L.TABLE) + dt, tt_, V,
                   L.ptr(wtab, L.F32), L.ptr(proj.text_cache, L.BYTES), L.ptr(au, L.FRAMES) + da,
                   L.ptr(vi, L.FRAMES), fk, *tail)
    # the old mirrors keep rejecting a 16-bit table
    for name, front in (("mm2_stream_project_narrow", P.mm2_stream_project_narrow),
                        ("mm2_stream_project_narrow_ft", P.mm2_stream_project_narrow_ft)):
        with pytest.raises(L.MMBError, match=f"{name}.* word table"):
            front(N, T_, D, A, Vd, au.float(), vi.float(), proj, ids, table, wtab, **kw)
    assert _untouched(out) and int(flag.item()) == 0 and int(colmax.abs().max().item()) == 0


# ------------------------------------------------------------------ C: the step
def _step_inputs(case, kind, frames, gpu):
    """(the inputs with the 16-bit table, the same with its f32 upcast); the
    frames are f32 or of the table's kind, the same tensors in both."""
    z = C.inputs(case)
    E16 = _dev(T.table(case, kind), gpu)
    au, vi = _frames_of(case, kind, frames, gpu)
    base = {"wtab": _dev(z["wt32"], gpu), "ids": _dev(z["ids"], gpu, torch.int32), "audio": au, "visual": vi}
    return dict(base, table=E16), dict(base, table=E16.float())


def _check_oracle(case, kind, frames, step, sif, mm2):
    """The bars of tests/test_gpu_table16.py::_check_oracle."""
    x = step.x.double().cpu().numpy()
    eo = M.row_rel_err(mm2.cpu().numpy(), T.oracle_rows(case, kind, T.fkind_of(kind, frames))) / TOL
    ep = np.abs(step.pc.cpu().numpy() - O.compute_pc(x, 1)).max() / 1e-10
    ref = O.remove_pc(x, 1)
    es = (np.abs(sif.cpu().numpy() - ref) / np.abs(ref).max(axis=1, keepdims=True)).max() / F32_ROW
    print(f"{C.shape_id(case)} {kind} table, {frames} frames: MMB2 {eo:.3f} of 1e-5, PC {ep:.3f} of 1e-10, "
          f"SIF rows {es:.3f} of 2^-23")
    assert eo < 1.0 and ep < 1.0 and es <= 1.0


@pytest.mark.parametrize("frames", NT.FRAME_CHOICES)
@pytest.mark.parametrize("kind", KIND_IDS)
def test_narrow_fused_step_on_a_16_bit_table_opted_in(gpu, kind, frames):
    case = NT.STEP
    inp16, inp32 = _step_inputs(case, kind, frames, gpu)
    nets = _networks(case, gpu)
    opt = dict(narrow_frames16=True) if frames == "same" else {}
    a = P.FusedStep(inp16, nets, narrow_table16=True, **opt)
    b = P.FusedStep(inp32, nets, **opt)  # the f32-table plan: the narrow fused kernel
    assert a.table_kind == kind and b.table_kind == "f32" and a.frames == b.frames
    assert a.plan.front == "narrow_fused" and a.plan.project == "front" and a.s is None and a.narrow_fused
    assert a.plan == b.plan
    # without the table's opt-in (and, on 16-bit frames, the frames' too): the two-kernel plan
    assert P.FusedStep(inp16, nets, **opt).plan.front == "stream"
    assert P.FusedStep(inp16, nets, narrow_table16=True, narrow_fused=False, **opt).plan.front == "stream"
    if frames == "same":
        assert P.FusedStep(inp16, nets, narrow_table16=True).plan.front == "stream"
    trace = {}
    s1, m1 = [t.clone() for t in a.run(check=True, trace=trace)]
    assert "mm2_stream_project_narrow" in trace and "mm2_stream" not in trace
    s2, m2 = _run(b)
    assert torch.equal(a.x, b.x) and torch.equal(a.aux, b.aux) and torch.equal(a.pc, b.pc)
    assert torch.equal(s1, s2) and torch.equal(m1, m2)
    _check_oracle(case, kind, frames, a, s1, m1)
    # captured into a graph and replayed: the same rows
    g = P.StepGraph(a)
    for _ in range(2):
        s3, m3 = g.run(check=True)
    torch.cuda.synchronize()
    assert torch.equal(s3, s1) and torch.equal(m3, m1)
