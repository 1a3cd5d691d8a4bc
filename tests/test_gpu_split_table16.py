"""GPU: the split stream on a word table kept in fp16 / bf16 storage
(mmb_mm2_stream_split_tt, pipeline.mm2_stream_split_tt,
FusedStep(split_table16=True)).

Only the text workgroups of utt_split_part_kernel and the row-0 shortcut of
utt_split_finish_kernel read the table: a 16-bit unit of 4 values is one
8-byte load, a scalar one a 2-byte load, widened to f32 in registers and
summed by the f32 instantiation's statements in their order; the partial sums
are f32.  Both widenings are exact, so the definition under test is an
equality: a launch on a 16-bit table writes, bit for bit, what the same launch
(the same parts) of mmb_mm2_stream_split_ft writes on that table upcast to f32
-- x, s in both s_half formats, aux, the column bounds and the flag word (A);
with one range also what the one-workgroup launch (mmb_mm2_stream_tt) writes
on the 16-bit table; and x, aux, PC, SIF and MMB2 rows of the step (C), which
also holds the bars of tests/test_gpu_table16.py against the oracle on the
upcast inputs.

The ids are row-0-heavy with row 0 planted non-zero (split_table16_cases), so
the shortcut carries most of every sum.
Product library only.
"""
import numpy as np
import pytest
import torch

import frames16_gpu as G16
import mmb2_cases as C
import mmb_lib as L
import pipeline as P
import split_frames16_cases as SF
import split_table16_cases as ST
import table16_cases as T
from common_gpu import F32_ROW, TOL, _dev, _i32, _networks, _off
from frames16_gpu import _frames_of, _run
from oracle import mmb2_oracle as M
from oracle import sif_oracle as O

pytestmark = pytest.mark.gpu

KIND_IDS = list(ST.KINDS)


def _sentinel_out(N, D, A, Vd, s_half, gpu):
    return (torch.full((N, D), -7.0, device=gpu), P.s_buffer(N, P.mm2_dims(D, A, Vd)[0], s_half, gpu).fill_(-7.0),
            torch.full((3, N), -7.0, device=gpu))


def _launch(text, au, vi, s_half, bounds, ws=None, parts=0, mirror="tt"):
    """(x, s, aux, colmax or None, flag word): the split stream through the
    16-bit table's mirror ("tt") or the f32 table's ("ft"), or pipeline.mm2_stream
    ("one": the one-workgroup launch, on either table)."""
    N, T_ = text["ids"].shape
    D = text["table"].shape[1]
    A, Vd, gpu = au.shape[-1], vi.shape[-1], au.device
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    colmax, cws = G16._colmax_bufs(D, gpu) if bounds else (None, None)
    kw = dict(wtab32=text["wtab"], flag=flag, s_half=s_half, colmax=colmax, colmax_ws=cws)
    if mirror == "one":
        x, s, aux = P.mm2_stream(N, T_, D, A, Vd, au, vi, ids32=text["ids"], table=text["table"], **kw)
    else:
        split = P.mm2_stream_split_tt if mirror == "tt" else P.mm2_stream_split_ft
        x, s, aux = split(N, T_, D, A, Vd, au, vi, text["ids"], text["table"], split=ws, parts=parts, **kw)
    torch.cuda.synchronize()
    return x, s, aux, colmax, int(flag.item())


def _equal(got, twin, what, nan_rows=False):
    for name, g, t in zip(("x", "s", "aux", "colmax"), got, twin):
        if g is None or t is None:  # the bounds: asked for on both sides or on neither
            assert g is None and t is None, (what, name)
            continue
        assert g.dtype == t.dtype and g.shape == t.shape, (what, name)
        # on the bits, so that +0 / -0 count as different ...
        assert torch.equal(_i32(g), _i32(t)), (what, name, "bits")
        # ... and on the values (a NaN fails here); a zero-weight utterance's x row is
        # 0 / 0 (nan_rows): there the values are compared beside the NaNs, which the bits cover
        if nan_rows and g.is_floating_point():
            assert torch.equal(torch.isnan(g), torch.isnan(t)), (what, name, "NaN places")
            g, t = g[~torch.isnan(g)], t[~torch.isnan(t)]
        assert torch.equal(g, t), (what, name)
    assert got[4] == twin[4], (what, "flag", got[4], twin[4])


def _twin_table(E16, off_bytes):
    """The f32 upcast of a 16-bit table; where the 16-bit view's alignment puts
    the text on the scalar path (not whole 8-byte units), the f32 table 4 bytes
    off a 16-byte boundary, on the scalar path too."""
    E32 = E16.float()
    return _off(E32, 1) if off_bytes % 8 else E32


def _pair(t16, au, vi, s_half, bounds, ws, parts, what, off_bytes=0, nan_rows=False):
    """The launch on the 16-bit table and its twin on the upcast table."""
    got = _launch(t16, au, vi, s_half, bounds, ws, parts)
    t32 = dict(t16, table=_twin_table(t16["table"], off_bytes))
    twin = _launch(t32, au, vi, s_half, bounds, ws, parts, mirror="ft")
    _equal(got, twin, what, nan_rows)
    return got


def _text_case(d, t, n, kind, off_bytes, gpu):
    E16, ids, wt = ST.text_inputs(d, t, n, kind)
    E16 = _dev(E16, gpu)
    if off_bytes:
        E16 = _off(E16, off_bytes // 2)
    assert E16.data_ptr() % 16 == off_bytes and (E16.data_ptr() % 8 == 0) == ST.vector(4, off_bytes)
    return {"ids": _dev(ids, gpu, torch.int32), "table": E16, "wtab": _dev(wt, gpu)}


def _frames(a, t, n, d, kind, frames, gpu):
    au, vi = (_dev(x, gpu) for x in ST.frames_of(a, t, n, d))
    return (au.to(ST.KINDS[kind]), vi.to(ST.KINDS[kind])) if frames == "same" else (au, vi)


# ------------------------------------------------------------------ A: the kernel, bit for bit
@pytest.mark.parametrize("frames", ST.FRAME_CHOICES)
@pytest.mark.parametrize("kind", KIND_IDS)
@pytest.mark.parametrize("d,t,parts,off,w,n", ST.TEXT_CASES, ids=[f"D{c[0]}-T{c[1]}-off{c[3]}" for c in ST.TEXT_CASES])
def test_split_text_shapes_bit_for_bit(gpu, d, t, parts, off, w, n, kind, frames):
    text = _text_case(d, t, n, kind, off, gpu)
    au, vi = _frames(w, t, n, d, kind, frames, gpu)
    bounds = (d, t, parts, off, w, n) == ST.BOUNDS_CASE and d <= 640
    for p in parts:
        ws = P.split_ws(n, t, d, w, w, gpu, parts=p)
        for s_half in (True, False):
            got = _pair(text, au, vi, s_half, bounds, ws, p, (d, t, p, off, kind, frames, s_half), off)
            assert got[4] == 0 and bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[2]).all())
            if bounds:  # the bounds are those of the x written
                assert torch.equal(got[3], _i32(got[0].abs().amax(dim=0)))
            if p == 1:
                # one range: the one-workgroup launch on the 16-bit table (mmb_mm2_stream_tt), bit for bit
                one = _launch(text, au, vi, s_half, bounds, mirror="one")
                _equal(got, one, (d, t, kind, frames, "one workgroup", s_half))
    # the all-row-0 utterance is the shortcut's alone: x = w0 E0 / count, Sx_e = c0 E0
    got = _launch(text, au, vi, False, False, P.split_ws(n, t, d, w, w, gpu, parts=parts[0]), parts[0])
    E0 = text["table"][0].float()
    assert torch.equal(got[1][0, :d], t * E0)


@pytest.mark.parametrize("frames", ST.FRAME_CHOICES)
@pytest.mark.parametrize("kind", KIND_IDS)
@pytest.mark.parametrize("N,T_,A,Vd,parts", ST.FRAME_SHAPE_CASES, ids=[C.shape_id(c[:4]) for c in ST.FRAME_SHAPE_CASES])
def test_split_at_d_300_bit_for_bit(gpu, N, T_, A, Vd, parts, kind, frames):
    case = SF.case_of(N, T_, A, Vd)
    z = C.inputs(case)
    E16 = _dev(T.special_table(case, kind), gpu)  # row 0 planted: +-0, a subnormal, a large value
    text = {"ids": _dev(z["ids"], gpu, torch.int32), "table": E16, "wtab": _dev(z["wt32"], gpu)}
    au, vi = _frames_of(case, kind, frames, gpu)
    D = ST.D_FRAME_SHAPES
    for p in parts:
        ws = P.split_ws(N, T_, D, A, Vd, gpu, parts=p)
        for s_half in (True, False):
            got = _pair(text, au, vi, s_half, True, ws, p, (case, kind, frames, p, s_half))
            assert got[4] == 0
            if p == 1:
                one = _launch(text, au, vi, s_half, True, mirror="one")
                _equal(got, one, (case, kind, frames, "one workgroup", s_half))


@pytest.mark.parametrize("kind", KIND_IDS)
def test_wrapped_out_of_range_and_zero_weight_ids(gpu, kind):
    N, T_, A, Vd, parts = ST.BAD_CASE
    case = SF.case_of(N, T_, A, Vd)
    z = C.inputs(case)
    text = {"ids": _dev(z["ids"], gpu, torch.int32), "table": _dev(T.table(case, kind), gpu),
            "wtab": _dev(z["wt32"], gpu)}
    # an utterance of rare words whose weights are all 0 (flagged: its x row is 0 / 0)
    zr = N - 2
    rare = SF.V - 1 - torch.arange(T_, device=gpu, dtype=torch.int32)
    text["ids"][zr] = rare
    text["wtab"][rare.long()] = 0.0
    # negative ids wrap (weight 0); an id >= V is flagged and contributes a zero row
    text["ids"][3, 5] = -7
    text["ids"][N - 1, 0] = -3
    text["ids"][N // 2, T_ - 1] = SF.V + 11
    au, vi = _frames_of(case, kind, "same", gpu)
    ws = P.split_ws(N, T_, SF.D, A, Vd, gpu, parts=parts)
    for s_half in (True, False):
        got = _pair(text, au, vi, s_half, True, ws, parts, (case, kind, "bad", s_half), nan_rows=True)
        assert got[4] == L.MMB_FLAG_ID_RANGE | L.MMB_FLAG_ZERO_WEIGHTS
        assert float(got[2][0, zr]) == 0.0 and bool(torch.isnan(got[0][zr]).all())
        assert int(torch.isnan(got[0]).any(dim=1).sum()) == 1


@pytest.mark.parametrize("kind", KIND_IDS)
def test_independent_of_what_the_workspace_held(gpu, kind):
    d, t, parts, off, w, n = ST.TEXT_CASES[2]
    text = _text_case(d, t, n, kind, off, gpu)
    au, vi = _frames(w, t, n, d, kind, "same", gpu)
    ws = P.split_ws(n, t, d, w, w, gpu, parts=parts[0])
    outs = []
    for fill in ST.WS_FILLS:
        ws.fill_(fill)
        outs.append(_launch(text, au, vi, True, False, ws, parts[0]))
    for o in outs[1:]:
        _equal(o, outs[0], (kind, "workspace"))


def test_f32_table_through_the_tt_mirror_is_the_ft_entry_point(gpu):
    d, t, parts, off, w, n = ST.TEXT_CASES[3]
    text = _text_case(d, t, n, "bf16", off, gpu)
    t32 = dict(text, table=text["table"].float())
    au, vi = _frames(w, t, n, d, "bf16", "same", gpu)
    ws = P.split_ws(n, t, d, w, w, gpu, parts=parts[0])
    _equal(_launch(t32, au, vi, True, False, ws, parts[0]), _launch(t32, au, vi, True, False, ws, parts[0], "ft"),
           "f32 table")


# ------------------------------------------------------------------ B: rejections, outputs untouched
@pytest.mark.parametrize("kind", KIND_IDS)
def test_rejections_leave_the_outputs_untouched(gpu, kind):
    d, t, parts, off, w, n = ST.TEXT_CASES[1][0], 97, (2,), 0, 8, 6
    text = _text_case(d, t, n, kind, 0, gpu)
    ids, table, wtab = text["ids"], text["table"], text["wtab"]
    au, vi = _frames(w, t, n, d, kind, "same", gpu)
    ws = P.split_ws(n, t, d, w, w, gpu, parts=2)
    out = _sentinel_out(n, d, w, w, True, gpu)
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    colmax, cws = G16._colmax_bufs(d, gpu)
    kw = dict(wtab32=wtab, flag=flag, out=out, colmax=colmax, colmax_ws=cws, parts=2)
    tt = P.mm2_stream_split_tt
    with pytest.raises(L.MMBError, match="gathered text"):  # dense text: no ids
        tt(n, t, d, w, w, au, vi, None, table, split=ws, **kw)
    with pytest.raises(L.MMBError, match="gathered text"):  # a missing table
        tt(n, t, d, w, w, au, vi, ids, None, split=ws, **kw)
    with pytest.raises(L.MMBError, match="mm2_stream_split_tt.* word table"):
        tt(n, t, d, w, w, au, vi, ids, table.double(), split=ws, **kw)
    with pytest.raises(L.MMBError, match="one dtype"):
        tt(n, t, d, w, w, au, vi.float(), ids, table, split=ws, **kw)
    with pytest.raises(L.MMBError, match="s buffer dtype"):
        tt(n, t, d, w, w, au, vi, ids, table, split=ws, s_half=False, **kw)
    # the C ABI's own: a workspace slice that is too short, a table at an odd address, a table type outside 0..2
    with pytest.raises(L.MMBError, match=r"code -1 \(invalid argument\)"):
        tt(n, t, d, w, w, au, vi, ids, table, split=ws[:64], **kw)
    tk, fk = P.TABLE_KINDS[kind][1], P.FRAME_KINDS[kind][1]
    for dt, tt_ in ((1, tk), (0, 3), (0, -1)):
        with pytest.raises(L.MMBError, match=r"code -1 \(invalid argument\)"):
            L.call("mmb_mm2_stream_split_tt", L.ptr(ids, L.I32), L.ptr(table, L.TABLE) + dt, tt_, ST.V,
                   L.ptr(wtab, L.F32), None, L.ptr(au, L.FRAMES), L.ptr(vi, L.FRAMES), fk, n, t, d, w, w,
                   L.ptr(out[0], L.F32), L.ptr(out[1], L.S_BUF), 1, L.ptr(out[2], L.F32), L.ptr(flag, L.I32),
                   L.ptr(colmax, L.I32), L.ptr(cws, L.BYTES), 2, L.ptr(ws, L.BYTES), ws.numel(), L.stream_ptr())
    # the old mirrors keep rejecting a 16-bit table
    with pytest.raises(L.MMBError, match="mm2_stream_split_ft.* word table"):
        P.mm2_stream_split_ft(n, t, d, w, w, au, vi, ids, table, split=ws, **kw)
    with pytest.raises(L.MMBError, match="split stream reads a float32 word table only"):
        P.mm2_stream(n, t, d, w, w, au.float(), vi.float(), ids32=ids, table=table, split=ws, **kw)
    assert G16._untouched(out) and int(flag.item()) == 0 and int(colmax.abs().max().item()) == 0


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


@pytest.mark.parametrize("frames", ST.FRAME_CHOICES)
@pytest.mark.parametrize("kind", KIND_IDS)
def test_split_step_on_a_16_bit_table_opted_in(gpu, kind, frames):
    case = SF.case_of(*ST.STEP)
    inp16, inp32 = _step_inputs(case, kind, frames, gpu)
    nets = _networks(case, gpu)
    opt = dict(split_frames16=True) if frames == "same" else {}
    a = P.FusedStep(inp16, nets, split_table16=True, **opt)
    b = P.FusedStep(inp32, nets, **opt)  # the f32-table plan: the split stream
    assert a.table_kind == kind and b.table_kind == "f32" and a.frames == b.frames
    assert a.plan.split is True and a.plan.front == "stream" and a.split is not None and a.s is not None
    assert a.plan == b.plan
    # without the table's opt-in (and, on 16-bit frames, the frames' too): one workgroup per transcript
    assert P.FusedStep(inp16, nets, **opt).plan == a.plan._replace(split=False)
    assert P.FusedStep(inp16, nets, split_table16=True, split_stream=False, **opt).plan.split is False
    if frames == "same":
        assert P.FusedStep(inp16, nets, split_table16=True).plan.split is False
    trace = {}
    s1, m1 = [t.clone() for t in a.run(check=True, trace=trace)]
    assert "mm2_stream" in trace
    s2, m2 = _run(b)
    assert torch.equal(a.x, b.x) and torch.equal(a.aux, b.aux) and torch.equal(a.pc, b.pc)
    assert torch.equal(a.s, b.s) and torch.equal(s1, s2) and torch.equal(m1, m2)
    _check_oracle(case, kind, frames, a, s1, m1)
    # captured into a graph and replayed: the same rows
    g = P.StepGraph(a)
    for _ in range(2):
        s3, m3 = g.run(check=True)
    torch.cuda.synchronize()
    assert torch.equal(s3, s1) and torch.equal(m3, m1)
