"""GPU: the split stream on audio / visual frames kept in fp16 / bf16 storage
(mmb_mm2_stream_split_ft, pipeline.mm2_stream_split_ft,
FusedStep(split_frames16=True)).

Only the frame workgroups of utt_split_part_kernel read the frames: a 16-bit
unit of 4 values is one 8-byte load, a scalar one a 2-byte load, widened to
f32 in registers and summed by the f32 instantiation's statements in their
order; the partial sums are f32 and the finish kernel is the same one.  Both
widenings are exact, so the definition under test is an equality: a launch on
16-bit frames writes, bit for bit, what the same launch (the same parts) of
mmb_mm2_stream_split writes on those frames upcast to f32 -- x, s, aux, the
column bounds and the flag word (A); with one range also what the
one-workgroup 16-bit launch (mmb_mm2_stream_ft) writes; and x, PC, SIF and
MMB2 rows of the step (C).  The f32 twin is the split stream the suite already
holds to the one-workgroup kernel and the oracle (tests/test_gpu_split.py);
the opted-in step at POM's real valid shape is also held to the oracle on the
rounded frames at that file's bars.

The 16-bit frame tensors are views into larger allocations whose other
elements hold 2^14 (split_frames16_cases.GUARD), so that a range or an offset
in the wrong unit reads a value that moves the sums.
Product library only.
"""
import copy

import numpy as np
import pytest
import torch

import frames16_cases as F
import frames16_gpu as G16
import mmb2_cases as C
import mmb_lib as L
import models
import pipeline as P
import split_frames16_cases as SF
import synth
from frames16_gpu import _dev, _i32
from mmb2_gpu import _pom
from oracle import mmb2_oracle as M
from oracle import sif_oracle as O

pytestmark = pytest.mark.gpu

KIND_IDS = list(SF.KINDS)
D = SF.D


def _guarded(t16, extra=0):
    """A contiguous copy of `t16` inside a larger allocation filled with GUARD,
    `extra` elements past a 16-byte boundary."""
    T, W = t16.shape[1:]
    g = SF.guard_elements(T, W) + extra
    flat = torch.full((t16.numel() + 2 * g,), SF.GUARD, dtype=t16.dtype, device=t16.device)
    view = flat[g:g + t16.numel()].view(t16.shape)
    view.copy_(t16)
    assert view.is_contiguous() and view.data_ptr() % 16 == (extra * t16.element_size()) % 16
    assert float(flat[g - 1]) == float(flat[g + t16.numel()]) == SF.GUARD
    return view


def _text(case, gpu):
    z = C.inputs(case)
    return {"ids": _dev(z["ids"], gpu, torch.int32), "table": _dev(z["E"], gpu), "wtab": _dev(z["wt32"], gpu)}


def _sentinel_out(N, A, Vd, s_half, gpu):
    return (torch.full((N, D), -7.0, device=gpu), P.s_buffer(N, P.mm2_dims(D, A, Vd)[0], s_half, gpu).fill_(-7.0),
            torch.full((3, N), -7.0, device=gpu))


def _launch(text, au, vi, s_half, bounds, ws=None, parts=0, ft=True):
    """(x, s, aux, colmax or None, flag word): the split stream through the
    16-bit mirror (`ft`), or pipeline.mm2_stream -- its split route with `ws`,
    the one-workgroup launch without."""
    N, T = text["ids"].shape
    A, Vd, gpu = au.shape[-1], vi.shape[-1], au.device
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    colmax, cws = G16._colmax_bufs(D, gpu) if bounds else (None, None)
    kw = dict(wtab32=text["wtab"], flag=flag, s_half=s_half, colmax=colmax, colmax_ws=cws, split=ws, parts=parts)
    if ft:
        x, s, aux = P.mm2_stream_split_ft(N, T, D, A, Vd, au, vi, text["ids"], text["table"], **kw)
    else:
        x, s, aux = P.mm2_stream(N, T, D, A, Vd, au, vi, ids32=text["ids"], table=text["table"], **kw)
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


def _twin_frames(t16, off):
    """The f32 upcast of a 16-bit view; where the view's alignment puts it on
    the scalar path (`off` elements, not whole units), the f32 tensor 4 bytes
    off a 16-byte boundary, on the scalar path too."""
    t32 = t16.float()
    return G16._off(t32, 1) if off % 4 else t32


def _pair(text, a16, v16, s_half, bounds, ws, parts, what, offs=(0, 0), nan_rows=False):
    """The launch on the 16-bit frames and its f32 twin on their upcast."""
    got = _launch(text, a16, v16, s_half, bounds, ws, parts)
    twin = _launch(text, _twin_frames(a16, offs[0]), _twin_frames(v16, offs[1]), s_half, bounds, ws, parts, ft=False)
    _equal(got, twin, what, nan_rows)
    return got


def _sweep(text, a16, v16, ws, parts, what, offs=(0, 0)):
    """s_half x column bounds; the outputs of (True, True)."""
    out = None
    for s_half in (True, False):
        for bounds in (True, False):
            got = _pair(text, a16, v16, s_half, bounds, ws, parts, what + (s_half, bounds), offs)
            assert got[4] == 0 and bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[2]).all())
            if bounds:  # the bounds are those of the x written
                assert torch.equal(got[3], _i32(got[0].abs().amax(dim=0)))
            out = out or got
    return out


# ------------------------------------------------------------------ A: the kernel, bit for bit
@pytest.mark.parametrize("kind", KIND_IDS)
@pytest.mark.parametrize("N,T,A,Vd,parts,ao,vo", SF.KERNEL_CASES, ids=[C.shape_id(c[:4]) for c in SF.KERNEL_CASES])
def test_split_kernel_bit_for_bit(gpu, N, T, A, Vd, parts, ao, vo, kind):
    case = SF.case_of(N, T, A, Vd)
    text = _text(case, gpu)
    a16, v16 = (_guarded(_dev(t, gpu), off) for t, off in zip(F.frames(case, kind), (ao, vo)))
    assert a16.dtype == v16.dtype == SF.KINDS[kind]
    assert (a16.data_ptr() % 8 == 0) == SF.vector(4, ao) and (v16.data_ptr() % 8 == 0) == SF.vector(4, vo)
    for p in parts:
        ws = P.split_ws(N, T, D, A, Vd, gpu, parts=p)
        _sweep(text, a16, v16, ws, p, (case, kind, p), (ao, vo))
        if p == 1:
            # one range: the one-workgroup 16-bit launch (mmb_mm2_stream_ft), bit for bit
            for s_half in (True, False):
                got = _launch(text, a16, v16, s_half, True, ws, 1)
                one = _launch(text, a16, v16, s_half, True, ft=False)
                _equal(got, one, (case, kind, "one workgroup", s_half))


@pytest.fixture(scope="module")
def pom_valid(gpu, golden):
    """POM's real valid split (100 x 1089, A = Vd = 300) as tests/test_gpu_split.py builds it."""
    inp, host = _pom(golden, "valid", 100, 300, 300, seed=93, dev=gpu)
    assert tuple(inp["ids"].shape) + (300, 300) == SF.POM_VALID
    return inp, host


def _rounded(inp, kind):
    """(the inputs with the frames rounded to the kind, the same with their f32 upcast)."""
    a16, v16 = (_guarded(inp[k].to(SF.KINDS[kind])) for k in ("audio", "visual"))
    return dict(inp, audio=a16, visual=v16), dict(inp, audio=a16.float(), visual=v16.float())


@pytest.mark.parametrize("kind", KIND_IDS)
def test_split_kernel_at_pom_valid_shape(gpu, pom_valid, kind):
    inp16, _ = _rounded(pom_valid[0], kind)
    N, T, A, Vd = SF.POM_VALID
    assert P.split_parts(N, T) >= 1
    ws = P.split_ws(N, T, D, A, Vd, gpu)  # the automatic plan
    _sweep(inp16, inp16["audio"], inp16["visual"], ws, 0, ("pom valid", kind))


@pytest.mark.parametrize("kind", KIND_IDS)
@pytest.mark.parametrize("case,parts", SF.SPECIAL_CASES, ids=[C.shape_id(c) for c, _ in SF.SPECIAL_CASES])
def test_special_values(gpu, case, parts, kind):
    """Trailing -10 pad frames, +-0, the smallest subnormal, the largest finite
    fp16 value; for bf16 a subnormal and 2^40 -- in 8-byte units and in scalar
    2-byte loads."""
    Dc, A, Vd, T, N, V = case
    text = _text(case, gpu)
    a16, v16 = (_guarded(_dev(t, gpu)) for t in F.special_frames(case, kind))
    ws = P.split_ws(N, T, D, A, Vd, gpu, parts=parts)
    _sweep(text, a16, v16, ws, parts, (case, kind, "special"))
    # the planted values reached the sums: the largest one squared dominates its column
    s = _launch(text, a16, v16, False, False, ws, parts)[1]
    big = float(F.SPECIALS[kind][-1][0]) ** 2
    assert bool(torch.isfinite(s).all())
    assert float(s[0, 2 * D + A]) >= big and float(s[1, 2 * (D + A) + Vd + Vd - 1]) >= big
    # and row 2 saw its pad frames: -10 each among T - 2 values of [-1, 1]
    pads = F.SPECIAL_PADS
    assert float(s[2, 2 * D]) <= -10.0 * pads + (T - pads) and float(s[2, 2 * D + A]) >= 100.0 * pads


@pytest.mark.parametrize("kind", KIND_IDS)
def test_wrapped_out_of_range_and_zero_weight_ids(gpu, kind):
    N, T, A, Vd, parts = SF.BAD_CASE
    case = SF.case_of(N, T, A, Vd)
    text = {k: v.clone() for k, v in _text(case, gpu).items()}
    # an utterance of rare words whose weights are all 0 (flagged: its x row is 0 / 0)
    z = N - 2
    rare = SF.V - 1 - torch.arange(T, device=gpu, dtype=torch.int32)
    text["ids"][z] = rare
    text["wtab"][rare.long()] = 0.0
    # negative ids wrap (weight 0); an id >= V is flagged and contributes a zero row
    text["ids"][3, 5] = -7
    text["ids"][N - 1, 0] = -3
    text["ids"][N // 2, T - 1] = SF.V + 11
    a16, v16 = (_guarded(_dev(t, gpu)) for t in F.frames(case, kind))
    ws = P.split_ws(N, T, D, A, Vd, gpu, parts=parts)
    for s_half in (True, False):
        for bounds in (True, False):
            got = _pair(text, a16, v16, s_half, bounds, ws, parts, (case, kind, "bad", s_half, bounds),
                        nan_rows=True)
            assert got[4] == L.MMB_FLAG_ID_RANGE | L.MMB_FLAG_ZERO_WEIGHTS
            assert float(got[2][0, z]) == 0.0 and bool(torch.isnan(got[0][z]).all())
            assert int(torch.isnan(got[0]).any(dim=1).sum()) == 1


@pytest.mark.parametrize("kind", KIND_IDS)
def test_deterministic_and_independent_of_the_workspace(gpu, kind):
    N, T, A, Vd, parts = 3, 200, 76, 48, 7
    case = SF.case_of(N, T, A, Vd)
    text = _text(case, gpu)
    a16, v16 = (_guarded(_dev(t, gpu)) for t in F.frames(case, kind))
    ws = P.split_ws(N, T, D, A, Vd, gpu, parts=parts)
    ws.zero_()
    first = _launch(text, a16, v16, True, True, ws, parts)
    again = _launch(text, a16, v16, True, True, ws, parts)
    _equal(again, first, (case, kind, "twice"))
    ws[:ws.numel() // 4 * 4].view(torch.int32).fill_(0x7FC00000)  # NaN bits in every partial
    dirty = _launch(text, a16, v16, True, True, ws, parts)
    _equal(dirty, first, (case, kind, "NaN workspace"))


def test_f32_frames_through_the_ft_mirror_are_the_f32_entry_point(gpu):
    N, T, A, Vd, parts = 3, 200, 76, 48, 7
    case = SF.case_of(N, T, A, Vd)
    text = _text(case, gpu)
    a32, v32 = (_dev(t, gpu).float() for t in F.frames(case, "bf16"))
    ws = P.split_ws(N, T, D, A, Vd, gpu, parts=parts)
    _equal(_launch(text, a32, v32, True, True, ws, parts), _launch(text, a32, v32, True, True, ws, parts, ft=False),
           (case, "f32"))


# ------------------------------------------------------------------ B: rejections, outputs untouched
@pytest.mark.parametrize("kind", KIND_IDS)
def test_rejections_leave_the_outputs_untouched(gpu, kind):
    N, T, A, Vd, parts = 6, 97, 76, 48, 2
    case = SF.case_of(N, T, A, Vd)
    text = _text(case, gpu)
    a16, v16 = (_guarded(_dev(t, gpu)) for t in F.frames(case, kind))
    ws = P.split_ws(N, T, D, A, Vd, gpu, parts=parts)
    out = _sentinel_out(N, A, Vd, True, gpu)
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    colmax, cws = G16._colmax_bufs(D, gpu)
    # a 16-bit frame base at an odd address (no tensor starts there: the C ABI itself)
    for da, dv in ((1, 0), (0, 1)):
        with pytest.raises(L.MMBError, match=r"code -1 \(invalid argument\)"):
            L.call("mmb_mm2_stream_split_ft", L.ptr(text["ids"]), L.ptr(text["table"]), SF.V, L.ptr(text["wtab"]),
                   None, L.ptr(a16) + da, L.ptr(v16) + dv, P.FRAME_KINDS[kind][1], N, T, D, A, Vd, L.ptr(out[0]),
                   L.ptr(out[1]), 1, L.ptr(out[2]), L.ptr(flag), L.ptr(colmax), L.ptr(cws), parts, L.ptr(ws),
                   ws.numel(), L.stream_ptr())
    kw = dict(wtab32=text["wtab"], flag=flag, out=out, colmax=colmax, colmax_ws=cws, parts=parts)
    # a workspace slice that is too short
    with pytest.raises(L.MMBError, match=r"code -1 \(invalid argument\)"):
        P.mm2_stream_split_ft(N, T, D, A, Vd, a16, v16, text["ids"], text["table"], split=ws[:1024], **kw)
    # the mirror's own checks come before any launch, and mm2_stream still refuses 16-bit frames with split=
    with pytest.raises(L.MMBError, match="one dtype"):
        P.mm2_stream_split_ft(N, T, D, A, Vd, a16, v16.float(), text["ids"], text["table"], split=ws, **kw)
    with pytest.raises(L.MMBError, match="gathered text"):
        P.mm2_stream_split_ft(N, T, D, A, Vd, a16, v16, None, text["table"], split=ws, **kw)
    with pytest.raises(L.MMBError, match="s buffer dtype"):
        P.mm2_stream_split_ft(N, T, D, A, Vd, a16, v16, text["ids"], text["table"], split=ws, s_half=False, **kw)
    with pytest.raises(L.MMBError, match="colmax_ws holds"):
        P.mm2_stream_split_ft(N, T, D, A, Vd, a16, v16, text["ids"], text["table"], split=ws,
                              **dict(kw, colmax_ws=cws[:64]))
    with pytest.raises(L.MMBError, match="split stream reads float32 frames only"):
        P.mm2_stream(N, T, D, A, Vd, a16, v16, ids32=text["ids"], table=text["table"], split=ws, **kw)
    assert G16._untouched(out) and int(flag.item()) == 0 and int(colmax.abs().max().item()) == 0


# ------------------------------------------------------------------ C: the step
def _generator(A, Vd, gpu, seed=4):
    torch.manual_seed(seed)
    return models.AudioVisualGeneratorMultimodal(D, A, Vd, norm=None).to(gpu)


def _steps(inp16, inp32, kind, gen):
    """(the opted-in step on the 16-bit frames, the f32 step on their upcast), run eagerly and compared."""
    a = P.FusedStep(inp16, gen.networks(), split_frames16=True)
    b = P.FusedStep(inp32, gen.networks())
    assert a.plan.split is True and a.plan.frames == kind and a.plan.front == "stream"
    assert a.split is not None and a.s is not None
    assert b.plan.split is True and a.plan._replace(frames="f32") == b.plan
    trace = {}
    s1, m1 = [t.clone() for t in a.run(check=True, trace=trace)]
    assert "mm2_stream" in trace
    s2, m2 = G16._run(b)
    torch.cuda.synchronize()
    assert torch.equal(a.x, b.x) and torch.equal(a.aux, b.aux) and torch.equal(a.pc, b.pc)
    assert torch.equal(s1, s2) and torch.equal(m1, m2)
    # through a graph, two replays: the same rows
    g = P.StepGraph(a)
    for _ in range(2):
        s3, m3 = g.run(check=True)
    torch.cuda.synchronize()
    assert torch.equal(s3, s2) and torch.equal(m3, m2) and torch.equal(a.x, b.x) and torch.equal(a.pc, b.pc)
    return a, s1, m1


@pytest.mark.parametrize("kind", KIND_IDS)
def test_split_step_on_16_bit_frames_opted_in(gpu, kind):
    N, T, A, Vd = SF.STEP
    inp16 = synth.device_workload(N, T, 5000, D=D, A=A, Vd=Vd, seed=120, device=gpu, frame_dtype=SF.KINDS[kind])
    inp16["audio"], inp16["visual"] = _guarded(inp16["audio"]), _guarded(inp16["visual"])
    inp32 = dict(inp16, audio=inp16["audio"].float(), visual=inp16["visual"].float())
    _steps(inp16, inp32, kind, _generator(A, Vd, gpu))


@pytest.mark.parametrize("kind", KIND_IDS)
def test_split_step_at_pom_valid_shape_and_oracle(gpu, pom_valid, kind):
    """The opted-in step at POM's real valid shape: the f32 step's rows bit for
    bit, and the oracle on the rounded frames at the bars of
    tests/test_gpu_split.py::test_split_step_vs_one_workgroup_step_and_oracle."""
    inp, (E, wt, ids, _, _) = pom_valid
    inp16, inp32 = _rounded(inp, kind)
    gen = _generator(300, 300, gpu)
    a, s1, m1 = _steps(inp16, inp32, kind, gen)
    es = M.row_rel_err(s1.cpu().numpy(), O.get_sentence_embeddings(E, wt, ids))
    r = np.arange(0, 100, 3)
    rows = torch.as_tensor(r, device=gpu)
    audio, visual = inp32["audio"][rows].cpu().numpy(), inp32["visual"][rows].cpu().numpy()
    sw = np.where(ids[r] >= 0, wt.astype(np.float32)[ids[r]], 0).astype(np.float32)
    text = E[ids[r]]
    ref = M.estimate_embedding_overall_gpu2(M.concat_inputs(text, audio, visual),
                                            M.params_from_module(copy.deepcopy(gen).cpu()), sw, text)
    em = M.row_rel_err(m1[rows].cpu().numpy(), ref)
    print(f"{kind}: SIF rows {es:.2e} (bar 1e-5), MMB2 rows {em:.2e} (bar 1e-5)")
    assert es < 1e-5 and em < 1e-5


@pytest.mark.parametrize("kind", KIND_IDS)
def test_step_without_the_keyword_keeps_its_plan(gpu, kind):
    N, T, A, Vd = SF.STEP
    inp16 = synth.device_workload(N, T, 5000, D=D, A=A, Vd=Vd, seed=120, device=gpu, frame_dtype=SF.KINDS[kind])
    nets = _generator(A, Vd, gpu).networks()
    base = P.FusedStep(inp16, nets, split_stream=False)
    for kw in ({}, dict(split_stream=True), dict(fused_frames16=True, narrow_frames16=True)):
        off = P.FusedStep(inp16, nets, **kw)
        assert off.plan.split is False and off.split is None and off.plan.frames == kind
        assert off.plan == base.plan
    assert P.FusedStep(inp16, nets, split_frames16=True, split_stream=False).plan == base.plan
