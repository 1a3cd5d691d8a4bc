"""GPU: the narrow fused kernel on audio / visual frames kept in fp16 / bf16
storage (mmb_mm2_stream_project_narrow_ft, pipeline.mm2_stream_project_narrow_ft,
FusedStep(narrow_frames16=True)).

On 16-bit rows a frame instruction keeps its lane mapping (lane = f U + c: row
f of the group, column unit c of 4 values) and loads the unit with one 8-byte
buffer load where an f32 row takes a 16-byte one; lane offsets, group offsets
and the descriptor range are in 16-bit bytes; the units stay packed and are
widened where the frame is summed.  Both widenings are exact and the sums are
the f32 instantiation's statements in their order, so the definition under
test is an equality: a launch on 16-bit frames writes, bit for bit, what the
same launch (the same n: the same rows per wave and grid) writes on those
frames upcast to f32 -- x, the three aux planes, the MMB2 rows, the column
bounds and the flag word (A), and x, aux, PC, SIF and MMB2 rows of the step
(C).  The f32 twin is the narrow fused kernel the suite already holds to the
two-kernel step and the oracle (tests/test_gpu_mmb2.py); the opted-in step is
also held to the oracle on the upcast frames at that test's bars.

The 16-bit frame tensors are views into a larger allocation whose other
elements hold 2^14 (narrow_frames16_cases.GUARD), so that a range or an offset
in the wrong unit, or a partial last group whose range is too long, reads a
value that moves the sums.
Product library only.
"""
import copy
import functools

import numpy as np
import pytest
import torch

import frames16_cases as F
import frames16_gpu as G16
import mmb2_cases as C
import mmb_lib as L
import models
import narrow_frames16_cases as NF
import pipeline as P
import synth
from frames16_gpu import TOL, _assert_bit_for_bit, _bufs, _i32, _launch
from oracle import mmb2_oracle as M
from oracle import sif_oracle as O

pytestmark = pytest.mark.gpu

KIND_IDS = list(NF.KINDS)


def _guarded(t16, extra=0):
    """A contiguous copy of `t16` inside a larger allocation filled with GUARD,
    `extra` elements past a 16-byte boundary."""
    T, W = t16.shape[1:]
    g = NF.guard_elements(T, W) + extra
    flat = torch.full((t16.numel() + 2 * g,), NF.GUARD, dtype=t16.dtype, device=t16.device)
    view = flat[g:g + t16.numel()].view(t16.shape)
    view.copy_(t16)
    assert view.is_contiguous() and view.data_ptr() % 16 == (extra * t16.element_size()) % 16
    assert float(flat[g - 1]) == float(flat[g + t16.numel()]) == NF.GUARD
    return view


# the launch on the 16-bit frames and its f32 twin on their upcast
_pair = functools.partial(G16._pair, (P.mm2_stream_project_narrow_ft, P.mm2_stream_project_narrow))


def _synth_case(A, Vd, T, N, V, kind, gpu, bad=False):
    """G16._synth_case with the frames inside guarded allocations."""
    inp, proj = G16._synth_case(NF.D, A, Vd, T, N, V, kind, gpu)
    inp["audio"], inp["visual"] = _guarded(inp["audio"]), _guarded(inp["visual"])
    zero_row = None
    if bad:
        # an utterance of rare words whose weights are all 0 (flagged: its x row is 0 / 0)
        zero_row = N - 2
        rare = V - 1 - torch.arange(T, device=gpu, dtype=torch.int32)
        inp["ids"][zero_row] = rare
        inp["wtab"][rare.long()] = 0.0
        # negative ids wrap (weight 0); an id >= V is flagged and contributes a zero row
        inp["ids"][3, min(5, T - 1)] = -7
        inp["ids"][N - 1, 0] = -3
        inp["ids"][N // 2, T - 1] = V + 11
    return inp, proj, zero_row


# ------------------------------------------------------------------ A: the kernel, bit for bit
@pytest.mark.parametrize("kind", KIND_IDS)
@pytest.mark.parametrize("A,Vd,T,N,V", NF.KERNEL_CASES, ids=[C.shape_id(c) for c in NF.KERNEL_CASES])
def test_narrow_fused_kernel_bit_for_bit(gpu, A, Vd, T, N, V, kind):
    assert P.narrow_fused_supported(T, NF.D, A, Vd, V)
    inp, proj, _ = _synth_case(A, Vd, T, N, V, kind, gpu)
    dims = (NF.D, A, Vd, T, N)
    for bounds in (True, False):
        got = _pair(dims, inp["audio"], inp["visual"], proj, inp, gpu, (dims, V, kind, bounds), bounds)
        assert got[4] == 0
        assert bool(torch.isfinite(got[2]).all()) and bool((got[2].abs().amax(dim=1) > 0).all())
        if bounds:  # the bounds are those of the x written
            assert torch.equal(got[3], _i32(got[0].abs().amax(dim=0)))


@pytest.mark.parametrize("kind", KIND_IDS)
@pytest.mark.parametrize("A,Vd,T,N,V", NF.BAD_CASES, ids=[C.shape_id(c) for c in NF.BAD_CASES])
def test_wrapped_out_of_range_and_zero_weight_ids(gpu, A, Vd, T, N, V, kind):
    inp, proj, z = _synth_case(A, Vd, T, N, V, kind, gpu, bad=True)
    dims = (NF.D, A, Vd, T, N)
    for bounds in (True, False):
        got = _pair(dims, inp["audio"], inp["visual"], proj, inp, gpu, (dims, V, kind, bounds, "bad"), bounds,
                    nan_rows=True)
        print(f"flag {got[4]}")
        assert got[4] == L.MMB_FLAG_ID_RANGE | L.MMB_FLAG_ZERO_WEIGHTS
        assert float(got[1][0, z]) == 0.0  # the zero-weight utterance counts no token


@pytest.mark.parametrize("kind", KIND_IDS)
@pytest.mark.parametrize("case", NF.SPECIAL_CASES, ids=C.shape_id)
def test_special_values(gpu, case, kind):
    """Trailing -10 pad frames, +-0, the smallest subnormal, the largest finite
    fp16 value; for bf16 a subnormal and 2^40 -- at MOSI's widths and on rows of
    one unit."""
    dims = case[:5]
    z = C.inputs(case)
    text = {"ids": G16._dev(z["ids"], gpu, torch.int32), "table": G16._dev(z["E"], gpu),
            "wtab": G16._dev(z["wt32"], gpu)}
    proj = P.MMB2Projection(G16._networks(case, gpu), *case[:4], gpu)
    a16, v16 = (_guarded(G16._dev(t, gpu)) for t in F.special_frames(case, kind))
    got = _pair(dims, a16, v16, proj, text, gpu, (dims, kind, "special"))
    assert got[4] == 0
    # the planted values reached the sums: rows 0 and 1 (the large value squared in
    # Sxx) and the padded rows 2.. differ from the plain rounded frames' rows
    b16, w16 = (_guarded(G16._dev(t, gpu)) for t in F.frames(case, kind))
    plain = _pair(dims, b16, w16, proj, text, gpu, (dims, kind, "plain"))
    assert torch.equal(got[0], plain[0])  # x is the text's
    assert bool((got[2] != plain[2]).any(dim=1).all())


# ------------------------------------------------------------------ B: alignment
def _alignment_case(kind, gpu):
    A, Vd, T, N, V = 76, 48, 20, 31, 3016
    inp, proj, _ = _synth_case(A, Vd, T, N, V, kind, gpu)
    return (NF.D, A, Vd, T, N), inp, proj


@pytest.mark.parametrize("kind", KIND_IDS)
def test_frames_8_bytes_off_are_whole_units(gpu, kind):
    """A 16-bit column unit is 8 bytes: frames 8 bytes past a 16-byte boundary
    are accepted and give the aligned launch's bits."""
    dims, inp, proj = _alignment_case(kind, gpu)
    want = _launch(P.mm2_stream_project_narrow_ft, dims, inp["audio"], inp["visual"], proj, inp, gpu)
    a8, v8 = _guarded(inp["audio"], extra=4), _guarded(inp["visual"], extra=4)
    assert a8.data_ptr() % 16 == 8 and v8.data_ptr() % 16 == 8
    got = _launch(P.mm2_stream_project_narrow_ft, dims, a8, v8, proj, inp, gpu)
    _assert_bit_for_bit(got, want, (dims, kind, "8 bytes off"))
    _pair(dims, a8, v8, proj, inp, gpu, (dims, kind, "8 bytes off, twin"))


@pytest.mark.parametrize("kind", KIND_IDS)
def test_frames_2_and_4_bytes_off_are_rejected(gpu, kind):
    dims, inp, proj = _alignment_case(kind, gpu)
    D, A, Vd, T, N = dims
    a16, v16 = inp["audio"], inp["visual"]
    out, flag, colmax, ws = _bufs(N, D, gpu, fill=-7.0)
    for elements in (1, 2):
        for au, vi in ((G16._off(a16, elements), v16), (a16, G16._off(v16, elements))):
            with pytest.raises(L.MMBError, match=r"code -1 \(invalid argument\)"):
                P.mm2_stream_project_narrow_ft(N, T, D, A, Vd, au, vi, proj, inp["ids"], inp["table"], inp["wtab"],
                                               flag=flag, out=out, colmax=colmax, colmax_ws=ws)
    assert G16._untouched(out) and int(flag.item()) == 0 and int(colmax.abs().max().item()) == 0
    # the mirror's own check comes before any launch, and the f32 mirror still refuses 16-bit frames
    with pytest.raises(L.MMBError, match="one dtype"):
        P.mm2_stream_project_narrow_ft(N, T, D, A, Vd, a16, v16.float(), proj, inp["ids"], inp["table"],
                                       inp["wtab"], out=out)
    with pytest.raises(L.MMBError, match="mm2_stream_project_narrow reads float32 frames only"):
        P.mm2_stream_project_narrow(N, T, D, A, Vd, a16, v16, proj, inp["ids"], inp["table"], inp["wtab"], out=out)
    assert G16._untouched(out)


def test_f32_frames_through_the_ft_mirror_are_the_f32_entry_point(gpu):
    dims, inp, proj = _alignment_case("bf16", gpu)
    a32, v32 = inp["audio"].float(), inp["visual"].float()
    got = _launch(P.mm2_stream_project_narrow_ft, dims, a32, v32, proj, inp, gpu)
    want = _launch(P.mm2_stream_project_narrow, dims, a32, v32, proj, inp, gpu)
    _assert_bit_for_bit(got, want, (dims, "f32"))


# ------------------------------------------------------------------ C: the step
def _step_inputs(kind, gpu):
    """(the step's inputs with 16-bit frames, the same with their f32 upcast)."""
    D, A, Vd, T, N, V = NF.STEP
    inp16 = synth.device_workload(N, T, V, D=D, A=A, Vd=Vd, seed=110, device=gpu, frame_dtype=NF.KINDS[kind])
    r = torch.as_tensor(np.random.default_rng(N + T).integers(0, N, 5), device=gpu)
    inp16["ids"][r, 0] = -3  # wraps to V - 3, like numpy fancy indexing
    return inp16, dict(inp16, audio=inp16["audio"].float(), visual=inp16["visual"].float())


def _generator(gpu):
    D, A, Vd = NF.STEP[:3]
    torch.manual_seed(0)
    return models.AudioVisualGeneratorMultimodal(D, A, Vd, norm=None).to(gpu)


@functools.lru_cache(maxsize=None)
def _sif_reference(E_bytes, wt_bytes, ids_bytes):
    """The oracle's SIF rows of the step's text (the same for both kinds)."""
    D, A, Vd, T, N, V = NF.STEP
    E = np.frombuffer(E_bytes, np.float32).reshape(V, D)
    wt = np.frombuffer(wt_bytes, np.float64)
    ids = np.frombuffer(ids_bytes, np.int64).reshape(N, T)
    return O.get_sentence_embeddings(E, wt, ids)


@pytest.mark.parametrize("kind", KIND_IDS)
def test_narrow_fused_step_on_16_bit_frames_opted_in(gpu, kind):
    D, A, Vd, T, N, V = NF.STEP
    inp16, inp32 = _step_inputs(kind, gpu)
    gen = _generator(gpu)
    a = P.FusedStep(inp16, gen.networks(), narrow_frames16=True)
    b = P.FusedStep(inp32, gen.networks())  # the f32 default: the narrow fused kernel
    assert a.frames == kind and b.frames == "f32"
    assert a.plan.front == "narrow_fused" and a.plan.project == "front" and a.s is None and a.narrow_fused
    assert b.plan.front == "narrow_fused" and a.plan._replace(frames="f32") == b.plan
    trace = {}
    s1, m1 = [t.clone() for t in a.run(check=True, trace=trace)]
    assert "mm2_stream_project_narrow" in trace and "mm2_stream" not in trace
    s2, m2 = G16._run(b)
    torch.cuda.synchronize()
    assert torch.equal(a.x, b.x) and torch.equal(a.aux, b.aux) and torch.equal(a.pc, b.pc)
    assert torch.equal(s1, s2) and torch.equal(m1, m2)
    # the oracle on the upcast frames, at the bars of test_narrow_fused_matches_two_kernel_step
    pc_sk = O.compute_pc(a.x.double().cpu().numpy())
    ep = np.abs(a.pc.cpu().numpy() - pc_sk).max()
    norms = torch.linalg.norm(m1.double(), dim=1)
    en = (norms - 1).abs().max().item()
    E = inp16["table"].cpu().numpy()
    wt = inp16["wtab"].cpu().numpy().astype(np.float64)
    ids = inp16["ids"].cpu().numpy().astype(np.int64)
    es = M.row_rel_err(s1.cpu().numpy(), _sif_reference(E.tobytes(), wt.tobytes(), ids.tobytes()))
    rows = np.sort(np.random.default_rng(N + T).choice(N, 256, replace=False))
    audio, visual = inp32["audio"].cpu().numpy()[rows], inp32["visual"].cpu().numpy()[rows]
    idr = ids[rows]
    sw = np.where(idr >= 0, wt.astype(np.float32)[idr], 0).astype(np.float32)
    ref = M.estimate_embedding_overall_gpu2(M.concat_inputs(E[idr], audio, visual),
                                            M.params_from_module(copy.deepcopy(gen).cpu()), sw, E[idr])
    em = M.row_rel_err(m1.cpu().numpy()[rows], ref)
    print(f"{kind}: PC {ep:.2e} (bar 1e-10), norms {en:.2e} (1e-5), SIF rows {es:.2e} (1e-5), "
          f"MMB2 rows {em:.2e} (1e-5)")
    assert ep < 1e-10 and en < 1e-5 and es < TOL and em < TOL


def test_step_graph_replays_the_bf16_narrow_fused_step(gpu):
    inp16, _ = _step_inputs("bf16", gpu)
    step = P.FusedStep(inp16, _generator(gpu).networks(), narrow_frames16=True)
    assert step.plan.front == "narrow_fused"
    G16._assert_graph_replays(step)


@pytest.mark.parametrize("kind", KIND_IDS)
def test_step_without_the_keyword_keeps_the_two_kernel_plan(gpu, kind):
    inp16, _ = _step_inputs(kind, gpu)
    nets = _generator(gpu).networks()
    for kw in ({}, dict(narrow_fused=True), dict(fused_frames16=True)):
        off = P.FusedStep(inp16, nets, **kw)
        assert off.plan.front == "stream" and off.s is not None and off.plan.frames == kind
    assert P.FusedStep(inp16, nets, narrow_frames16=True, narrow_fused=False).plan == P.FusedStep(inp16, nets).plan
