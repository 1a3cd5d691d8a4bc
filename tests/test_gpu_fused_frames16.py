"""GPU: the fused stream + projection kernel on audio / visual frames kept in
fp16 / bf16 storage (mmb_mm2_stream_project_ft, pipeline.mm2_stream_project_ft,
FusedStep(fused_frames16=True)).

On 16-bit rows the pipelined streamers load a frame with one 8-byte and one
2-byte buffer load where the f32 rows take a 16-byte and a 4-byte one, keep the
units packed and widen them where the frame is summed; the group-at-a-time
fallback reads the same 8-byte units.  Both widenings are exact and the sums
are the f32 instantiation's statements in their order, so the definition under
test is an equality: a launch on 16-bit frames writes, bit for bit, what the
same launch writes on those frames upcast to f32 -- x, the three aux planes,
the MMB2 rows, the column bounds and the flag word (A), and x, aux, PC, SIF and
MMB2 rows of the step (C).  The f32 twin is the fused kernel the suite already
holds to the two-kernel step and the oracle (tests/test_gpu_fused_tail.py,
tests/test_gpu_mmb2.py).  The step is also held to the oracle on the upcast
inputs with the suite's bars (MMB2 rows 1e-5, PC 1e-10, SIF rows 2^-23;
tests/test_frames16_cases.py pins the family's conditions on those inputs);
the int8-Gram pair, whose PC is ~1e-9 of the exact one by design
(tests/test_gpu_mmb2.py), is held to its f32 twin only.
Product library only.
"""
import pytest
import torch

import frames16_cases as F
import frames16_gpu as G16
import fused_frames16_cases as FF
import mmb2_cases as C
import mmb_lib as L
import pipeline as P
from frames16_gpu import _assert_bit_for_bit, _bufs, _i32, _launch

pytestmark = pytest.mark.gpu

KIND_IDS = list(FF.KINDS)


def _pair(dims, a16, v16, proj, text, gpu, what):
    """The launch on the 16-bit frames and its f32 twin on their upcast."""
    got = G16._pair((P.mm2_stream_project_ft, P.mm2_stream_project), dims, a16, v16, proj, text, gpu, what)
    assert bool(torch.isfinite(got[2]).all()) and bool((got[2].abs().amax(dim=1) > 0).all())
    return got


def _synth_case(D, A, Vd, T, N, kind, gpu, bad=False):
    """G16._synth_case over KERNEL_V words, with out-of-range ids if `bad`."""
    inp, proj = G16._synth_case(D, A, Vd, T, N, FF.KERNEL_V, kind, gpu)
    if bad:  # a negative id wraps (weight 0); an id >= V is flagged and contributes a zero row
        inp["ids"][3, 5] = -7
        inp["ids"][N // 2, T - 1] = FF.KERNEL_V + 11
    return inp, proj


# ------------------------------------------------------------------ A: the kernel, bit for bit
@pytest.mark.parametrize("kind", KIND_IDS)
@pytest.mark.parametrize("D,A,Vd,T,N,bad", FF.KERNEL_CASES, ids=[C.shape_id(c[:5]) + ("-bad" if c[5] else "")
                                                              for c in FF.KERNEL_CASES])
def test_fused_kernel_bit_for_bit(gpu, D, A, Vd, T, N, bad, kind):
    assert P.stream_project_supported(T, D, A, Vd)
    inp, proj = _synth_case(D, A, Vd, T, N, kind, gpu, bad)
    got = _pair((D, A, Vd, T, N), inp["audio"], inp["visual"], proj, inp, gpu, (D, A, Vd, T, N, kind))
    print(f"flag {got[4]}")
    assert (got[4] != 0) == bad
    # the bounds are those of the x written
    assert torch.equal(got[3], _i32(got[0].abs().amax(dim=0)))


@pytest.mark.parametrize("kind", KIND_IDS)
def test_dynamic_order_and_rows_past_2_31_bytes(gpu, kind):
    """200,018 rows: the dynamic batch order (>= 16 rounds of batches) with a
    2-row last unit, and 16-bit visual rows whose byte offsets pass 2^31."""
    D, A, Vd, T, N = FF.LARGE
    assert -(-N // 48) >= 16 * L.cu_count(gpu), "the launch would keep the static order on this chip"
    inp, proj = _synth_case(D, A, Vd, T, N, kind, gpu)
    assert inp["visual"].numel() * inp["visual"].element_size() > 2 ** 31
    _pair(FF.LARGE, inp["audio"], inp["visual"], proj, inp, gpu, (FF.LARGE, kind))


def _family_case(shape, n, gpu):
    case = C.case_of(shape, n)
    D, A, Vd, T, N, V = case
    z = C.inputs(case)
    text = {"ids": G16._dev(z["ids"], gpu, torch.int32), "table": G16._dev(z["E"], gpu),
            "wtab": G16._dev(z["wt32"], gpu)}
    proj = P.MMB2Projection(G16._networks(case, gpu), D, A, Vd, T, gpu)
    return case, text, proj


@pytest.mark.parametrize("kind", KIND_IDS)
@pytest.mark.parametrize("shape", FF.SPECIAL_SHAPES, ids=C.shape_id)
def test_special_values(gpu, shape, kind):
    """Trailing -10 pad frames, +-0, the smallest subnormal, the largest finite
    fp16 value; for bf16 a subnormal and 2^40 -- on the group-at-a-time
    fallback (T = 7) and the pipelined streamer (T = 21)."""
    case, text, proj = _family_case(shape, FF.SPECIAL_N, gpu)
    dims = case[:5]
    a16, v16 = (G16._dev(t, gpu) for t in F.special_frames(case, kind))
    got = _pair(dims, a16, v16, proj, text, gpu, (dims, kind, "special"))
    assert got[4] == 0
    # the planted values reached the sums: rows 0 and 1 (the large value squared in
    # Sxx) and the padded rows 2.. differ from the plain rounded frames' rows
    b16, w16 = (G16._dev(t, gpu) for t in F.frames(case, kind))
    plain = _pair(dims, b16, w16, proj, text, gpu, (dims, kind, "plain"))
    assert torch.equal(got[0], plain[0])  # x is the text's
    assert bool((got[2] != plain[2]).any(dim=1).all())


# ------------------------------------------------------------------ B: alignment
@pytest.mark.parametrize("kind", KIND_IDS)
def test_frames_8_bytes_off_are_whole_units(gpu, kind):
    """A 16-bit column unit is 8 bytes: frames 8 bytes past a 16-byte boundary
    are accepted and give the aligned launch's bits."""
    case, text, proj = _family_case(FF.SPECIAL_SHAPES[1], FF.SPECIAL_N, gpu)
    dims = case[:5]
    a16, v16 = (G16._dev(t, gpu) for t in F.frames(case, kind))
    want = _launch(P.mm2_stream_project_ft, dims, a16, v16, proj, text, gpu)
    got = _launch(P.mm2_stream_project_ft, dims, G16._off(a16, 4), G16._off(v16, 4), proj, text, gpu)
    _assert_bit_for_bit(got, want, (dims, kind, "8 bytes off"))
    _pair(dims, G16._off(a16, 4), G16._off(v16, 4), proj, text, gpu, (dims, kind, "8 bytes off, twin"))


@pytest.mark.parametrize("kind", KIND_IDS)
def test_frames_2_and_4_bytes_off_are_rejected(gpu, kind):
    case, text, proj = _family_case(FF.SPECIAL_SHAPES[1], FF.SPECIAL_N, gpu)
    D, A, Vd, T, N, V = case
    a16, v16 = (G16._dev(t, gpu) for t in F.frames(case, kind))
    out, flag, colmax, ws = _bufs(N, D, gpu, fill=-7.0)
    for elements in (1, 2):
        for au, vi in ((G16._off(a16, elements), v16), (a16, G16._off(v16, elements))):
            with pytest.raises(L.MMBError, match=r"code -1 \(invalid argument\)"):
                P.mm2_stream_project_ft(N, T, D, A, Vd, au, vi, proj, text["ids"], text["table"], text["wtab"],
                                        flag=flag, out=out, colmax=colmax, colmax_ws=ws)
    assert G16._untouched(out) and int(flag.item()) == 0 and int(colmax.abs().max().item()) == 0
    # and the mirror's own checks come before any launch
    with pytest.raises(L.MMBError, match="one dtype"):
        P.mm2_stream_project_ft(N, T, D, A, Vd, a16, v16.float(), proj, text["ids"], text["table"], text["wtab"],
                                out=out)
    with pytest.raises(L.MMBError, match="gathered text"):
        P.mm2_stream_project_ft(N, T, D, A, Vd, a16, v16, proj, None, text["table"], text["wtab"], out=out)
    assert G16._untouched(out)


# ------------------------------------------------------------------ C: the step
def _step_pair(case, kind, gpu, **kw):
    inp16, inp32 = G16._step_inputs(case, kind, gpu)
    nets = G16._networks(case, gpu)
    a = P.FusedStep(inp16, nets, fused_frames16=True, **kw)
    b = P.FusedStep(inp32, nets, **kw)  # the f32 fused default
    assert a.frames == kind and b.frames == "f32"
    assert a.plan.front == "fused" and a.plan.project == "front" and a.s is None
    assert b.plan.front == "fused" and a.plan._replace(frames="f32") == b.plan
    trace = {}
    s1, m1 = [t.clone() for t in a.run(check=True, trace=trace)]
    assert "mm2_stream_project" in trace and "mm2_stream" not in trace
    s2, m2 = G16._run(b)
    torch.cuda.synchronize()
    assert torch.equal(a.x, b.x) and torch.equal(a.aux, b.aux) and torch.equal(a.pc, b.pc)
    assert torch.equal(s1, s2) and torch.equal(m1, m2)
    return a, b, s1, m1


@pytest.mark.parametrize("kind", KIND_IDS)
def test_fused_step_on_16_bit_frames_opted_in(gpu, kind):
    case = F.step_case(FF.STEP)
    a, b, sif, mm2 = _step_pair(case, kind, gpu)
    G16._check_oracle(case, kind, a, sif, mm2)


@pytest.mark.parametrize("kind", KIND_IDS)
def test_fused_step_feeds_the_int8_gram(gpu, kind):
    """The column bounds of the 16-bit fused front feed mmb_gram_i8."""
    case = F.step_case(FF.STEP)
    a, b, _, _ = _step_pair(case, kind, gpu, gram_kind="i8")
    assert a.plan.gram == "i8" and torch.equal(a.colmax, b.colmax)
    assert torch.equal(a.colmax, _i32(a.x.abs().amax(dim=0)))


@pytest.mark.parametrize("kind", KIND_IDS)
@pytest.mark.parametrize("dims", FF.STEP_UNCHANGED, ids=C.shape_id)
def test_keyword_leaves_the_other_plans_alone(gpu, dims, kind):
    case = F.step_case(dims)
    inp16, _ = G16._step_inputs(case, kind, gpu)
    nets = G16._networks(case, gpu)
    on, off = P.FusedStep(inp16, nets, fused_frames16=True), P.FusedStep(inp16, nets)
    assert on.plan == off.plan and on.plan.front == "stream" and on.s is not None


def test_step_graph_replays_the_bf16_fused_step(gpu):
    case = F.step_case(FF.STEP)
    inp16, _ = G16._step_inputs(case, "bf16", gpu)
    step = P.FusedStep(inp16, G16._networks(case, gpu), fused_frames16=True)
    assert step.plan.front == "fused"
    G16._assert_graph_replays(step)
