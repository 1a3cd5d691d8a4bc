"""GPU: the fused stream + projection kernel on a word table kept in fp16 /
bf16 storage (mmb_mm2_stream_project_tt, pipeline.mm2_stream_project_tt,
FusedStep(fused_table16=True)).

On a 16-bit table the pipelined streamers load a gathered row with one 8-byte
and one 2-byte buffer load where an f32 row takes a 16-byte and a 4-byte one
(row offset r D 2, descriptor range V D 2), keep the units packed and widen
them where the row is summed; the group-at-a-time fallback reads the same
8-byte units.  Both widenings are exact and the sums are the f32-table
instantiation's statements in their order, so the definition under test is an
equality: a launch on a 16-bit table writes, bit for bit, what the same launch
writes on that table upcast to f32 -- x, the three aux planes, the MMB2 rows,
the column bounds and the flag word (1, 2, 3), and x, aux, PC, SIF and MMB2
rows of the step (4) -- for each frame type.  The twin is the fused kernel the
suite already holds to the two-kernel step and the oracle
(tests/test_gpu_fused_tail.py, tests/test_gpu_fused_frames16.py).  The step is
also held to the oracle on the upcast inputs with the suite's bars (MMB2 rows
1e-5, PC 1e-10, SIF rows 2^-23; tests/test_table16_cases.py pins the family's
conditions on those inputs); the int8-Gram pair, whose PC is ~1e-9 of the exact
one by design (tests/test_gpu_mmb2.py), is held to its twin only.  The
descriptor guard (5) runs the last table size the pipelined streamer takes and
the first it refuses on one 2 GiB bf16 buffer.
Product library only.
"""
import numpy as np
import pytest
import torch

import frames16_cases as F
import frames16_gpu as G16
import fused_table16_cases as FT16
import large_cases as LC
import large_gpu as LG  # the large cases' device fills and host copies
import mmb2_cases as C
import mmb_lib as L
import models
import pipeline as P
import synth
import table16_cases as T
from common_gpu import TOL, _flag, _frac  # the bars of the large cases' row check
from frames16_gpu import TWIN, _assert_bit_for_bit, _bufs, _dev, _frames_of, _i32, _launch, _off
from oracle import mmb2_oracle as M

pytestmark = pytest.mark.gpu

KIND_IDS = list(FT16.KINDS)
DTYPES = {"f32": torch.float32, **FT16.KINDS}


def _twin_front(frames):
    """The f32-table mirror that takes these frames."""
    return P.mm2_stream_project if frames.dtype == torch.float32 else P.mm2_stream_project_ft


def _pair(dims, tab16, au, vi, proj, text, gpu, what):
    """The launch on the 16-bit table and its twin on the table's upcast (the
    same frames): equal bits, MMB2 rows finite and non-zero, the bounds those
    of the x written."""
    got = _launch(P.mm2_stream_project_tt, dims, au, vi, proj, dict(text, table=tab16), gpu)
    twin = _launch(_twin_front(au), dims, au, vi, proj, dict(text, table=tab16.float()), gpu)
    _assert_bit_for_bit(got, twin, what)
    assert bool(torch.isfinite(got[2]).all()) and bool((got[2].abs().amax(dim=1) > 0).all()), what
    assert torch.equal(got[3], _i32(got[0].abs().amax(dim=0))), what
    return got


def _synth_case(D, A, Vd, T_, N, tkind, fkind, gpu, bad=False):
    """A device workload over KERNEL_V words with the table rounded to `tkind`
    and the frames to `fkind` (torch's round to nearest even: the caller's
    rounding), and the projection of a generator."""
    inp = synth.device_workload(N, T_, FT16.KERNEL_V, D=D, A=A, Vd=Vd, seed=83, device=gpu,
                                frame_dtype=DTYPES[fkind])
    assert inp["audio"].dtype == inp["visual"].dtype == DTYPES[fkind]
    if bad:  # a negative id wraps (weight 0); an id >= V is flagged and contributes a zero row
        inp["ids"][3, 5] = -7
        inp["ids"][N // 2, T_ - 1] = FT16.KERNEL_V + 11
    torch.manual_seed(0)
    gen = models.AudioVisualGeneratorMultimodal(D, A, Vd, norm=None).to(gpu)
    tab16 = inp["table"].to(DTYPES[tkind])
    return inp, tab16, P.MMB2Projection(gen.networks(), D, A, Vd, T_, gpu)


# ------------------------------------------------------------------ 1: the kernel, bit for bit
@pytest.mark.parametrize("frames", FT16.FRAME_CHOICES)
@pytest.mark.parametrize("kind", KIND_IDS)
@pytest.mark.parametrize("D,A,Vd,T_,N,bad", FT16.KERNEL_CASES,
                         ids=[C.shape_id(c[:5]) + ("-bad" if c[5] else "") for c in FT16.KERNEL_CASES])
def test_fused_kernel_bit_for_bit(gpu, D, A, Vd, T_, N, bad, kind, frames):
    assert P.stream_project_supported(T_, D, A, Vd)
    fkind = "f32" if frames == "f32" else kind
    inp, tab16, proj = _synth_case(D, A, Vd, T_, N, kind, fkind, gpu, bad)
    got = _pair((D, A, Vd, T_, N), tab16, inp["audio"], inp["visual"], proj, inp, gpu, (D, A, Vd, T_, N, kind, fkind))
    print(f"flag {got[4]}")
    assert (got[4] != 0) == bad


@pytest.mark.parametrize("fkind", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("kind", KIND_IDS)
def test_all_six_new_pairs(gpu, kind, fkind):
    D, A, Vd, T_, N, bad = FT16.ALL_PAIRS_CASE
    inp, tab16, proj = _synth_case(D, A, Vd, T_, N, kind, fkind, gpu, bad)
    got = _pair((D, A, Vd, T_, N), tab16, inp["audio"], inp["visual"], proj, inp, gpu, (kind, fkind))
    assert got[4] == L.MMB_FLAG_ID_RANGE


# ------------------------------------------------------------------ 2: special values in the table
def _family_case(shape, n, gpu):
    case = C.case_of(shape, n)
    D, A, Vd, T_, N, V = case
    z = C.inputs(case)
    text = {"ids": _dev(z["ids"], gpu, torch.int32), "wtab": _dev(z["wt32"], gpu)}
    proj = P.MMB2Projection(G16._networks(case, gpu), D, A, Vd, T_, gpu)
    return case, text, proj, _dev(z["audio"], gpu), _dev(z["visual"], gpu)


@pytest.mark.parametrize("kind", KIND_IDS)
@pytest.mark.parametrize("shape", FT16.SPECIAL_SHAPES, ids=C.shape_id)
def test_special_values(gpu, shape, kind):
    """+-0, the smallest subnormal and the largest planted value (65504 for
    fp16, 2^40 for bf16) in table row 0 and in the last columns of the row the
    ids use most (at D = 260 the b16 tail's) -- on the group-at-a-time
    fallback (T = 7) and the pipelined streamer (T = 21)."""
    case, text, proj, au, vi = _family_case(shape, FT16.SPECIAL_N, gpu)
    D, A, Vd, T_, N, V = case
    dims = case[:5]
    got = _pair(dims, _dev(T.special_table(case, kind), gpu), au, vi, proj, text, gpu, (dims, kind, "special"))
    assert got[4] == 0
    plain = _pair(dims, _dev(T.table(case, kind), gpu), au, vi, proj, text, gpu, (dims, kind, "plain"))
    # the planted values reached the sums: x differs in the rows that gather the hot
    # row with a weight (its planted last columns enter the weighted sum) ...
    z = C.inputs(case)
    ids, hot = z["ids"], T.hot_row(case)
    weighted = (ids == hot) & (z["wt32"][np.clip(ids, 0, V - 1)] != 0)
    rows_x = torch.as_tensor(weighted.any(axis=1), device=gpu)
    assert bool(rows_x.any())
    assert bool((got[0] != plain[0]).any(dim=1)[rows_x].all())
    # ... and the MMB2 rows in every row that names row 0 or the hot row (Sx, Sxx)
    wrapped = np.where(ids < 0, ids + V, ids)
    rows_m = torch.as_tensor(((wrapped == hot) | (wrapped == 0)).any(axis=1), device=gpu)
    assert bool((got[2] != plain[2]).any(dim=1)[rows_m].all())


# ------------------------------------------------------------------ 3: alignment
@pytest.mark.parametrize("kind", KIND_IDS)
def test_table_8_bytes_off_is_whole_units(gpu, kind):
    """A 16-bit text column unit is 8 bytes: a table 8 bytes past a 16-byte
    boundary is accepted and gives the aligned launch's bits."""
    case, text, proj, au, vi = _family_case(FT16.SPECIAL_SHAPES[1], FT16.SPECIAL_N, gpu)
    dims = case[:5]
    tab16 = _dev(T.table(case, kind), gpu)
    want = _launch(P.mm2_stream_project_tt, dims, au, vi, proj, dict(text, table=tab16), gpu)
    got = _launch(P.mm2_stream_project_tt, dims, au, vi, proj, dict(text, table=_off(tab16, 4)), gpu)
    _assert_bit_for_bit(got, want, (dims, kind, "8 bytes off"))
    _pair(dims, _off(tab16, 4), au, vi, proj, text, gpu, (dims, kind, "8 bytes off, twin"))


@pytest.mark.parametrize("kind", KIND_IDS)
def test_table_2_and_4_bytes_off_is_rejected(gpu, kind):
    case, text, proj, au, vi = _family_case(FT16.SPECIAL_SHAPES[1], FT16.SPECIAL_N, gpu)
    D, A, Vd, T_, N, V = case
    tab16 = _dev(T.table(case, kind), gpu)
    out, flag, colmax, ws = _bufs(N, D, gpu, fill=-7.0)
    for elements in (1, 2):
        with pytest.raises(L.MMBError, match=r"code -1 \(invalid argument\)"):
            P.mm2_stream_project_tt(N, T_, D, A, Vd, au, vi, proj, text["ids"], _off(tab16, elements), text["wtab"],
                                    flag=flag, out=out, colmax=colmax, colmax_ws=ws)
    assert G16._untouched(out) and int(flag.item()) == 0 and int(colmax.abs().max().item()) == 0
    # and the mirror's own checks come before any launch
    with pytest.raises(L.MMBError, match="float32, float16 or bfloat16, not torch.float64"):
        P.mm2_stream_project_tt(N, T_, D, A, Vd, au, vi, proj, text["ids"], tab16.double(), text["wtab"], out=out)
    with pytest.raises(L.MMBError, match="gathered text"):
        P.mm2_stream_project_tt(N, T_, D, A, Vd, au, vi, proj, None, tab16, text["wtab"], out=out)
    with pytest.raises(L.MMBError, match="one dtype"):
        P.mm2_stream_project_tt(N, T_, D, A, Vd, au, vi.half(), proj, text["ids"], tab16, text["wtab"], out=out)
    assert G16._untouched(out)


# ------------------------------------------------------------------ 4: the step
def _step_inputs(case, kind, fkind, gpu):
    """(the inputs with the 16-bit table, the same with its f32 upcast); the
    frames are of `fkind`, the same tensors in both."""
    z = C.inputs(case)
    E16 = _dev(T.table(case, kind), gpu)
    au, vi = _frames_of(case, fkind, "f32" if fkind == "f32" else "same", gpu)
    base = {"wtab": _dev(z["wt32"], gpu), "ids": _dev(z["ids"], gpu, torch.int32), "audio": au, "visual": vi}
    return dict(base, table=E16), dict(base, table=E16.float())


def _step_pair(case, kind, fkind, gpu, **kw):
    inp16, inp32 = _step_inputs(case, kind, fkind, gpu)
    nets = G16._networks(case, gpu)
    a = P.FusedStep(inp16, nets, fused_table16=True, **kw)
    b = P.FusedStep(inp32, nets, **kw)  # the f32-table fused step of these frames
    assert a.table_kind == kind and b.table_kind == "f32" and a.frames == b.frames == fkind
    assert a.plan.front == "fused" and a.plan.project == "front" and a.s is None
    assert b.plan.front == "fused" and a.plan == b.plan
    trace = {}
    s1, m1 = [t.clone() for t in a.run(check=True, trace=trace)]
    assert "mm2_stream_project" in trace and "mm2_stream" not in trace
    s2, m2 = G16._run(b)
    torch.cuda.synchronize()
    assert torch.equal(a.x, b.x) and torch.equal(a.aux, b.aux) and torch.equal(a.pc, b.pc)
    assert torch.equal(s1, s2) and torch.equal(m1, m2)
    return a, b, s1, m1


def _check_oracle(case, kind, fkind, step, sif, mm2):
    # (tests/test_gpu_table16.py's check names the frames "f32" or "same": the oracle rows are per frame kind)
    x = step.x.double().cpu().numpy()
    from oracle import sif_oracle as O

    eo = M.row_rel_err(mm2.cpu().numpy(), T.oracle_rows(case, kind, None if fkind == "f32" else fkind)) / G16.TOL
    ep = np.abs(step.pc.cpu().numpy() - O.compute_pc(x, 1)).max() / 1e-10
    ref = O.remove_pc(x, 1)
    es = (np.abs(sif.cpu().numpy() - ref) / np.abs(ref).max(axis=1, keepdims=True)).max() / G16.F32_ROW
    print(f"{C.shape_id(case)} {kind} table, {fkind} frames: MMB2 {eo:.3f} of 1e-5, PC {ep:.3f} of 1e-10, "
          f"SIF rows {es:.3f} of 2^-23")
    assert eo < 1.0 and ep < 1.0 and es <= 1.0


@pytest.mark.parametrize("kind", KIND_IDS)
def test_fused_step_on_a_16_bit_table_opted_in(gpu, kind):
    case = F.step_case(FT16.STEP)
    a, b, sif, mm2 = _step_pair(case, kind, "f32", gpu)
    _check_oracle(case, kind, "f32", a, sif, mm2)


@pytest.mark.parametrize("kind", KIND_IDS)
def test_fused_step_feeds_the_int8_gram(gpu, kind):
    """The column bounds of the 16-bit-table fused front feed mmb_gram_i8."""
    case = F.step_case(FT16.STEP)
    a, b, _, _ = _step_pair(case, kind, "f32", gpu, gram_kind="i8")
    assert a.plan.gram == "i8" and torch.equal(a.colmax, b.colmax)
    assert torch.equal(a.colmax, _i32(a.x.abs().amax(dim=0)))


@pytest.mark.parametrize("kind", KIND_IDS)
def test_fused_step_on_bf16_frames_with_both_opt_ins(gpu, kind):
    case = F.step_case(FT16.STEP)
    a, b, sif, mm2 = _step_pair(case, kind, "bf16", gpu, fused_frames16=True)
    _check_oracle(case, kind, "bf16", a, sif, mm2)
    # the table's opt-in alone leaves 16-bit frames on the two-kernel step
    inp16, _ = _step_inputs(case, kind, "bf16", gpu)
    alone = P.FusedStep(inp16, G16._networks(case, gpu), fused_table16=True)
    assert alone.plan.front == "stream" and alone.s is not None


@pytest.mark.parametrize("kind", KIND_IDS)
def test_without_the_opt_in_the_step_is_the_two_kernel_one(gpu, kind):
    case = F.step_case(FT16.STEP)
    inp16, inp32 = _step_inputs(case, kind, "f32", gpu)
    nets = G16._networks(case, gpu)
    off = P.FusedStep(inp16, nets)
    assert off.plan == P.FusedStep(inp32, nets, **TWIN).plan
    assert off.plan.front == "stream" and off.plan.split is False and off.s is not None
    assert P.FusedStep(inp16, nets, fused_table16=False).plan == off.plan


@pytest.mark.parametrize("kind", KIND_IDS)
@pytest.mark.parametrize("dims", FT16.STEP_UNCHANGED, ids=C.shape_id)
def test_keyword_leaves_the_other_plans_alone(gpu, dims, kind):
    case = F.step_case(dims)
    inp16, _ = _step_inputs(case, kind, "f32", gpu)
    nets = G16._networks(case, gpu)
    on, off = P.FusedStep(inp16, nets, fused_table16=True), P.FusedStep(inp16, nets)
    assert on.plan == off.plan and on.plan.front == "stream" and on.s is not None


def test_step_graph_replays_the_bf16_table_fused_step(gpu):
    case = F.step_case(FT16.STEP)
    inp16, _ = _step_inputs(case, "bf16", "f32", gpu)
    step = P.FusedStep(inp16, G16._networks(case, gpu), fused_table16=True)
    assert step.plan.front == "fused" and step.table_kind == "bf16"
    G16._assert_graph_replays(step)


# ------------------------------------------------------------------ 5: the descriptor guard
def _check_rows(c, inp, out, gpu, flag, what):
    """x, count and weight sum of every row against mmb2_cases.stream_reference
    (sum_bar), the MMB2 rows against the oracle on the rows' inputs (1e-5
    row-relative): the check tests/test_gpu_large.py holds the fused kernels to."""
    z = c.dims
    x, aux, mmb2 = out
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    ids = inp["ids"].long()
    text, sw = LG._host_upcast(inp["table"][ids]), LG._host_upcast(inp["wtab"][ids])
    audio, visual = LG._host_upcast(inp["audio"]), LG._host_upcast(inp["visual"])
    ref = C.stream_reference(text, text, sw, audio, visual)
    a = aux.cpu().numpy()
    assert np.array_equal(a[0], ref["cnt"])
    fx = _frac(np.abs(x.cpu().numpy() - ref["x"]), C.sum_bar(z["t"], ref["x_abs"]))
    fw = _frac(np.abs(a[1] - ref["sw"]), C.sum_bar(z["t"], ref["sw_abs"]))
    oracle = M.estimate_embedding_overall_gpu2(M.concat_inputs(text, audio, visual),
                                               C.params(z["d"], z["a"], z["vd"]), sw, text)
    got = mmb2.cpu().numpy()
    assert np.isfinite(got).all()
    fo = M.row_rel_err(got, oracle) / TOL
    print(f"{c.name}, {what}: x {fx:.3f} and weight sum {fw:.3f} of sum_bar, MMB2 rows {fo:.3f} of 1e-5")
    assert fx <= 1.0 and fw <= 1.0 and fo < 1.0


def test_descriptor_guard_on_a_2_gib_bf16_table(gpu):
    """fused_pipe_ok with 2-byte elements: a bf16 [2^22 - 1, 256] table (2^31 -
    512 bytes) takes the pipelined streamer, a [2^22, 256] one (2^31 bytes) the
    group-at-a-time fallback -- twice the rows of the f32 guard
    (tests/test_gpu_large.py::test_fused_table_guard).  The first table is the
    second one's rows but the last and the ids reach its top rows, so the two
    launches gather the same rows: identical bits, and the f64 reference's rows.
    Then the larger table's own last row."""
    last, c = FT16.GUARD_LAST, FT16.GUARD_REFUSED
    z = c.dims
    dims = (z["n"], z["t"], z["d"], z["a"], z["vd"])
    assert P.stream_project_supported(*dims[1:]) and z["t"] >= 21
    torch.cuda.empty_cache()
    table = LG._word_table(z["v"], z["d"], LG._gen(c, gpu), gpu, dtype=torch.bfloat16)
    assert table.numel() * table.element_size() == LC.B31 and last.dims["v"] == z["v"] - 1
    ids_small = LC.gather_ids(last, z["n"], z["t"])
    assert ids_small.max() == z["v"] - 2
    inp = LG._stream_inputs(c, gpu, table=table, ids=_dev(ids_small, gpu, torch.int32))
    proj = LG._projection(c, gpu)
    outs = []
    for v in (z["v"] - 1, z["v"]):
        flag = _flag(gpu)
        out = P.mm2_stream_project_tt(*dims, inp["audio"], inp["visual"], proj, ids32=inp["ids"], table=table[:v],
                                      wtab32=inp["wtab"][:v], flag=flag)
        _check_rows(last if v < z["v"] else c, inp, out, gpu, flag, f"V = {v}")
        outs.append(out)
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    inp["ids"] = _dev(LC.gather_ids(c, z["n"], z["t"]), gpu, torch.int32)
    assert int(inp["ids"].max()) == z["v"] - 1
    flag = _flag(gpu)
    out = P.mm2_stream_project_tt(*dims, inp["audio"], inp["visual"], proj, ids32=inp["ids"], table=table,
                                  wtab32=inp["wtab"], flag=flag)
    _check_rows(c, inp, out, gpu, flag, "the last table row")
    del table, inp
    torch.cuda.empty_cache()
