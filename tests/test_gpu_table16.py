"""GPU: the SIF gather and the MMB2 stream kernels on a word table kept in
fp16 / bf16 storage (mmb_sif_wavg_tt, mmb_mm2_stream_tt; pipeline.weighted_sum,
mm2_stream, FusedStep).

The widening of a 16-bit table value to f32 is exact and the kernels sum the
widened values with the statements, and in the order, of their f32-table
instantiations -- the weighted sum, the text sums, the workgroup kernel's
row-0 shortcut, the column bounds.  So the definition under test is an
equality: a launch on a 16-bit table writes, bit for bit, what the same launch
writes on that table upcast to f32 by the caller -- x, s (both s_half
formats), aux, the column bounds and the flag word of the stream kernels (A),
x / num / cnt of the SIF gather (B), and x, aux, PC, SIF and MMB2 rows of the
step (D) -- for f32 frames and for frames of the table's own 16-bit kind.
Where the f32 twin would take the narrow-frame route, which a 16-bit table
never takes, the twin is steered onto the wave kernel as
tests/test_gpu_frames16.py does; the one step whose twin cannot be steered
holds the MMB2 rows to that file's 1e-6 row-relative bar.  The steps are also
held to the oracle on the upcast inputs with the suite's bars (MMB2 rows 1e-5,
PC 1e-10, SIF rows 2^-23); tests/test_table16_cases.py pins the family's
conditions on those inputs.  Every mirror that reads the table as f32 rejects
any other table before a launch, with its outputs untouched (C).
Product library only.
"""
import numpy as np
import pytest
import torch

import frames16_cases as F
import mmb2_cases as C
import mmb_lib as L
import pipeline as P
import table16_cases as T
from frames16_gpu import (F32_ROW, TOL, TWIN, _assert_graph_replays, _bufs, _colmax_bufs, _dev, _frames_of, _networks,
                          _off, _run, _untouched)
from mmb2_gpu import _is_narrow_route
from oracle import mmb2_oracle as M
from oracle import sif_oracle as O

pytestmark = pytest.mark.gpu

MODES = ("ids+table", "ids+w")
KIND_IDS = list(T.KINDS)


class _Launcher:
    """The device copies of one case's ids and weights, and stream launches on
    them with a table and frames given per call."""

    def __init__(self, case, gpu):
        self.case, self.gpu = case, gpu
        z = C.inputs(case)
        self.ids = _dev(z["ids"], gpu, torch.int32)
        self.wtab, self.sw = _dev(z["wt32"], gpu), _dev(z["sw"], gpu)

    def __call__(self, table, au, vi, mode, s_half, colmax):
        """(x, s, aux, colmax bits or None) as numpy, flag checked clear."""
        D, A, Vd, T_, N, V = self.case
        kw = {"wtab32": self.wtab} if mode == "ids+table" else {"w_dense": self.sw}
        cm, ws = _colmax_bufs(D, self.gpu) if colmax else (None, None)
        flag = torch.zeros(1, dtype=torch.int32, device=self.gpu)
        num, s, aux = P.mm2_stream(N, T_, D, A, Vd, au, vi, ids32=self.ids, table=table, s_half=bool(s_half),
                                   flag=flag, colmax=cm, colmax_ws=ws, **kw)
        torch.cuda.synchronize()
        assert int(flag.item()) == 0
        return (num.cpu().numpy(), s.cpu().numpy(), aux.cpu().numpy(),
                None if cm is None else cm.cpu().numpy().view(np.uint32))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint16)


def _equal(got, twin, what, names=("x", "s", "aux", "colmax")):
    for name, g, t in zip(names, got, twin):
        if g is None:
            assert t is None
            continue
        assert g.dtype == t.dtype and g.shape == t.shape, (what, name)
        # np.array_equal on the values (no NaN in these inputs) ...
        assert np.array_equal(g, t), (what, name)
        # ... and on the bits, so that +0 / -0 count as different
        assert np.array_equal(_bits(g), _bits(t)), (what, name, "bits")


def _sweep(case, gpu, table16=T.table, off16=0, off32=0):
    """Both kinds x frames (f32, the kind's) x (ids+table, ids+w) x s_half x
    colmax: the launch on the 16-bit table against the same launch on its
    upcast.  `off16` / `off32`: the tables that many elements past a 16-byte
    boundary."""
    run = _Launcher(case, gpu)
    n = 0
    for kind in T.KINDS:
        E16 = _dev(table16(case, kind), gpu)
        tab16, tab32 = _off(E16, off16), _off(E16.float(), off32)
        assert tab16.dtype == T.KINDS[kind] and tab32.dtype == torch.float32
        for frames in T.FRAME_CHOICES:
            au, vi = _frames_of(case, kind, frames, gpu)
            for mode in MODES:
                for s_half in (0, 1):
                    # the f32 twin on f32 frames may take the narrow-frame route, whose frame
                    # sums are in another order: given the gathered weights it stays on the
                    # wave kernel (16-bit frames never take that route)
                    narrow = frames == "f32" and _is_narrow_route(case, mode, s_half) and not off32
                    twin_mode = "ids+w" if narrow else mode
                    for colmax in (False, True):
                        got = run(tab16, au, vi, mode, s_half, colmax)
                        twin = run(tab32, au, vi, twin_mode, s_half, colmax)
                        _equal(got, twin, (C.shape_id(case), kind, frames, mode, s_half, colmax))
                        n += 1
    return n


# ------------------------------------------------------------------ A: stream outputs, bit for bit
@pytest.mark.parametrize("shape", C.WAVE_D256 + C.WAVE_D512 + C.NARROW_ROUTE, ids=C.shape_id)
def test_wave_kernel_bit_for_bit(gpu, shape):
    assert _sweep(C.case_of(shape), gpu) == 32


def test_wave_kernel_rows_of_a_workgroup_and_grid_stride(gpu):
    for n in C.WAVE_ROWS:
        _sweep(C.case_of(C.WAVE_ROWS_SHAPE, n), gpu)
    _sweep(C.case_of((4, 4, 4, 1), 4 * 2 * L.cu_count(gpu) + 3), gpu)


@pytest.mark.parametrize("shape", C.WG_SCALAR_TEXT + C.WG_VECTOR_TEXT + C.COMBOS, ids=C.shape_id)
def test_workgroup_kernel_bit_for_bit(gpu, shape):
    _sweep(C.case_of(shape, 3 if shape[3] > 512 else None), gpu)


def test_workgroup_kernel_either_side_of_the_cu_count(gpu):
    cus = L.cu_count(gpu)
    for n in (cus, cus + 1):
        _sweep(C.case_of(C.WG_CU_EDGE, n), gpu)


@pytest.mark.parametrize("shape", [(52, 8, 12, 7), (400, 300, 260, 40)], ids=C.shape_id)
def test_table_8_bytes_off_stays_on_the_wave_kernel(gpu, shape):
    """A 16-bit text column unit is 8 bytes: a table 8 bytes past a 16-byte
    boundary is still whole units (the f32 twin, aligned, is the wave kernel)."""
    _sweep(C.case_of(shape), gpu, off16=4)


def test_table_2_bytes_off_takes_the_scalar_text_route(gpu):
    """2 bytes off: the workgroup kernel with scalar 2-byte text loads -- as
    the f32 twin whose table is 4 bytes off."""
    _sweep(C.case_of(C.WG_UNALIGNED), gpu, off16=1, off32=1)


@pytest.mark.parametrize("shape", T.SPECIAL_SHAPES, ids=C.shape_id)
def test_special_values(gpu, shape):
    """+-0, the smallest subnormal and the largest planted value (65504 for
    fp16, 2^40 for bf16) in table row 0 and in the row the ids use most -- on
    the wave kernel (52, 8, 12, 7) and on the scalar workgroup kernel (50, 5,
    3, 9), whose row-0 shortcut the planted row 0 exercises."""
    case = C.case_of(shape)
    _sweep(case, gpu, table16=T.special_table)
    run = _Launcher(case, gpu)
    D, A, Vd, T_, N, V = case
    ids = C.inputs(case)["ids"]
    with0, hot = (ids == 0).any(axis=1), (ids == T.hot_row(case)).any(axis=1)
    assert with0.any() and hot.any()
    au, vi = _frames_of(case, "f16", "f32", gpu)
    for kind in T.KINDS:
        x, s, aux, _ = run(_dev(T.special_table(case, kind), gpu), au, vi, "ids+table", 0, False)
        k = len(T.SPECIALS[kind])
        big = np.float32(T.SPECIALS[kind][-1][0])
        assert np.isfinite(s).all() and np.isfinite(x).all()
        # the planted row-0 value reached s: c0 E0^2 dominates its column of Sxx_e (E[0, k - 1]) ...
        assert (s[with0, D + k - 1] >= big * big).all()
        assert (s[~with0, D + k - 1] < big * big).all()
        # ... and Sx_e: c0 E0 among at most T values of the family's table
        assert (s[with0, k - 1] >= big - T_ * 4.0).all()
        # and the hot row's (E[hot, D - k]) in the rows that name it
        assert (s[hot, D + D - k] >= big * big).all()


# ------------------------------------------------------------------ B: the SIF gather, bit for bit
def _sif_pair(gpu, E16, ids, wt32, w, off16=0, off32=0, want_flag=0):
    """weighted_sum on the 16-bit table against weighted_sum on its upcast:
    x, num and cnt, both weight sources; the flag words equal `want_flag`."""
    E16 = _dev(E16, gpu)
    tab16, tab32 = _off(E16, off16), _off(E16.float(), off32)
    ids32 = _dev(ids, gpu, torch.int32)
    for src, kw in (("wtab32", {"wtab32": _dev(wt32, gpu)}), ("w", {"w": _dev(w, gpu)})):
        for x_out in (True, False):
            f16, f32 = (torch.zeros(1, dtype=torch.int32, device=gpu) for _ in range(2))
            got = P.weighted_sum(tab16, ids32, flag=f16, x_out=x_out, **kw)
            twin = P.weighted_sum(tab32, ids32, flag=f32, x_out=x_out, **kw)
            torch.cuda.synchronize()
            got, twin = ((o,) if x_out else o for o in (got, twin))
            _equal([g.cpu().numpy() for g in got], [t.cpu().numpy() for t in twin],
                   (tuple(E16.shape), tuple(ids.shape), str(E16.dtype), src), ("x",) if x_out else ("num", "cnt"))
            assert int(f16.item()) == int(f32.item()) == want_flag, (src, x_out)


@pytest.mark.parametrize("kind", KIND_IDS)
@pytest.mark.parametrize("d,l", T.SIF_WAVE, ids=[C.shape_id(c) for c in T.SIF_WAVE])
def test_sif_wave_kernel_bit_for_bit(gpu, d, l, kind):
    _sif_pair(gpu, *T.sif_inputs(d, l, kind))


@pytest.mark.parametrize("kind", KIND_IDS)
@pytest.mark.parametrize("d,l", T.SIF_WG, ids=[C.shape_id(c) for c in T.SIF_WG])
def test_sif_workgroup_kernel_bit_for_bit(gpu, d, l, kind):
    _sif_pair(gpu, *T.sif_inputs(d, l, kind))


@pytest.mark.parametrize("kind", KIND_IDS)
def test_sif_table_2_bytes_off(gpu, kind):
    """The scalar workgroup kernel at a width % 4 == 0, as the f32 twin 4 bytes off."""
    _sif_pair(gpu, *T.sif_inputs(*T.SIF_UNALIGNED, kind), off16=1, off32=1)


@pytest.mark.parametrize("kind", KIND_IDS)
@pytest.mark.parametrize("d,l", [(52, 7), (50, 9)], ids=["52-7", "50-9"])
def test_sif_out_of_range_id_sets_the_same_flag_and_row(gpu, d, l, kind):
    E16, ids, wt32, w = T.sif_inputs(d, l, kind)
    assert (ids < 0).any()  # the negative ids that wrap are part of every case with l >= 7
    bad = ids.copy()
    bad[0, 0] = T.SIF_V + 5
    _sif_pair(gpu, E16, bad, wt32, w, want_flag=L.MMB_FLAG_ID_RANGE)


def test_sif_embeddings_on_a_16_bit_table(gpu):
    E16, ids, wt32, w = T.sif_inputs(52, 7, "bf16", n=64)
    E16 = _dev(E16, gpu)
    ids = _dev(ids, gpu, torch.int32)
    wtab = _dev(wt32, gpu)
    got, pc1 = P.sif_embeddings(E16, ids, wtab32=wtab)
    twin, pc2 = P.sif_embeddings(E16.float(), ids, wtab32=wtab)
    assert torch.equal(got, twin) and torch.equal(pc1, pc2)


# ------------------------------------------------------------------ C: rejections, outputs untouched
def _sentinel_out(N, D, kp, s_half, gpu):
    num = torch.full((N, D), -7.0, device=gpu)
    s = P.s_buffer(N, kp, s_half, gpu).fill_(-7.0)
    aux = torch.full((3, N), -7.0, device=gpu)
    return num, s, aux


def test_mm2_stream_rejections_leave_the_outputs_untouched(gpu):
    case = C.case_of((52, 8, 12, 70), 4)
    D, A, Vd, T_, N, V = case
    z = C.inputs(case)
    kp = L.query("mmb_mm2_k", D, A, Vd)
    ids, table, wtab = _dev(z["ids"], gpu, torch.int32), _dev(z["E"], gpu), _dev(z["wt32"], gpu)
    text, sw = _dev(z["text"], gpu), _dev(z["sw"], gpu)
    a32, v32 = _dev(z["audio"], gpu), _dev(z["visual"], gpu)
    for s_half in (False, True):
        out = _sentinel_out(N, D, kp, s_half, gpu)
        for kind, dt in T.KINDS.items():
            tab16 = table.to(dt)
            for au, vi in ((a32, v32), (a32.to(dt), v32.to(dt))):
                gather = dict(ids32=ids, table=tab16, wtab32=wtab)
                # (16-bit frames with `split` are rejected for the frames first)
                why = "a float32 word table only" if au is a32 else "float32 frames only"
                with pytest.raises(L.MMBError, match="split stream reads " + why):
                    P.mm2_stream(N, T_, D, A, Vd, au, vi, s_half=s_half, out=out,
                                 split=P.split_ws(N, T_, D, A, Vd, gpu, parts=2), parts=2, **gather)
                with pytest.raises(L.MMBError, match="reads a float32 word table only"):
                    P.mm2_stream_split_ft(N, T_, D, A, Vd, au, vi, ids, tab16, wtab32=wtab, s_half=s_half,
                                          out=out, parts=2)
            with pytest.raises(L.MMBError, match="word table goes with gathered text"):
                P.mm2_stream(N, T_, D, A, Vd, a32, v32, table=tab16, text_dense=text, emb_dense=text,
                             w_dense=sw, s_half=s_half, out=out)
        t64 = table.double()
        with pytest.raises(L.MMBError, match="float32, float16 or bfloat16, not torch.float64"):
            P.mm2_stream(N, T_, D, A, Vd, a32, v32, ids32=ids, table=t64, wtab32=wtab, s_half=s_half, out=out)
        with pytest.raises(L.MMBError, match="float32, float16 or bfloat16, not torch.float64"):
            P.mm2_stream(N, T_, D, A, Vd, a32, v32, table=t64, text_dense=text, emb_dense=text, w_dense=sw,
                         s_half=s_half, out=out)
        with pytest.raises(L.MMBError, match="float32, float16 or bfloat16, not torch.float64"):
            P.mm2_stream_split_ft(N, T_, D, A, Vd, a32, v32, ids, t64, wtab32=wtab, s_half=s_half, out=out)
        assert _untouched(out)
    for call in (P.weighted_sum, P.sif_embeddings):
        with pytest.raises(L.MMBError, match="float32, float16 or bfloat16, not torch.float64"):
            call(table.double(), ids, wtab32=wtab)


def test_fused_mirrors_and_the_text_cache_reject_a_non_f32_table(gpu):
    case = C.NARROW_FUSED[1]  # (260, 76, 48, 20, 31, 3016): both fused fronts take the shape at f32
    D, A, Vd, T_, N, V = case
    assert P.stream_project_supported(T_, D, A, Vd) and P.narrow_fused_supported(T_, D, A, Vd, V)
    z = C.inputs(case)
    proj = P.MMB2Projection(_networks(case, gpu), D, A, Vd, T_, gpu)
    ids, table, wtab = _dev(z["ids"], gpu, torch.int32), _dev(z["E"], gpu), _dev(z["wt32"], gpu)
    au, vi = _dev(z["audio"], gpu), _dev(z["visual"], gpu)
    out = _bufs(N, D, gpu, bounds=False, fill=-7.0)[0]
    mirrors = {"mm2_stream_project": P.mm2_stream_project, "mm2_stream_project_ft": P.mm2_stream_project_ft,
               "mm2_stream_project_narrow": P.mm2_stream_project_narrow,
               "mm2_stream_project_narrow_ft": P.mm2_stream_project_narrow_ft}
    for bad in (table.half(), table.bfloat16(), table.double()):
        for name, front in mirrors.items():
            with pytest.raises(L.MMBError, match=f"{name}.* word table"):
                front(N, T_, D, A, Vd, au, vi, proj, ids32=ids, table=bad, wtab32=wtab, out=out)
        with pytest.raises(L.MMBError, match="enable_text_cache.* word table"):
            proj.enable_text_cache(bad, wtab)
        assert getattr(proj, "text_cache", None) is None
    assert _untouched(out)
    with pytest.raises(L.MMBError, match="FusedStep.* word table"):
        P.FusedStep({"table": table.double(), "wtab": wtab, "ids": ids, "audio": au, "visual": vi},
                    _networks(case, gpu))


# ------------------------------------------------------------------ D: the step
EVERYTHING = dict(stream_project=True, narrow_fused=True, split_stream=True, fused_frames16=True,
                  narrow_frames16=True, split_frames16=True)


def _step_inputs(case, kind, frames, gpu):
    """(the inputs with the 16-bit table, the same with its f32 upcast); the
    frames are f32 or of the table's kind, the same tensors in both."""
    z = C.inputs(case)
    E16 = _dev(T.table(case, kind), gpu)
    au, vi = _frames_of(case, kind, frames, gpu)
    base = {"wtab": _dev(z["wt32"], gpu), "ids": _dev(z["ids"], gpu, torch.int32), "audio": au, "visual": vi}
    return dict(base, table=E16), dict(base, table=E16.float())


def _check_oracle(case, kind, frames, step, sif, mm2):
    x = step.x.double().cpu().numpy()
    eo = M.row_rel_err(mm2.cpu().numpy(), T.oracle_rows(case, kind, T.fkind_of(kind, frames))) / TOL
    ep = np.abs(step.pc.cpu().numpy() - O.compute_pc(x, 1)).max() / 1e-10
    ref = O.remove_pc(x, 1)
    es = (np.abs(sif.cpu().numpy() - ref) / np.abs(ref).max(axis=1, keepdims=True)).max() / F32_ROW
    print(f"{C.shape_id(case)} {kind} table, {frames} frames: MMB2 {eo:.3f} of 1e-5, PC {ep:.3f} of 1e-10, "
          f"SIF rows {es:.3f} of 2^-23")
    assert eo < 1.0 and ep < 1.0 and es <= 1.0


@pytest.mark.parametrize("frames", T.FRAME_CHOICES)
@pytest.mark.parametrize("kind", KIND_IDS)
@pytest.mark.parametrize("dims", T.STEP, ids=C.shape_id)
def test_fused_step_on_a_16_bit_table(gpu, dims, kind, frames):
    case = F.step_case(dims)
    inp16, inp32 = _step_inputs(case, kind, frames, gpu)
    nets = _networks(case, gpu)
    a = P.FusedStep(inp16, nets)
    b = P.FusedStep(inp32, nets, **TWIN)
    assert a.table_kind == kind and b.table_kind == "f32" and a.frames == b.frames
    assert a.plan.front == "stream" and a.plan.split is False
    assert a.plan == b.plan
    # whatever the overrides and opt-ins allow, the 16-bit table keeps the plain stream kernel
    assert P.FusedStep(inp16, nets, **EVERYTHING).plan == a.plan
    s1, m1 = _run(a)
    s2, m2 = _run(b)
    assert torch.equal(a.x, b.x) and torch.equal(a.aux, b.aux) and torch.equal(a.pc, b.pc)
    assert torch.equal(s1, s2)
    if tuple(dims) == T.STEP_NARROW_TWIN and frames == "f32":
        # the twin's stream kernel is the narrow-frame route (another order of
        # the frame sums): the bar of tests/test_gpu_frames16.py between the two
        e = M.row_rel_err(m1.cpu().numpy(), m2.cpu().numpy())
        print(f"MMB2 rows vs the narrow-route twin: {e:.2e} (bar 1e-6)")
        assert e < 1e-6
    else:
        assert torch.equal(m1, m2)
    _check_oracle(case, kind, frames, a, s1, m1)


def test_step_graph_replays_the_bf16_table_step(gpu):
    case = F.step_case(T.STEP[0])
    inp16, _ = _step_inputs(case, "bf16", "f32", gpu)
    _assert_graph_replays(P.FusedStep(inp16, _networks(case, gpu)))


@pytest.mark.parametrize("frames", T.FRAME_CHOICES)
@pytest.mark.parametrize("kind", KIND_IDS)
def test_chunked_step_on_a_16_bit_table(gpu, kind, frames):
    case = F.step_case(T.CHUNKED)
    inp16, inp32 = _step_inputs(case, kind, frames, gpu)
    nets = _networks(case, gpu)
    a = P.FusedStep(inp16, nets, chunks=3)
    b = P.FusedStep(inp32, nets, chunks=3, **TWIN)
    assert len(a.bounds) == 3 and a.plan == b.plan and a.table_kind == kind
    s1, m1 = _run(a)
    s2, m2 = _run(b)
    assert torch.equal(a.x, b.x) and torch.equal(a.aux_flat, b.aux_flat) and torch.equal(a.pc, b.pc)
    assert torch.equal(s1, s2) and torch.equal(m1, m2)
