"""GPU parity of the MMB2 stream and projection kernels at text widths other than 300.

FusedStep and sif2.estimate_embedding_overall_gpu2 take a word table of any
width (GloVe 50 / 100 / 200 are a normal configuration of the reference);
under them libmmb dispatches on the text, audio and visual widths, the frame
count, the row count and pointer alignment (csrc/sif_kernels.hip: the wave
stream kernel's eight instantiations and its narrow-frame route, the
workgroup kernel's eight vector / scalar ones, split_rows_kernel, the split
stream; csrc/mm2_kernels.hip: both c0 routes of mmb_mm2_prepare, the f32
projection at CT = 1 .. 6, the fp16 x3 projection at CT = 1 .. 5 with its tile
epilogue and fused PC removal, the text cache).  tests/mmb2_cases.py holds
the smallest shapes that reach each route and edge; every comparison is with
f64 numpy of the same operation or the CPU oracle, each stage at a bar
derived from the case's own terms (mmb2_cases.sum_bar / project_reference /
prepare_reference), the end-to-end rows at 1e-5:

  1 wave stream kernel, D <= 256      x, s, weight sum: 2 (T + 1) 2^-24 sum |term|; count,
  2 wave kernel 320..512, narrow route  pads, bounds, aux[2] exact; fp16 hi + lo against the
  3 workgroup stream kernel             fp32 row of the same route: 2^-21 |s| + 2^-25 / aux[2]
  4 split stream                      parts = 1 bit-identical to the one-workgroup kernel
  5 mmb_mm2_prepare                   2 * 2^-24 |value| + 1e-12 sum |terms|; pads exactly 0
  6 mmb_mm2_project                   f64 from the device's own operands: beta (see
  7 mmb_mm2_project_x3 / _rmpc          project_reference) AND the flat 1e-5; removed rows 2^-23
  8 mmb_calc_weights                  8 * 2^-24 |q_mean|; 10 * 2^-24 d^2 / e + 2^-23 |q_sigma|
  9 narrow fused kernel, text cache   as test_narrow_fused_matches_two_kernel_step
 10 FusedStep, the sif2 drop-in       MMB2 rows 1e-5; PC 1e-10; SIF rows 2^-23

tests/test_mmb2_cases.py (CPU) pins the conditions on the inputs that these
bars rest on.  Unsupported shapes are pinned as MMBError (MMB_EINVAL before any
launch) with the outputs untouched.  Every test prints its largest error as a
fraction of its bar; the module prints the per-group maxima at the end.

Only the product library is loaded.
"""
import functools

import numpy as np
import pytest
import torch

import mmb2_cases as C
import mmb2_gpu as MG
import mmb_lib as L
import pipeline as P
import sif2
import width_cases as W
from common_gpu import TOL, Ledger, _colmax_bufs, _dev, _frac, _networks, _off, _untouched
from mmb2_gpu import MODES, _dequant, _device_inputs, _is_narrow_route, _operands, _ref, _stream
from oracle import mmb2_oracle as M

pytestmark = pytest.mark.gpu

_WORST = Ledger()  # (group, what) -> [comparisons, largest error / bar]


def _note(group, what, frac):
    return _WORST.note((group, what), frac)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for (group, what), (cases, frac) in sorted(_WORST.items()):
        print(f"\nmmb2 widths group {group} {what}: {cases} comparisons, largest {frac:.3f} of its bar",
              end="")
    print()


# the shared checkers (tests/mmb2_gpu.py), noted in this module's report
_check_stream = functools.partial(MG._check_stream, _note)
_check_rows = functools.partial(MG._check_rows, _note)
_check_removed = functools.partial(MG._check_removed, _note)
_check_step = functools.partial(MG._check_step, _note)


def _stream_sweep(group, case, gpu, modes=MODES, colmaxes=(False, True), **kw):
    """Every mode with s_half 0 and 1, with and without the column bounds."""
    worst = 0.0
    for mode in modes:
        ref = _ref(case, emb2=mode == "dense+emb2")
        for cmx in colmaxes:
            o32 = _stream(case, mode, gpu, False, colmax=cmx, **kw)
            worst = max(worst, _check_stream(group, case, o32, ref, False))
            o16 = _stream(case, mode, gpu, True, colmax=cmx, **kw)
            narrow = _is_narrow_route(case, mode, True) and not kw
            worst = max(worst, _check_stream(group, case, o16, ref, True,
                                             twin=None if narrow else o32[1]))
            # x, count and the weight sum do not depend on the s format
            assert np.array_equal(o16[0], o32[0]) and np.array_equal(o16[2][:2], o32[2][:2])
    print(f"{C.shape_id(case)}: largest error {worst:.3f} of its bar")


# ------------------------------------------------------------------ 1: wave kernel, D <= 256
@pytest.mark.parametrize("shape", C.WAVE_D256, ids=C.shape_id)
def test_wave_stream_d256(gpu, shape):
    _stream_sweep(1, C.case_of(shape), gpu)


def test_wave_stream_rows_of_a_workgroup_and_grid_stride(gpu):
    for n in C.WAVE_ROWS:
        _stream_sweep(1, C.case_of(C.WAVE_ROWS_SHAPE, n), gpu, modes=("ids+table",), colmaxes=(True,))
    # more rows than the grid's waves (4 per workgroup, 2 workgroups per CU): the grid-stride loop
    _stream_sweep(1, C.case_of((4, 4, 4, 1), 4 * 2 * L.cu_count(gpu) + 3), gpu,
                  modes=("ids+table", "dense"), colmaxes=(True,))


@pytest.mark.filterwarnings("ignore:invalid value encountered")
@pytest.mark.parametrize("shape", [(52, 8, 12, 7), (50, 5, 3, 9), (316, 128, 4, 33)], ids=C.shape_id)
def test_stream_flags_and_nan_row(gpu, shape):
    """A negative id (wraps for its row, weight 0), an id >= V (flagged, the
    token dropped) and an utterance whose weights are all 0 (flagged, x = 0 / 0
    = NaN) on the wave, workgroup and narrow-frame routes."""
    case = C.case_of(shape)
    D, A, Vd, T, N, V = case
    z = C.inputs(case)
    ids = z["ids"].copy()
    ids[1, 0], ids[2, min(1, T - 1)], ids[3, :] = -3, V + 7, 0
    wt32 = z["wt32"].copy()
    wt32[0] = 0.0
    ok = (ids >= 0) & (ids < V)
    wrapped = np.where(ids < 0, ids + V, ids)
    inr = (wrapped >= 0) & (wrapped < V)
    text = np.where(inr[:, :, None], z["E"][np.where(inr, wrapped, 0)], 0).astype(np.float32)
    sw = np.where(ok, wt32[np.where(ok, ids, 0)], 0).astype(np.float32)
    ref = C.stream_reference(text, text, sw, z["audio"], z["visual"])
    assert np.isnan(ref["x"][3]).all() and ref["cnt"][3] == 0
    good = ref["cnt"] != 0  # (a ragged row left with the negative id alone has no weight either)
    assert good.sum() >= 2 and np.isfinite(ref["x"][good]).all()
    for s_half in (False, True):
        flag = torch.zeros(1, dtype=torch.int32, device=gpu)
        num, s, aux = P.mm2_stream(N, T, D, A, Vd, _dev(z["audio"], gpu), _dev(z["visual"], gpu),
                                   ids32=_dev(ids, gpu, torch.int32), table=_dev(z["E"], gpu),
                                   wtab32=_dev(wt32, gpu), s_half=s_half, flag=flag)
        torch.cuda.synchronize()
        assert int(flag.item()) == L.MMB_FLAG_ID_RANGE | L.MMB_FLAG_ZERO_WEIGHTS
        num, aux = num.cpu().numpy(), aux.cpu().numpy()
        assert np.isnan(num[~good]).all() and np.isfinite(num[good]).all()
        assert np.array_equal(aux[0], ref["cnt"])
        e = _note(1, "x (flagged ids)", _frac(np.abs(num - ref["x"])[good],
                                              C.sum_bar(T, ref["x_abs"])[good]))
        assert e <= 1.0
        if not s_half:
            K = 2 * (D + A + Vd)
            e = _note(1, "s (flagged ids)", _frac(np.abs(s.cpu().numpy()[:, :K] - ref["s"]),
                                                  C.sum_bar(T, ref["s_abs"])))
            assert e <= 1.0


# ------------------------------------------------------------------ 2: wave kernel, 320 <= D <= 512
@pytest.mark.parametrize("shape", C.WAVE_D512, ids=C.shape_id)
def test_wave_stream_d512(gpu, shape):
    _stream_sweep(2, C.case_of(shape), gpu)


@pytest.mark.parametrize("shape", C.NARROW_ROUTE, ids=C.shape_id)
def test_narrow_frame_route(gpu, shape):
    """utt_narrow_kernel (ids + weight table, fp16 s) at D != 300: its text
    sums are the wave kernel's operations in its order, so x, count, weight
    sum and the bounds equal the fp32 launch's bit for bit; the frame sums
    (slot partials) are held to the sums' own bar against f64."""
    case = C.case_of(shape)
    ref = _ref(case)
    worst = 0.0
    for cmx in (False, True):
        o16 = _stream(case, "ids+table", gpu, True, colmax=cmx)
        o32 = _stream(case, "ids+table", gpu, False, colmax=cmx)
        worst = max(worst, _check_stream(2, case, o16, ref, True))
        assert np.array_equal(o16[0], o32[0]) and np.array_equal(o16[2][:2], o32[2][:2])
        assert cmx is False or np.array_equal(o16[3], o32[3])
    print(f"{C.shape_id(case)}: largest error {worst:.3f} of its bar")


# ------------------------------------------------------------------ 3: workgroup kernel
@pytest.mark.parametrize("shape", C.WG_SCALAR_TEXT + C.WG_VECTOR_TEXT, ids=C.shape_id)
def test_workgroup_stream(gpu, shape):
    n = 3 if shape[3] > 512 else None
    _stream_sweep(3, C.case_of(shape, n), gpu)


@pytest.mark.parametrize("shape", C.COMBOS, ids=C.shape_id)
def test_workgroup_stream_vector_scalar_combinations(gpu, shape):
    _stream_sweep(3, C.case_of(shape), gpu, modes=("ids+table", "dense+emb2"), colmaxes=(True,))


def test_workgroup_stream_unaligned_table(gpu):
    """D % 4 == 0 with the table 4 bytes off alignment: the scalar text route."""
    _stream_sweep(3, C.case_of(C.WG_UNALIGNED), gpu, modes=("ids+table", "ids+w"), table_off=True)


def test_workgroup_stream_either_side_of_the_cu_count(gpu):
    """N <= CUs takes the FU = 16, TU = 8 variant, N > CUs the default."""
    cus = L.cu_count(gpu)
    for n in (cus, cus + 1):
        _stream_sweep(3, C.case_of(C.WG_CU_EDGE, n), gpu, modes=("ids+table",), colmaxes=(True,))


def _sentinel_out(N, D, kp, s_half, gpu):
    num = torch.full((N, D), -7.0, device=gpu)
    s = P.s_buffer(N, kp, s_half, gpu).fill_(-7.0)
    aux = torch.full((3, N), -7.0, device=gpu)
    return num, s, aux


@pytest.mark.parametrize("shape,colmax", [((321, 4, 4, 3), False), ((644, 4, 4, 2), True),
                                          ((52, 321, 4, 3), False), ((52, 4, 321, 3), False)],
                         ids=["scalar-D321", "colmax-D644", "scalar-A321", "scalar-Vd321"])
def test_stream_rejections(gpu, shape, colmax):
    """The C entry point returns MMB_EINVAL before any launch (outputs
    untouched); the mirror names the width limit."""
    D, A, Vd, T = shape
    N, V = 3, 50
    kp = L.query("mmb_mm2_k", D, A, Vd)
    ids = torch.ones((N, T), dtype=torch.int32, device=gpu)
    table, wtab = torch.zeros((V, D), device=gpu), torch.ones(V, device=gpu)
    au, vi = torch.zeros((N, T, A), device=gpu), torch.zeros((N, T, Vd), device=gpu)
    cm, ws = _colmax_bufs(D, gpu) if colmax else (None, None)
    for s_half in (False, True):
        num, s, aux = out = _sentinel_out(N, D, kp, s_half, gpu)
        with pytest.raises(L.MMBError, match="invalid argument"):
            L.call("mmb_mm2_stream", L.ptr(ids), L.ptr(table), V, L.ptr(wtab), None, None, None,
                   L.ptr(au), L.ptr(vi), N, T, D, A, Vd, L.ptr(num), L.ptr(s), int(s_half), L.ptr(aux),
                   None, L.ptr(cm), L.ptr(ws), L.stream_ptr())
        assert _untouched(out)
        if not colmax:
            with pytest.raises(L.MMBError, match="width 321 is past the stream kernels' limit"):
                P.mm2_stream(N, T, D, A, Vd, au, vi, ids32=ids, table=table, wtab32=wtab,
                             s_half=s_half, out=out)
            assert _untouched(out)
    if colmax:  # the same shape without the bounds is a supported vector row
        P.mm2_stream(N, T, D, A, Vd, au, vi, ids32=ids, table=table, wtab32=wtab, s_half=False)
        torch.cuda.synchronize()


# ------------------------------------------------------------------ 4: split stream
@pytest.mark.parametrize("shape", C.COMBOS, ids=C.shape_id)
def test_split_stream(gpu, shape):
    case = C.case_of(shape)
    D, A, Vd, T, N, V = case
    worst = 0.0
    for mode in ("ids+table", "dense+emb2"):
        ref = _ref(case, emb2=mode == "dense+emb2")
        one32 = _stream(case, mode, gpu, False, colmax=True)
        one16 = _stream(case, mode, gpu, True, colmax=True)
        for parts in (1, 3, 200, 0):
            o32 = _stream(case, mode, gpu, False, colmax=True, split_parts=parts)
            o16 = _stream(case, mode, gpu, True, colmax=True, split_parts=parts)
            worst = max(worst, _check_stream(4, case, o32, ref, False),
                        _check_stream(4, case, o16, ref, True, twin=o32[1]))
            if parts == 1:  # one range: the one-workgroup kernel's sums in its order
                for a, b in zip(o32 + o16, one32 + one16):
                    assert np.array_equal(a, b)
    assert P.split_parts(N, T) == 1  # parts = 0 at T = 70: no range under 64 frames
    q = P.split_ws(N, T, D, A, Vd, gpu, parts=3).numel()
    assert q == 4 * N * 3 * ((3 * D + 4 + 3) // 4 * 4 + (2 * A + 2 * Vd + 3) // 4 * 4)  # ranges 24, 24, 22
    assert P.split_ws(N, T, D, A, Vd, gpu, parts=200).numel() == q // 3 * T  # clipped to T
    print(f"{C.shape_id(case)}: largest error {worst:.3f} of its bar")


def test_split_stream_rejects_past_the_finish_kernels_columns(gpu):
    D, A, Vd, T, N, V = 512, 300, 300, 70, 3, 50
    assert 3 * D + 2 * A + 2 * Vd == 2736
    kp = L.query("mmb_mm2_k", D, A, Vd)
    au, vi = torch.zeros((N, T, A), device=gpu), torch.zeros((N, T, Vd), device=gpu)
    for s_half in (False, True):
        out = _sentinel_out(N, D, kp, s_half, gpu)
        with pytest.raises(L.MMBError):
            P.mm2_stream(N, T, D, A, Vd, au, vi, ids32=torch.ones((N, T), dtype=torch.int32, device=gpu),
                         table=torch.zeros((V, D), device=gpu), wtab32=torch.ones(V, device=gpu),
                         s_half=s_half, out=out, split=P.split_ws(N, T, D, A, Vd, gpu, parts=2), parts=2)
        assert _untouched(out)


# ------------------------------------------------------------------ 5: mmb_mm2_prepare
def _param_arrays(D, A, Vd, gpu):
    """The generator's parameters on the device and mmb_mm2_prepare's four host
    arrays of device pointers (the tensors are returned to keep them alive)."""
    nets = C.generator(D, A, Vd).networks()
    prm = [tuple(p.detach().to(gpu).contiguous() for p in (mu.weight, mu.bias, ls.weight, ls.bias))
           for mu, ls in (nets[k] for k in sif2.KEYS)]
    return prm, [P.ctypes_ptr_array([p[i].data_ptr() for p in prm]) for i in range(4)]


def _prepare(D, A, Vd, T, gpu, wsplit):
    """mmb_mm2_prepare into NaN-filled buffers; returns (wm, c0) as numpy."""
    kp, ldw = P.mm2_dims(D, A, Vd)
    prm, ptrs = _param_arrays(D, A, Vd, gpu)
    arr = lambda i: ptrs[i]
    wm = torch.full((kp, ldw), float("nan"), device=gpu)
    c0 = torch.full((ldw,), float("nan"), device=gpu)
    ws = None
    if wsplit:
        nb = L.query("mmb_mm2_split_bytes", D, A, Vd)
        ws = torch.empty((nb + 15) // 16 * 16, dtype=torch.uint8, device=gpu)
    L.call("mmb_mm2_prepare", arr(0), arr(1), arr(2), arr(3), D, A, Vd, T, L.ptr(wm), ldw, L.ptr(c0),
           L.ptr(ws), L.stream_ptr())
    torch.cuda.synchronize()
    return wm.cpu().numpy(), c0.cpu().numpy()


@pytest.mark.parametrize("dims", [(D, 8, 12) for D in C.PREPARE_D] + C.PREPARE_KP, ids=C.shape_id)
def test_prepare(gpu, dims):
    D, A, Vd = dims
    K = 2 * (D + A + Vd)
    worst = 0.0
    for T in C.PREPARE_T:
        Wm, c0, wbar, cbar = C.prepare_reference(D, A, Vd, T)
        for wsplit in (False, True):  # both c0 routes on either side of Kp = 128
            wm, c = _prepare(D, A, Vd, T, gpu, wsplit)
            assert not wm[K:].any() and not wm[:, D + 1:].any() and not c[D + 1:].any()  # exactly 0
            e1 = _note(5, "Wm", _frac(np.abs(wm[:K, :D + 1] - Wm), wbar))
            e2 = _note(5, "c0", _frac(np.abs(c[:D + 1] - c0), cbar))
            worst = max(worst, e1, e2)
            assert e1 <= 1.0 and e2 <= 1.0, (T, wsplit, e1, e2)
    print(f"D={D} A={A} Vd={Vd} (Kp {(K + 31) // 32 * 32}, ldw {(D + 64) // 64 * 64}): "
          f"largest error {worst:.3f} of its bar")


def test_projection_rejects_d384(gpu):
    """ldw = 448 > 384 (D = 383 is the last width of ldw 384: tests above): no
    projection kernel takes it.  The C entry points return MMB_EINVAL before
    any launch; the mirror and the drop-in name the limit."""
    D, A, Vd = 384, 4, 4
    kp, ldw = P.mm2_dims(D, A, Vd)
    assert ldw == 448 and P.mm2_dims(383, A, Vd)[1] == 384
    with pytest.raises(L.MMBError, match="d <= 383"):
        P.MMB2Projection(C.generator(D, A, Vd).networks(), D, A, Vd, 5, gpu)
    prm, ptrs = _param_arrays(D, A, Vd, gpu)
    arr = lambda i: ptrs[i]
    wm = torch.full((kp, ldw), -7.0, device=gpu)
    c0 = torch.full((ldw,), -7.0, device=gpu)
    with pytest.raises(L.MMBError):
        L.call("mmb_mm2_prepare", arr(0), arr(1), arr(2), arr(3), D, A, Vd, 5, L.ptr(wm), ldw,
               L.ptr(c0), None, L.stream_ptr())
    n = 3
    s = torch.zeros((n, kp), device=gpu)
    num, aux = torch.ones((n, D), device=gpu), torch.ones((3, n), device=gpu)
    out = torch.full((n, D), -7.0, device=gpu)
    with pytest.raises(L.MMBError):
        L.call("mmb_mm2_project", L.ptr(s), L.ptr(num), L.ptr(aux), L.ptr(wm), ldw, L.ptr(c0), n, kp, D,
               L.ptr(out), L.stream_ptr())
    assert _untouched((wm, c0, out))
    # the drop-in reports the same limit (D = 400)
    z = C.inputs((400, 4, 4, 3, 4, 50))
    t_ = lambda a: _dev(a, gpu)
    tx = t_(z["text"])
    data = {k: t_(v) for k, v in M.concat_inputs(z["text"], z["audio"], z["visual"]).items()}
    nets = _networks((400, 4, 4), gpu)
    with pytest.raises(L.MMBError, match="d <= 383"):
        sif2.estimate_embedding_overall_gpu2(data, {k: None for k in data}, nets, t_(z["sw"]), tx)


# ------------------------------------------------------------------ 6 / 7: the projections
PROJECT_CASES = C.project_cases()


@pytest.mark.parametrize("D", C.PROJECT_D + ["short-K"])
def test_project_f32(gpu, D):
    worst = 0.0
    for case in [c for c in PROJECT_CASES if (c[0] == D if D != "short-K" else c[0] < 63)]:
        num, s32, s16, aux, aux16, proj = _operands(case, gpu)
        got = P.mm2_project(s32, num, aux, proj)
        worst = max(worst, _check_rows(6, "mmb_mm2_project", case, got, s32.cpu().numpy(), num, aux,
                                       proj, x3=False))
    print(f"D={D}: largest error {worst:.3f} of its bar")


PROJECT_X3_CASES = C.project_x3_cases()


@pytest.mark.parametrize("D", C.PROJECT_X3_D + ["short-K"])
def test_project_x3_and_fused_removal(gpu, D):
    worst = 0.0
    for case in [c for c in PROJECT_X3_CASES if (c[0] == D if D != "short-K" else c[0] < 63)]:
        d, A, Vd, T, N, V = case
        num, s32, s16, aux, aux16, proj = _operands(case, gpu)
        assert torch.equal(aux, aux16)
        s = _dequant(s16, aux16, proj.kp)
        got = P.mm2_project(s16, num, aux16, proj)
        worst = max(worst, _check_rows(7, "mmb_mm2_project_x3", case, got, s, num, aux16, proj, x3=True))
        pch = W.orthonormal_rows(1, d, seed=d + N)
        sif = torch.full((N, d), -7.0, device=gpu)
        got_pc = P.mm2_project(s16, num, aux16, proj, pc=_dev(pch, gpu), sif_out=sif)
        assert torch.equal(got_pc, got)  # the removal does not touch the MMB2 rows
        _check_removed(case, sif, num, pch, gpu)
        if d < 256:  # nothing to split below the row-wise epilogue's widths: the one-pass kernel
            ws = P.project_split_ws(N, proj.kp, gpu, slices=4)
            sif2_ = torch.empty_like(sif)
            got_sp = P.mm2_project(s16, num, aux16, proj, pc=_dev(pch, gpu), sif_out=sif2_, split=ws,
                                   slices=4)
            assert torch.equal(got_sp, got) and torch.equal(sif2_, sif)
    print(f"D={D}: largest error {worst:.3f} of its bar")


def test_project_x3_tile_epilogue_at_the_bench_width(gpu):
    """D = 300 with sif_out 4 bytes off alignment: CT = 5 with the tile-layout
    epilogue and its fused removal, against the row-wise epilogue's rows."""
    for n in (1, 129, 300):
        case = C.case_of((300, 8, 12, 7), n)
        num, s32, s16, aux, aux16, proj = _operands(case, gpu)
        s = _dequant(s16, aux16, proj.kp)
        pch = W.orthonormal_rows(1, 300, seed=300 + n)
        pc = _dev(pch, gpu)
        sif_row = torch.empty((n, 300), device=gpu)
        row = P.mm2_project(s16, num, aux16, proj, pc=pc, sif_out=sif_row)
        sif_tile = _off(torch.empty((n, 300), device=gpu), 1)
        tile = P.mm2_project(s16, num, aux16, proj, pc=pc, sif_out=sif_tile)
        for got in (row, tile):
            _check_rows(7, "x3 at D=300", case, got, s, num, aux16, proj, x3=True)
        _check_removed(case, sif_row, num, pch, gpu)
        _check_removed(case, sif_tile.contiguous(), num, pch, gpu)
        assert M.row_rel_err(tile.cpu().numpy(), row.cpu().numpy()) < 1e-6


# ------------------------------------------------------------------ 8: mmb_calc_weights
@pytest.mark.parametrize("f", [1, 3, 76, 301])
def test_calc_weights_widths(gpu, f):
    """d = x - b is one rounding; e = expf(2 b_ls) is within 2 ulp; q_mean = d / e
    one more: 6 * 2^-24 relative, held to 8.  q_sigma = d * d / e - 1: 9 * 2^-24
    of d^2 / e before the subtraction (held to 10), whose own rounding is 2^-24 of
    the result (held to 2)."""
    worst = 0.0
    for rows in (1, 257, 5000):
        rng = np.random.default_rng(1000 * rows + f)
        x = rng.uniform(-1, 1, (rows, f)).astype(np.float32)
        b = (0.1 * rng.standard_normal(f)).astype(np.float32)
        ls = (0.1 * rng.standard_normal(f)).astype(np.float32)
        qm, qs = P.calc_weights(_dev(x, gpu), _dev(b, gpu), _dev(ls, gpu))
        d, e = x.astype(np.float64) - b, np.exp(2.0 * ls.astype(np.float64))
        rm, rsq = d / e, d * d / e
        e1 = _note(8, "q_mean", _frac(np.abs(qm.cpu().numpy() - rm), 8 * C.U * np.abs(rm)))
        e2 = _note(8, "q_sigma", _frac(np.abs(qs.cpu().numpy() - (rsq - 1.0)),
                                       10 * C.U * rsq + 2 * C.U * np.abs(rsq - 1.0)))
        worst = max(worst, e1, e2)
        assert e1 <= 1.0 and e2 <= 1.0, (rows, e1, e2)
    print(f"f={f}: largest error {worst:.3f} of its bar")


# ------------------------------------------------------------------ 9 / 10: the steps
@pytest.mark.parametrize("case", C.NARROW_FUSED, ids=C.shape_id)
def test_narrow_fused_widths(gpu, case):
    D, A, Vd, T, N, V = case
    inp, nets = _device_inputs(case, gpu), _networks(case, gpu)
    if not P.narrow_fused_supported(T, D, A, Vd, V):
        # past the kernel's K limit: the step keeps the stream kernel + x3 projection
        assert ((2 * A + 31) // 32 + (2 * Vd + 31) // 32) * 32 > 256
        step = P.FusedStep(inp, nets, narrow_fused=True)
        assert step.plan.front == "stream" and step.plan.s_half
        _, m = step.run(check=True)
        e = _note(9, "two-kernel step vs oracle (of 1e-5)",
                  M.row_rel_err(m.cpu().numpy(), C.oracle_rows(case)) / TOL)
        assert e < 1.0
        return
    a = P.FusedStep(inp, nets, narrow_fused=True, gram_kind="i8")
    b = P.FusedStep(inp, nets, narrow_fused=False, gram_kind="i8")
    assert a.narrow_fused and not b.narrow_fused and a.gram_i8 and b.gram_i8
    s1, m1 = [t.clone() for t in a.run()]
    s2, m2 = b.run()
    torch.cuda.synchronize()
    assert int(a.flag.item()) == int(b.flag.item()) == 0
    assert torch.equal(a.aux[0], b.aux[0])
    assert torch.allclose(a.aux[1], b.aux[1], rtol=1e-6, atol=0)
    ex = _note(9, "x vs two-kernel (of 2e-6)", M.row_rel_err(a.x.cpu().numpy(), b.x.cpu().numpy()) / 2e-6)
    assert torch.equal(a.colmax, P.colmax(a.x))  # bit-equal bounds
    em = _note(9, "MMB2 vs two-kernel (of 1e-6)", M.row_rel_err(m1.cpu().numpy(), m2.cpu().numpy()) / 1e-6)
    print(f"x {ex:.3f} of 2e-6, MMB2 rows {em:.3f} of 1e-6 against the two-kernel step")
    assert ex < 1.0 and em < 1.0
    if N > 1:  # (the reference's gpu2 cannot take one utterance)
        eo = _note(9, "MMB2 vs oracle (of 1e-5)", M.row_rel_err(m1.cpu().numpy(), C.oracle_rows(case)) / TOL)
        assert eo < 1.0
        xmax = a.x.abs().max().item()
        assert (s1 - s2).abs().max().item() <= 1e-6 * xmax


@pytest.mark.parametrize("fork", [True, False], ids=["forked", "fused-removal"])
@pytest.mark.parametrize("dims", C.STEP, ids=C.shape_id)
def test_fused_step_glove_widths(gpu, dims, fork):
    case = C.case_of(dims[:4], dims[4])
    step = P.FusedStep(_device_inputs(case, gpu), _networks(case, gpu), fork_projection=fork)
    p = step.plan
    assert p.front == "stream" and p.s_half and not p.split and p.gram == "f64"
    assert p.project == ("fork" if fork else "remove") and (step.fork is not None) == fork
    trace = {}
    sif, mm2 = step.run(trace=trace, check=True)
    assert ("mm2_project" if fork else "mm2_project+pc_remove") in trace
    _check_step(case, step, sif, mm2)


def test_fused_step_glove_width_graph_replay(gpu):
    case = C.case_of(C.STEP[0][:4], C.STEP[0][4])
    step = P.FusedStep(_device_inputs(case, gpu), _networks(case, gpu))
    sif, mm2 = [t.clone() for t in step.run(check=True)]
    g = P.StepGraph(step)
    for _ in range(2):
        s1, m1 = g.run(check=True)
    assert torch.equal(s1, sif) and torch.equal(m1, mm2)
    _check_step(case, step, s1, m1)


@pytest.mark.parametrize("dims", C.STEP_WIDE, ids=C.shape_id)
def test_fused_step_ldw_384(gpu, dims):
    """D = 320 and 380 (the widest width % 4 == 0 of ldw 384): the fp32-MFMA
    projection at CT = 6, whose MMB2 rows no other test reads."""
    case = C.case_of(dims[:4], dims[4])
    step = P.FusedStep(_device_inputs(case, gpu), _networks(case, gpu))
    assert step.plan.front == "stream" and not step.plan.s_half and step.plan.project == "chunk"
    sif, mm2 = step.run(check=True)
    _check_step(case, step, sif, mm2)


def test_fused_step_d382_names_the_stream_limit(gpu):
    """D = 382 fits the projection (ldw 384) but not the stream kernels
    (382 % 4 != 0: scalar rows, at most 320 wide): MMBError before any launch."""
    case = C.case_of((382, 8, 12, 7), 6)
    step = P.FusedStep(_device_inputs(case, gpu), _networks(case, gpu))
    with pytest.raises(L.MMBError, match="text width 382 is past the stream kernels' limit"):
        step.run()


@pytest.mark.parametrize("dims", C.DROP_IN, ids=C.shape_id)
def test_drop_in_glove_widths(gpu, dims):
    """sif2.estimate_embedding_overall_gpu2 at D = 50 (the wave / scalar
    workgroup kernels), D = 50 at T = 130 with 16 rows (the split stream) and
    D = 100 with L = 9 != T = 20 (the mmb_sif_wavg branch)."""
    D, A, Vd, T, N, Lw = dims
    case = C.case_of(dims[:4], N)
    z = C.inputs(case)
    t_ = lambda a: _dev(a, gpu)
    if Lw == T:
        emb, sw = z["text"], z["sw"]
    else:
        ids = np.ascontiguousarray(z["ids"][:, :Lw])
        emb, sw = z["E"][ids], z["wt32"][ids]
    data = {k: t_(v) for k, v in M.concat_inputs(z["text"], z["audio"], z["visual"]).items()}
    nets = _networks(case, gpu)
    with torch.no_grad():
        cs = sif2.estimate_embedding_overall_gpu2(data, {k: None for k in data}, nets, t_(sw),
                                                  data["text"] if Lw == T else t_(emb))
    assert cs.shape == (N, D) and cs.dtype == torch.float32
    ref = M.estimate_embedding_overall_gpu2(M.concat_inputs(z["text"], z["audio"], z["visual"]),
                                            C.params(D, A, Vd), sw, emb)
    e = _note(10, "drop-in vs oracle (of 1e-5)", M.row_rel_err(cs.cpu().numpy(), ref) / TOL)
    print(f"{C.shape_id(dims)}: {e:.3f} of 1e-5")
    assert e < 1.0
