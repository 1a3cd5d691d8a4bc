"""GPU: the MMB2 stream kernels on audio / visual frames kept in fp16 / bf16
storage (mmb_mm2_stream_ft, pipeline.mm2_stream, FusedStep).

The widening of a 16-bit frame value to f32 is exact and the kernels sum the
widened values with the statements, and in the order, of their f32
instantiations.  So the definition under test is an equality: a launch on
16-bit frames writes, bit for bit, what the same launch writes on those frames
upcast to f32 by the caller -- x, s, aux and the column bounds of the stream
kernels (A), and x, aux, PC, SIF and MMB2 rows of the step (C).  Where the
f32 twin would take a kernel the 16-bit types never take (the narrow-frame
route, the fused fronts, the split stream) the twin is steered onto the same
kernel; the one step whose twin cannot be (its stream kernel is the
narrow-frame route) holds the MMB2 rows to the 1e-6 row-relative bar
tests/test_gpu_mmb2_widths.py::test_narrow_fused_widths uses between those two
sum orders.  The steps are also held to the oracle on the upcast inputs with
the suite's bars (MMB2 rows 1e-5, PC 1e-10, SIF rows 2^-23);
tests/test_frames16_cases.py pins the family's conditions on those inputs.
Product library only.
"""
import numpy as np
import pytest
import torch

import frames16_cases as F
import mmb2_cases as C
import mmb_lib as L
import pipeline as P
from frames16_gpu import (TWIN, _assert_graph_replays, _bufs, _check_oracle, _colmax_bufs, _dev, _networks, _off,
                          _run, _step_inputs, _untouched)
from mmb2_gpu import _is_narrow_route
from oracle import mmb2_oracle as M

pytestmark = pytest.mark.gpu

MODES = ("ids+table", "ids+w")
KIND_IDS = list(F.KINDS)


class _Launcher:
    """The device copies of one case's text inputs, and stream launches on them."""

    def __init__(self, case, gpu):
        self.case, self.gpu = case, gpu
        z = C.inputs(case)
        self.text = {"ids32": _dev(z["ids"], gpu, torch.int32), "table": _dev(z["E"], gpu)}
        self.wtab, self.sw = _dev(z["wt32"], gpu), _dev(z["sw"], gpu)

    def __call__(self, au, vi, mode, s_half, colmax):
        """(x, s, aux, colmax bits or None) as numpy, flag checked clear."""
        D, A, Vd, T, N, V = self.case
        kw = dict(self.text, **({"wtab32": self.wtab} if mode == "ids+table" else {"w_dense": self.sw}))
        cm, ws = _colmax_bufs(D, self.gpu) if colmax else (None, None)
        flag = torch.zeros(1, dtype=torch.int32, device=self.gpu)
        num, s, aux = P.mm2_stream(N, T, D, A, Vd, au, vi, s_half=bool(s_half), flag=flag, colmax=cm,
                                   colmax_ws=ws, **kw)
        torch.cuda.synchronize()
        assert int(flag.item()) == 0
        return (num.cpu().numpy(), s.cpu().numpy(), aux.cpu().numpy(),
                None if cm is None else cm.cpu().numpy().view(np.uint32))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint16)


def _equal(got, twin, what):
    for name, g, t in zip(("x", "s", "aux", "colmax"), got, twin):
        if g is None:
            assert t is None
            continue
        assert g.dtype == t.dtype and g.shape == t.shape, (what, name)
        # np.array_equal on the values (no NaN in these inputs) ...
        assert np.array_equal(g, t), (what, name)
        # ... and on the bits, so that +0 / -0 count as different
        assert np.array_equal(_bits(g), _bits(t)), (what, name, "bits")


def _sweep(case, gpu, frames16=None, off16=0, off32=0):
    """Both kinds x (ids+table, ids+w) x s_half x colmax: the launch on the
    16-bit frames against the f32 launch on their upcast.  `off16` / `off32`:
    the frame tensors that many elements past a 16-byte boundary."""
    run = _Launcher(case, gpu)
    n = 0
    for kind in F.KINDS:
        a16, v16 = (frames16 or F.frames)(case, kind)
        au16, vi16 = (_off(_dev(t, gpu), off16) for t in (a16, v16))
        au32, vi32 = (_off(_dev(t, gpu).float(), off32) for t in (a16, v16))
        assert au16.dtype == F.KINDS[kind] and au32.dtype == torch.float32
        for mode in MODES:
            for s_half in (0, 1):
                # the f32 twin on the narrow-frame route sums the frames in another
                # order: given the gathered weights it stays on the wave kernel
                twin_mode = "ids+w" if _is_narrow_route(case, mode, s_half) and not off32 else mode
                for colmax in (False, True):
                    got = run(au16, vi16, mode, s_half, colmax)
                    twin = run(au32, vi32, twin_mode, s_half, colmax)
                    _equal(got, twin, (C.shape_id(case), kind, mode, s_half, colmax))
                    n += 1
    return n


# ------------------------------------------------------------------ A: stream outputs, bit for bit
@pytest.mark.parametrize("shape", C.WAVE_D256 + C.WAVE_D512 + C.NARROW_ROUTE, ids=C.shape_id)
def test_wave_kernel_bit_for_bit(gpu, shape):
    assert _sweep(C.case_of(shape), gpu) == 16


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
def test_frames_8_bytes_off_stay_on_the_wave_kernel(gpu, shape):
    """A 16-bit column unit is 8 bytes: frames 8 bytes past a 16-byte boundary
    are still whole units (the f32 twin, aligned, is the wave kernel)."""
    _sweep(C.case_of(shape), gpu, off16=4)


def test_frames_2_bytes_off_take_the_scalar_frame_route(gpu):
    """2 bytes off: the workgroup kernel with scalar frame loads -- as the f32
    twin whose frames are 4 bytes off."""
    _sweep(C.case_of((52, 8, 12, 7)), gpu, off16=1, off32=1)


@pytest.mark.parametrize("shape", F.SPECIAL_SHAPES, ids=C.shape_id)
def test_special_values(gpu, shape):
    """Trailing -10 pad frames, +-0, the smallest subnormal, the largest finite
    fp16 value; for bf16 a subnormal and 2^40 -- on the wave kernel (52, 8,
    12, 7) and the scalar workgroup kernel (50, 5, 3, 9)."""
    case = C.case_of(shape)
    _sweep(case, gpu, frames16=F.special_frames)
    # the planted values reached the sums: the largest one squared dominates its column
    run = _Launcher(case, gpu)
    D, A, Vd, T, N, V = case
    for kind in F.KINDS:
        a16, v16 = F.special_frames(case, kind)
        x, s, aux, _ = run(_dev(a16, gpu), _dev(v16, gpu), "ids+table", 0, False)
        big = float(F.SPECIALS[kind][-1][0])
        assert np.isfinite(s).all()
        assert s[0, 2 * D + A] >= np.float32(big) ** 2 and s[1, 2 * (D + A) + Vd + Vd - 1] >= np.float32(big) ** 2
        # and row 2 saw its pad frames: -10 each among T - 2 values of [-1, 1]
        pads = F.SPECIAL_PADS
        assert s[2, 2 * D] <= -10.0 * pads + (T - pads) and s[2, 2 * D + A] >= 100.0 * pads


# ------------------------------------------------------------------ B: rejections, outputs untouched
def _sentinel_out(N, D, kp, s_half, gpu):
    num = torch.full((N, D), -7.0, device=gpu)
    s = P.s_buffer(N, kp, s_half, gpu).fill_(-7.0)
    aux = torch.full((3, N), -7.0, device=gpu)
    return num, s, aux


def test_mirror_rejections_leave_the_outputs_untouched(gpu):
    case = C.case_of((52, 8, 12, 70), 4)
    D, A, Vd, T, N, V = case
    z = C.inputs(case)
    kp = L.query("mmb_mm2_k", D, A, Vd)
    ids, table, wtab = _dev(z["ids"], gpu, torch.int32), _dev(z["E"], gpu), _dev(z["wt32"], gpu)
    text, sw = _dev(z["text"], gpu), _dev(z["sw"], gpu)
    a32, v32 = _dev(z["audio"], gpu), _dev(z["visual"], gpu)
    gather = dict(ids32=ids, table=table, wtab32=wtab)
    for s_half in (False, True):
        out = _sentinel_out(N, D, kp, s_half, gpu)
        for kind, dt in F.KINDS.items():
            au, vi = a32.to(dt), v32.to(dt)
            with pytest.raises(L.MMBError, match="gathered text"):
                P.mm2_stream(N, T, D, A, Vd, au, vi, text_dense=text, emb_dense=text, w_dense=sw,
                             s_half=s_half, out=out)
            with pytest.raises(L.MMBError, match="split stream reads float32 frames only"):
                P.mm2_stream(N, T, D, A, Vd, au, vi, s_half=s_half, out=out,
                             split=P.split_ws(N, T, D, A, Vd, gpu, parts=2), parts=2, **gather)
            with pytest.raises(L.MMBError, match="one dtype"):
                P.mm2_stream(N, T, D, A, Vd, au, v32, s_half=s_half, out=out, **gather)
            with pytest.raises(L.MMBError, match="one dtype"):
                P.mm2_stream(N, T, D, A, Vd, a32, vi, s_half=s_half, out=out, **gather)
        with pytest.raises(L.MMBError, match="one dtype"):
            P.mm2_stream(N, T, D, A, Vd, a32.to(torch.float16), v32.to(torch.bfloat16), s_half=s_half,
                         out=out, **gather)
        with pytest.raises(L.MMBError, match="float32, float16 or bfloat16"):
            P.mm2_stream(N, T, D, A, Vd, a32.double(), v32.double(), s_half=s_half, out=out, **gather)
        assert _untouched(out)


def test_fused_fronts_reject_16_bit_frames(gpu):
    case = C.NARROW_FUSED[1]  # (260, 76, 48, 20, 31, 3016): both fused fronts take the shape at f32
    D, A, Vd, T, N, V = case
    assert P.stream_project_supported(T, D, A, Vd) and P.narrow_fused_supported(T, D, A, Vd, V)
    z = C.inputs(case)
    proj = P.MMB2Projection(_networks(case, gpu), D, A, Vd, T, gpu)
    ids, table, wtab = _dev(z["ids"], gpu, torch.int32), _dev(z["E"], gpu), _dev(z["wt32"], gpu)
    au, vi = _dev(z["audio"], gpu).bfloat16(), _dev(z["visual"], gpu).bfloat16()
    out = _bufs(N, D, gpu, bounds=False, fill=-7.0)[0]
    with pytest.raises(L.MMBError, match="mm2_stream_project reads float32 frames only"):
        P.mm2_stream_project(N, T, D, A, Vd, au, vi, proj, ids32=ids, table=table, wtab32=wtab, out=out)
    with pytest.raises(L.MMBError, match="mm2_stream_project_narrow reads float32 frames only"):
        P.mm2_stream_project_narrow(N, T, D, A, Vd, au, vi, proj, ids, table, wtab, out=out)
    assert _untouched(out)


# ------------------------------------------------------------------ C: the step
@pytest.mark.parametrize("kind", KIND_IDS)
@pytest.mark.parametrize("dims", F.STEP, ids=C.shape_id)
def test_fused_step_on_16_bit_frames(gpu, dims, kind):
    case = F.step_case(dims)
    D, A, Vd, T, N, V = case
    inp16, inp32 = _step_inputs(case, kind, gpu)
    nets = _networks(case, gpu)
    a = P.FusedStep(inp16, nets)
    b = P.FusedStep(inp32, nets, **TWIN)
    assert a.frames == kind and b.frames == "f32"
    assert a.plan.front == "stream" and a.plan.split is False and a.plan.frames == kind
    assert a.plan._replace(frames="f32") == b.plan
    # whatever the overrides allow, the 16-bit step keeps the plain stream kernel
    assert P.FusedStep(inp16, nets, stream_project=True, narrow_fused=True, split_stream=True).plan == a.plan
    s1, m1 = _run(a)
    s2, m2 = _run(b)
    assert torch.equal(a.x, b.x) and torch.equal(a.aux, b.aux) and torch.equal(a.pc, b.pc)
    assert torch.equal(s1, s2)
    if tuple(dims) == F.STEP_NARROW_TWIN:
        # the twin's stream kernel is the narrow-frame route (another order of
        # the frame sums): the bar of test_narrow_fused_widths between the two
        e = M.row_rel_err(m1.cpu().numpy(), m2.cpu().numpy())
        print(f"MMB2 rows vs the narrow-route twin: {e:.2e} (bar 1e-6)")
        assert e < 1e-6
    else:
        assert torch.equal(m1, m2)
    _check_oracle(case, kind, a, s1, m1)


def test_step_graph_replays_the_bf16_step(gpu):
    case = F.step_case(F.STEP[0])
    inp16, _ = _step_inputs(case, "bf16", gpu)
    _assert_graph_replays(P.FusedStep(inp16, _networks(case, gpu)))


@pytest.mark.parametrize("kind", KIND_IDS)
def test_chunked_step_on_16_bit_frames(gpu, kind):
    case = F.step_case(F.CHUNKED)
    inp16, inp32 = _step_inputs(case, kind, gpu)
    nets = _networks(case, gpu)
    a = P.FusedStep(inp16, nets, chunks=3)
    b = P.FusedStep(inp32, nets, chunks=3, **TWIN)
    assert len(a.bounds) == 3 and a.plan._replace(frames="f32") == b.plan and a.plan.frames == kind
    s1, m1 = _run(a)
    s2, m2 = _run(b)
    assert torch.equal(a.x, b.x) and torch.equal(a.aux_flat, b.aux_flat) and torch.equal(a.pc, b.pc)
    assert torch.equal(s1, s2) and torch.equal(m1, m2)
