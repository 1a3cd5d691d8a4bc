"""What the GPU tests of the 16-bit frame fronts and word tables share
(tests/test_gpu_frames16.py, tests/test_gpu_fused_frames16.py,
tests/test_gpu_narrow_frames16.py, tests/test_gpu_split_frames16.py,
tests/test_gpu_table16.py, tests/test_gpu_fused_table16.py): the device copies
of tests/common_gpu.py under their names, the buffers and the launch of a
fused front, the launch on 16-bit frames beside its f32 twin and their
bit-for-bit comparison, and the two-kernel step's twin inputs, twin keywords
and oracle check.  Plain helper module: no test is collected from it.
"""
import numpy as np
import torch

import frames16_cases as F
import mmb2_cases as C
import models
import pipeline as P
import synth
from common_gpu import F32_ROW, TOL, _colmax_bufs, _dev, _i32, _networks, _off, _untouched  # noqa: F401  (passed on)
from oracle import mmb2_oracle as M
from oracle import sif_oracle as O

# the f32 twin of a step on 16-bit storage: the plain stream kernel + projection
TWIN = dict(stream_project=False, narrow_fused=False, split_stream=False)


# ------------------------------------------------------------------ the fused fronts
def _bufs(N, D, gpu, bounds=True, fill=None):
    """(out, flag, colmax, colmax_ws) of one launch of a fused front."""
    mk = (lambda *s: torch.empty(s, device=gpu)) if fill is None else (lambda *s: torch.full(s, fill, device=gpu))
    colmax, ws = _colmax_bufs(D, gpu) if bounds else (None, None)
    return (mk(N, D), mk(3, N), mk(N, D)), torch.zeros(1, dtype=torch.int32, device=gpu), colmax, ws


def _launch(front, dims, audio, visual, proj, text, gpu, bounds=True):
    """(x, aux, mmb2, colmax or None, flag word) of a fused kernel through the mirror `front`."""
    D, A, Vd, T, N = dims
    out, flag, colmax, ws = _bufs(N, D, gpu, bounds)
    x, aux, m = front(N, T, D, A, Vd, audio, visual, proj, ids32=text["ids"], table=text["table"],
                      wtab32=text["wtab"], flag=flag, out=out, colmax=colmax, colmax_ws=ws)
    torch.cuda.synchronize()
    return x, aux, m, colmax, int(flag.item())


def _assert_bit_for_bit(got, twin, what, nan_rows=False):
    for name, g, t in zip(("x", "aux", "mmb2", "colmax"), got, twin):
        if g is None or t is None:  # the bounds: asked for on both sides or on neither
            assert g is None and t is None, (what, name)
            continue
        assert g.dtype == t.dtype and g.shape == t.shape, (what, name)
        # on the bits, so that +0 / -0 count as different ...
        assert torch.equal(_i32(g), _i32(t)), (what, name, "bits")
        # ... and on the values (a NaN fails here); a zero-weight utterance's x row is
        # 0 / 0 (nan_rows): there the values are compared beside the NaNs, which the
        # bits cover
        if nan_rows and g.is_floating_point():
            assert torch.equal(torch.isnan(g), torch.isnan(t)), (what, name, "NaN places")
            g, t = g[~torch.isnan(g)], t[~torch.isnan(t)]
        assert torch.equal(g, t), (what, name)
    assert got[4] == twin[4], (what, "flag", got[4], twin[4])


def _pair(fronts, dims, a16, v16, proj, text, gpu, what, bounds=True, nan_rows=False):
    """The launch on the 16-bit frames through fronts[0] and its f32 twin, on
    their upcast, through fronts[1]."""
    got = _launch(fronts[0], dims, a16, v16, proj, text, gpu, bounds)
    twin = _launch(fronts[1], dims, a16.float(), v16.float(), proj, text, gpu, bounds)
    _assert_bit_for_bit(got, twin, what, nan_rows)
    return got


def _synth_case(D, A, Vd, T, N, V, kind, gpu):
    """A device workload with frames rounded to the kind (torch's round to
    nearest even: the caller's rounding), and the projection of a generator."""
    inp = synth.device_workload(N, T, V, D=D, A=A, Vd=Vd, seed=83, device=gpu, frame_dtype=F.KINDS[kind])
    assert inp["audio"].dtype == inp["visual"].dtype == F.KINDS[kind]
    torch.manual_seed(0)
    gen = models.AudioVisualGeneratorMultimodal(D, A, Vd, norm=None).to(gpu)
    return inp, P.MMB2Projection(gen.networks(), D, A, Vd, T, gpu)


# ------------------------------------------------------------------ the step
def _frames_of(case, kind, frames, gpu):
    """The case's frames on the device: f32, or rounded to the table's kind."""
    if frames == "f32":
        z = C.inputs(case)
        return _dev(z["audio"], gpu), _dev(z["visual"], gpu)
    return tuple(_dev(t, gpu) for t in F.frames(case, kind))


def _step_inputs(case, kind, gpu):
    """(the inputs with 16-bit frames, the same with their f32 upcast)."""
    z = C.inputs(case)
    a16, v16 = F.frames(case, kind)
    base = {"table": _dev(z["E"], gpu), "wtab": _dev(z["wt32"], gpu), "ids": _dev(z["ids"], gpu, torch.int32)}
    au, vi = _dev(a16, gpu), _dev(v16, gpu)
    return dict(base, audio=au, visual=vi), dict(base, audio=au.float(), visual=vi.float())


def _run(step):
    sif, mm2 = step.run(check=True)
    torch.cuda.synchronize()
    return sif, mm2


def _assert_graph_replays(step):
    """A StepGraph of `step`, replayed twice, gives the eager run's rows."""
    sif, mm2 = [t.clone() for t in step.run(check=True)]
    g = P.StepGraph(step)
    for _ in range(2):
        s1, m1 = g.run(check=True)
    assert torch.equal(s1, sif) and torch.equal(m1, mm2)


def _check_oracle(case, kind, step, sif, mm2):
    x = step.x.double().cpu().numpy()
    eo = M.row_rel_err(mm2.cpu().numpy(), F.oracle_rows(case, kind)) / TOL
    ep = np.abs(step.pc.cpu().numpy() - O.compute_pc(x, 1)).max() / 1e-10
    ref = O.remove_pc(x, 1)
    es = (np.abs(sif.cpu().numpy() - ref) / np.abs(ref).max(axis=1, keepdims=True)).max() / F32_ROW
    print(f"{C.shape_id(case)} {kind}: MMB2 {eo:.3f} of 1e-5, PC {ep:.3f} of 1e-10, SIF rows {es:.3f} of 2^-23")
    assert eo < 1.0 and ep < 1.0 and es <= 1.0
