"""What the GPU tests of the MMB2 stream, projection and step kernels share
(tests/test_gpu_mmb2_widths.py, tests/test_gpu_scratch.py,
tests/test_gpu_large.py, tests/test_gpu_split.py,
tests/test_gpu_split_frames16.py, tests/test_gpu_frames16.py,
tests/test_gpu_table16.py): device copies of a case of tests/mmb2_cases.py,
one stream launch of it, which launches take the narrow-frame route, the
device's own projection operands, the POM-length inputs, and the checkers that hold stream outputs, projected rows, removed
rows and a whole step to mmb2_cases' bars.  Plain helper module: no test is
collected from it.

A checker records every comparison through the `note(group, what, fraction)`
its caller hands it, so each lands in the calling module's report.
"""
import functools

import numpy as np
import torch

import mmb2_cases as C
import pipeline as P
import synth
from common_gpu import F32_ROW, TOL, _colmax_bufs, _dev, _frac, _off
from oracle import mmb2_oracle as M
from oracle import sif_oracle as O

MODES = ("ids+table", "ids+w", "dense", "dense+emb2")


@functools.lru_cache(maxsize=None)
def _ref(case, emb2=False):
    z = C.inputs(case)
    return C.stream_reference(z["text"], z["emb2"] if emb2 else z["text"], z["sw"], z["audio"],
                              z["visual"])


def _text_args(z, mode, gpu, table_off=False):
    if mode.startswith("ids"):
        table = _dev(z["E"], gpu)
        kw = {"ids32": _dev(z["ids"], gpu, torch.int32), "table": _off(table, 1) if table_off else table}
        if mode == "ids+table":
            kw["wtab32"] = _dev(z["wt32"], gpu)
        else:
            kw["w_dense"] = _dev(z["sw"], gpu)
        return kw
    text = _dev(z["text"], gpu)
    return {"text_dense": text, "emb_dense": _dev(z["emb2"], gpu) if mode == "dense+emb2" else text,
            "w_dense": _dev(z["sw"], gpu)}


def _stream(case, mode, gpu, s_half, colmax=False, table_off=False, split_parts=None):
    """One launch of the case in `mode`; returns (num, s, aux, colmax bits or None) as numpy."""
    D, A, Vd, T, N, V = case
    z = C.inputs(case)
    au, vi = _dev(z["audio"], gpu), _dev(z["visual"], gpu)
    cm, ws = _colmax_bufs(D, gpu) if colmax else (None, None)
    kw = _text_args(z, mode, gpu, table_off)
    if split_parts is not None:
        kw.update(split=P.split_ws(N, T, D, A, Vd, gpu, parts=split_parts), parts=split_parts)
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    num, s, aux = P.mm2_stream(N, T, D, A, Vd, au, vi, s_half=s_half, flag=flag, colmax=cm,
                               colmax_ws=ws, **kw)
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    return (num.cpu().numpy(), s.cpu().numpy(), aux.cpu().numpy(),
            None if cm is None else cm.cpu().numpy().view(np.float32))


def _check_stream(note, group, case, out, ref, s_half, twin=None):
    """The outputs of one stream launch against f64 numpy (`ref`); `twin`: the
    fp32 s of the same launch route, which the fp16 planes must dequantise to."""
    D, A, Vd, T, N, V = case
    num, s, aux, cm = out
    K, kp = 2 * (D + A + Vd), (2 * (D + A + Vd) + 31) // 32 * 32
    assert np.array_equal(aux[0], ref["cnt"])  # the count is exact
    fr = [note(group, "weight sum", _frac(np.abs(aux[1] - ref["sw"]), C.sum_bar(T, ref["sw_abs"]))),
          note(group, "x", _frac(np.abs(num - ref["x"]), C.sum_bar(T, ref["x_abs"])))]
    if cm is not None:  # the bounds: max |x| of the device's own x, bit for bit
        assert np.array_equal(cm, np.abs(num).max(0))
    sbar = C.sum_bar(T, ref["s_abs"])
    if not s_half:
        assert s.dtype == np.float32 and s.shape == (N, kp)
        assert not s[:, K:].any()  # pad columns exactly 0
        fr.append(note(group, "s (fp32)", _frac(np.abs(s[:, :K] - ref["s"]), sbar)))
        assert np.array_equal(aux[2], C.row_scale_of(np.abs(s).max(1)))
    else:
        assert s.dtype == np.float16 and s.shape == (N, 2 * kp)
        assert not s[:, K:kp].any() and not s[:, kp + K:].any()
        rs = aux[2].astype(np.float64)[:, None]
        q = s[:, :K].astype(np.float64) + s[:, kp:kp + K].astype(np.float64)
        # hi + lo of s * aux[2]: 2^-21 of the element plus the fp16 subnormal step
        tol = 2.0 ** -21 * np.abs(ref["s"] if twin is None else twin[:, :K]) + 2.0 ** -25 / rs
        if twin is None:  # no fp32 launch on this route: against f64 with the sums' own bar
            fr.append(note(group, "s (fp16 hi + lo)", _frac(np.abs(q / rs - ref["s"]), sbar + tol)))
        else:
            fr.append(note(group, "s (fp16 hi + lo vs fp32)", _frac(np.abs(q / rs - twin[:, :K]), tol)))
            assert np.array_equal(aux[2], C.row_scale_of(np.abs(twin).max(1)))
        # aux[2] is the power of two that puts max |s| into [2^14, 2^15) (the
        # planes' sum is within the lo plane's rounding, 2^-8, of s * aux[2])
        m = np.abs(q).max(1)
        assert np.array_equal(np.frexp(aux[2])[0], np.full(N, 0.5, np.float32))
        assert ((m >= 2.0 ** 14 - 2.0 ** -8) & (m <= 2.0 ** 15 + 2.0 ** -8)).all()
    assert max(fr) <= 1.0, fr
    return max(fr)


def _is_narrow_route(case, mode, s_half):
    """Whether mmb_mm2_stream takes the case on utt_narrow_kernel (ids + weight table, fp16 s)."""
    D, A, Vd, T, N, V = case
    return (mode == "ids+table" and s_half and 256 < D <= 512 and max(A, Vd) <= 128 and T <= 64
            and D % 4 == A % 4 == Vd % 4 == 0)


# ------------------------------------------------------------------ the projections
def _operands(case, gpu):
    """The device's own stream outputs of the case (ids + weight table), fp32
    and fp16 s, and its merged projection."""
    D, A, Vd, T, N, V = case
    z = C.inputs(case)
    proj = P.MMB2Projection(C.generator(D, A, Vd).networks(), D, A, Vd, T, gpu)
    if D % 4 and D > P.STREAM_MAX_SCALAR_WIDTH:
        # past the scalar stream kernel (D = 382, 383): the f64 sums rounded to f32, uploaded
        ref = _ref(case)
        s = np.zeros((N, proj.kp), np.float32)
        s[:, :ref["s"].shape[1]] = ref["s"]
        aux = np.stack([ref["cnt"], ref["sw"], C.row_scale_of(np.abs(s).max(1))]).astype(np.float32)
        return _dev(ref["x"].astype(np.float32), gpu), _dev(s, gpu), None, _dev(aux, gpu), None, proj
    au, vi = _dev(z["audio"], gpu), _dev(z["visual"], gpu)
    kw = _text_args(z, "ids+table", gpu)
    num, s32, aux = P.mm2_stream(N, T, D, A, Vd, au, vi, s_half=False, **kw)
    _, s16, aux16 = P.mm2_stream(N, T, D, A, Vd, au, vi, s_half=True, **kw)
    torch.cuda.synchronize()
    return num, s32, s16, aux, aux16, proj


def _check_rows(note, group, what, case, got, s, num, aux, proj, x3):
    """Projected rows against f64 of the device's own operands (the stage bar
    AND the flat 1e-5) and against the oracle (1e-5)."""
    D, A, Vd, T, N, V = case
    K = 2 * (D + A + Vd)
    rows, bar = C.project_reference(s, num.cpu().numpy(), aux.cpu().numpy(), proj.wm.cpu().numpy(),
                                    proj.c0.cpu().numpy(), D, K, x3=x3)
    got = got.cpu().numpy().astype(np.float64)
    err = np.abs(got - rows).max(1) / np.abs(rows).max(1)
    e = note(group, what + " (of beta)", (err / bar).max())
    f = note(group, what + " (of 1e-5)", err.max() / TOL)
    o = note(group, what + " vs oracle (of 1e-5)", M.row_rel_err(got, C.oracle_rows(case)) / TOL)
    assert e <= 1.0 and f < 1.0 and o < 1.0, (C.shape_id(case), e, f, o)
    return max(e, f, o)


def _dequant(s16, aux16, kp):
    s = s16.cpu().numpy().astype(np.float64)
    return (s[:, :kp] + s[:, kp:]) / aux16.cpu().numpy().astype(np.float64)[2][:, None]


def _check_removed(note, case, sif, num, pch, gpu):
    """The fused removal's rows: one f32 rounding of x - (x . pc) pc in f64, as
    mmb_pc_remove's of the same x."""
    x = num.double().cpu().numpy()
    ref = x - (x @ pch.T) @ pch
    rmax = np.abs(ref).max(axis=1, keepdims=True)
    sep = P.remove_pc(num, None, _dev(pch, gpu), torch.float32).cpu().numpy()
    e1 = note(7, "fused removal (of 2^-23)", (np.abs(sif.cpu().numpy() - ref) / rmax).max() / F32_ROW)
    e2 = note(7, "mmb_pc_remove (of 2^-23)", (np.abs(sep - ref) / rmax).max() / F32_ROW)
    assert e1 <= 1.0 and e2 <= 1.0, (C.shape_id(case), e1, e2)


# ------------------------------------------------------------------ the steps
def _device_inputs(case, gpu):
    z = C.inputs(case)
    return {"table": _dev(z["E"], gpu), "wtab": _dev(z["wt32"], gpu),
            "ids": _dev(z["ids"], gpu, torch.int32), "audio": _dev(z["audio"], gpu),
            "visual": _dev(z["visual"], gpu)}


def _check_step(note, case, step, sif, mm2):
    x = step.x.double().cpu().numpy()
    eo = note(10, "MMB2 rows vs oracle (of 1e-5)",
              M.row_rel_err(mm2.cpu().numpy(), C.oracle_rows(case)) / TOL)
    ep = note(10, "PC (of 1e-10)", np.abs(step.pc.cpu().numpy() - O.compute_pc(x, 1)).max() / 1e-10)
    ref = O.remove_pc(x, 1)
    es = note(10, "SIF rows (of 2^-23)",
              (np.abs(sif.cpu().numpy() - ref) / np.abs(ref).max(axis=1, keepdims=True)).max() / F32_ROW)
    print(f"{C.shape_id(case)} plan {step.plan.front}/{step.plan.project}: MMB2 {eo:.3f} of 1e-5, "
          f"PC {ep:.3f} of 1e-10, SIF rows {es:.3f} of 2^-23")
    assert eo < 1.0 and ep < 1.0 and es <= 1.0


# ------------------------------------------------------------------ the long transcripts
def _pom(golden, case, n, A, Vd, seed, dev):
    """The reference's own POM split ids (pom_valid_ids 100 x 1089 /
    pom_test_ids 203 x 1357, g11) and weights, the seeded V = 7763 table,
    word-aligned frames set to -10 past each transcript's last token."""
    z = golden("g11_pom_splits")
    ids = z[f"{case}_ids"][:n]
    N, T = ids.shape
    E = synth.word_table(len(z["weights"]), 300, seed=int(z["table_seed"]))
    last = np.where(ids != 0, np.arange(T)[None, :], -1).max(1)
    pad = np.arange(T)[None, :] > last[:, None]
    audio = synth.frames(N, T, A, seed=seed)
    visual = synth.frames(N, T, Vd, seed=seed + 1)
    audio[pad] = -10.0
    visual[pad] = -10.0
    inp = {"table": torch.tensor(E, device=dev),
           "wtab": torch.tensor(z["weights"], device=dev, dtype=torch.float32),
           "ids": torch.as_tensor(ids, dtype=torch.int32, device=dev),
           "audio": torch.tensor(audio, device=dev), "visual": torch.tensor(visual, device=dev)}
    return inp, (E, z["weights"], ids, audio, visual)
