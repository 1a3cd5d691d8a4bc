"""No kernel's output depends on what its scratch, its outputs or a derived
weight image held before the launch.

pipeline.py allocates every workspace and image with torch.empty, and the
training loops run the kernels out of a caching allocator that hands back
whatever the last tensor left.  A consumer that reads a slot no producer wrote
sees 0 on a fresh process -- the identity of every sum and max here -- and
wrong numbers later, with no flag.  Every test below runs one call three times:
with its scratch and outputs filled with the byte 0x00 (Z), 0xFF (N: NaN, -1)
and 0x7F (H: a huge finite f32 / f64, NaN in fp16); tests/scratch_cases.py
holds the patterns, the protected synchronisation words that are never
poisoned, and the case tables.  One assertion shape throughout:

  * the Z run twice is byte-identical to itself (the kernel is repeatable);
  * every output of the N and H runs is byte-identical to the Z run's, the
    flag word included; an output that `accumulate` adds to is preloaded with
    a known matrix instead of a pattern;
  * pad regions documented as zero are zero.

No tolerance is involved: the bar is the same kernel on clean scratch.  One Z
run per family is also held to the float64 bar of that family's own test
(through the family's checker in tests/mmb2_gpu.py, widths_gpu.py,
regressor_gpu.py or word_cases.py), so the baseline is not garbage, and
test_control_poison_reaches_the_output shows that both patterns are visible
through a reduction.  Each family prints one line per case, "<case>: N ok / H
ok"; the module prints at its end, per family and quantity, how many Z runs
were held to a bar and the largest fraction of it they reached.

Only the product library is loaded.
"""
import numpy as np
import pytest
import torch

import frames16_cases as F
import fused_cases as FC
import latent as LT
import mmb2_cases as C
import mmb2_gpu as MG
import mmb_lib as L
import models
import pipeline as P
import regressor_cases as R
import regressor_gpu as RG
import scratch_cases as S
import synth
import width_cases as W
import widths_gpu as WG
import word_cases as WC
from common_gpu import TOL, Ledger, _dev, _dev32, _networks
from oracle import mmb2_oracle as M
from oracle import sif_oracle as O

pytestmark = pytest.mark.gpu

U8 = torch.uint8

_WORST = Ledger()  # (family, what) -> [comparisons, largest error as a fraction of its bar]


def _note(family, what, value, bar=1.0):
    """The `note` handed to the families' checkers, (family, what, fraction) or
    (family, what, error, bar): the Z runs held to their family's float64 bars."""
    _WORST.note((str(family), what), value / bar)
    return float(value)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for (family, what), (n, frac) in sorted(_WORST.items()):
        print(f"\nscratch, Z run against family {family} {what}: {n} comparisons, largest {frac:.3f} of its bar",
              end="")
    print()


# ------------------------------------------------------------------ the engine
def _buf(shape, dtype, pattern, gpu, keep=()):
    """A device tensor whose bytes hold the pattern (zero in `keep`)."""
    return S.poison(torch.empty(shape, dtype=dtype, device=gpu), pattern, keep)


def _cpu(t):
    return t.detach().contiguous().cpu()


def _diff(a, b):
    a, b = S._bytes_of(a), S._bytes_of(b)
    if a.shape != b.shape:
        return f"{a.shape[0]} against {b.shape[0]} bytes"
    bad = torch.nonzero(a != b).flatten()
    return f"{bad.numel()} of {a.numel()} bytes differ, the first at byte {int(bad[0])}"


def _assert_same(label, what, ref, got):
    assert ref.keys() == got.keys(), (label, what)
    for k in ref:
        assert S.same_bytes(ref[k], got[k]), \
            f"{label}: {k} of the {what} run differs from the Z run ({_diff(ref[k], got[k])})"


def _sweep(label, run, report=True):
    """run(pattern) -> {name: host tensor}.  The Z run twice, then N and H;
    returns the Z run's outputs."""
    z = run("Z")
    _assert_same(label, "second Z", z, run("Z"))
    for p in S.POISONS:
        _assert_same(label, p, z, run(p))
    if report:
        print(f"{label}: N ok / H ok")
    return z


def _sync():
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the control
def test_control_poison_reaches_the_output(gpu):
    """mmb_gram_finish on a poisoned workspace with no mmb_gram_part before it:
    G comes back non-finite or non-zero, so both patterns are visible through a
    fixed-order reduction.  The read stays inside mmb_gram_workspace_bytes.  The
    only test here that expects poison in an output."""
    n_plan, d = S.GRAM_CONTROL
    nb = L.query("mmb_gram_workspace_bytes", n_plan, d)
    for p in S.POISONS:
        ws = _buf(nb, U8, p, gpu)
        G = torch.zeros((d, d), dtype=torch.float64, device=gpu)
        L.call("mmb_gram_finish", n_plan, d, L.ptr(G), 0, L.ptr(ws), L.stream_ptr())
        _sync()
        g = G.cpu().numpy()
        bad = ~np.isfinite(g) | (g != 0)
        print(f"control {p}: {int(bad.sum())} of {g.size} entries of G carry the poison")
        assert bad.all()


# ------------------------------------------------------------------ 1: Gram
def _gram_rows(n, d, gpu):
    num32 = W.x32(n, d).astype(np.float32)
    cnt32 = WG._counts(n, n + d)
    return num32, cnt32, _dev(num32, gpu), _dev(cnt32, gpu)


def _known_matrix(d, gpu):
    """The matrix an accumulating call adds to (symmetric, f64, exact in f32)."""
    a = np.random.default_rng(d).integers(-8, 9, size=(d, d)).astype(np.float64)
    return _dev(a + a.T, gpu), a + a.T


def _gram_sweep(label, launch, n, d, gpu, G0=None, ws_rows=None):
    """launch(G, accumulate, ws) on a poisoned GramWorkspace; G poisoned, or a
    clone of the known matrix G0 where the call accumulates."""
    def run(p):
        ws = P.GramWorkspace(n if ws_rows is None else ws_rows, d, gpu)
        S.poison(ws.buf, p)
        G = G0.clone() if G0 is not None else _buf((d, d), torch.float64, p, gpu)
        launch(G, G0 is not None, ws)
        _sync()
        return {"G": _cpu(G)}
    return _sweep(label, run)["G"].numpy()


@pytest.mark.parametrize("n,d", S.GRAM_TRI + S.GRAM_GENERIC + S.GRAM_SMALL, ids=lambda v: str(v))
def test_gram_f32_rows(gpu, n, d):
    route = S.gram_route(n, d)
    num32, cnt32, num, cnt = _gram_rows(n, d, gpu)
    K0, k0 = _known_matrix(d, gpu)
    for use_cnt in (False, True):
        X = WG._x_of(num32, cnt32 if use_cnt else None)
        exact = X.T @ X
        for acc in (False, True):
            label = f"gram {route} n={n} d={d} cnt={int(use_cnt)} accumulate={int(acc)}"
            G = _gram_sweep(label, lambda G, a, ws: P.gram(num, cnt if use_cnt else None, G, a, ws),
                            n, d, gpu, G0=K0 if acc else None)
            WG._check_gram(_note, G, exact + k0 if acc else exact, label)  # the family's float64 bar


@pytest.mark.parametrize("n,d", S.GRAM_F64, ids=lambda v: str(v))
def test_gram_f64_rows(gpu, n, d):
    X = W.x64(n, d)
    x = _dev(X, gpu)
    K0, k0 = _known_matrix(d, gpu)
    for acc in (False, True):
        def launch(G, a, ws):
            L.call("mmb_gram_f64", L.ptr(x), n, d, L.ptr(G), int(a), L.ptr(ws.buf), L.stream_ptr())
        label = f"gram_f64 n={n} d={d} accumulate={int(acc)}"
        G = _gram_sweep(label, launch, n, d, gpu, G0=K0 if acc else None)
        WG._check_gram(_note, G, X.T @ X + (k0 if acc else 0.0), label)


@pytest.mark.parametrize("chunks", S.GRAM_PART_CHUNKS, ids=lambda v: "-".join(map(str, v)))
def test_gram_two_phase(gpu, chunks):
    """mmb_gram_part per chunk + mmb_gram_finish at n_plan = 5000: fewer rows
    than the plan's ranges hold, and an empty first chunk at accumulate = 0,
    whose ranges must still overwrite the partials."""
    n_plan, d = S.GRAM_PARTS
    rows = sum(chunks)
    num32, cnt32, num, cnt = _gram_rows(n_plan, d, gpu)
    K0, k0 = _known_matrix(d, gpu)
    for use_cnt in (False, True):
        X = WG._x_of(num32[:rows], cnt32[:rows] if use_cnt else None)
        for acc in (False, True):
            def launch(G, a, ws):
                r0 = 0
                for i, c in enumerate(chunks):  # (bare addresses: an empty slice has no data pointer)
                    L.call("mmb_gram_part", num.data_ptr() + 4 * r0 * d,
                           cnt.data_ptr() + 4 * r0 if use_cnt else None, c, n_plan, d, int(i > 0),
                           L.ptr(ws.buf), L.stream_ptr())
                    r0 += c
                L.call("mmb_gram_finish", n_plan, d, L.ptr(G), int(a), L.ptr(ws.buf), L.stream_ptr())
            label = f"gram two-phase chunks={chunks} cnt={int(use_cnt)} accumulate={int(acc)}"
            G = _gram_sweep(label, launch, n_plan, d, gpu, G0=K0 if acc else None)
            WG._check_gram(_note, G, X.T @ X + (k0 if acc else 0.0), label)


@pytest.mark.parametrize("n,d", S.GRAM_I8, ids=lambda v: str(v))
def test_gram_i8(gpu, n, d):
    x = WG._i8_rows(n, d)
    xt = _dev(x, gpu)
    K0, k0 = _known_matrix(d, gpu)
    for acc in (False, True):
        cms = []

        def launch(G, a, ws):
            cm = _buf((d,), torch.int32, "H", gpu)  # mmb_colmax (accumulate = 0) overwrites it
            P.colmax(xt, out=cm)
            cms.append(cm)
            P.gram_i8(xt, cm, G, a, ws)
        label = f"gram_i8 n={n} d={d} accumulate={int(acc)}"
        G = _gram_sweep(label, launch, n, d, gpu, G0=K0 if acc else None)
        assert all(np.array_equal(cm.cpu().numpy().view(np.float32), np.abs(x).max(0)) for cm in cms)
        if not acc and n <= 5000:  # the family's bars (the sliced oracle costs O(n d^2) on the CPU)
            WG._check_gram_i8(_note, G, x)


# ------------------------------------------------------------------ 2: stream kernels, column bounds
def _colmax_bufs(D, p, gpu):
    nb = L.query("mmb_mm2_colmax_ws_bytes", D)
    return (_buf((D,), torch.int32, p, gpu),
            _buf(((nb + 15) // 16 * 16,), U8, p, gpu, keep=S.colmax_ws_keep(nb)))


def _stream_outputs(case, s_half, p, gpu):
    D, A, Vd, T, N, V = case
    kp, _ = P.mm2_dims(D, A, Vd)
    return (_buf((N, D), torch.float32, p, gpu), S.poison(P.s_buffer(N, kp, s_half, gpu), p),
            _buf((3, N), torch.float32, p, gpu))


def _stream_checks(case, s_half, z):
    """The documented zeros and the bounds, on the outputs of a run."""
    D, A, Vd, T, N, V = case
    K = 2 * (D + A + Vd)
    kp = (K + 31) // 32 * 32
    s, num = z["s"].numpy(), z["x"].numpy()
    if s_half:
        assert s.shape == (N, 2 * kp) and not s[:, K:kp].any() and not s[:, kp + K:].any()
    else:
        assert s.shape == (N, kp) and not s[:, K:].any()
    # colmax: the bits of max |x| of the returned x
    assert np.array_equal(z["colmax"].numpy().view(np.float32), np.abs(num).max(0))


def _stream_sweep(case, gpu, modes=S.STREAM_MODES, kind=None, split_parts=None, anchor=False):
    D, A, Vd, T, N, V = case
    z = C.inputs(case)
    if kind is None:
        au, vi = _dev(z["audio"], gpu), _dev(z["visual"], gpu)
    else:
        au, vi = (t.to(gpu) for t in F.frames(case, kind))
    for mode in modes:
        kw = MG._text_args(z, mode, gpu)
        for s_half in (False, True):
            def run(p):
                out = _stream_outputs(case, s_half, p, gpu)
                colmax, ws = _colmax_bufs(D, p, gpu)
                flag = torch.zeros(1, dtype=torch.int32, device=gpu)
                extra = {}
                if split_parts is not None:
                    extra = {"split": S.poison(P.split_ws(N, T, D, A, Vd, gpu, parts=split_parts), p),
                             "parts": split_parts}
                num, s, aux = P.mm2_stream(N, T, D, A, Vd, au, vi, s_half=s_half, flag=flag, out=out,
                                           colmax=colmax, colmax_ws=ws, **kw, **extra)
                _sync()
                return {"x": _cpu(num), "s": _cpu(s), "aux": _cpu(aux), "colmax": _cpu(colmax),
                        "flag": _cpu(flag)}
            label = (f"stream {C.shape_id(case)} {mode} s_half={int(s_half)}"
                     + (f" {kind}" if kind else "") + (f" parts={split_parts}" if split_parts is not None else ""))
            out = _sweep(label, run)
            assert int(out["flag"]) == 0
            _stream_checks(case, s_half, out)
            if anchor:  # the family's float64 bars (tests/test_gpu_mmb2_widths.py)
                MG._check_stream(_note, 11, case, (out["x"].numpy(), out["s"].numpy(), out["aux"].numpy(),
                                                   out["colmax"].numpy().view(np.float32)),
                                 MG._ref(case, emb2=mode == "dense+emb2"), s_half)


@pytest.mark.parametrize("shape,n,family", S.STREAM_CASES,
                         ids=[f"{C.shape_id(s)}-N{n}" for s, n, _ in S.STREAM_CASES])
def test_stream_kernels(gpu, shape, n, family):
    _stream_sweep(C.case_of(shape, n), gpu, anchor=(n == 5))


def test_stream_either_side_of_the_cu_count(gpu):
    cus = L.cu_count(gpu)
    for n in (cus, cus + 1):
        _stream_sweep(C.case_of(S.STREAM_CU_EDGE, n), gpu)


@pytest.mark.parametrize("shape", S.STREAM_SPLIT, ids=C.shape_id)
def test_split_stream(gpu, shape):
    for parts in S.STREAM_SPLIT_PARTS:
        _stream_sweep(C.case_of(shape), gpu, split_parts=parts, anchor=(parts == 3))


@pytest.mark.parametrize("kind", S.frames16_kinds())
@pytest.mark.parametrize("shape", S.STREAM_FRAMES16, ids=C.shape_id)
def test_stream_16_bit_frames(gpu, shape, kind):
    _stream_sweep(C.case_of(shape), gpu, modes=("ids+table",), kind=kind)


# ------------------------------------------------------------------ 3: split-K projection
def _split_ws(n, kp, slices, p, gpu):
    nb = int(L.query("mmb_mm2_project_x3_split_ws_bytes", n, kp, slices))
    return _buf((max(nb, 16),), U8, p, gpu)


@pytest.mark.parametrize("A,Vd", S.PROJECT_FRAMES, ids=lambda v: str(v))
@pytest.mark.parametrize("D", S.PROJECT_D)
def test_split_k_projection(gpu, D, A, Vd):
    for N in S.PROJECT_N:
        case = C.case_of((D, A, Vd, S.PROJECT_T), N)
        num, s32, s16, aux, aux16, proj = MG._operands(case, gpu)
        pc = _dev(W.orthonormal_rows(1, D, seed=D + N), gpu)
        for slices in S.PROJECT_SLICES:
            for with_pc in (False, True):
                def run(p):
                    out = _buf((N, D), torch.float32, p, gpu)
                    sif = _buf((N, D), torch.float32, p, gpu) if with_pc else None
                    P.mm2_project(s16, num, aux16, proj, out=out, pc=pc if with_pc else None, sif_out=sif,
                                  split=_split_ws(N, proj.kp, slices, p, gpu), slices=slices)
                    _sync()
                    return {"mmb2": _cpu(out), **({"sif": _cpu(sif)} if with_pc else {})}
                z = _sweep(f"split-K {C.shape_id(case)} slices={slices} pc={int(with_pc)}", run)
                if case == S.PROJECT_ANCHOR and slices == 2:  # the family's float64 bars
                    MG._check_rows(_note, 7, "split-K projection", case, z["mmb2"], MG._dequant(s16, aux16, proj.kp),
                                   num, aux16, proj, x3=True)
                    if with_pc:
                        MG._check_removed(_note, case, z["sif"], num, pc.cpu().numpy(), gpu)


# ------------------------------------------------------------------ 4: derived images
IMAGES = ("wm", "c0", "wsplit", "wpieces", "text_cache")


def _image_sizes(proj, V):
    d, a, vd = proj.d, proj.a, proj.vd
    return {"wm": proj.wm.numel() * 4, "c0": proj.c0.numel() * 4,
            "wsplit": L.query("mmb_mm2_split_bytes", d, a, vd),
            "wpieces": L.query("mmb_mm2_split_pieces_bytes", d, a, vd),
            "text_cache": L.query("mmb_mm2_text_cache_bytes", V, d)}


def _rebuilt_projection(nets, dims, p, gpu, text=None):
    """An MMB2Projection whose every image was filled with the pattern before
    refresh() built it; returns (proj, {image: the bytes each *_bytes query sizes})."""
    D, A, Vd, T = dims
    proj = P.MMB2Projection(nets, D, A, Vd, T, gpu)
    proj.enable_pieces()
    if text is not None:
        proj.enable_text_cache(*text)
    _sync()
    sizes = _image_sizes(proj, text[0].shape[0] if text is not None else 0)
    for name in IMAGES:
        if getattr(proj, name, None) is not None:
            S.poison(getattr(proj, name), p)
    proj.refresh()
    _sync()
    img = {name: _cpu(S._bytes_of(getattr(proj, name))[:sizes[name]]) for name in IMAGES
           if getattr(proj, name, None) is not None}
    return proj, img


def _images_and_consumers(label, nets, dims, N, inp, front, gpu, text=None, anchor_case=None):
    D, A, Vd, T = dims
    num, s32, aux = P.mm2_stream(N, T, D, A, Vd, inp["audio"], inp["visual"], ids32=inp["ids"],
                                 table=inp["table"], wtab32=inp["wtab"], s_half=False)
    _, s16, aux16 = P.mm2_stream(N, T, D, A, Vd, inp["audio"], inp["visual"], ids32=inp["ids"],
                                 table=inp["table"], wtab32=inp["wtab"], s_half=True)
    _sync()
    keep = {}

    def run(p):
        proj, out = _rebuilt_projection(nets, dims, p, gpu, text)
        keep["proj"] = proj
        o32, o16 = _buf((N, D), torch.float32, p, gpu), _buf((N, D), torch.float32, p, gpu)
        P.mm2_project(s32, num, aux, proj, out=o32)     # mmb_mm2_project reads wm, c0
        P.mm2_project(s16, num, aux16, proj, out=o16)   # mmb_mm2_project_x3 reads wsplit, c0
        fo = (_buf((N, D), torch.float32, p, gpu), _buf((3, N), torch.float32, p, gpu),
              _buf((N, D), torch.float32, p, gpu))
        colmax, ws = _colmax_bufs(D, p, gpu)
        flag = torch.zeros(1, dtype=torch.int32, device=gpu)
        x, fa, m = front(N, T, D, A, Vd, inp["audio"], inp["visual"], proj, ids32=inp["ids"],
                         table=inp["table"], wtab32=inp["wtab"], flag=flag, out=fo, colmax=colmax,
                         colmax_ws=ws)  # the fused kernels read wpieces, c0 (and the text cache)
        _sync()
        out.update({"project": _cpu(o32), "project_x3": _cpu(o16), "fused x": _cpu(x),
                    "fused aux": _cpu(fa), "fused mmb2": _cpu(m), "fused colmax": _cpu(colmax),
                    "flag": _cpu(flag)})
        return out
    z = _sweep(label, run)
    assert int(z["flag"]) == 0
    wm, c0 = z["wm"].view(torch.float32).view(-1, keep["proj"].ldw).numpy(), z["c0"].view(torch.float32).numpy()
    K = 2 * (D + A + Vd)
    assert not wm[K:].any() and not wm[:, D + 1:].any() and not c0[D + 1:].any()  # the K and ldw pads
    if anchor_case is not None:  # the family's float64 bars, on the x3 consumer and the fused rows
        proj = keep["proj"]
        MG._check_rows(_note, 7, "x3 on a rebuilt image", anchor_case, z["project_x3"],
                       MG._dequant(s16, aux16, proj.kp), num, aux16, proj, x3=True)
        e = M.row_rel_err(z["fused mmb2"].numpy(), C.oracle_rows(anchor_case))
        print(f"{label}: fused rows vs the oracle {e:.3e} (bar {TOL})")
        assert e < TOL


@pytest.mark.parametrize("row", S.FUSED_TAIL_ROWS)
def test_projection_images_and_the_fused_kernel(gpu, row):
    D, A, Vd, T, N, bad = FC.CASES[row]
    assert not bad and P.stream_project_supported(T, D, A, Vd)
    inp = synth.device_workload(N, T, FC.V, D=D, A=A, Vd=Vd, seed=83, device=gpu)
    torch.manual_seed(0)
    gen = models.AudioVisualGeneratorMultimodal(D, A, Vd, norm=None).to(gpu)
    _images_and_consumers(f"images + fused D{D}-A{A}-V{Vd}-T{T}-N{N}", gen.networks(), (D, A, Vd, T), N,
                          inp, P.mm2_stream_project, gpu)


@pytest.mark.parametrize("case", S.NARROW_FUSED, ids=C.shape_id)
def test_projection_images_and_the_narrow_fused_kernel(gpu, case):
    D, A, Vd, T, N, V = case
    assert P.narrow_fused_supported(T, D, A, Vd, V)
    inp = MG._device_inputs(case, gpu)
    _images_and_consumers(f"images + narrow fused {C.shape_id(case)}", _networks(case, gpu),
                          (D, A, Vd, T), N, inp, P.mm2_stream_project_narrow, gpu,
                          text=(inp["table"], inp["wtab"]), anchor_case=case if N > 1 else None)


@pytest.mark.parametrize("D", S.WORD_TABLE_D)
def test_normalised_word_table(gpu, D):
    V = S.WORD_TABLE_V
    table = _dev32(WC.make_inputs(WC.WordCase(D, V, 1, 1, 0))["table"], gpu)
    Dp = L.query("mmb_word_pad", D)

    def run(p):
        wn = _buf((V, Dp), torch.float32, p, gpu)
        L.call("mmb_word_normalize", L.ptr(table), V, D, L.ptr(wn), L.stream_ptr())
        _sync()
        return {"wn": _cpu(wn)}
    wn = _sweep(f"word table D={D} V={V}", run)["wn"].numpy().astype(np.float64)
    assert Dp > D and not wn[:, D:].any()  # the pad columns
    assert np.abs(np.linalg.norm(wn, axis=1) - 1.0).max() < 1e-6


# ------------------------------------------------------------------ 5: PC solve workspace
def _solve_ws(d, p, gpu):
    return _buf((L.query("mmb_pc_solve_mc_ws_bytes", d),), U8, p, gpu, keep=S.solve_keep(d))


SOLVE_CASES = S.solve_cases()


@pytest.mark.parametrize("n,d,npc", SOLVE_CASES, ids=["n{}-d{}-npc{}".format(*c) for c in SOLVE_CASES])
def test_pc_solve_workspace(gpu, n, d, npc):
    assert (n, d, npc) in WG.SOLVE_CASES
    G, z0, tr, Gd, z0d = WG._solver_inputs(n, d, npc, gpu)
    for n_iter in ((7, 0) if npc == 1 else (7,)):  # 7: the squared rounds read G2 from the workspace
        def run(p):
            ws = _solve_ws(d, p, gpu)
            pc = _buf((npc, d), torch.float64, p, gpu)
            flag = torch.zeros(1, dtype=torch.int32, device=gpu)
            P.pc_solve(Gd, z0d, npc, tr, n_iter=n_iter, out=pc, flag=flag, ws=ws)
            _sync()
            assert not bool(ws[:16].any()), "control words left non-zero"
            return {"pc": _cpu(pc), "flag": _cpu(flag)}
        z = _sweep(f"pc_solve n={n} d={d} npc={npc} n_iter={n_iter}", run)
        assert int(z["flag"]) == 0
        if (n, d, npc) == S.SOLVE_ANCHOR:  # the family's float64 bar
            e = np.abs(z["pc"].numpy() - O.pc_from_gram(G, z0, npc, tr, n_iter=n_iter)).max()
            print(f"anchor: {e:.3e} (bar {W.SOLVE_BAR[npc]})")
            assert e < W.SOLVE_BAR[npc]


@pytest.mark.parametrize("n,d", S.SOLVE_XT, ids=lambda v: str(v))
def test_pc_solve_xt_workspace(gpu, n, d):
    X = W.make_x(n, d)
    x, Gd = _dev(X.astype(np.float32), gpu), _dev(X.T @ X, gpu)
    k = min(1 + P.N_OVERSAMPLES, d)
    om = P.omega(n, k, gpu)

    def run(p):
        ws = _solve_ws(d, p, gpu)
        pc = _buf((1, d), torch.float64, p, gpu)
        flag = torch.zeros(1, dtype=torch.int32, device=gpu)
        L.call("mmb_pc_solve_mc_xt", L.ptr(Gd), d, L.ptr(x), n, L.ptr(om), k, 1, P.N_ITER, L.ptr(pc),
               L.ptr(ws), L.ptr(flag), L.stream_ptr())
        _sync()
        assert not bool(ws[:16].any()), "control words left non-zero"
        return {"pc": _cpu(pc), "flag": _cpu(flag)}
    z = _sweep(f"pc_solve_mc_xt n={n} d={d}", run)
    assert int(z["flag"]) == 0
    if W.full_rank(n, d, 1):  # the family's float64 bar
        ref = O.pc_from_gram(X.T @ X, X.T @ om.cpu().numpy(), 1, True)
        assert np.abs(z["pc"].numpy() - ref).max() < W.SOLVE_BAR[1]


# ------------------------------------------------------------------ 6: word likelihood
def _word_inputs(c, dense, gpu):
    z, lp_ref, g_ref = WC.reference(c, dense)
    wt = LT.WordTable(_dev32(z["table"], gpu))
    d = {"lat": _dev32(z["lat"], gpu), "w": _dev32(z["w"], gpu), "mask": _dev32(z["mask"], gpu),
         "up": _dev32(z["up"], gpu), "wt": wt,
         "ids": None if dense else _dev32(z["ids"], gpu, torch.int32),
         "sent": _dev32(z["dense"], gpu) if dense else None}
    return d, lp_ref, g_ref


def _word_run(c, d, p, gpu, ws=None):
    """Forward (want_grad) into poisoned lp / state / gsum / cos, then the
    backward from that forward's own state into a poisoned dlat."""
    wt = d["wt"]
    if ws is None:
        ws = _buf((max(L.query("mmb_word_workspace_bytes", c.B, c.D, c.V), 16),), U8, p, gpu)
    lp, state = _buf((c.B,), torch.float32, p, gpu), _buf((c.B, 4), torch.float32, p, gpu)
    gsum, cosv = _buf((c.B, wt.Dp), torch.float32, p, gpu), _buf((c.B, c.L), torch.float32, p, gpu)
    dlat = _buf((c.B, c.D), torch.float32, p, gpu)
    table = L.ptr(wt.table) if d["ids"] is not None else None
    L.call("mmb_word_logprob_forward", L.ptr(d["lat"]), c.B, c.D, L.ptr(wt.wn), c.V, L.ptr(d["ids"]), table,
           L.ptr(d["sent"]), c.L, L.ptr(d["w"]), L.ptr(d["mask"]), WC.A, 1, L.ptr(ws), L.ptr(lp),
           L.ptr(state), L.ptr(gsum), L.ptr(cosv), L.stream_ptr())
    L.call("mmb_word_logprob_backward", L.ptr(d["lat"]), c.B, c.D, c.V, L.ptr(d["ids"]), table,
           L.ptr(d["sent"]), c.L, L.ptr(d["w"]), L.ptr(d["mask"]), WC.A, L.ptr(state), L.ptr(gsum),
           L.ptr(cosv), L.ptr(d["up"]), L.ptr(dlat), L.stream_ptr())
    _sync()
    return {"lp": _cpu(lp), "state": _cpu(state), "gsum": _cpu(gsum), "cos": _cpu(cosv),
            "dlat": _cpu(dlat)}


@pytest.mark.parametrize("dense", [False, True], ids=["ids", "dense"])
@pytest.mark.parametrize("c", S.WORD_CASES, ids=[WC.word_id(c) for c in S.WORD_CASES])
def test_word_likelihood(gpu, c, dense):
    d, lp_ref, g_ref = _word_inputs(c, dense, gpu)
    z = _sweep(f"word {WC.word_id(c)} {'dense' if dense else 'ids'}", lambda p: _word_run(c, d, p, gpu))
    assert not z["gsum"].numpy()[:, c.D:].any()  # the pad columns of the G sums
    # the family's float64 bars (tests/test_gpu_word_widths.py)
    assert WC.lp_ratio(z["lp"].numpy(), lp_ref) <= 1.0
    assert WC.grad_ratio(z["dlat"].numpy(), g_ref) <= 1.0


# ------------------------------------------------------------------ 7: regressor
@pytest.mark.parametrize("want", S.BACKWARD_WANTS)
@pytest.mark.parametrize("c", S.BACKWARD_CASES, ids=[R.fwd_id(c) for c in S.BACKWARD_CASES])
def test_mlp_backward_workspace(gpu, c, want):
    z = R.fwd_inputs(c)
    hid32 = R.f32(z["hid"])
    w1, _, w2, _ = z["params"]
    g, bounds = R.backward_bounds(z["x"], hid32, w1, w2, z["dy"])
    x, hid, dy = RG._dev(z["x"], gpu), RG._dev(hid32, gpu), RG._dev(z["dy"], gpu)
    w1d, w2d = RG._dev(w1, gpu), RG._dev(w2, gpu)
    names = ("dh", "dx", "dw1", "db1", "dw2", "db2")
    skip = {"all": (), "no_dx": ("dx",), "no_params": ("dw1", "db1", "dw2", "db2")}[want]

    def run(p):
        out = {k: None if k in skip else _buf(g[k].shape, torch.float32, p, gpu) for k in names}
        L.call("mmb_mlp_backward", L.ptr(x), L.ptr(hid), c.b, c.d, c.h, c.o, L.ptr(w1d), L.ptr(w2d),
               L.ptr(dy), *[L.ptr(out[k]) for k in names], L.stream_ptr())
        _sync()
        return {k: _cpu(t) for k, t in out.items() if t is not None}
    zr = _sweep(f"mlp_backward {R.fwd_id(c)} {want}", run)
    for k, t in zr.items():  # the family's float64 bars (tests/test_gpu_regressor_widths.py)
        RG._check(_note, "a", "mmb_mlp_backward " + k, RG._host64(t), g[k], bounds[k])


def _train_outputs(run):
    rc, params, sl, vl, flag = run
    assert rc == 0 and int(flag.item()) == 0
    return {**{f"p{i}": _cpu(t) for i, t in enumerate(params)}, "step_loss": _cpu(sl),
            **({"valid_loss": _cpu(vl)} if vl is not None else {})}


def test_mlp_train_leaves_its_workspace_zero(gpu):
    """mmb_mlp_train's workspace is never poisoned (its workgroups synchronise
    on it).  A completed launch leaves ALL of it zero, and a smaller case run
    next on the same workspace equals its run on a fresh zeroed one."""
    small = S.TRAIN_SMALLER
    fresh = _train_outputs(RG._launch_train(gpu, small, R.make_train_inputs(small),
                                            RG._workspace(gpu, small.d, small.h)))
    for c in S.TRAIN_CASES:
        ws = RG._workspace(gpu, c.d, c.h)
        assert ws.numel() * 4 >= L.query("mmb_mlp_workspace_bytes", small.d, small.h)
        _train_outputs(RG._launch_train(gpu, c, R.make_train_inputs(c), ws))
        left = int(torch.count_nonzero(ws))
        assert left == 0, f"{R.train_id(c)}: {left} of {ws.numel()} workspace words left non-zero"
        again = _train_outputs(RG._launch_train(gpu, small, R.make_train_inputs(small), ws))
        _assert_same(f"mlp_train {R.train_id(small)} after {R.train_id(c)}", "reused workspace", fresh, again)
        assert not ws.any().item()
        print(f"mlp_train {R.train_id(c)}: workspace zero after the launch; {R.train_id(small)} on it "
              f"equals its fresh run")


# ------------------------------------------------------------------ 8: reuse across shapes
def _reuse(label, runs, gpu):
    """runs: [(name, run(ws or None, pattern))], large first.  Each case's
    fresh-Z run, then large, small.., large on ONE workspace filled with H once
    and never re-filled."""
    fresh = {name: run(None, "Z") for name, run in runs}
    order = runs + runs[:1]
    shared = {}
    for name, run in order:
        got = run(shared, "H")
        _assert_same(f"{label} {name}", "reused workspace", fresh[name], got)
    print(f"{label} ({' -> '.join(n for n, _ in order)}): reuse ok")


def test_reuse_gram_workspace(gpu):
    shapes = [(5000, 320), (4100, 4), (4097, 17)]  # tri (the largest), tri, generic
    nbytes = max(L.query("mmb_gram_workspace_bytes", n, d) for n, d in shapes)
    assert nbytes == L.query("mmb_gram_workspace_bytes", *shapes[0])

    def make(n, d):
        _, _, num, cnt = _gram_rows(n, d, gpu)

        def run(shared, p):
            if shared is None:
                ws = S.poison(P.GramWorkspace(n, d, gpu).buf, p)
            else:
                if "ws" not in shared:
                    shared["ws"] = _buf((nbytes,), U8, p, gpu)
                ws = shared["ws"]
            holder = P.GramWorkspace.__new__(P.GramWorkspace)
            holder.buf, holder.n, holder.d = ws, n, d
            assert holder.fits(n, d)
            G = _buf((d, d), torch.float64, p, gpu)
            P.gram(num, cnt, G, False, holder)
            _sync()
            return {"G": _cpu(G)}
        return f"({n}, {d})", run
    _reuse("gram", [make(n, d) for n, d in shapes], gpu)


def test_reuse_split_stream_workspace(gpu):
    cases = [(C.case_of(S.STREAM_SPLIT[0]), 200), (C.case_of(S.STREAM_SPLIT[1]), 3)]
    nbytes = max(P.split_ws(c[4], c[3], c[0], c[1], c[2], gpu, parts=q).numel() for c, q in cases)

    def make(case, parts):
        D, A, Vd, T, N, V = case
        z = C.inputs(case)
        au, vi = _dev(z["audio"], gpu), _dev(z["visual"], gpu)
        kw = MG._text_args(z, "ids+table", gpu)

        def run(shared, p):
            if shared is None:
                ws = S.poison(P.split_ws(N, T, D, A, Vd, gpu, parts=parts), p)
            else:
                if "ws" not in shared:
                    shared["ws"] = _buf((nbytes,), U8, p, gpu)
                ws = shared["ws"]
            out = _stream_outputs(case, True, p, gpu)
            num, s, aux = P.mm2_stream(N, T, D, A, Vd, au, vi, s_half=True, out=out, split=ws, parts=parts, **kw)
            _sync()
            return {"x": _cpu(num), "s": _cpu(s), "aux": _cpu(aux)}
        return f"{C.shape_id(case)} parts={parts}", run
    _reuse("split stream", [make(c, q) for c, q in cases], gpu)


def test_reuse_split_k_workspace(gpu):
    cases = [(C.case_of((316, 300, 300, S.PROJECT_T), 300), 7), (C.case_of((256, 8, 12, S.PROJECT_T), 2), 2)]
    ops = {c: MG._operands(c, gpu) for c, _ in cases}
    nbytes = max(int(L.query("mmb_mm2_project_x3_split_ws_bytes", c[4], ops[c][5].kp, q)) for c, q in cases)

    def make(case, slices):
        num, s32, s16, aux, aux16, proj = ops[case]
        N, D = case[4], case[0]
        pc = _dev(W.orthonormal_rows(1, D, seed=D + N), gpu)

        def run(shared, p):
            if shared is None:
                ws = _split_ws(N, proj.kp, slices, p, gpu)
            else:
                if "ws" not in shared:
                    shared["ws"] = _buf((max(nbytes, 16),), U8, p, gpu)
                ws = shared["ws"]
            out, sif = _buf((N, D), torch.float32, p, gpu), _buf((N, D), torch.float32, p, gpu)
            P.mm2_project(s16, num, aux16, proj, out=out, pc=pc, sif_out=sif, split=ws, slices=slices)
            _sync()
            return {"mmb2": _cpu(out), "sif": _cpu(sif)}
        return f"{C.shape_id(case)} slices={slices}", run
    _reuse("split-K projection", [make(c, q) for c, q in cases], gpu)


def test_reuse_word_workspace(gpu):
    cases = [S.WORD_CASES[4], S.WORD_CASES[0], S.WORD_CASES[2]]  # the largest first
    nbytes = max(L.query("mmb_word_workspace_bytes", c.B, c.D, c.V) for c in cases)
    assert nbytes == L.query("mmb_word_workspace_bytes", cases[0].B, cases[0].D, cases[0].V)

    def make(c):
        d, _, _ = _word_inputs(c, False, gpu)

        def run(shared, p):
            if shared is None:
                return _word_run(c, d, p, gpu)
            if "ws" not in shared:
                shared["ws"] = _buf((max(nbytes, 16),), U8, p, gpu)
            return _word_run(c, d, p, gpu, ws=shared["ws"])
        return WC.word_id(c), run
    _reuse("word likelihood", [make(c) for c in cases], gpu)


# ------------------------------------------------------------------ 9: the whole step
def _make_step(name, gpu):
    case, kw, want = S.STEPS[name]
    step = P.FusedStep(MG._device_inputs(case, gpu), _networks(case, gpu), **kw)
    for k, v in want.items():
        assert getattr(step.plan, k) == v, (name, step.plan)
    if want.get("project") == "fork":
        assert step.fork is not None  # the projection on its own stream, beside Gram -> solve
    return case, step


def _fill_step(step, p):
    """Every buffer the step owns (scratch_cases.STEP_BUFFERS and gws.buf), the
    protected words excepted; inputs, parameters and the flag are not filled."""
    filled = []
    for name in S.STEP_BUFFERS:
        t = getattr(step, name, None)
        if t is None:
            continue
        keep = ()
        if name == "solve_ws":
            keep = S.solve_keep(step.d)
        if name == "colmax_ws":
            keep = S.colmax_ws_keep(L.query("mmb_mm2_colmax_ws_bytes", step.d))
        S.poison(t, p, keep)
        filled.append(name)
    S.poison(step.gws.buf, p)
    return filled + ["gws.buf"]


def _step_outputs(step, sif, mmb2):
    _sync()
    return {"sif": _cpu(sif), "mmb2": _cpu(mmb2), "pc": _cpu(step.pc), "x": _cpu(step.x),
            "flag": _cpu(step.flag)}


@pytest.mark.parametrize("name", list(S.STEPS))
def test_whole_step(gpu, name):
    case, step = _make_step(name, gpu)
    sif, mmb2 = step.run(check=True)
    ref = _step_outputs(step, sif, mmb2)
    if name == "fused":  # the family's float64 bars (tests/test_gpu_mmb2_widths.py)
        MG._check_step(_note, case, step, sif, mmb2)
    for p in S.POISONS:
        filled = _fill_step(step, p)
        sif, mmb2 = step.run(check=True)
        _assert_same(f"step {name}", p, ref, _step_outputs(step, sif, mmb2))
    print(f"step {name} {C.shape_id(case)} plan {step.plan.front}/{step.plan.gram}/{step.plan.project} "
          f"(filled: {', '.join(filled)}): N ok / H ok")


@pytest.mark.parametrize("name", list(S.STEPS))
def test_whole_step_graph_replay(gpu, name):
    """Captured once; every buffer poisoned between two replays."""
    case, step = _make_step(name, gpu)
    g = P.StepGraph(step)
    sif, mmb2 = g.run(check=True)
    ref = _step_outputs(step, sif, mmb2)
    for p in S.POISONS:
        _fill_step(step, p)
        sif, mmb2 = g.run(check=True)
        _assert_same(f"graph of step {name}", p, ref, _step_outputs(step, sif, mmb2))
    print(f"graph of step {name} {C.shape_id(case)}: N ok / H ok")
