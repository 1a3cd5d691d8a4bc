"""GPU: the PC solvers, the int8 Gram and the removals on spectra with a
dominant component (tests/spectrum_cases.py holds the families, the case
tables and the bar rule; tests/test_spectrum_cases.py pins, on the CPU, the
conditions the bars rest on).

Every other PC input of the suite is mild (0.4 N(0, 1) noise plus a 0.3
offset, l1/l11 <= ~300) or exactly rank-deficient.  Real SIF rows carry a
strong common component; the arithmetic that depends on the spectrum -- one
CholeskyQR pass between products, the squared rounds, the direct tail's
A = L^-1 H L^-T, p16_top_eig's squarings and deflation, pc_solve_kernel's
orth_block and Jacobi, the removals' cancellation, the int8 Gram's
per-column fixed point -- is reached here from the other side.

  1 solvers from (G, z0)    spike npc 1, 2; geom npc 1, 2, 6; mean npc 1, 2, 3; R up to
                            1e10, c up to 300, over the six shapes: mmb_pc_solve_mc /
                            pc_solve_kernel (P.pc_solve) and pc_solve16_kernel (mmb_pc_solve)
  2 squared-round counts    geom R 1e4, 1e6, npc 1, n_iter 3, 4, 5, 8
  3 mmb_pc_solve_mc_xt      f32 rows in; bit-equal to mmb_xt_omega + mmb_pc_solve_mc
  4 power-of-two scale      2^+-20: the PC within 1e-13 of the unscaled device result
  5 close top pair          l1/l2 = 1 + gap, gap down to 1e-6, npc 1, 2
  6 int8 Gram, dominant mean  G at test_gram_i8_widths' bars; the PC solved from it
  7 removal under cancellation  mmb_pc_remove (f32 / f64 out, cnt or not), mmb_pc_remove_f64,
                            the fused epilogue of mmb_mm2_project_x3_rmpc
  8 FusedStep end to end    c g added to the word table

Bars (1-3, 5, 6): per component max(floor, 8 dev) capped at 1e-9 against
O.compute_pc on X itself, dev the difference of the two CPU routes; an exempt
component (8 dev past the cap: only what spectrum_cases.allowed_exempt
admits) is held finite, unit-norm to 1e-12 and orthogonal to the earlier
components to 1e-9.  The error against O.pc_from_gram is printed as
information.  Removal bars, derived: f64 out |out - ref| <= 1e-12 max|x_row|
(d eps |x| with margin); f32 out 2^-23 max|ref_row| + 1e-12 max|x_row|.

Every test prints what it measured; the module prints, per group, the number
of comparisons, the largest error as a fraction of its bar and where it
occurred.  Only the product library is loaded.
"""
import functools

import numpy as np
import pytest
import torch

import mmb_lib as L
import models
import pipeline as P
import spectrum_cases as S
import synth
import width_cases as W
from common_gpu import Ledger, _dev
from oracle import sif_oracle as O
from width_cases import F32_ROW
from widths_gpu import _pc_solve_checked, _pc_solve_direct

pytestmark = pytest.mark.gpu

_WORST = Ledger()  # (group, what) -> [comparisons, largest error / bar, where]


def _note(group, what, err, bar, where):
    _WORST.note((group, what), float(err) / bar, where)
    return float(err)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for (group, what), (cases, frac, where) in sorted(_WORST.items()):
        print(f"\nspectrum group {group} {what}: {cases} comparisons, largest {frac:.3f} of its bar"
              f" at {where}", end="")
    print()


def _hold(group, what, pc, ref, bars, case, alt=None, i8=False):
    """The device PC against the reference, component by component."""
    where = S.case_id(case) + f"-npc{len(bars)}"
    assert pc.shape == ref.shape and np.isfinite(pc).all(), where
    out = []
    for c, (bar, exempt) in enumerate(bars):
        e = np.abs(pc[c] - ref[c]).max()
        info = "" if alt is None else f" (vs pc_from_gram {np.abs(pc[c] - alt[c]).max():.1e})"
        if exempt:
            assert S.allowed_exempt(case, c, i8), (where, c)
            S.check_exempt_component(pc, c)
            _note(group, f"{what}, exempt components: |norm - 1|",
                  abs(np.linalg.norm(pc[c]) - 1.0), 1e-12, where)
            out.append(f"c{c} exempt: {e:.1e}{info}")
            continue
        _note(group, f"{what}, component {min(c, 1) + 1}{'+' if c else ''}", e, bar, where)
        out.append(f"c{c} {e:.1e} / {bar:.1e}{info}")
        assert e <= bar, (where, c, e, bar)
    print(f"  {what} npc={len(bars)}: " + "; ".join(out))


def _agree(group, what, a, b, bars, case):
    for c, (bar, exempt) in enumerate(bars):
        if not exempt:
            e = _note(group, what, np.abs(a[c] - b[c]).max(), bar, S.case_id(case) + f"-npc{len(bars)}")
            assert e <= bar, (case, c, e, bar)


def _host_inputs(case, npc):
    X = S.make(case)
    z0, tr = W.start_block(X, npc)
    return X, z0, tr


def _solver_name(d):
    return "mmb_pc_solve_mc" if d <= P.PC_SOLVE_MC_MAX_D else "pc_solve_kernel"


def _both_solvers(group, case, npc, Gd, z0d, tr, ref, alt, bars, n_iter=P.N_ITER, i8=False):
    d = Gd.shape[0]
    pc = _pc_solve_checked(Gd, z0d, npc, tr, n_iter)
    _hold(group, _solver_name(d), pc, ref, bars, case, alt, i8)
    if d <= P.PC_SOLVE_MC_MAX_D:  # the single-workgroup pc_solve16_kernel on the same G, z0
        pc1 = _pc_solve_direct(Gd, z0d, npc, tr, n_iter)
        _hold(group, "pc_solve16_kernel", pc1, ref, bars, case, alt, i8)
        _agree(group, "pc_solve16_kernel vs mmb_pc_solve_mc", pc1, pc, bars, case)
    return pc


# ------------------------------------------------------------------ 1: solvers from (G, z0)
G1_CASES = [c for fam in ("spike", "geom", "mean") for c in S.family_cases(fam)]


@pytest.mark.parametrize("case", G1_CASES, ids=[S.case_id(c) for c in G1_CASES])
def test_solvers_on_dominant_spectra(gpu, case):
    X = S.make(case)
    Gd = _dev(X.T @ X, gpu)
    for npc in S.NPCS[case[0]]:
        _, z0, tr = _host_inputs(case, npc)
        ref, alt = S.refs(case, npc)
        _both_solvers(1, case, npc, Gd, _dev(z0, gpu), tr, ref, alt, S.bars(case, npc))


# ------------------------------------------------------------------ 2: squared-round counts
G2_CASES = [("geom", n, d, R) for n, d in S.SHAPES[:3] for R in (1e4, 1e6)]


@pytest.mark.parametrize("n_iter", [3, 4, 5, 8])  # 1, 1, 2, 3 G2 rounds; 4, 8: a left-over G round
@pytest.mark.parametrize("case", G2_CASES, ids=[S.case_id(c) for c in G2_CASES])
def test_squared_round_counts(gpu, case, n_iter):
    """n_iter = 3 sends the block of a squared round straight into the direct
    branch's tail.  Before the last factor's pivot-ratio test (kPnTailPivot,
    csrc/pc_kernels.hip) mmb_pc_solve_mc was 2.7e-13 (R = 1e4), 9.4e-12 and
    1.35e-11 (R = 1e6; (4096, 300) and (700, 64)) from the reference here, with
    every pivot positive and pc_solve16_kernel at 1e-16; since then 3e-15."""
    X, z0, tr = _host_inputs(case, 1)
    G = X.T @ X
    ref = O.randomized_svd_components(X, 1, n_iter=n_iter)
    alt = O.pc_from_gram(G, z0, 1, tr, n_iter=n_iter)
    dv = np.abs(ref - alt).max(axis=1)
    print(f"  dev {dv[0]:.1e}")
    assert dv[0] <= 1e-13  # measured <= 6e-16: the 1e-12 floor is the bar
    _both_solvers(2, case, 1, _dev(G, gpu), _dev(z0, gpu), tr, ref, alt, S.bars_of(dv), n_iter)


# ------------------------------------------------------------------ 3: mmb_pc_solve_mc_xt
def _mc_xt(Gd, x, npc):
    n, d = x.shape
    k = npc + P.N_OVERSAMPLES
    om = P.omega(n, k, x.device)
    flag = torch.zeros(1, dtype=torch.int32, device=x.device)
    ws = torch.zeros(L.query("mmb_pc_solve_mc_ws_bytes", d), dtype=torch.uint8, device=x.device)
    pc = torch.full((npc, d), float("nan"), dtype=torch.float64, device=x.device)
    L.call("mmb_pc_solve_mc_xt", L.ptr(Gd), d, L.ptr(x), n, L.ptr(om), k, npc, P.N_ITER, L.ptr(pc),
           L.ptr(ws), L.ptr(flag), L.stream_ptr())
    torch.cuda.synchronize()
    assert int(flag.item()) == 0 and not bool(ws[:16].any())
    return pc, om


XT_SHAPES = [(n, d) for n, d in S.SHAPES if n < d <= P.PC_SOLVE_MC_MAX_D]
G3_CASES = [c for fam in ("spike", "mean") for c in S.family_cases(fam) if c[1:3] in XT_SHAPES]


@pytest.mark.parametrize("case", G3_CASES, ids=[S.case_id(c) for c in G3_CASES])
def test_transposed_start_in_one_launch(gpu, case):
    X = S.make(case)
    x = _dev(X, gpu, torch.float32)
    assert np.array_equal(x.double().cpu().numpy(), X)
    Gd = _dev(X.T @ X, gpu)
    for npc in S.NPCS[case[0]]:
        pc, om = _mc_xt(Gd, x, npc)
        two = _pc_solve_checked(Gd, P.xt_omega(x, None, om), npc, True)
        assert np.array_equal(pc.cpu().numpy(), two), (case, npc)
        ref, alt = S.refs(case, npc)
        _hold(3, "mmb_pc_solve_mc_xt", pc.cpu().numpy(), ref, S.bars(case, npc), case, alt)


# ------------------------------------------------------------------ 4: power-of-two scale
G4_CASES = [(fam, n, d, p) for n, d in S.SHAPES for fam, p in (("spike", 1e6), ("mean", 30.0))]


@pytest.mark.parametrize("case", G4_CASES, ids=[S.case_id(c) for c in G4_CASES])
def test_power_of_two_scale(gpu, case):
    """Every threshold of the solvers reads as relative: X -> 2^s X (G by
    2^(2s), the transposed start block by 2^s, the direct one unchanged)
    leaves the PC where it was."""
    npc = S.max_npc(case)
    X, z0, tr = _host_inputs(case, npc)
    n, d = X.shape
    G = X.T @ X
    entries = [("P.pc_solve", lambda Gd, z0d, xd: _pc_solve_checked(Gd, z0d, npc, tr))]
    if d <= P.PC_SOLVE_MC_MAX_D:
        entries.append(("mmb_pc_solve", lambda Gd, z0d, xd: _pc_solve_direct(Gd, z0d, npc, tr)))
        if tr:
            entries.append(("mmb_pc_solve_mc_xt", lambda Gd, z0d, xd: _mc_xt(Gd, xd, npc)[0].cpu().numpy()))
    for name, f in entries:
        base = f(_dev(G, gpu), _dev(z0, gpu), _dev(X, gpu, torch.float32))
        assert np.isfinite(base).all()
        for s in (-20, 20):
            Xs = np.ldexp(X, s)
            assert np.array_equal(Xs.astype(np.float32).astype(np.float64), Xs)
            pc = f(_dev(np.ldexp(G, 2 * s), gpu), _dev(np.ldexp(z0, s) if tr else z0, gpu),
                   _dev(Xs, gpu, torch.float32))
            e = _note(4, name, np.abs(pc - base).max(), 1e-13, S.case_id(case) + f"-2^{s}")
            print(f"  {name} 2^{s}: {e:.1e} (bar 1e-13), bit-equal: {np.array_equal(pc, base)}")
            assert e <= 1e-13


# ------------------------------------------------------------------ 5: close top pair
G5_CASES = S.family_cases("pair")


@pytest.mark.parametrize("case", G5_CASES, ids=[S.case_id(c) for c in G5_CASES])
def test_close_top_pair(gpu, case):
    X = S.make(case)  # f64 rows: only G and z0 go to the device
    Gd = _dev(X.T @ X, gpu)
    for npc in S.NPCS["pair"]:
        _, z0, tr = _host_inputs(case, npc)
        ref, alt = S.refs(case, npc)
        bars = S.bars(case, npc)
        assert not any(ex for _, ex in bars)
        _both_solvers(5, case, npc, Gd, _dev(z0, gpu), tr, ref, alt, bars)


# ------------------------------------------------------------------ 6: int8 Gram under a dominant mean
G6_CASES = S.i8_cases()


@pytest.mark.parametrize("case", G6_CASES, ids=[S.case_id(c) for c in G6_CASES])
def test_gram_i8_dominant_mean(gpu, case):
    X = S.make(case)
    x32 = X.astype(np.float32)
    xt = _dev(x32, gpu)
    cm = P.colmax(xt)
    assert np.array_equal(cm.cpu().numpy().view(np.float32), np.abs(x32).max(0))
    Gd = P.gram_i8(xt, cm)
    G = Gd.cpu().numpy()
    sliced, exact = O.sliced_gram(x32), X.T @ X
    e1 = _note(6, "G vs sliced oracle", np.abs(G - sliced).max() / np.abs(sliced).max(), 1e-13,
               S.case_id(case))
    e2 = _note(6, "G vs exact", np.abs(G - exact).max() / np.abs(exact).max(), 2e-9, S.case_id(case))
    print(f"  int8 Gram vs sliced oracle {e1:.3e} (bar 1e-13), vs exact {e2:.3e} (bar 2e-9)")
    assert e1 <= 1e-13 and e2 <= 2e-9 and np.array_equal(G, G.T)
    for npc in S.NPCS["mean"]:
        _, z0, tr = _host_inputs(case, npc)
        ref, alt = S.i8_refs(case, npc)
        _both_solvers(6, case, npc, Gd, _dev(z0, gpu), tr, ref, alt, S.i8_bars(case, npc), i8=True)


# ------------------------------------------------------------------ 7: removal under cancellation
REMOVE_N = 600


def _remove_errs(out, ref, X):
    """(f64-bar fraction, f32-bar fraction) of the largest row error."""
    err = np.abs(out - ref).max(axis=1)
    xm, rm = np.abs(X).max(axis=1), np.abs(ref).max(axis=1)
    return (err / (1e-12 * xm)).max(), (err / (F32_ROW * rm + 1e-12 * xm)).max()


@pytest.mark.parametrize("c", [3.0, 30.0, 300.0])
@pytest.mark.parametrize("d", [64, 260, 300, 400])
def test_remove_under_cancellation(gpu, d, c):
    case = ("mean", REMOVE_N, d, c)
    num32 = S.make(case).astype(np.float32)
    cnt32 = np.random.default_rng(d).integers(1, 8, size=REMOVE_N).astype(np.float32)
    num, cnt = _dev(num32, gpu), _dev(cnt32, gpu)
    X64 = S.make(case) * (1.0 + 1e-6 * np.random.default_rng(3).standard_normal((REMOVE_N, d)))
    for npc in (1, 2, 3):
        pch = S.refs(case, npc)[0]  # the oracle's PC of the rows: the removal cancels
        pc = _dev(pch, gpu)
        msg = []
        for c32, cd in ((None, None), (cnt32, cnt)):
            X = (num32 if c32 is None else (num32 / c32[:, None]).astype(np.float32)).astype(np.float64)
            ref = X - (X @ pch.T) @ pch
            cancel = (np.abs(X).max(axis=1) / np.abs(ref).max(axis=1)).max()
            o64 = P.remove_pc(num, cd, pc, torch.float64).cpu().numpy()
            o32 = P.remove_pc(num, cd, pc, torch.float32).cpu().numpy()
            assert o64.dtype == np.float64 and o32.dtype == np.float32
            where = f"d{d}-c{c:g}-npc{npc}" + ("-cnt" if cd is not None else "")
            e64 = _note(7, "mmb_pc_remove f64 out", _remove_errs(o64, ref, X)[0], 1.0, where)
            e32 = _note(7, "mmb_pc_remove f32 out", _remove_errs(o32, ref, X)[1], 1.0, where)
            msg.append(f"f64 out {e64:.3f}, f32 out {e32:.3f} (|x|/|ref| up to {cancel:.1e})")
            assert e64 <= 1.0 and e32 <= 1.0, (where, e64, e32)
        ref = X64 - (X64 @ pch.T) @ pch
        o = P.remove_pc_f64(_dev(X64, gpu), pc).cpu().numpy()
        e = _note(7, "mmb_pc_remove_f64", _remove_errs(o, ref, X64)[0], 1.0, f"d{d}-c{c:g}-npc{npc}")
        print(f"  npc={npc}: " + "; with cnt ".join(msg) + f"; f64 rows {e:.3f} (fractions of the bars)")
        assert e <= 1.0


# ------------------------------------------------------------------ 7 (epilogue), 8: FusedStep
STEP_DIMS = {260: (256, 320), 300: (300, 300)}  # D: (A, Vd)
PLANS = {"default": {},
         "remove": dict(stream_project=False, narrow_fused=False, fork_projection=False),
         "fork": dict(stream_project=False, narrow_fused=False, fork_projection=True)}


@functools.lru_cache(maxsize=2)
def _workload(N, D, c):
    """synth.device_workload with c g added to every word's row (a strong
    common component in the SIF rows); the pad row stays zero."""
    A, Vd = STEP_DIMS[D]
    inp = synth.device_workload(N, 20, 5000, D=D, A=A, Vd=Vd, seed=83, device="cuda")
    g = torch.randn(D, generator=torch.Generator().manual_seed(D), dtype=torch.float32)
    inp["table"][1:] += c * g.to(inp["table"].device)
    torch.manual_seed(0)
    gen = models.AudioVisualGeneratorMultimodal(D, A, Vd, norm=None).to("cuda")
    return inp, gen


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("kind", ["f64", "i8"])
@pytest.mark.parametrize("c", [3.0, 30.0])
@pytest.mark.parametrize("N", [97, 600])  # 97: the mmb_pc_solve_mc_xt gate of FusedStep._solve
@pytest.mark.parametrize("D", [260, 300])
def test_fused_step_common_component(gpu, D, N, c, kind, plan):
    inp, gen = _workload(N, D, c)
    step = P.FusedStep(inp, gen.networks(), gram_kind=kind, **PLANS[plan])
    assert step.plan.gram == kind, step.plan
    if plan != "default":
        assert step.plan.project == plan, step.plan
    s, _ = step.run()
    step.check()
    x = step.x.double().cpu().numpy()
    w = np.linalg.eigvalsh(x.T @ x)
    where = f"D{D}-N{N}-c{c:g}-{kind}-{plan}"
    bar = 1e-9 if kind == "i8" else 1e-10
    pc = step.pc.cpu().numpy()
    e = _note(8, f"PC ({kind} Gram)", np.abs(pc - O.compute_pc(x, 1)).max(), bar, where)
    # the rows against the f64 removal by the step's OWN pc: the removal
    # (its own launch, or the projection's epilogue) apart from the solve
    ref = x - (x @ pc.T) @ pc
    group, what = ((7, "mmb_mm2_project_x3_rmpc epilogue") if step.plan.project == "remove"
                   else (8, "SIF rows"))
    r = _note(group, what, _remove_errs(s.cpu().numpy(), ref, x)[1], 1.0, where)
    print(f"  plan {step.plan.front}/{step.plan.gram}/{step.plan.project}: l1/l2 of x {w[-1] / w[-2]:.3e}; "
          f"PC {e:.3e} (bar {bar}); SIF rows {r:.3f} of the f32 bar")
    assert e < bar and r <= 1.0
