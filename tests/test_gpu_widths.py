"""GPU parity of the SIF and PC kernels at widths other than 300.

The drop-ins (sif_functions.compute_pc / remove_pc / get_weighted_average,
sif.get_sentence_embeddings) take an X or a word table of any width; under
them libmmb dispatches on the width d, the row count n, npc and pointer
alignment (csrc/gram_kernels.hip: mmb_gram's three routes; csrc/pc_kernels.hip:
the X^T Omega wave / generic kernels, the multi- and single-workgroup solvers;
csrc/pc_remove_kernels.hip: the vector / scalar removal; csrc/sif_kernels.hip:
the wave / workgroup weighted average).  The
shape table of tests/width_cases.py holds the smallest shapes at which each
route, partial tile and threshold is reached; every comparison is against
plain f64 numpy or the CPU oracle of the same operation, at the bar the
suite already holds the 300-wide path to:

  1 drop-ins over the table       PC 1e-10 (npc 1, 2) / 1e-8 (npc 6); removal rows
                                  1e-9 (f32-representable X) / 1e-12 (f64 rows) against
                                  the oracle's removal; where the PCs span X's whole row
                                  space (npc >= min(n, d): (2,2), (40,2) at npc 2, (1,300),
                                  (1,512)) both sides are rounding noise and the rows are
                                  held to a bound from the PC bar instead
  2 mmb_gram                      1e-13 of max |G| against exact f64; G == G^T
  3 mmb_colmax / mmb_gram_i8      bit-equal bounds; 1e-13 vs the sliced oracle; 2e-9 vs exact
  4 mmb_xt_omega(_f64)            1e-13 of max |Z0|
  5 mmb_pc_solve_mc, mmb_pc_solve 1e-12 (npc 1) / 1e-10 (npc 2) vs pc_from_gram; 1e-9 vs
                                  the Gram's top eigenvectors where the block is rank-deficient
  6 mmb_pc_remove(_f64)           f64 out 1e-12 row-relative; f32 out 2^-23 of the row's max
  7 mmb_sif_wavg                  2e-6 row-relative
  8 get_sentence_embeddings       1e-5 row-relative
  9 FusedStep at D != 300         PC 1e-10 (f64 Gram) / 1e-9 (int8 Gram); SIF rows 2^-23

tests/test_width_cases.py (CPU) pins that the oracle's own routes agree 4e4
times below the PC bars on this input family.  Unsupported widths are pinned
as MMBError (MMB_EINVAL before any launch).  Every test prints the largest
error it measured; the module prints the per-group maxima at the end.

Only the product library is loaded.
"""
import numpy as np
import pytest
import torch

import mmb_lib as L
import models
import pipeline as P
import sif
import sif_functions as SF
import synth
import width_cases as W
import widths_gpu as WG
from common_gpu import Ledger, _dev, _off
from oracle import mmb2_oracle as M
from oracle import sif_oracle as O
from width_cases import EMB_TOL, F32_ROW, PC_BAR, SOLVE_BAR
from widths_gpu import (SOLVE_CASES, _counts, _i8_rows, _pc_solve_checked, _pc_solve_direct, _solver_inputs,
                        _x_of)

pytestmark = pytest.mark.gpu

_WORST = Ledger()  # (group, what) -> [cases, largest error, bar]


def _note(group, what, err, bar):
    return _WORST.note((group, what), err, bar)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for (group, what), (cases, err, bar) in sorted(_WORST.items()):
        print(f"\nwidths group {group} {what}: {cases} comparisons, largest {err:.3e}, bar {bar:.3e}",
              end="")
    print()


def _off4(t):
    """A contiguous copy of f32 `t` that starts 4 bytes past a 16-byte boundary."""
    return _off(t, 1)


# ------------------------------------------------------------------ 1: drop-ins over the table
@pytest.mark.parametrize("f64rows", [False, True], ids=["f32rows", "f64rows"])
@pytest.mark.parametrize("n,d", W.SHAPES, ids=[W.shape_id(s) for s in W.SHAPES])
def test_dropins_over_the_table(gpu, n, d, f64rows):
    X = W.x64(n, d) if f64rows else W.x32(n, d)
    assert np.array_equal(X.astype(np.float32).astype(np.float64), X) != f64rows
    rbar = 1e-12 if f64rows else 1e-9
    for npc in W.npcs_of(n, d):
        ref = W.oracle_pc(n, d, npc, f64rows)
        pc = SF.compute_pc(X, npc)
        assert pc.shape == (npc, d) and pc.dtype == np.float64
        e = _note(1, f"PC npc={npc}", np.abs(pc - ref).max(), PC_BAR[npc])
        print(f"npc={npc}: PC {e:.3e} (bar {PC_BAR[npc]})", end="")
        assert e < PC_BAR[npc]
        out = SF.remove_pc(X, npc)
        assert out.shape == X.shape and out.dtype == np.float64
        if npc >= min(n, d):
            # the PCs span X's whole row space: the removal annihilates the
            # rows and both sides are rounding noise.  |x - (x.v) v| for a
            # unit v within dv of the exact one is <= 2 |x|_2 |dv|_2
            lim = 2 * np.sqrt(npc * d) * PC_BAR[npc] * np.linalg.norm(X, axis=1).max()
            r = np.abs(out).max()
            print(f"  annihilated rows {r:.3e} (bound {lim:.3e})")
            assert r < lim
            continue
        # O.remove_pc's expressions (sif_functions.py:77-80) on the oracle PC
        # computed above.  Closest to its bar: (5000, 17), f64 rows, npc = 6,
        # 9.8e-13 of 1e-12 with the device PC 1.4e-13 from the oracle's -- the
        # 6th and 7th singular values lie 0.9 % apart there, and on the CPU a
        # random PC perturbation of that size moves these rows by up to 3.7e-12
        ref_out = X - X.dot(ref.T) * ref if npc == 1 else X - X.dot(ref.T).dot(ref)
        r = _note(1, "removal " + ("f64 rows" if f64rows else "f32 rows") + f" npc={npc}",
                  M.row_rel_err(out, ref_out), rbar)
        print(f"  removal {r:.3e} (bar {rbar})")
        assert r < rbar


def test_dropins_reject_d513_and_npc7(gpu):
    X = W.make_x(40, 513)
    for f in (SF.compute_pc, SF.remove_pc):
        with pytest.raises(L.MMBError):
            f(X, 1)
        with pytest.raises(L.MMBError):
            f(X * (1.0 + 1e-6 * np.random.default_rng(3).standard_normal(X.shape)), 1)
        with pytest.raises(ValueError, match="npc"):
            f(W.x32(63, 64), 7)


# ------------------------------------------------------------------ 2: the Gram alone
@pytest.mark.parametrize("n,d", W.SHAPES, ids=[W.shape_id(s) for s in W.SHAPES])
def test_gram_routes(gpu, n, d):
    num32 = W.x32(n, d).astype(np.float32)
    cnt32 = _counts(n, n + d)
    num, cnt = _dev(num32, gpu), _dev(cnt32, gpu)
    worst = 0.0

    def check(G, ref, what):
        nonlocal worst
        worst = max(worst, WG._check_gram(_note, G, ref, what))

    X = _x_of(num32, None)
    exact = X.T @ X
    G0 = P.gram(num, None)
    check(G0, exact, "cnt=None")
    Xc = _x_of(num32, cnt32)
    exact_c = Xc.T @ Xc
    check(P.gram(num, cnt), exact_c, "cnt")
    check(P.gram(num, cnt, G0.clone(), accumulate=True), exact + exact_c, "accumulate")
    # 4 bytes off a 16-byte boundary: never the float4 row-range kernel
    check(P.gram(_off4(num), None), exact, "off alignment")
    check(P.gram(_off4(num), cnt), exact_c, "off alignment, cnt")
    print(f"largest |G - exact| / max |G|: {worst:.3e} (bar 1e-13)")


# ------------------------------------------------------------------ 3: the int8 Gram
@pytest.mark.parametrize("n", [7, 320, 5000])
@pytest.mark.parametrize("d", [4, 12, 20, 64, 260, 304])
def test_gram_i8_widths(gpu, n, d):
    x = _i8_rows(n, d)
    xt = _dev(x, gpu)
    cm = P.colmax(xt)
    assert np.array_equal(cm.cpu().numpy().view(np.float32), np.abs(x).max(0))
    WG._check_gram_i8(_note, P.gram_i8(xt, cm).cpu().numpy(), x)


@pytest.mark.parametrize("d", [308, 302])
def test_gram_i8_rejects(gpu, d):
    xt = _dev(W.make_x(64, d).astype(np.float32), gpu)
    cm = P.colmax(xt)
    assert np.array_equal(cm.cpu().numpy().view(np.float32), xt.abs().amax(0).cpu().numpy())
    with pytest.raises(L.MMBError):
        P.gram_i8(xt, cm)


# ------------------------------------------------------------------ 4: X^T Omega
T_SHAPES = [s for s in W.SHAPES if W.transposed(*s)]


@pytest.mark.parametrize("n,d", T_SHAPES, ids=[W.shape_id(s) for s in T_SHAPES])
def test_xt_omega_transposed_shapes(gpu, n, d):
    num32 = W.x32(n, d).astype(np.float32)
    cnt32 = _counts(n, n + d)
    num, cnt = _dev(num32, gpu), _dev(cnt32, gpu)
    x64 = W.x64(n, d)
    worst = 0.0
    for k in (11, 16):  # npc = 1 and npc = 6
        om = P.omega(n, k, gpu)
        omh = om.cpu().numpy()
        assert np.array_equal(omh, W.omega(n, k))
        for what, got, ref in (
                ("cnt=None", P.xt_omega(num, None, om), _x_of(num32, None).T @ omh),
                ("cnt", P.xt_omega(num, cnt, om), _x_of(num32, cnt32).T @ omh),
                ("f64 rows", P.xt_omega_f64(_dev(x64, gpu), None, om), x64.T @ omh)):
            assert got.shape == (d, k)
            e = _note(4, "X^T Omega", np.abs(got.cpu().numpy() - ref).max() / np.abs(ref).max(),
                      1e-13)
            worst = max(worst, e)
            assert e < 1e-13, (what, k, e)
    print(f"largest |Z0 - ref| / max |Z0|: {worst:.3e} (bar 1e-13)")


# ------------------------------------------------------------------ 5: the solvers from G, z0
@pytest.mark.parametrize("n,d,npc", SOLVE_CASES, ids=["n{}-d{}-npc{}".format(*c) for c in SOLVE_CASES])
def test_solvers_from_gram(gpu, n, d, npc):
    G, z0, tr, Gd, z0d = _solver_inputs(n, d, npc, gpu)
    if W.full_rank(n, d, npc):
        ref, bar, what = O.pc_from_gram(G, z0, npc, tr), SOLVE_BAR[npc], f"npc={npc} vs pc_from_gram"
    else:  # the block spans G's whole range: the PC is G's top eigenvectors
        ref, bar, what = W.top_eigvecs(G, npc), 1e-9, "rank-deficient vs eigenvectors"
    pc = _pc_solve_checked(Gd, z0d, npc, tr)
    assert np.isfinite(pc).all()
    name = "mmb_pc_solve_mc" if d <= P.PC_SOLVE_MC_MAX_D else "mmb_pc_solve (pc_solve_kernel)"
    e = _note(5, f"{name} {what}", np.abs(pc - ref).max(), bar)
    print(f"{name}: {e:.3e} (bar {bar})")
    assert e < bar
    if d <= P.PC_SOLVE_MC_MAX_D:  # the single-workgroup pc_solve16_kernel on the same G, z0
        if z0d.shape[1] > d:
            # a block wider than the space is rejected by the entry points
            # (pipeline.pc_solve narrows it to its first d columns, the same span)
            ws = torch.zeros(L.query("mmb_pc_solve_mc_ws_bytes", d), dtype=torch.uint8, device=gpu)
            with pytest.raises(L.MMBError):
                _pc_solve_direct(Gd, z0d, npc, tr)
            with pytest.raises(L.MMBError):
                L.call("mmb_pc_solve_mc", L.ptr(Gd), d, L.ptr(z0d), z0d.shape[1], npc, P.N_ITER,
                       int(tr), L.ptr(torch.empty_like(Gd[:npc])), L.ptr(ws), None, L.stream_ptr())
            z0d = z0d[:, :d].contiguous()
        pc1 = _pc_solve_direct(Gd, z0d, npc, tr)
        assert np.isfinite(pc1).all()
        e1 = _note(5, f"mmb_pc_solve (pc_solve16_kernel) {what}", np.abs(pc1 - ref).max(), bar)
        e2 = _note(5, "pc_solve16_kernel vs mmb_pc_solve_mc", np.abs(pc1 - pc).max(), 1e-12)
        print(f"pc_solve16_kernel: {e1:.3e} (bar {bar}); against mmb_pc_solve_mc {e2:.3e} (bar 1e-12)")
        assert e1 < bar and e2 < 1e-12


@pytest.mark.parametrize("n_iter", [0, 1, 7])
@pytest.mark.parametrize("n,d", [(5000, 17), (64, 64), (700, 321), (512, 512)])
def test_solvers_iteration_counts(gpu, n, d, n_iter):
    G, z0, tr, Gd, z0d = _solver_inputs(n, d, 1, gpu)
    ref = O.pc_from_gram(G, z0, 1, tr, n_iter=n_iter)
    e = _note(5, "n_iter 0/1/7", np.abs(_pc_solve_checked(Gd, z0d, 1, tr, n_iter) - ref).max(), 1e-12)
    if d <= P.PC_SOLVE_MC_MAX_D:
        e = max(e, _note(5, "n_iter 0/1/7",
                         np.abs(_pc_solve_direct(Gd, z0d, 1, tr, n_iter) - ref).max(), 1e-12))
    print(f"n_iter={n_iter}: {e:.3e} (bar 1e-12)")
    assert e < 1e-12


def test_solver_rejects_d513(gpu):
    G = torch.eye(513, dtype=torch.float64, device=gpu)
    z0 = P.omega(513, 11, gpu)
    with pytest.raises(L.MMBError):
        P.pc_solve(G, z0, 1, False)


# ------------------------------------------------------------------ 6: removal with a given PC
REMOVE_D = [2, 5, 50, 64, 128, 129, 255, 256, 260, 300, 301, 512, 516, 1024, 1028, 2048]


def _remove_supported(d, npc, vector):
    """mmb_pc_remove's limits: float4 rows (d % 4 == 0, 16-byte aligned num and
    out32) up to 2048 wide, scalar rows up to 512, the PCs (npc x d f64) in
    64 KiB of LDS."""
    return d <= (2048 if vector else 512) and npc * d * 8 <= 64 * 1024


@pytest.mark.parametrize("off", [False, True], ids=["aligned", "off4"])
@pytest.mark.parametrize("d", REMOVE_D)
def test_remove_given_pc(gpu, d, off):
    w32 = w64 = 0.0
    for n in (1, 5, 1000):
        rng = np.random.default_rng(1000 * n + d)
        num32 = (0.4 * rng.standard_normal((n, d)) + 0.3).astype(np.float32)
        cnt32 = _counts(n, n + d)
        num = _dev(num32, gpu)
        num = _off4(num) if off else num
        cnt = _dev(cnt32, gpu)
        vector = d % 4 == 0 and not off
        for npc in (npc for npc in W.NPCS if npc <= d):
            pch = W.orthonormal_rows(npc, d, seed=d + npc)
            assert np.abs(pch @ pch.T - np.eye(npc)).max() < 1e-14
            pc = _dev(pch, gpu)
            for c32, c in ((None, None), (cnt32, cnt)):
                if not _remove_supported(d, npc, vector):
                    for dt in (torch.float32, torch.float64):
                        with pytest.raises(L.MMBError):
                            P.remove_pc(num, c, pc, dt)
                    continue
                X = _x_of(num32, c32)
                ref = X - (X @ pch.T) @ pch
                o64 = P.remove_pc(num, c, pc, torch.float64).cpu().numpy()
                o32 = P.remove_pc(num, c, pc, torch.float32).cpu().numpy()
                assert o64.dtype == np.float64 and o32.dtype == np.float32
                rmax = np.abs(ref).max(axis=1, keepdims=True)
                if npc == d:  # the whole space removed: rounding noise of |x| on both sides
                    assert np.abs(o64).max() < 1e-13 * np.abs(X).max()
                    assert np.abs(o32).max() < 1e-13 * np.abs(X).max()
                    continue
                e64 = _note(6, "f64 out", M.row_rel_err(o64, ref), 1e-12)
                e32 = _note(6, "f32 out (of 2^-23)", (np.abs(o32 - ref) / rmax).max() / F32_ROW, 1.0)
                w64, w32 = max(w64, e64), max(w32, e32)
                assert e64 < 1e-12, (n, npc, c is not None, e64)
                assert e32 <= 1.0, (n, npc, c is not None, e32)
    print(f"f64 out {w64:.3e} (bar 1e-12); f32 out {w32:.3f} of 2^-23 of the row's max")


@pytest.mark.parametrize("d", [d for d in REMOVE_D if d <= 512])
def test_remove_f64_rows_given_pc(gpu, d):
    worst = 0.0
    for n in (1, 5, 1000):
        rng = np.random.default_rng(1000 * n + d)
        X = 0.4 * rng.standard_normal((n, d)) + 0.3
        for npc in (npc for npc in W.NPCS if npc < d):
            pch = W.orthonormal_rows(npc, d, seed=d + npc)
            ref = X - (X @ pch.T) @ pch
            out = P.remove_pc_f64(_dev(X, gpu), _dev(pch, gpu)).cpu().numpy()
            e = _note(6, "f64 rows", M.row_rel_err(out, ref), 1e-12)
            worst = max(worst, e)
            assert e < 1e-12, (n, npc, e)
    print(f"mmb_pc_remove_f64: {worst:.3e} (bar 1e-12)")


def test_remove_rejections(gpu):
    pc1 = lambda d: _dev(W.orthonormal_rows(1, d, seed=d), gpu)
    for d, off in ((2052, False), (513, False), (516, True)):  # vector, scalar, scalar by alignment
        num = torch.zeros((8, d), dtype=torch.float32, device=gpu)
        num = _off4(num) if off else num
        for dt in (torch.float32, torch.float64):
            with pytest.raises(L.MMBError):
                P.remove_pc(num, None, pc1(d), dt)
    with pytest.raises(L.MMBError):
        P.remove_pc_f64(torch.zeros((8, 513), dtype=torch.float64, device=gpu), pc1(513))


# ------------------------------------------------------------------ 7: the weighted average
WAVG_N, WAVG_V = 300, 2000


def _wavg_inputs(D, Lw):
    E = synth.word_table(WAVG_V, D, seed=D)
    wt = synth.sif_weights(WAVG_V, w0=0.0)
    ids = synth.token_ids(WAVG_N, Lw, WAVG_V, seed=Lw, ragged=True)
    return E, ids, O.seq2weight(ids, np.ones(ids.shape), wt)


@pytest.mark.parametrize("D", [2, 5, 50, 100, 200, 256, 260, 301, 320, 512, 516, 1280])
def test_weighted_average_widths(gpu, D):
    worst = 0.0
    for Lw in (1, 40, 64, 65, 256):  # 64 | 65: the wave / workgroup kernels' boundary
        E, ids, w = _wavg_inputs(D, Lw)
        ref = O.get_weighted_average(E, ids, w)
        got = SF.get_weighted_average(E, ids, w)
        assert got.dtype == np.float64 and got.shape == (WAVG_N, D)
        assert np.isfinite(ref).all()
        e = _note(7, "weighted average", M.row_rel_err(got, ref), 2e-6)
        worst = max(worst, e)
        assert e < 2e-6, (Lw, e)
    print(f"largest row-relative error: {worst:.3e} (bar 2e-6)")


@pytest.mark.filterwarnings("ignore:invalid value encountered")
def test_weighted_average_edges(gpu):
    """D = 300 with the table 4 bytes off alignment (the scalar workgroup
    kernel at any L), a negative id (wraps; weight 0) and an all-padding row
    (0 / 0 = NaN on both sides)."""
    for Lw in (40, 65):
        E, ids, w = _wavg_inputs(300, Lw)
        ids[3, :2] = -5, 7  # (a real token beside the negative id)
        ids[1, :] = 0
        w = O.seq2weight(ids, np.ones(ids.shape), synth.sif_weights(WAVG_V, w0=0.0))
        ref = O.get_weighted_average(E, ids, w)
        assert np.isnan(ref[1]).all()
        ok = ~np.isnan(ref).any(axis=1)
        assert ok.sum() == WAVG_N - 1
        got = SF.get_weighted_average(E, ids, w)
        table = _off4(_dev(E, gpu))
        flag = torch.zeros(1, dtype=torch.int32, device=gpu)
        got_off = P.weighted_sum(table, _dev(ids, gpu, torch.int32), w=_dev(w, gpu), flag=flag,
                                 x_out=True).double().cpu().numpy()
        assert int(flag.item()) == L.MMB_FLAG_ZERO_WEIGHTS  # the all-padding row; no id out of range
        for what, g in (("aligned", got), ("off alignment", got_off)):
            assert np.isnan(g[1]).all(), what
            e = _note(7, "edges (D=300)", M.row_rel_err(g[ok], ref[ok]), 2e-6)
            print(f"L={Lw} {what}: {e:.3e} (bar 2e-6)")
            assert e < 2e-6


@pytest.mark.parametrize("D", [321, 1284])
def test_weighted_average_rejects(gpu, D):
    E, ids, w = _wavg_inputs(D, 40)
    with pytest.raises(L.MMBError):
        SF.get_weighted_average(E, ids, w)
    E, ids, w = _wavg_inputs(D, 65)
    with pytest.raises(L.MMBError):
        SF.get_weighted_average(E, ids, w)


# ------------------------------------------------------------------ 8: end to end
@pytest.mark.parametrize("N,Lw,V", [(700, 40, 5000), (150, 70, 5000)])
@pytest.mark.parametrize("D", [5, 17, 50, 100, 200, 512])
def test_sentence_embeddings_widths(gpu, D, N, Lw, V):
    E = synth.word_table(V, D, seed=N + D)
    wt = synth.sif_weights(V, w0=1.0)
    ids = synth.token_ids(N, Lw, V, seed=Lw + D, ragged=True)
    ref = O.get_sentence_embeddings(E, wt, ids)
    got = sif.get_sentence_embeddings(E, wt, ids)
    assert got.dtype == np.float64 and got.shape == (N, D)
    e = _note(8, "sentence embeddings", M.row_rel_err(got, ref), EMB_TOL)
    print(f"row-relative error {e:.3e} (bar {EMB_TOL})")
    assert e < EMB_TOL


# ------------------------------------------------------------------ 9: FusedStep at other widths
# (D, A, Vd) with the frame widths of tests/test_gpu_fused_tail.py
STEP_DIMS = {256: (300, 4), 260: (256, 320), 316: (300, 20), 320: (260, 256)}
STEP_CASES = [(D, N, kind, None) for D in STEP_DIMS for N in (97, 2500)
              for kind in (("f64", "i8") if D % 4 == 0 and D <= 304 else ("f64",))]
STEP_CASES.append((260, 2500, "f64", 2))  # two chunks: the "parts" Gram


@pytest.mark.parametrize("D,N,kind,chunks", STEP_CASES,
                         ids=["D{}-N{}-{}{}".format(D, N, k, "-chunks2" if c else "")
                              for D, N, k, c in STEP_CASES])
def test_fused_step_pc_and_sif_rows(gpu, D, N, kind, chunks):
    A, Vd = STEP_DIMS[D]
    inp = synth.device_workload(N, 40, 5000, D=D, A=A, Vd=Vd, seed=83, device=gpu)
    torch.manual_seed(0)
    gen = models.AudioVisualGeneratorMultimodal(D, A, Vd, norm=None).to(gpu)
    step = P.FusedStep(inp, gen.networks(), gram_kind=kind, chunks=chunks)
    assert step.plan.gram == ("parts" if chunks else kind), step.plan
    s, _ = step.run()
    step.check()
    x = step.x.double().cpu().numpy()
    ref_pc = O.compute_pc(x, 1)
    bar = 1e-9 if kind == "i8" else 1e-10
    e = _note(9, f"PC ({step.plan.gram} Gram)", np.abs(step.pc.cpu().numpy() - ref_pc).max(), bar)
    ref = O.remove_pc(x, 1)
    r = _note(9, "SIF rows (of 2^-23)",
              (np.abs(s.cpu().numpy() - ref) / np.abs(ref).max(axis=1, keepdims=True)).max() / F32_ROW,
              1.0)
    print(f"plan {step.plan.front}/{step.plan.gram}: PC {e:.3e} (bar {bar}); "
          f"SIF rows {r:.3f} of 2^-23 of the row's max")
    assert e < bar and r <= 1.0
