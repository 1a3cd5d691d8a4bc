"""What the GPU tests of the Gram, PC solve, removal and SIF kernels share
(tests/test_gpu_widths.py, tests/test_gpu_spectrum.py, tests/test_gpu_scratch.py,
tests/test_gpu_large.py): the seeded row counts and the f32 division the
kernels do, the int8 Gram's input family, the solvers' inputs from a Gram, the
two solver launches (mmb_pc_solve itself; P.pc_solve with its flag and control
words checked), and the two Gram checkers.  The
bars themselves (PC_BAR, SOLVE_BAR, EMB_TOL, F32_ROW) are pure numbers and
stand in tests/width_cases.py.  Plain helper module: no test is collected
from it.

A checker records every comparison through the `note(group, what, error, bar)`
its caller hands it, so each lands in the calling module's report.
"""
import numpy as np
import torch

import mmb_lib as L
import pipeline as P
import width_cases as W
from common_gpu import _dev
from oracle import sif_oracle as O
from width_cases import SOLVE_BAR

SOLVE_CASES = [(n, d, npc) for n, d, npc in W.pc_cases() if npc in SOLVE_BAR]


def _counts(n, seed):
    """Positive per-row counts as f32 (count_nonzero(w) of sif_functions.py:55)."""
    return np.random.default_rng(seed).integers(1, 8, size=n).astype(np.float32)


def _x_of(num32, cnt32):
    """X = f32(num) / f32(cnt), the f32 division the kernels do, widened."""
    if cnt32 is None:
        return num32.astype(np.float64)
    return (num32 / cnt32[:, None]).astype(np.float32).astype(np.float64)


def _check_gram(note, G, ref, what):
    """G (device or numpy) is symmetric and within 1e-13 of max |G| of the
    exact f64 Gram `ref`; returns the error."""
    G = G.cpu().numpy() if isinstance(G, torch.Tensor) else G
    assert np.array_equal(G, G.T), what
    e = note(2, "Gram", np.abs(G - ref).max() / np.abs(ref).max(), 1e-13)
    assert e < 1e-13, (what, e)
    return e


def _i8_rows(n, d):
    """Heavy-tailed t(3) rows with one all-zero column (f32)."""
    rng = np.random.default_rng(1000 * n + d)
    x = rng.standard_t(3, size=(n, d)).astype(np.float32)
    x[:, d // 2] = 0.0
    return x


def _check_gram_i8(note, G, x):
    """The int8 Gram G (numpy) of the f32 rows x: symmetric, 1e-13 against the
    sliced oracle, 2e-9 against the exact f64 Gram."""
    ref = O.sliced_gram(x)
    exact = x.astype(np.float64).T @ x.astype(np.float64)
    e1 = note(3, "vs sliced oracle", np.abs(G - ref).max() / np.abs(ref).max(), 1e-13)
    e2 = note(3, "vs exact", np.abs(G - exact).max() / np.abs(exact).max(), 2e-9)
    print(f"int8 Gram vs sliced oracle {e1:.3e} (bar 1e-13), vs exact {e2:.3e} (bar 2e-9)")
    assert e1 <= 1e-13 and e2 <= 2e-9
    assert np.array_equal(G, G.T)


def _solver_inputs(n, d, npc, gpu):
    X = W.x32(n, d)
    G = X.T @ X
    z0, tr = W.start_block(X, npc)
    return G, z0, tr, _dev(G, gpu), _dev(z0, gpu)


def _pc_solve_direct(Gd, z0d, npc, tr, n_iter=P.N_ITER):
    """mmb_pc_solve itself: pc_solve16_kernel (d <= 320) or pc_solve_kernel."""
    d, k = Gd.shape[0], z0d.shape[1]
    pc = torch.full((npc, d), float("nan"), dtype=torch.float64, device=Gd.device)
    L.call("mmb_pc_solve", L.ptr(Gd), d, L.ptr(z0d), k, npc, n_iter, int(tr), L.ptr(pc),
           L.stream_ptr())
    return pc.cpu().numpy()


def _pc_solve_checked(Gd, z0d, npc, tr, n_iter=P.N_ITER):
    """P.pc_solve with a flag and a workspace of the test's own: the flag stays
    0 and the multi-workgroup solver leaves its control words zero."""
    d = Gd.shape[0]
    flag = torch.zeros(1, dtype=torch.int32, device=Gd.device)
    ws = (torch.zeros(L.query("mmb_pc_solve_mc_ws_bytes", d), dtype=torch.uint8, device=Gd.device)
          if d <= P.PC_SOLVE_MC_MAX_D else None)
    pc = P.pc_solve(Gd, z0d, npc, tr, n_iter=n_iter, flag=flag, ws=ws).cpu().numpy()
    assert int(flag.item()) == 0
    assert ws is None or not bool(ws[:16].any())
    return pc
