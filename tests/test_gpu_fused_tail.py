"""GPU parity of the fused stream + projection kernel's row-tail layout.

The pipelined streamers of mmb_mm2_stream_project load a row's columns from
256 on with one 32-bit load per lane (lane l: column 256 + l, clamped to the
row's last column) and keep one float per lane of tail sums; a piece of at
most 256 columns issues no tail load at all.  The cases are the smallest
shapes at which that layout can go wrong: no tail (256), a 4-float tail
(260), 44 (300), 60 (316) and all 64 tail lanes live (320); frame pieces far
narrower than a wave's 64 float4 columns (4, 20); the three modalities'
widths different within a case, so that each piece's choice and the
prefetch of the next piece's first group (another width, with or without a
tail) are exercised in every combination of neighbours; row lengths of one
frame, partial last groups, whole groups, T = 64, and the lengths either
side of the pipelined streamer's ">= 3 groups per row" rule for 8-frame
groups (16 | 17) and 10-frame groups (20 | 21) -- below it the launch falls
back to the group-at-a-time streamer, which keeps the float4 tail; row
counts giving a single row, partial 48-row batches and partial 12-row
shares of the four streamer waves.

Asserted as tests/test_gpu_mmb2.py::test_stream_project_matches_two_kernel_step
does: x, the count and the column bounds bit-identical to the two-kernel step
(mmb_mm2_stream -> HBM s -> mmb_mm2_project_x3), MMB2 rows < 1e-6
row-relative against it and < 1e-5 against the CPU oracle, flag word 0 (the
bad-id case: the out-of-range bit, as the two-kernel step reports it).

Only the product library is loaded.
"""
import numpy as np
import pytest
import torch

import mmb_lib as L
import models
import pipeline as P
import synth
from fused_cases import CASES, V, _ids
from mmb2_cases import TOL
from oracle import mmb2_oracle as M

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("D,A,Vd,T,N,bad", CASES, ids=[_ids(c) for c in CASES])
def test_fused_tail_matches_two_kernel_step_and_oracle(gpu, D, A, Vd, T, N, bad):
    assert A != Vd and P.stream_project_supported(T, D, A, Vd)
    inp = synth.device_workload(N, T, V, D=D, A=A, Vd=Vd, seed=83, device=gpu)
    if bad:  # a negative id wraps (weight 0); an id >= V is flagged and contributes a zero row
        inp["ids"][3, 5] = -7
        inp["ids"][N // 2, T - 1] = V + 11
    torch.manual_seed(0)
    gen = models.AudioVisualGeneratorMultimodal(D, A, Vd, norm=None).to(gpu)
    # the two-kernel step (one-pass projection: the split-K one sums K in another f32 order)
    b = P.FusedStep(inp, gen.networks(), stream_project=False, split_projection=False)
    assert not b.stream_project and b.proj_split is None
    _, m2 = b.run()
    # the fused kernel, launched as the step launches it, with the column bounds at every D
    proj = P.MMB2Projection(gen.networks(), D, A, Vd, T, gpu)
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    colmax = torch.empty(D, dtype=torch.int32, device=gpu)
    ws = torch.empty(L.query("mmb_mm2_colmax_ws_bytes", D), dtype=torch.uint8, device=gpu)
    x, aux, m1 = P.mm2_stream_project(N, T, D, A, Vd, inp["audio"], inp["visual"], proj,
                                      ids32=inp["ids"], table=inp["table"], wtab32=inp["wtab"],
                                      flag=flag, colmax=colmax, colmax_ws=ws)
    torch.cuda.synchronize()
    f1, f2 = int(flag.item()), int(b.flag.item())
    print(f"flag fused {f1} two-kernel {f2}")
    assert f1 == f2 and (f1 != 0) == bad
    # column bounds: the bits of max |x| per column (non-negative floats order like their bits)
    bounds = b.x.abs().amax(dim=0).contiguous().view(torch.int32)
    print("x equal", torch.equal(x, b.x), "count equal", torch.equal(aux[0], b.aux[0]),
          "bounds equal", torch.equal(colmax, bounds))
    assert torch.equal(x, b.x) and torch.equal(aux[0], b.aux[0])
    assert torch.equal(colmax, bounds)
    e2 = M.row_rel_err(m1.cpu().numpy(), m2.cpu().numpy())
    print(f"MMB2 rows vs the two-kernel step: {e2:.3e} (bar 1e-6)")
    assert e2 < 1e-6
    if N == 1 or bad:  # the reference's gpu2 cannot take one utterance; it raises on an id >= V
        return
    E = inp["table"].cpu().numpy()
    wt = inp["wtab"].cpu().numpy().astype(np.float64)
    ids = inp["ids"].cpu().numpy().astype(np.int64)
    sw = np.where(ids >= 0, wt.astype(np.float32)[ids], 0).astype(np.float32)
    text = E[ids]
    ref = M.estimate_embedding_overall_gpu2(
        M.concat_inputs(text, inp["audio"].cpu().numpy(), inp["visual"].cpu().numpy()),
        M.params_from_module(gen.cpu()), sw, text)
    e1 = M.row_rel_err(m1.cpu().numpy(), ref)
    print(f"MMB2 rows vs the oracle: {e1:.3e} (bar {TOL})")
    assert e1 < TOL
