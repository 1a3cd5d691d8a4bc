"""What the GPU tests of the sentiment regressor's kernels share
(tests/test_gpu_regressor_widths.py, tests/test_gpu_scratch.py,
tests/test_gpu_large.py): float32 device copies, float64 host copies, the
element-by-element checker against the float64 reference at the derived bound,
and one mmb_mlp_train launch with its workspace.  The floor of the training
bars (regressor_cases.FLOOR) is a pure number and stands with the case tables.
Plain helper module: no test is collected from it.

The checker records its comparison through the `note(group, what, ratio)` its
caller hands it, so it lands in the calling module's report.
"""
import numpy as np
import torch

import mmb_lib as L
import regressor_cases as C
from common_gpu import _dev32 as _dev


def _host64(t):
    return t.cpu().numpy().astype(np.float64)


def _ratio(err, bar):
    """The largest err / bar, elementwise (bar 0 means the value must be exact)."""
    err, bar = np.asarray(err, np.float64), np.broadcast_to(np.asarray(bar, np.float64), np.shape(err))
    ratio = np.where(err == 0, 0.0, err / np.maximum(bar, 1e-300))
    return float(ratio.max()) if ratio.size else 0.0


def _check(note, group, what, got, ref, bound):
    """|got - ref| <= 2 bound, element by element."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    r = note(group, what, _ratio(np.abs(got - ref), 2 * bound))
    assert r <= 1.0, f"{what}: {r:.3f} of the derived bar"
    return r


def _launch_train(gpu, c, z, ws):
    """One mmb_mlp_train launch of a case from its initial parameters; returns
    (rc, params, step_loss, valid_loss, flag) as device tensors."""
    d, h, o, batch = c.d, c.h, c.o, c.batch
    x, y = _dev(z["x"], gpu), _dev(z["y"], gpu)
    P = [_dev(p, gpu) for p in z["params"]]
    perm = _dev(z["perm"], gpu, torch.int64)
    spe = -(-c.n // batch)
    sl = torch.full((C.N_EPOCHS * spe,), np.nan, device=gpu)
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    vl, keep = None, []
    vargs = (None, None, None, 0, 1, c.epoch0, None)
    if z["valid"] is not None:
        xv, yv, vperm, every, epoch0 = z["valid"]
        keep = [_dev(xv, gpu), _dev(yv, gpu), _dev(vperm, gpu, torch.int64)]
        vl = torch.full((max(C.n_validations(c), 1) * -(-c.nv // batch),), np.nan, device=gpu)
        vargs = (*[L.ptr(t) for t in keep], c.nv, every, epoch0, L.ptr(vl))
    rc = L.query("mmb_mlp_train", L.ptr(x), L.ptr(y), L.ptr(perm), c.n, C.N_EPOCHS, batch, d, h, o,
                 C.LR, *[L.ptr(p) for p in P], L.ptr(sl), *vargs, L.ptr(ws), L.ptr(flag), L.stream_ptr())
    torch.cuda.synchronize()
    return rc, P, sl, vl, flag


def _workspace(gpu, d, h, slack=1):
    return torch.zeros(slack * (L.query("mmb_mlp_workspace_bytes", d, h) // 4 + 4), dtype=torch.int32,
                       device=gpu)
