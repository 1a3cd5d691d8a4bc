"""The entry-by-entry checker of the Gaussian likelihood and LayerNorm tests
(tests/test_gpu_gauss.py, tests/test_gpu_large.py) against the references and
bars of tests/gauss_cases.py.  Plain helper module: no test is collected from
it.

The checker records its comparison through the `note(what, ratio)` its caller
hands it, so it lands in the calling module's report.
"""
import numpy as np
import torch


def within(note, what, got, ref, bar):
    """Every entry within its bar; an entry whose bar is 0 (no frames) exact."""
    got = np.asarray(got.detach().cpu() if torch.is_tensor(got) else got, np.float64)
    ref, bar = np.asarray(ref), np.asarray(bar)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    err, pos = np.abs(got - ref), bar > 0
    assert (err[~pos] == 0).all(), what
    r = note(what, (err[pos] / bar[pos]).max() if pos.any() else 0.0)
    print(f"{what}: {r:.3f} of the bar")
    assert r <= 1.0, f"{what}: {r:.3f} of the bar"
