"""What every GPU test module shares: device copies, misaligned copies, the
small launch buffers, the error-as-a-fraction-of-its-bar helper and the ledger
behind each module's "largest error" report.  Plain helper module: no test is
collected from it.  Used by the family helpers (tests/frames16_gpu.py,
mmb2_gpu.py, widths_gpu.py, regressor_gpu.py, gauss_gpu.py, large_gpu.py) and
by the GPU test modules directly.

The two bars every family shares are defined with the case tables
(mmb2_cases.TOL, width_cases.F32_ROW) and passed on here under their names.
"""
import copy

import numpy as np
import torch

import mmb2_cases as C
import mmb_lib as L
from mmb2_cases import TOL  # noqa: F401  (the end-to-end bar of the suite)
from width_cases import F32_ROW  # noqa: F401  (one f32 rounding of the row's max, doubled)


class Ledger:
    """Per key, the number of comparisons noted, the largest value among them
    and what came with that value (its bar, or where it was measured).  Each
    reporting test module owns one and prints it from its own `_report`
    fixture; a checker in a helper module is handed the module's `note` and
    never keeps a ledger of its own."""

    def __init__(self):
        self.worst = {}  # key -> [comparisons, largest value, *extra of the note that set it]

    def note(self, key, value, *extra):
        w = self.worst.setdefault(key, [0, 0.0, *extra])
        w[0] += 1
        if float(value) >= w[1]:
            w[1:] = [float(value), *extra]
        return float(value)

    def items(self):
        """(key, [comparisons, largest value, *extra]), in the order of first notes."""
        return self.worst.items()


def _unnoted(group, what, value, *bar):
    """The `note` of a caller that records the checker's returned value itself."""
    return float(value)


def _dev(a, gpu, dtype=None):
    """A contiguous device copy of a tensor or an array-like (None stays None).
    A host array is copied first: several case tables hand out read-only
    cached arrays."""
    if a is None:
        return None
    t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.array(a))
    return (t if dtype is None else t.to(dtype)).to(gpu).contiguous()


def _dev32(a, gpu, dtype=torch.float32):
    """_dev for the families whose uploads are float32 unless told otherwise
    (the regressor, the word likelihood, the Gaussian likelihood)."""
    return _dev(a, gpu, dtype)


def _off(t, elements):
    """A contiguous copy of `t` that starts `elements` elements past a 16-byte boundary."""
    flat = torch.empty(t.numel() + elements, dtype=t.dtype, device=t.device)
    out = flat[elements:].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 == elements * t.element_size()
    return out


def _i32(t):
    return t.contiguous().view(torch.int32)


def _flag(gpu):
    return torch.zeros(1, dtype=torch.int32, device=gpu)


def _colmax_bufs(D, gpu):
    nb = L.query("mmb_mm2_colmax_ws_bytes", D)
    return (torch.zeros(D, dtype=torch.int32, device=gpu),
            torch.empty((nb + 15) // 16 * 16, dtype=torch.uint8, device=gpu))


def _untouched(out):
    torch.cuda.synchronize()
    return all(bool((t == -7.0).all()) for t in out)


def _networks(case, gpu):
    """The case's generator on the device (a copy: the cached one stays on the CPU)."""
    return copy.deepcopy(C.generator(*case[:3])).to(gpu).networks()


def _frac(err, bar):
    """max err / bar; where the bar is 0 (no term at all) the value must be exact."""
    err, bar = np.asarray(err, np.float64), np.asarray(bar, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        f = np.where(bar > 0, err / bar, np.where(err == 0, 0.0, np.inf))
    return float(f.max()) if f.size else 0.0
