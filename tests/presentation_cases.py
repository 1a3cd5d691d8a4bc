"""Presentations: the same logical values handed over in another form.

The reference's numpy and torch functions take float64, Fortran-order,
strided, broadcast and read-only operands; the mirrors hand bare pointers to
the C ABI (include/mmb.h), so each must bring every such form to the layout
and element type its kernels read.  Every value here is float32-representable,
so every presentation reaches the kernels with identical bits and the results
must be bit for bit the baseline's (tests/test_gpu_presentations.py; the
builders themselves are pinned by tests/test_presentation_cases.py on the
CPU).  Plain helper module: no test is collected from it.

numpy (sif_functions, sif)                 torch (sif2, losses, latent, sentiment_model)
  N0 float32 / int64, C order                T0 float32 / int64, contiguous, on the GPU
  N1 float64, the same values                T1 the same on the CPU
  N2 Fortran order                           T2 float64, the same values
  N3 big[::2, 1::2] of a larger array        T3a a column block of a wider tensor
  N4 a negative row stride                   T3b a stepped slice in the leading axis
  N5 ids as int32 / int16 / uint8 / list     T3c storage that is the transpose
  N6 a read-only array                       T4 broadcast with stride 0
  N7 the mask as bool / int / float          T5 a requires_grad leaf, no-grad call
                                             T6 ids as int32 and int64

The filler around a strided view is NaN (floats) or a valid but different
value (integers), so an element read at a wrong stride changes the result.
"""
from __future__ import annotations

import collections

import numpy as np
import torch

# ---------------------------------------------------------------- numpy builders
# each takes the baseline (a C-contiguous array) and returns the presentation


def _filler(a):
    return np.nan if a.dtype.kind == "f" else 1


def n_float64(a):
    return np.array(a, dtype=np.float64, order="C")


def n_fortran(a):
    return np.array(a, order="F")


def n_stepped(a):
    """big[::2, 1::2] (2-D) or big[1::2] (1-D) of a larger array."""
    if a.ndim == 1:
        big = np.full(2 * a.shape[0] + 1, _filler(a), dtype=a.dtype)
        big[1::2] = a
        return big[1::2]
    big = np.full((2 * a.shape[0], 2 * a.shape[1] + 1), _filler(a), dtype=a.dtype)
    big[::2, 1::2] = a
    return big[::2, 1::2]


def n_negative(a):
    """A view that walks its rows backwards in memory."""
    return np.ascontiguousarray(a[::-1])[::-1]


def n_readonly(a):
    b = a.copy()
    b.setflags(write=False)
    return b


NUMPY_FORMS = {"N1": n_float64, "N2": n_fortran, "N3": n_stepped, "N4": n_negative, "N6": n_readonly}
# N5: token ids (uint8 where every id fits; the list is nested Python ints)
ID_FORMS = {"N5-int32": lambda a: a.astype(np.int32), "N5-int16": lambda a: a.astype(np.int16),
            "N5-uint8": lambda a: a.astype(np.uint8), "N5-list": lambda a: a.tolist()}
# N7: the seq2weight mask (0 / 1 values)
MASK_FORMS = {"N7-bool": lambda a: a > 0, "N7-int": lambda a: a.astype(np.int64),
              "N7-float": lambda a: a.astype(np.float64)}


def numpy_forms(a, ids=False):
    """(id, builder) of every numpy presentation that applies to the baseline
    `a`: float64 only to floats, Fortran order only past one axis."""
    out = []
    for k, f in NUMPY_FORMS.items():
        if k == "N1" and a.dtype.kind != "f":
            continue
        if k == "N2" and a.ndim < 2:
            continue
        out.append((k, f))
    if ids:
        out += [(k, f) for k, f in ID_FORMS.items() if k != "N5-uint8" or int(a.max()) <= 255]
    return out


# ---------------------------------------------------------------- torch builders
# each takes the baseline (a contiguous tensor, on any device) and returns the
# presentation on the same device


def _tfill(t):
    return float("nan") if t.is_floating_point() else 1


def t_cpu(t):
    return t.cpu()


def t_float64(t):
    return t.double()


def t_colblock(t):
    """T3a: columns 2 .. 2 + F of a tensor 5 columns wider (unit column stride,
    longer row stride)."""
    wide = torch.full((*t.shape[:-1], t.shape[-1] + 5), _tfill(t), dtype=t.dtype, device=t.device)
    wide[..., 2:2 + t.shape[-1]] = t
    return wide[..., 2:2 + t.shape[-1]]


def t_stepped(t):
    """T3b: every second slice along the leading axis of a tensor twice as long."""
    big = torch.full((2 * t.shape[0], *t.shape[1:]), _tfill(t), dtype=t.dtype, device=t.device)
    big[::2] = t
    return big[::2]


def t_transposed(t):
    """T3c: the last two axes stored transposed."""
    return t.transpose(-1, -2).contiguous().transpose(-1, -2)


def t_int32(t):
    return t.to(torch.int32)


def t_int64(t):
    return t.to(torch.int64)


TORCH_FORMS = {"T1": t_cpu, "T2": t_float64, "T3a": t_colblock, "T3b": t_stepped, "T3c": t_transposed,
               "T6-int32": t_int32, "T6-int64": t_int64}


def torch_forms(t, cpu=False, ids=False):
    """The ids of the presentations that apply to the baseline `t`: T1 where
    the mirror documents that it moves the argument (`cpu`), T2 for floats, T3a
    past 0 axes, T3c past one axis with both last extents > 1 (a transpose of
    a one-row tensor is the same memory), T6 for token ids."""
    out = ["T1"] if cpu else []
    if t.is_floating_point():
        out.append("T2")
    out += ["T3a", "T3b"]
    if t.dim() >= 2 and t.shape[-1] > 1 and t.shape[-2] > 1:
        out.append("T3c")
    if ids:
        out += ["T6-int32", "T6-int64"]
    return out


def bits(t):
    """A tensor's (or array's) values as raw integers, on the host: equality of
    these is bit equality, NaN payloads and signed zeros included."""
    a = t.detach().cpu().contiguous().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return a.view({2: np.int16, 4: np.int32, 8: np.int64, 1: np.int8}[a.dtype.itemsize])


def same_result(got, base):
    """`got` is bit for bit `base`, with its dtype and shape (tensors or arrays)."""
    if torch.is_tensor(base):
        return (torch.is_tensor(got) and got.dtype == base.dtype and got.shape == base.shape
                and np.array_equal(bits(got), bits(base)))
    return (isinstance(got, np.ndarray) and got.dtype == base.dtype and got.shape == base.shape
            and np.array_equal(bits(got), bits(base)))


def snapshot(x):
    """A copy of an argument to compare after the call (inputs are left alone)."""
    if torch.is_tensor(x):
        return x.detach().clone()
    if isinstance(x, np.ndarray):
        return x.copy()
    return [list(r) for r in x]


def unchanged(x, snap):
    if torch.is_tensor(x):
        return np.array_equal(bits(x), bits(snap))
    if isinstance(x, np.ndarray):
        return np.array_equal(bits(x), bits(snap))
    return x == snap


# ---------------------------------------------------------------- shapes
# the smallest at which a wrong stride or element type changes the result
SIF_V, SIF_D, SIF_N, SIF_L = 40, 20, 7, 5
PC_SHAPES = ((33, 20), (7, 20))  # sklearn's direct and transposed branch
# the bar tests/test_gpu_sif.py and tests/test_gpu_widths.py hold mmb_sif_wavg's rows to
WAVG_TOL = 2e-6
# the bar they hold the removal of a float32-representable X to, against the oracle's removal
REMOVE_TOL = 1e-9
# the bar those two modules hold the float64 rows' PC and removal to
F64_ROUTE_TOL = 1e-12
REGRESSOR = dict(d=28, h=31, b=20)  # one regressor_cases forward shape; o = 1 and 2

SifInputs = collections.namedtuple("SifInputs", "We ids w weights mask")


def sif_inputs():
    """f32-representable inputs of the numpy drop-ins: table [V, D], ids [N, L]
    int64, token weights [N, L] f32, the weight table [V] (f64 values that are
    f32-representable) and a 0/1 mask."""
    rng = np.random.default_rng([SIF_V, SIF_D, SIF_N, SIF_L])
    g = rng.standard_normal(SIF_D)
    We = (0.4 * rng.standard_normal((SIF_V, SIF_D)) + 0.3 * g).astype(np.float32)
    ids = rng.integers(0, SIF_V, size=(SIF_N, SIF_L)).astype(np.int64)
    w = rng.uniform(0.05, 1.0, (SIF_N, SIF_L)).astype(np.float32)
    weights = rng.uniform(0.05, 1.0, SIF_V).astype(np.float32).astype(np.float64)
    mask = (rng.random((SIF_N, SIF_L)) > 0.3).astype(np.float32)
    mask[:, 0] = 1.0
    return SifInputs(We, ids, w, weights, mask)


def pc_rows(n, d, f32_representable=True):
    rng = np.random.default_rng([n, d, int(f32_representable)])
    g = rng.standard_normal(d)
    X = 0.5 * rng.standard_normal((n, d)) + 0.4 * rng.standard_normal((n, 1)) * g
    return X.astype(np.float32) if f32_representable else X
