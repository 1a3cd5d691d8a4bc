"""Shared inputs and references of tests/test_gpu_frames16.py (GPU) and
tests/test_frames16_cases.py (CPU): the MMB2 stream kernels on audio / visual
frames kept in 16-bit storage; and the scaffolding of the `_ft` entry points'
argument tables (this one's, fused_frames16_cases', narrow_frames16_cases').
Plain helper module: no test is collected from it.

A case is one of mmb2_cases (D, A, Vd, T, N, V); a kind is "bf16" or "f16"
(pipeline.FRAME_KINDS).  The case's U(-1, 1) frames are rounded to the kind on
the CPU (round to nearest even, torch's conversion) -- that is the caller's
rounding, the library converts nothing -- and every reference here is taken
on the UPCAST image of those 16-bit frames, which is what a 16-bit launch
must reproduce: bit for bit against an f32 launch on the image, to the usual
bars against the oracle on the image.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import mmb2_cases as C
import mmb_lib
from oracle import mmb2_oracle as M
from plan_cases import _plan_cases

KINDS = {"bf16": torch.bfloat16, "f16": torch.float16}

# ---------------------------------------------------------------- argument tables
# An `_ft` entry point's table is ARGS (its parameter names), BASE (a call it
# takes) and rows (what, change, want): BASE with `change` returns `want`.
# Nothing is launched: the checks and the empty call return first.
P = 0x7F0000001000  # a stand-in device pointer: 16-byte aligned, never dereferenced
EINVAL, OK = -1, 0
F32, F16, BF16 = mmb_lib.MMB_FRAMES_F32, mmb_lib.MMB_FRAMES_F16, mmb_lib.MMB_FRAMES_BF16
ALL_TYPES = (("f32", F32), ("f16", F16), ("bf16", BF16))
TYPES16 = ALL_TYPES[1:]


def arg_rows(types, rows):
    """Every (what, change, want) of `rows` once per frame type of `types`:
    named "<type> <what>", the one thing changed beside that frame_type."""
    return [(f"{name} {what}", dict(frame_type=ft, **change), want)
            for name, ft in types for what, change, want in rows]


def check_arg_row(entry, args, base, change, want):
    """The call of `entry` on `base` with `change` returns `want`."""
    call = [dict(base, **change)[k] for k in args]
    if want == OK:
        assert mmb_lib.call(entry, *call) == 0
    else:
        with pytest.raises(mmb_lib.MMBError, match=r"code -1 \(invalid argument\)"):
            mmb_lib.call(entry, *call)


# mmb_mm2_stream_ft's parameter names (the split `_ft` entry point's table builds on them)
ARGS = ("ids table v wtab32 w_dense audio visual frame_type n t d a vd num_out s_out s_half aux_out "
        "flag colmax colmax_ws stream").split()


# ---------------------------------------------------------------- the plan
def _shapes():
    """The four real shapes of plan_cases' table, by name, for the 16-bit fronts' plan tests."""
    by_name = {}
    for shape, kw, want in _plan_cases():
        key = (shape["n"], shape["t"], shape["a"], shape["vd"], shape["V"])
        by_name.setdefault(key, shape)
    want = {"c3": (1_000_000, 40, 300, 300, 400_000), "mosi": (1284, 20, 76, 48, 3016),
            "pom": (100, 1089, 300, 300, 7763), "mid": (700, 40, 300, 300, 5000)}
    return {name: by_name[key] for name, key in want.items()}


# the steps test_gpu_frames16.py compares with the oracle: (D, A, Vd, T, N), V = DEFAULT_V
STEP = [C.STEP[0], C.STEP[1], (300, 300, 300, 40, 97), (300, 76, 48, 20, 97), (50, 76, 48, 130, 16)]
STEP_NARROW_TWIN = (300, 76, 48, 20, 97)  # the f32 twin's stream kernel there is the narrow-frame route
CHUNKED = (100, 300, 300, 40, 700)         # chunks = 3


def step_case(dims):
    return C.case_of(dims[:4], dims[4])


def oracle_cases():
    return [(step_case(d), kind) for d in STEP for kind in KINDS]


# ---------------------------------------------------------------- rounding
def to_kind(a: np.ndarray, kind: str) -> torch.Tensor:
    """f32 numpy -> a CPU tensor of the kind (round to nearest even)."""
    return torch.tensor(np.asarray(a, np.float32)).to(KINDS[kind])


def upcast(t: torch.Tensor) -> np.ndarray:
    """The exact f32 image of a 16-bit tensor (read-only numpy)."""
    a = t.to(torch.float32).numpy()
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def frames(case, kind):
    """(audio16, visual16) of the case: its mmb2_cases frames rounded to `kind`."""
    z = C.inputs(case)
    return to_kind(z["audio"], kind), to_kind(z["visual"], kind)


@functools.lru_cache(maxsize=None)
def inputs(case, kind):
    """mmb2_cases.inputs(case) with audio / visual replaced by the upcast image
    of their rounding to `kind`; "audio16" / "visual16" hold the 16-bit tensors."""
    a16, v16 = frames(case, kind)
    return dict(C.inputs(case), audio=upcast(a16), visual=upcast(v16), audio16=a16, visual16=v16)


# ---------------------------------------------------------------- special values
# planted into the rounded frames of SPECIAL_SHAPES: value j of the kind's list at
# audio[0, j, 0] and at visual[1, j, Vd - 1]; rows 2.. end in SPECIAL_PADS frames of
# the reference's pad value -10 (exact in both kinds) in both modalities
SPECIAL_SHAPES = [(52, 8, 12, 7), (50, 5, 3, 9)]
SPECIAL_PADS = 2
PAD_VALUE = -10.0
# (value, its 16 bits)
SPECIALS = {
    "f16": [(0.0, 0x0000), (-0.0, 0x8000), (2.0 ** -24, 0x0001),    # +-0, the smallest subnormal
            (65504.0, 0x7BFF)],                                      # the largest finite fp16 value
    "bf16": [(0.0, 0x0000), (-0.0, 0x8000), (2.0 ** -133, 0x0001),  # +-0, the smallest subnormal
             (2.0 ** 40, 0x5380)],
}


@functools.lru_cache(maxsize=None)
def special_frames(case, kind):
    """(audio16, visual16) of the case with the special values planted."""
    D, A, Vd, T, N, V = case
    assert N >= 3 and T >= len(SPECIALS[kind]) and T > SPECIAL_PADS
    a16, v16 = (t.clone() for t in frames(case, kind))
    vals = torch.tensor([v for v, _ in SPECIALS[kind]], dtype=torch.float64).to(KINDS[kind])
    a16[0, :len(vals), 0] = vals
    v16[1, :len(vals), Vd - 1] = vals
    a16[2:, T - SPECIAL_PADS:, :] = PAD_VALUE
    v16[2:, T - SPECIAL_PADS:, :] = PAD_VALUE
    return a16, v16


def bits(t: torch.Tensor) -> np.ndarray:
    """The 16 bits of every element."""
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


# ---------------------------------------------------------------- oracle on the upcast inputs
@functools.lru_cache(maxsize=None)
def oracle_rows(case, kind, f32=False):
    """mmb2_cases.oracle_rows of the upcast inputs: the oracle's
    estimate_embedding_overall_gpu2 (f64, or the reference's f32 arithmetic)."""
    D, A, Vd, T, N, V = case
    z = inputs(case, kind)
    out = []
    for r in C._chunks(N):
        cat = M.concat_inputs(z["text"][r], z["audio"][r], z["visual"][r])
        out.append(M.estimate_embedding_overall_gpu2(cat, C.params(D, A, Vd), z["sw"][r], z["text"][r],
                                                     dtype=np.float32 if f32 else np.float64))
    out = np.concatenate(out)
    out.setflags(write=False)
    return out


def total_weight(case, kind, f32=False):
    D, A, Vd, T, N, V = case
    z = inputs(case, kind)
    tot, ab = [], []
    for r in C._chunks(N):
        cat = M.concat_inputs(z["text"][r], z["audio"][r], z["visual"][r])
        t, a = M.total_weight(cat, C.params(D, A, Vd), z["sw"][r], dtype=np.float32 if f32 else np.float64)
        tot.append(t)
        ab.append(a)
    return np.concatenate(tot).astype(np.float64), np.concatenate(ab).astype(np.float64)


def family_conditions(case, kind):
    """mmb2_cases.family_conditions on the upcast inputs: (f32 error,
    cancellation, sign flips)."""
    e32 = M.row_rel_err(oracle_rows(case, kind, f32=True), oracle_rows(case, kind))
    t64, a64 = total_weight(case, kind)
    t32, _ = total_weight(case, kind, f32=True)
    return e32, float((a64 / np.abs(t64)).max()), int((np.sign(t32) != np.sign(t64)).sum())
