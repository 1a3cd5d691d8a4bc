"""CPU: the 16-bit frame entry point's argument table, the step plan with
16-bit frames, and the inputs tests/test_gpu_frames16.py rests on.

mmb_mm2_stream_ft reads audio / visual frames stored as fp16 or bf16 and must
give, bit for bit, what mmb_mm2_stream gives on the same frames upcast to f32.
Nothing here needs a device: the argument checks and the empty call return
before any launch (stand-in pointers, as tests/test_lib_abi.py), the plan is
host logic, and the family conditions are the three caps of
tests/test_mmb2_cases.py on the upcast inputs of every step the GPU file
compares with the oracle.
"""
import numpy as np
import pytest
import torch

import frames16_cases as F
import mmb2_cases as C
import mmb_lib
from frames16_cases import ARGS, BF16, EINVAL, F16, F32, OK, P, _shapes

BASE = dict(ids=P, table=P, v=1000, wtab32=P, w_dense=None, audio=P, visual=P, frame_type=BF16, n=100,
            t=40, d=300, a=300, vd=300, num_out=P, s_out=P, s_half=1, aux_out=P, flag=None,
            colmax=None, colmax_ws=None, stream=None)
CASES = [("frame_type -1", dict(frame_type=-1), EINVAL),
         ("frame_type 3", dict(frame_type=3), EINVAL),
         ("frame_type 3, n 0", dict(frame_type=3, n=0), EINVAL)]
CASES += F.arg_rows(F.ALL_TYPES, [("n 0", dict(n=0), OK),
                                  ("bounds without workspace", dict(colmax=P), EINVAL),
                                  ("scalar A 321", dict(a=321), EINVAL),
                                  ("scalar Vd 321", dict(vd=321), EINVAL),
                                  ("bounds at D 644", dict(d=644, colmax=P, colmax_ws=P), EINVAL),
                                  ("dense text (no ids)", dict(ids=None), EINVAL)])
CASES += F.arg_rows(F.TYPES16, [("odd audio pointer", dict(audio=P + 1), EINVAL),
                                ("odd visual pointer, n 0", dict(visual=P + 3, n=0), EINVAL)])


def test_signature_mirrors_the_header():
    assert len(mmb_lib.SIGNATURES["mmb_mm2_stream_ft"][1]) == len(ARGS)
    assert (F32, F16, BF16) == (0, 1, 2)


@pytest.mark.parametrize("what,change,want", CASES, ids=[c[0].replace(" ", "_") for c in CASES])
def test_stream_ft_argument_table_without_gpu(what, change, want):
    F.check_arg_row("mmb_mm2_stream_ft", ARGS, BASE, change, want)


# ---------------------------------------------------------------- the plan
@pytest.mark.parametrize("name", ["c3", "mosi", "pom", "mid"])
def test_step_plan_with_16_bit_frames(name):
    import pipeline as PL

    shape = _shapes()[name]
    shape = {"n_total": shape["n"], **shape}
    plan = lambda **kw: PL.step_plan(d=300, npc=1, cus=256, **shape, **kw)  # noqa: E731
    assert plan() == plan(frames="f32") and plan().frames == "f32"
    # the f32 plan of the same shape is not the two-kernel one (what the 16-bit frames give up)
    f32 = plan()
    assert (f32.front, f32.split) != ("stream", False)
    base = plan(stream_project=False, narrow_fused=False, split_stream=False)
    assert base.front == "stream" and base.split is False
    for kind in ("f16", "bf16"):
        for kw in ({}, dict(stream_project=True, narrow_fused=True, split_stream=True)):
            got = plan(frames=kind, **kw)
            assert got.front == "stream" and got.split is False and got.frames == kind
            assert got[:8] == base[:8] and got._replace(frames="f32") == base
    with pytest.raises(ValueError, match="frames"):
        plan(frames="f64")


def test_step_plan_keeps_its_eight_leading_fields():
    import pipeline as PL

    assert PL.StepPlan._fields[:8] == ("front", "split", "gram", "project", "proj_split", "bounds",
                                       "step_rows", "s_half")
    assert PL.StepPlan._fields[8:] == ("frames",) and PL.StepPlan._field_defaults == {"frames": "f32"}
    assert {k: v[0] for k, v in PL.FRAME_KINDS.items()} == {"f32": torch.float32, **F.KINDS}


def test_frame_kind_names_the_dtype():
    import pipeline as PL

    z = {k: torch.zeros(2, 3, 4, dtype=d) for k, d in (("f32", torch.float32), ("f16", torch.float16),
                                                       ("bf16", torch.bfloat16), ("f64", torch.float64))}
    for kind in ("f32", "f16", "bf16"):
        assert PL.frame_kind(z[kind], z[kind]) == kind
    with pytest.raises(mmb_lib.MMBError, match="one dtype"):
        PL.frame_kind(z["f16"], z["bf16"])
    with pytest.raises(mmb_lib.MMBError, match="float32, float16 or bfloat16"):
        PL.frame_kind(z["f64"], z["f64"])


# ---------------------------------------------------------------- the family on the upcast inputs
F32_CAP, CANCEL_CAP = 1e-6, 10.0  # the caps of tests/test_mmb2_cases.py


@pytest.mark.parametrize("case,kind", F.oracle_cases(), ids=lambda v: v if isinstance(v, str) else C.shape_id(v))
def test_family_conditions_on_rounded_frames(case, kind):
    e32, cancel, flips = F.family_conditions(case, kind)
    print(f"f32 run {e32:.2e} (cap {F32_CAP}); cancellation {cancel:.2f} (cap {CANCEL_CAP}); "
          f"sign flips {flips}")
    assert e32 <= F32_CAP
    assert cancel <= CANCEL_CAP
    assert flips == 0


# ---------------------------------------------------------------- the rounding helper
@pytest.mark.parametrize("kind", list(F.KINDS))
def test_upcast_image_round_trips(kind):
    case = C.case_of((52, 8, 12, 7))
    z, z0 = F.inputs(case, kind), C.inputs(case)
    for key in ("audio", "visual"):
        t16 = z[key + "16"]
        assert t16.dtype == F.KINDS[kind] and z[key].dtype == np.float32 and z[key].shape == z0[key].shape
        # the image is exactly representable: rounding it again changes nothing
        assert np.array_equal(F.bits(F.to_kind(z[key], kind)), F.bits(t16))
        assert np.array_equal(F.upcast(F.to_kind(z[key], kind)), z[key])
        # and it is the nearest 16-bit value: half an ulp of the kind's 11 / 8 significant bits
        rel = 2.0 ** -(11 if kind == "f16" else 8)
        assert (np.abs(z[key].astype(np.float64) - z0[key]) <= rel * np.abs(z0[key]) + 2.0 ** -25).all()
        assert not np.array_equal(z[key], z0[key])  # the rounding is not a no-op on U(-1, 1)
    for key in ("E", "wt32", "ids", "sw", "text"):
        assert z[key] is z0[key]


@pytest.mark.parametrize("kind", list(F.KINDS))
@pytest.mark.parametrize("shape", F.SPECIAL_SHAPES, ids=C.shape_id)
def test_special_values_are_where_the_gpu_test_expects_them(shape, kind):
    case = C.case_of(shape)
    D, A, Vd, T, N, V = case
    a16, v16 = F.special_frames(case, kind)
    want = np.array([b for _, b in F.SPECIALS[kind]], np.uint16)
    k = len(want)
    assert np.array_equal(F.bits(a16)[0, :k, 0], want) and np.array_equal(F.bits(v16)[1, :k, Vd - 1], want)
    vals = np.array([v for v, _ in F.SPECIALS[kind]])
    for t16, got in ((a16, F.upcast(a16)[0, :k, 0]), (v16, F.upcast(v16)[1, :k, Vd - 1])):
        assert np.array_equal(got.astype(np.float64), vals) and np.array_equal(np.signbit(got), np.signbit(vals))
    assert np.signbit(vals[1]) and vals[1] == 0 and 0 < vals[2] < 2.0 ** -14  # -0; subnormal in either kind
    if kind == "f16":
        assert vals[3] == float(np.finfo(np.float16).max) and vals[2] == float(np.finfo(np.float16).smallest_subnormal)
    else:
        assert vals[3] == 2.0 ** 40 and vals[2] < float(np.finfo(np.float32).tiny)
    for t16 in (a16, v16):
        up = F.upcast(t16)
        assert (up[2:, T - F.SPECIAL_PADS:, :] == F.PAD_VALUE).all()
        assert np.isfinite(up).all()
        # the sums of squares stay finite in f32
        assert np.isfinite((up.astype(np.float64) ** 2).sum(1)).all() and (up.astype(np.float64) ** 2).sum(1).max() < 3e38
    # the rest is the plain rounded family
    b16 = F.frames(case, kind)[0]
    assert np.array_equal(F.bits(a16)[1, :, :], F.bits(b16)[1, :, :])
