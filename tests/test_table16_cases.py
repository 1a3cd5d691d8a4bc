"""CPU: the 16-bit word-table entry points' argument tables, the step plan
with a 16-bit table, and the inputs tests/test_gpu_table16.py rests on.

mmb_sif_wavg_tt and mmb_mm2_stream_tt read a word table stored as fp16 or bf16
and must give, bit for bit, what mmb_sif_wavg / mmb_mm2_stream_ft give on the
same table upcast to f32.  Nothing here needs a device: the argument checks
and the empty call return before any launch (stand-in pointers, as
tests/test_lib_abi.py), the plan is host logic, and the family conditions are
the three caps of tests/test_mmb2_cases.py on the upcast inputs of every step
the GPU file compares with the oracle -- and, for the PC and SIF bars of those
steps, the agreement of the oracle's own two routes to the PC on them.
"""
import inspect

import numpy as np
import pytest
import torch

import frames16_cases as F
import mmb2_cases as C
import mmb_lib
import table16_cases as T
from frames16_cases import EINVAL, OK, P
from table16_cases import OVERRIDES, _ids

# ---------------------------------------------------------------- argument tables
SIF_CASES = [("table_type -1", dict(table_type=-1), EINVAL),
             ("table_type 3", dict(table_type=3), EINVAL),
             ("table_type 3, n 0", dict(table_type=3, n=0), EINVAL)]
SIF_CASES += T.table_rows(T.TABLE_TYPES, [("n 0", dict(n=0), OK),
                                          ("null ids", dict(ids=None), EINVAL),
                                          ("null ids, n 0", dict(ids=None, n=0), EINVAL),
                                          ("no output", dict(x_out=None), EINVAL),
                                          ("no weights", dict(wtab32=None), EINVAL),
                                          ("scalar D 321", dict(d=321), EINVAL),
                                          ("vector D 1284", dict(d=1284), EINVAL)])
SIF_CASES += T.table_rows(T.TABLE_TYPES16, [("odd table pointer", dict(table=P + 1), EINVAL),
                                            ("odd table pointer, n 0", dict(table=P + 3, n=0), EINVAL)])

STREAM_CASES = [("table_type -1", dict(table_type=-1), EINVAL),
                ("table_type 3", dict(table_type=3), EINVAL),
                ("table_type 3, n 0", dict(table_type=3, n=0), EINVAL),
                ("frame_type 3 on a bf16 table", dict(frame_type=3), EINVAL)]
# all nine (table type, frame type) pairs: the empty call, and the frame-side rows of
# tests/test_frames16_cases.py with the text's own
STREAM_CASES += T.pair_rows([("n 0", dict(n=0), OK),
                             ("null ids", dict(ids=None), EINVAL),
                             ("bounds without workspace", dict(colmax=P), EINVAL),
                             ("scalar D 321", dict(d=321), EINVAL),
                             ("scalar A 321", dict(a=321), EINVAL),
                             ("scalar Vd 321", dict(vd=321), EINVAL),
                             ("bounds at D 644", dict(d=644, colmax=P, colmax_ws=P), EINVAL)])
STREAM_CASES += T.table_rows(T.TABLE_TYPES16, [("odd table pointer", dict(table=P + 1), EINVAL),
                                               ("odd table pointer, n 0", dict(table=P + 3, n=0), EINVAL)])
STREAM_CASES += [(f"{tn} table, {what}", dict(table_type=tt, **change), want)
                 for tn, tt in T.TABLE_TYPES
                 for what, change, want in F.arg_rows(F.TYPES16, [
                     ("odd audio pointer", dict(audio=P + 1), EINVAL),
                     ("odd visual pointer, n 0", dict(visual=P + 3, n=0), EINVAL)])]


def test_signatures_mirror_the_header():
    assert len(mmb_lib.SIGNATURES["mmb_sif_wavg_tt"][1]) == len(T.SIF_ARGS)
    assert len(mmb_lib.SIGNATURES["mmb_mm2_stream_tt"][1]) == len(T.STREAM_ARGS)
    assert (mmb_lib.MMB_TABLE_F32, mmb_lib.MMB_TABLE_F16, mmb_lib.MMB_TABLE_BF16) == (0, 1, 2)
    # the _tt lists are the existing ones plus the table type, right after the table
    a = mmb_lib.SIGNATURES["mmb_sif_wavg"][1]
    assert mmb_lib.SIGNATURES["mmb_sif_wavg_tt"][1] == a[:1] + [mmb_lib._I] + a[1:]
    b = mmb_lib.SIGNATURES["mmb_mm2_stream_ft"][1]
    assert mmb_lib.SIGNATURES["mmb_mm2_stream_tt"][1] == b[:2] + [mmb_lib._I] + b[2:]


@pytest.mark.parametrize("what,change,want", SIF_CASES, ids=_ids(SIF_CASES))
def test_sif_wavg_tt_argument_table_without_gpu(what, change, want):
    F.check_arg_row("mmb_sif_wavg_tt", T.SIF_ARGS, T.SIF_BASE, change, want)


@pytest.mark.parametrize("what,change,want", STREAM_CASES, ids=_ids(STREAM_CASES))
def test_stream_tt_argument_table_without_gpu(what, change, want):
    F.check_arg_row("mmb_mm2_stream_tt", T.STREAM_ARGS, T.STREAM_BASE, change, want)


def test_all_nine_pairs_are_in_the_table():
    pairs = {(c[1]["table_type"], c[1]["frame_type"]) for c in STREAM_CASES
             if c[2] == OK and "frame_type" in c[1]}
    assert pairs == {(t, f) for t in (0, 1, 2) for f in (0, 1, 2)}


# ---------------------------------------------------------------- the plan
@pytest.mark.parametrize("name", ["c3", "mosi", "pom", "mid"])
def test_step_plan_with_a_16_bit_table(name):
    import pipeline as PL

    shape = F._shapes()[name]
    shape = {"n_total": shape["n"], **shape}
    plan = lambda **kw: PL.step_plan(d=300, npc=1, cus=256, **shape, **kw)  # noqa: E731
    # the f32 plan of the shape is not the two-kernel one (what the 16-bit table gives up) ...
    f32 = plan()
    assert (f32.front, f32.split) != ("stream", False)
    # ... and it is untouched by the new keyword
    for frames in ("f32", "f16", "bf16"):
        for kw in OVERRIDES:
            assert plan(table="f32", frames=frames, **kw) == plan(frames=frames, **kw)
    base = plan(stream_project=False, narrow_fused=False, split_stream=False)
    assert base.front == "stream" and base.split is False
    for tk in ("f16", "bf16"):
        for frames in ("f32", "f16", "bf16"):
            for kw in OVERRIDES:
                got = plan(table=tk, frames=frames, **kw)
                assert got.front == "stream" and got.split is False
                assert got == base._replace(frames=frames), (tk, frames, kw)
    with pytest.raises(ValueError, match="table"):
        plan(table="f64")


def test_signatures_that_may_not_change():
    import pipeline as PL

    assert PL.StepPlan._fields == ("front", "split", "gram", "project", "proj_split", "bounds", "step_rows",
                                   "s_half", "frames")
    assert list(inspect.signature(PL.mm2_stream).parameters) == (
        "n t d a vd audio visual ids32 table wtab32 text_dense emb_dense w_dense flag out s_half colmax "
        "colmax_ws split parts").split()
    sp = inspect.signature(PL.step_plan).parameters
    assert list(sp)[-1] == "table" and sp["table"].default == "f32"
    assert {k: v[0] for k, v in PL.TABLE_KINDS.items()} == {"f32": torch.float32, **T.KINDS}
    assert {k: v[1] for k, v in PL.TABLE_KINDS.items()} == dict(T.TABLE_TYPES)


def test_table_kind_names_the_dtype():
    import pipeline as PL

    for kind, dt in (("f32", torch.float32), ("f16", torch.float16), ("bf16", torch.bfloat16)):
        assert PL.table_kind(torch.zeros(3, 4, dtype=dt)) == kind
    for dt in (torch.float64, torch.int32):
        with pytest.raises(mmb_lib.MMBError, match="float32, float16 or bfloat16"):
            PL.table_kind(torch.zeros(3, 4, dtype=dt), "weighted_sum")


# ---------------------------------------------------------------- the rounding helper
@pytest.mark.parametrize("kind", list(T.KINDS))
def test_upcast_image_round_trips(kind):
    case = C.case_of((52, 8, 12, 7))
    z, z0 = T.inputs(case, kind), C.inputs(case)
    E16 = z["E16"]
    assert E16.dtype == T.KINDS[kind] and z["E"].dtype == np.float32 and z["E"].shape == z0["E"].shape
    # the image is exactly representable: rounding it again changes nothing
    assert np.array_equal(F.bits(F.to_kind(z["E"], kind)), F.bits(E16))
    assert np.array_equal(F.upcast(F.to_kind(z["E"], kind)), z["E"])
    # and it is the nearest 16-bit value: half an ulp of the kind's 11 / 8 significant bits
    rel = 2.0 ** -(11 if kind == "f16" else 8)
    assert (np.abs(z["E"].astype(np.float64) - z0["E"]) <= rel * np.abs(z0["E"]) + 2.0 ** -25).all()
    assert not np.array_equal(z["E"], z0["E"])  # the rounding is not a no-op on the family's table
    assert np.array_equal(z["text"], z["E"][z0["ids"]])
    for key in ("wt32", "ids", "sw", "audio", "visual"):
        assert z[key] is z0[key]
    # with frames of the kind: frames16_cases' image of them
    zf = T.inputs(case, kind, kind)
    assert zf["audio"] is F.inputs(case, kind)["audio"] and zf["E"] is not z0["E"]


@pytest.mark.parametrize("kind", list(T.KINDS))
@pytest.mark.parametrize("shape", T.SPECIAL_SHAPES, ids=C.shape_id)
def test_special_values_are_where_the_gpu_test_expects_them(shape, kind):
    case = C.case_of(shape)
    D, A, Vd, T_, N, V = case
    E16 = T.special_table(case, kind)
    want = np.array([b for _, b in T.SPECIALS[kind]], np.uint16)
    k = len(want)
    hot = T.hot_row(case)
    assert hot > 0 and np.array_equal(F.bits(E16)[0, :k], want)
    assert np.array_equal(F.bits(E16)[hot, D - k:], want[::-1])
    vals = np.array([v for v, _ in T.SPECIALS[kind]])
    up = F.upcast(E16)
    for got in (up[0, :k], up[hot, D - k:][::-1]):
        assert np.array_equal(got.astype(np.float64), vals) and np.array_equal(np.signbit(got), np.signbit(vals))
    # the family's row 0 is zero: without the planting the row-0 shortcut multiplies zeros
    assert not F.upcast(T.table(case, kind))[0].any()
    ids = C.inputs(case)["ids"]
    assert (ids == 0).any(axis=1).any() and (ids == hot).sum() == max((ids == r).sum() for r in range(1, V))
    # the sums stay finite in f32: T tokens of the largest value squared, and weighted
    big = float(vals[-1])
    assert np.isfinite(up).all() and T_ * big * big < 3e38
    # the rest is the plain rounded table
    rest = np.ones(V, bool)
    rest[[0, hot]] = False
    assert np.array_equal(F.bits(E16)[rest], F.bits(T.table(case, kind))[rest])


def test_sif_cases_reach_what_they_name():
    for d, l in T.SIF_WAVE:
        assert d % 4 == 0 and d <= 512 and l <= 64
    assert {d > 256 for d, _ in T.SIF_WAVE} == {False, True}  # one and two column units
    (ds, ls), (dv, lv), (d2, _), (dw, _) = T.SIF_WG
    assert ds % 4 and ds <= 320 and dv % 4 == 0 and lv > 512 and d2 % 4 == 0 and d2 > 512 and dw == 1280
    E16, ids, wt32, w = T.sif_inputs(52, 7, "bf16")
    assert (ids < 0).sum() == 2 and (ids == -T.SIF_V).sum() == 1 and (ids == 0).any() and F.upcast(E16)[0].all()


# ---------------------------------------------------------------- the family on the upcast inputs
F32_CAP, CANCEL_CAP = 1e-6, 10.0  # the caps of tests/test_mmb2_cases.py


def _case_id(v):
    return v if isinstance(v, str) else C.shape_id(v)


@pytest.mark.parametrize("case,kind,frames", T.oracle_cases(), ids=_case_id)
def test_family_conditions_on_a_rounded_table(case, kind, frames):
    e32, cancel, flips = T.family_conditions(case, kind, T.fkind_of(kind, frames))
    print(f"f32 run {e32:.2e} (cap {F32_CAP}); cancellation {cancel:.2f} (cap {CANCEL_CAP}); "
          f"sign flips {flips}")
    assert e32 <= F32_CAP
    assert cancel <= CANCEL_CAP
    assert flips == 0


# The step's PC bar is 1e-10 against compute_pc on the device's own rows, and the SIF rows
# follow the PC.  The device solves from the Gram; the oracle's Gram route restates it.  So
# the bar is met by the method only where the oracle's two routes agree well inside it: a
# decade, 1e-11 (the golden splits sit near 6e-11 WITH the int8 Gram's own 1e-10; these
# steps take the exact f64 Gram).
PC_ROUTES_CAP = 1e-11


@pytest.mark.parametrize("kind", list(T.KINDS))
@pytest.mark.parametrize("dims", T.STEP + [T.CHUNKED], ids=C.shape_id)
def test_pc_routes_agree_on_a_rounded_table(dims, kind):
    ref, alt = T.pc_routes(F.step_case(dims), kind)
    dev = float(np.abs(ref - alt).max())
    print(f"compute_pc vs the Gram route: {dev:.2e} (cap {PC_ROUTES_CAP})")
    assert np.isfinite(ref).all() and dev <= PC_ROUTES_CAP
