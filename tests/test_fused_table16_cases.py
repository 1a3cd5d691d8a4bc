"""CPU: the fused stream + projection kernel on a 16-bit word table -- the
entry point's argument table, the step plan with the `fused_table16` keyword,
and the tables tests/test_gpu_fused_table16.py rests on.

mmb_mm2_stream_project_tt reads a word table stored as fp16 or bf16 (and
frames of any of the three types) and must give, bit for bit, what
mmb_mm2_stream_project_ft gives on the same table upcast to f32.  Nothing here
needs a device: the argument checks and the empty call return before any
launch (stand-in pointers, as tests/test_lib_abi.py), and the plan is host
logic.
"""
import inspect
import itertools

import pytest

import frames16_cases as F
import fused_frames16_cases as FF
import fused_table16_cases as FT16
import large_cases as LC
import mmb_lib
import table16_cases as T

KINDS = list(FT16.KINDS)
FRAMES = ("f32", "f16", "bf16")


# ---------------------------------------------------------------- the entry point
def test_signature_mirrors_the_header():
    assert len(mmb_lib.SIGNATURES["mmb_mm2_stream_project_tt"][1]) == len(FT16.ARGS)
    # mmb_mm2_stream_project_ft with the table type right after the table
    ft = list(mmb_lib.SIGNATURES["mmb_mm2_stream_project_ft"][1])
    tt = list(mmb_lib.SIGNATURES["mmb_mm2_stream_project_tt"][1])
    i = FT16.ARGS.index("table_type")
    assert FT16.ARGS[i - 1] == "table" and tt == ft[:i] + [mmb_lib._I] + ft[i:]
    assert FT16.ARGS[:i] + FT16.ARGS[i + 1:] == FF.ARGS


def test_header_declares_and_documents_the_entry_point():
    import pathlib

    text = (pathlib.Path(__file__).resolve().parents[1] / "include" / "mmb.h").read_text()
    assert "int mmb_mm2_stream_project_tt(const int32_t* ids, const void* table, int table_type, int64_t v," in text
    head = text[:text.index("int mmb_mm2_stream_project_tt(")]
    comment = head[head.rindex("/*"):]
    assert "replaces" in comment and "sif2.py" in comment and "MMB_EINVAL" in comment


def test_argument_table_starts_from_a_supported_call():
    b = FT16.BASE
    assert mmb_lib.query("mmb_mm2_stream_project_supported", b["t"], b["d"], b["a"], b["vd"])
    assert FT16.P % 16 == 0
    F.check_arg_row("mmb_mm2_stream_project_tt", FT16.ARGS, dict(b, n=0), {}, FT16.OK)
    for what, change, want in FT16.ARG_CASES:
        rest = {k: v for k, v in change.items() if k not in ("table_type", "frame_type")}
        if want == FT16.EINVAL:
            rest.pop("n", None)  # (", n 0" rows: the rejection comes before the empty call)
            assert len(rest) <= 1, what
            for k, v in rest.items():
                assert v != b[k], what
        else:
            assert set(rest) <= {"n", "table"}, what


def test_all_nine_pairs_are_in_the_table():
    ok = {(c[1]["table_type"], c[1]["frame_type"]) for c in FT16.ARG_CASES
          if c[2] == FT16.OK and "frame_type" in c[1]}
    bad = {(c[1]["table_type"], c[1]["frame_type"]) for c in FT16.ARG_CASES
           if c[2] == FT16.EINVAL and "frame_type" in c[1] and c[1].get("ids", 1) is None}
    nine = set(itertools.product((0, 1, 2), (0, 1, 2)))
    assert ok == nine and bad == nine
    # every table type carries the rejections, the 16-bit ones their alignment rows
    for tn, _ in T.TABLE_TYPES:
        assert sum(c[0].startswith(f"{tn} table, ") for c in FT16.ARG_CASES) >= 9 + 9
    for tn, _ in T.TABLE_TYPES16:
        for off in (2, 4):
            assert any(c[0] == f"{tn} table, table {off} bytes off" and c[2] == FT16.EINVAL
                       for c in FT16.ARG_CASES)


@pytest.mark.parametrize("what,change,want", FT16.ARG_CASES, ids=T._ids(FT16.ARG_CASES))
def test_stream_project_tt_argument_table_without_gpu(what, change, want):
    F.check_arg_row("mmb_mm2_stream_project_tt", FT16.ARGS, FT16.BASE, change, want)


# ---------------------------------------------------------------- the plan
def _plan(name):
    import pipeline as PL

    shape = F._shapes()[name]
    shape = {"n_total": shape["n"], **shape}
    return lambda **kw: PL.step_plan(d=300, npc=1, cus=256, **shape, **kw)


# every override set of tests/table16_cases.py, and the ones a plan can differ by
OVERRIDES = T.OVERRIDES + (dict(stream_project=False), dict(chunks=3), dict(gram_kind="i8"),
                            dict(fused_frames16=True), dict(narrow_fused=False))


@pytest.mark.parametrize("name", ["c3", "mosi", "pom", "mid"])
def test_keyword_off_every_plan_is_todays(name):
    """fused_table16=False (the default): for all three tables, all three
    frames and every override set the plan is the one without the keyword --
    and for a 16-bit table that is the two-kernel plan
    (tests/test_table16_cases.py)."""
    plan = _plan(name)
    base = plan(stream_project=False, narrow_fused=False, split_stream=False)
    for table in ("f32", "f16", "bf16"):
        for frames in FRAMES:
            for kw in OVERRIDES:
                off = plan(table=table, frames=frames, fused_table16=False, **kw)
                assert off == plan(table=table, frames=frames, **kw), (table, frames, kw)
                if table != "f32" and "chunks" not in kw and "gram_kind" not in kw:
                    assert off == base._replace(frames=frames), (table, frames, kw)
                # and on an f32 table the keyword changes nothing either way
                if table == "f32":
                    assert plan(frames=frames, fused_table16=True, **kw) == off, (frames, kw)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["c3", "mosi", "pom", "mid"])
def test_step_plan_with_the_fused_table16_keyword(name, kind):
    """The front is "fused" exactly where the f32-table plan of the same shape
    and frames chooses it: c3 (and mid, the same widths on 700 rows) on f32
    frames, on 16-bit frames only together with fused_frames16; mosi (narrow
    frames) and pom (T > 64) keep the two-kernel plan.  Never split, never the
    narrow fused front."""
    plan = _plan(name)
    two_kernel = plan(stream_project=False, narrow_fused=False, split_stream=False)
    f32 = plan()
    for frames in FRAMES:
        off = plan(table=kind, frames=frames)
        assert off == two_kernel._replace(frames=frames)
        on = plan(table=kind, frames=frames, fused_table16=True)
        both = plan(table=kind, frames=frames, fused_table16=True, fused_frames16=True)
        if name in ("c3", "mid"):
            assert f32.front == "fused"
            want = plan(frames=frames)  # the f32-table plan of the same shape and frames
            assert on == want, frames
            assert on.front == ("fused" if frames == "f32" else "stream")
            assert both == plan(frames=frames, fused_frames16=True) and both.front == "fused"
            assert both.project == "front" and both.proj_split is False and both.frames == frames
            assert both._replace(frames="f32") == f32
        else:
            assert f32.front != "fused"
            assert on == off and both == off
        for p in (on, both):
            assert p.split is False and p.front in ("fused", "stream")
        # the narrow fused front and the split stream stay off whatever is asked for
        forced = plan(table=kind, frames=frames, fused_table16=True, stream_project=True, narrow_fused=True,
                      split_stream=True, fused_frames16=True, narrow_frames16=True, split_frames16=True)
        assert forced.split is False and forced.front in ("fused", "stream")
        assert (forced.front == "fused") == (plan(frames=frames, stream_project=True, narrow_fused=False,
                                                  split_stream=False, fused_frames16=True).front == "fused")
        # the caller's stream_project is kept: off, or more than one chunk asked for
        assert plan(table=kind, frames=frames, fused_table16=True, fused_frames16=True,
                    stream_project=False) == off
        assert plan(table=kind, frames=frames, fused_table16=True, fused_frames16=True, chunks=3) == \
            plan(table=kind, frames=frames, chunks=3)


def test_keyword_is_opt_in_and_adds_no_plan_field():
    import pipeline as PL

    for fn in (PL.step_plan, PL.FusedStep.__init__):
        par = inspect.signature(fn).parameters["fused_table16"]
        assert par.default is False
    sp = list(inspect.signature(PL.step_plan).parameters)
    assert sp[-1] == "table" and sp[-2] == "fused_table16"
    assert PL.StepPlan._fields == ("front", "split", "gram", "project", "proj_split", "bounds", "step_rows",
                                   "s_half", "frames")
    sig = inspect.signature(PL.mm2_stream_project_tt)
    assert list(sig.parameters) == ("n t d a vd audio visual proj ids32 table wtab32 w_dense flag out colmax "
                                    "colmax_ws").split()


# ---------------------------------------------------------------- the GPU file's tables
def test_gpu_cases_are_shapes_the_fused_kernel_takes():
    sup = lambda T_, D, A, Vd: bool(mmb_lib.query("mmb_mm2_stream_project_supported", T_, D, A, Vd))  # noqa: E731
    text, lens, rows = set(), set(), set()
    for D, A, Vd, T_, N, bad in FT16.KERNEL_CASES:
        assert sup(T_, D, A, Vd)
        text.add(D)
        lens.add(T_)
        rows.add(N)
    # text with no tail and with 4, 44 and 60 tail lanes
    assert {d - 256 for d in text} == {0, 4, 44, 60}
    assert {20, 21} <= lens and {1, 2500} <= rows and 2500 > 48 * 52
    assert sum(c[5] for c in FT16.KERNEL_CASES) == 1 and FT16.ALL_PAIRS_CASE in FT16.KERNEL_CASES
    assert FT16.ALL_PAIRS_CASE[5] and FT16.ALL_PAIRS_CASE[0] > 256 and FT16.ALL_PAIRS_CASE[3] >= 21
    assert max(c[4] for c in FT16.KERNEL_CASES) <= 2500
    for D, A, Vd, T_ in FT16.SPECIAL_SHAPES:
        assert sup(T_, D, A, Vd) and D >= 2 * max(len(v) for v in T.SPECIALS.values())
    (d0, _, _, t0), (d1, _, _, t1) = FT16.SPECIAL_SHAPES
    assert t0 < 21 <= t1 and d1 > 256
    # the planted last columns of the hot row are the b16 tail's at D = 260
    assert d1 - max(len(v) for v in T.SPECIALS.values()) >= 256


def test_gpu_step_is_one_the_family_conditions_cover():
    """The step compared with the oracle is in table16_cases.STEP, whose
    conditions tests/test_table16_cases.py pins on the upcast table."""
    assert FT16.STEP in [tuple(d) for d in T.STEP]
    assert all(tuple(d) in [tuple(s) for s in T.STEP] for d in FT16.STEP_UNCHANGED)


def test_guard_cases_sit_either_side_of_2_31_bytes():
    last, refused = FT16.GUARD_LAST, FT16.GUARD_REFUSED
    assert last.op("table").nbytes == LC.B31 - FT16.GUARD_D * 2 < LC.B31 == refused.op("table").nbytes
    assert refused.op("table").nbytes == LC.CASES["fused_table_refused"].op("table").nbytes
    assert last.dims["v"] == refused.dims["v"] - 1 == 2 ** 22 - 1 and last.dims["t"] >= 21
    assert mmb_lib.query("mmb_mm2_stream_project_supported", *(last.dims[k] for k in ("t", "d", "a", "vd")))
    # the ids of the smaller case stop short of the larger table's last row; the larger case's reach it
    n, t = last.dims["n"], last.dims["t"]
    assert LC.gather_ids(last, n, t).max() == refused.dims["v"] - 2
    assert LC.gather_ids(refused, n, t).max() == refused.dims["v"] - 1
    assert refused.total_bytes <= LC.MAX_CASE_BYTES
