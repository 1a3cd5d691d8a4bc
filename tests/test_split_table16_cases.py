"""CPU: the split stream on a 16-bit word table -- the entry point's argument
table, the step plan with the `split_table16` keyword, and the tables
tests/test_gpu_split_table16.py rests on.

mmb_mm2_stream_split_tt reads a word table stored as fp16 or bf16 (and frames
of any of the three types) and must give, bit for bit, what
mmb_mm2_stream_split_ft gives, with the same parts, on the same table upcast
to f32.  Nothing here needs a device: the argument checks and the empty call
return before any launch or device query (stand-in pointers and an explicit
part count, as tests/test_lib_abi.py), and the plan is host logic.
"""
import inspect
import itertools
import pathlib

import pytest

import abi_cases as ABI
import frames16_cases as F
import mmb_lib
import split_frames16_cases as SF
import split_table16_cases as ST
import table16_cases as T

KINDS = list(ST.KINDS)
FRAMES = ("f32", "f16", "bf16")
NAME = "mmb_mm2_stream_split_tt"
CUS = 256


# ---------------------------------------------------------------- the entry point
def test_header_declares_and_library_exports_the_entry_point():
    assert NAME in ABI.declared_functions()
    assert hasattr(mmb_lib.load(), NAME)


def test_header_documents_the_entry_point():
    text = (pathlib.Path(__file__).resolve().parents[1] / "include" / "mmb.h").read_text()
    decl = "int mmb_mm2_stream_split_tt(const int32_t* ids, const void* table, int table_type, int64_t v,"
    assert decl in text
    head = text[:text.index(decl)]
    comment = " ".join(head[head.rindex("/*"):].replace(" * ", " ").split())
    for w in ("replaces", "sif2.py", "MMB_EINVAL", "captured into a graph", "MMB_TABLE_F32 is", "bit for bit",
              "2-byte aligned", "8-byte aligned", "d up to 1280", "d up to 320", "<= 2240", "n == 0",
              "before the workspace is looked at", "mmb_mm2_stream_split_ws_bytes", "null ids"):
        assert w in comment, w


def test_signature_mirrors_the_header():
    sig = mmb_lib.SIGNATURES
    assert len(sig[NAME][1]) == len(ST.ARGS)
    # mmb_mm2_stream_split_ft with the table type right after the table
    ft, tt = list(sig["mmb_mm2_stream_split_ft"][1]), list(sig[NAME][1])
    i = ST.ARGS.index("table_type")
    assert ST.ARGS[i - 1] == "table" and tt == ft[:i] + [mmb_lib._I] + ft[i:]
    assert ST.ARGS[:i] + ST.ARGS[i + 1:] == SF.ARGS
    # and mmb_mm2_stream_tt, then parts, ws, ws_bytes in front of the stream
    assert tt == list(sig["mmb_mm2_stream_tt"][1])[:-1] + list(sig["mmb_mm2_stream_split"][1])[-4:]
    assert sig[NAME][0] is sig["mmb_mm2_stream_split"][0]


def test_mirror_signature():
    import pipeline as PL

    sig = inspect.signature(PL.mm2_stream_split_tt)
    assert list(sig.parameters) == list(inspect.signature(PL.mm2_stream_split_ft).parameters)
    for name, par in inspect.signature(PL.mm2_stream_split_ft).parameters.items():
        assert sig.parameters[name].default == par.default, name


def test_argument_table_starts_from_a_call_the_library_takes():
    b = ST.BASE
    assert 3 * b["d"] + 2 * b["a"] + 2 * b["vd"] <= SF.FINISH_COLUMNS
    assert b["parts"] > 0 and 0 < SF.ws_bytes() < b["ws_bytes"] and b["n"] <= SF.MAX_BOUND_ROWS
    # 3 * 324 + 2 a + 2 vd still fits the finish kernel: the scalar limit rejects those rows
    assert 3 * 324 + 2 * b["a"] + 2 * b["vd"] <= SF.FINISH_COLUMNS and 324 % 4 == 0 and 324 > SF.NT >= b["d"]
    whats = [w for w, _, _ in ST.ARG_CASES]
    assert len(set(whats)) == len(whats)
    for tn, _ in T.TABLE_TYPES:
        for row in ("null table", "workspace one byte short", "null workspace", "parts -1", "D 512",
                    "bounds with n 8193", "bounds without workspace"):
            assert f"{tn} table, {row}" in whats
    for tn, _ in T.TABLE_TYPES16:
        want = {"table 1 byte off": ST.EINVAL, "table 1 byte off, n 0": ST.EINVAL, "table 2 bytes off, n 0": ST.OK,
                "table 4 bytes off, n 0": ST.OK, "table 2 bytes off, D 324": ST.EINVAL,
                "table 4 bytes off, D 324": ST.EINVAL}
        for what, w in want.items():
            assert any(c[0] == f"{tn} table, {what}" and c[2] == w for c in ST.ARG_CASES), (tn, what)
    assert sum(c[1].get("table_type") in (-1, 3) and c[1].get("n") == 0 for c in ST.ARG_CASES) == 2


def test_all_nine_pairs_are_in_the_table():
    ok = {(c[1]["table_type"], c[1]["frame_type"]) for c in ST.ARG_CASES
          if c[2] == ST.OK and "frame_type" in c[1] and c[1].get("ws", 1) is None}
    bad = {(c[1]["table_type"], c[1]["frame_type"]) for c in ST.ARG_CASES
           if c[2] == ST.EINVAL and "frame_type" in c[1] and c[1].get("ids", 1) is None}
    nine = set(itertools.product((0, 1, 2), (0, 1, 2)))
    assert ok == nine and bad == nine


@pytest.mark.parametrize("what,change,want", ST.ARG_CASES, ids=T._ids(ST.ARG_CASES))
def test_stream_split_tt_argument_table_without_gpu(what, change, want):
    F.check_arg_row(NAME, ST.ARGS, ST.BASE, ST.resolve(change), want)


def test_a_whole_unit_off_is_whole_units():
    """8 bytes off is a 16-bit table's unit: past the checks at any width the
    vector route takes (D = 324 there is rejected only on the scalar route)."""
    for _, tt in T.TABLE_TYPES16:
        F.check_arg_row(NAME, ST.ARGS, ST.BASE, dict(table_type=tt, table=F.P + 8, d=324, n=0), F.OK)


# ---------------------------------------------------------------- the plan
def _plan(name):
    import pipeline as PL

    shape = F._shapes()[name]
    shape = {"n_total": shape["n"], **shape}
    return lambda **kw: PL.step_plan(d=300, npc=1, cus=CUS, **shape, **kw)


OVERRIDES = T.OVERRIDES + (dict(split_stream=False), dict(chunks=3), dict(gram_kind="i8"),
                            dict(split_frames16=True), dict(fused_table16=True), dict(stream_project=False))


@pytest.mark.parametrize("name", ["c3", "mosi", "pom", "mid"])
def test_keyword_off_every_plan_is_todays(name):
    plan = _plan(name)
    for table in ("f32", "f16", "bf16"):
        for frames in FRAMES:
            for kw in OVERRIDES:
                off = plan(table=table, frames=frames, split_table16=False, **kw)
                assert off == plan(table=table, frames=frames, **kw), (table, frames, kw)
                assert table == "f32" or off.split is False
                # on an f32 table the keyword changes nothing either way
                if table == "f32":
                    assert plan(frames=frames, split_table16=True, **kw) == off, (frames, kw)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["c3", "mosi", "pom", "mid"])
def test_step_plan_with_the_split_table16_keyword(name, kind):
    """`split` is set exactly where the f32-table plan of the same shape and
    frames sets it: pom on f32 frames, on 16-bit frames only together with
    split_frames16; c3 / mid (T <= 64, more rows than CUs) and mosi keep the
    plan they have without the keyword, and no fused front comes with it."""
    plan = _plan(name)
    f32 = plan()
    for frames in FRAMES:
        off = plan(table=kind, frames=frames)
        on = plan(table=kind, frames=frames, split_table16=True)
        both = plan(table=kind, frames=frames, split_table16=True, split_frames16=True)
        assert off.split is False
        if name == "pom":
            assert f32.split is True and f32.front == "stream"
            assert on == plan(frames=frames)  # the f32-table plan of the same shape and frames
            assert on.split is (frames == "f32")
            assert both == plan(frames=frames, split_frames16=True) and both.split is True
            assert both._replace(frames="f32") == f32 and both == off._replace(split=True)
        else:
            assert f32.split is False
            assert on == off and both == off
        assert on.front == "stream" and both.front == "stream"
        # the fused fronts stay off whatever is asked for
        forced = plan(table=kind, frames=frames, split_table16=True, stream_project=True, narrow_fused=True,
                      split_stream=True, fused_frames16=True, narrow_frames16=True, split_frames16=True)
        assert forced.front == "stream" and forced.split is (name == "pom")
        # the caller's split_stream and chunks are kept
        assert plan(table=kind, frames=frames, split_table16=True, split_frames16=True, split_stream=False) == off
        # (more than one chunk asked for: no fused front in any plan, so the whole f32-table plan; at pom,
        # fewer rows than features, that plan is forced back to one chunk and splits)
        assert plan(table=kind, frames=frames, split_table16=True, split_frames16=True, chunks=3) == \
            plan(frames=frames, split_frames16=True, chunks=3)
        if name != "pom":
            assert plan(table=kind, frames=frames, split_table16=True, split_frames16=True, chunks=3) == \
                plan(table=kind, frames=frames, chunks=3)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["c3", "mosi", "pom", "mid"])
def test_the_three_table_keywords_together_give_the_f32_table_plan(name, kind):
    plan = _plan(name)
    all3 = dict(fused_table16=True, narrow_table16=True, split_table16=True)
    frames3 = dict(fused_frames16=True, narrow_frames16=True, split_frames16=True)
    for kw in ({}, dict(split_stream=True), dict(stream_project=True), dict(narrow_fused=False), dict(chunks=3)):
        for frames in FRAMES:
            assert plan(table=kind, frames=frames, **all3, **kw) == plan(frames=frames, **kw), (frames, kw)
            assert plan(table=kind, frames=frames, **all3, **frames3, **kw) == plan(frames=frames, **frames3, **kw)


def test_keyword_is_opt_in_and_adds_no_plan_field():
    import pipeline as PL

    for fn in (PL.step_plan, PL.FusedStep.__init__):
        names = list(inspect.signature(fn).parameters)
        assert inspect.signature(fn).parameters["split_table16"].default is False
        assert names[names.index("fused_table16") - 1] == "split_table16"
    assert list(inspect.signature(PL.step_plan).parameters)[-2:] == ["fused_table16", "table"]
    assert PL.StepPlan._fields == ("front", "split", "gram", "project", "proj_split", "bounds", "step_rows",
                                   "s_half", "frames")


# ---------------------------------------------------------------- the GPU file's tables
def test_gpu_cases_reach_what_they_are_there_for():
    assert ST.FRAME_SHAPE_CASES == [(5, 65, 300, 300, (1, 2, 0)), (3, 200, 76, 48, (7,))]
    assert len(ST.TEXT_CASES) == 5
    for d, t, parts, off, w, n in ST.TEXT_CASES:
        assert 3 * d + 4 * w <= SF.FINISH_COLUMNS and n <= 6 and t > SF.PLAN_MIN_T and off in (0, 2)
        assert all(0 < p <= t for p in parts)
    (d0, _, _, o0, _, _), (d1, _, _, o1, _, _), (d2, _, p2, o2, w2, _), (d3, _, _, o3, _, _), (d4, t4, p4, o4, _, _) = \
        ST.TEXT_CASES
    # scalar by width; scalar by alignment at a width % 4 == 0
    assert not ST.vector(d0, o0) and ST.units(d0, o0) == (50, 6)
    assert d1 % 4 == 0 and o1 == 2 and not ST.vector(d1, o1) and ST.units(d1, o1) == (52, 6)
    # 166 units x ONE row slot, the widest text beside the narrowest frames
    assert ST.vector(d2, o2) and ST.units(d2, o2) == (166, 1) and 3 * d2 + 4 * w2 <= SF.FINISH_COLUMNS < 3 * d2 + 4 * 64
    assert p2 == (3,)
    # one unit, 320 row slots for ranges of 35 tokens
    assert ST.units(d3, o3) == (1, 320)
    # one range past a staging chunk: with parts = 1 also held to the one-workgroup kernel
    assert p4 == (1,) and t4 > ST.TOK_CHUNK and ST.vector(d4, o4)
    assert ST.BOUNDS_CASE in ST.TEXT_CASES and ST.BAD_CASE == SF.BAD_CASE
    assert len(set(ST.WS_FILLS)) == 3 and set(ST.WS_FILLS) >= {0x00, 0xFF}


def test_text_inputs_are_row_0_heavy():
    import numpy as np

    for d, t, parts, off, w, n in ST.TEXT_CASES:
        for kind in KINDS:
            E16, ids, wt = ST.text_inputs(d, t, n, kind)
            assert E16.dtype == ST.KINDS[kind] and tuple(E16.shape) == (ST.V, d) and ids.shape == (n, t)
            assert bool((E16[0] != 0).any())  # row 0 planted: the shortcut multiplies no zeros
            rows = np.where(ids < 0, ids + ST.V, ids)
            assert (rows == 0).mean() > 0.5 and (rows[0] == 0).all()
            assert (rows[1, t // 3:-(-2 * t // 3)] == 0).all() and (rows[1] != 0).any()
            assert (ids < 0).sum() == 2 and rows.min() >= 0 and rows.max() < ST.V


def test_gpu_step_shape_takes_the_split():
    import pipeline as PL

    n, t, a, vd = ST.STEP
    for kind in KINDS:
        for frames in ("f32", kind):
            p = PL.step_plan(n, n, t, SF.D, a, vd, SF.V, 1, CUS, table=kind, frames=frames, split_table16=True,
                             split_frames16=True)
            assert p.split is True and p.front == "stream" and p.frames == frames
            assert PL.step_plan(n, n, t, SF.D, a, vd, SF.V, 1, CUS, table=kind, frames=frames,
                                split_frames16=True).split is False
