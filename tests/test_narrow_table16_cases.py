"""CPU: the narrow fused kernel and its text cache on a 16-bit word table --
the two entry points' argument tables, the step plan with the
`narrow_table16` keyword, and the tables tests/test_gpu_narrow_table16.py
rests on.

mmb_mm2_text_cache_tt builds the text cache from a word table stored as fp16
or bf16, byte for byte the cache mmb_mm2_text_cache builds from the same table
upcast to f32; mmb_mm2_stream_project_narrow_tt runs the narrow fused kernel on
it (the kernel reads the cache, never the table) and must give, bit for bit,
what mmb_mm2_stream_project_narrow_ft gives on the upcast table.  Nothing here
needs a device: the argument checks and the empty call return before any
launch (stand-in pointers, as tests/test_lib_abi.py), and the plan is host
logic.
"""
import ctypes
import inspect
import itertools
import pathlib

import pytest

import frames16_cases as F
import mmb_lib
import narrow_frames16_cases as NF
import narrow_table16_cases as NT
import table16_cases as T

KINDS = list(NT.KINDS)
FRAMES = ("f32", "f16", "bf16")
HEADER = (pathlib.Path(__file__).resolve().parents[1] / "include" / "mmb.h").read_text()


# ---------------------------------------------------------------- the entry points
def test_signatures_mirror_the_header():
    sig = mmb_lib.SIGNATURES
    assert len(sig["mmb_mm2_stream_project_narrow_tt"][1]) == len(NT.ARGS)
    # mmb_mm2_stream_project_narrow_ft with the table type right after the table
    ft, tt = list(sig["mmb_mm2_stream_project_narrow_ft"][1]), list(sig["mmb_mm2_stream_project_narrow_tt"][1])
    i = NT.ARGS.index("table_type")
    assert NT.ARGS[i - 1] == "table" and tt == ft[:i] + [mmb_lib._I] + ft[i:]
    assert NT.ARGS[:i] + NT.ARGS[i + 1:] == NF.ARGS
    # mmb_mm2_text_cache likewise
    c32, c16 = list(sig["mmb_mm2_text_cache"][1]), list(sig["mmb_mm2_text_cache_tt"][1])
    assert NT.CACHE_ARGS[:2] == ["table", "table_type"] and c16 == c32[:1] + [mmb_lib._I] + c32[1:]
    assert len(c16) == len(NT.CACHE_ARGS)
    assert sig["mmb_mm2_text_cache_tt"][0] is mmb_lib._I and sig["mmb_mm2_stream_project_narrow_tt"][0] is mmb_lib._I


def test_library_exports_the_entry_points():
    lib = ctypes.CDLL(mmb_lib.LIB_PATH)
    for name in ("mmb_mm2_text_cache_tt", "mmb_mm2_stream_project_narrow_tt"):
        assert getattr(lib, name) is not None


@pytest.mark.parametrize("decl,words", [
    ("int mmb_mm2_text_cache_tt(const void* table, int table_type, int64_t v, int d, const float* wtab32,",
     ("byte for byte", "mmb_mm2_text_cache_bytes", "stay unwritten", "2-byte aligned")),
    ("int mmb_mm2_stream_project_narrow_tt(const int32_t* ids, const void* table, int table_type, int64_t v,",
     ("NOT read by", "bit for bit", "n == 0", "2-byte aligned", "mmb_mm2_stream_project_narrow_supported")),
])
def test_header_declares_and_documents_the_entry_points(decl, words):
    assert decl in HEADER
    head = HEADER[:HEADER.index(decl)]
    comment = " ".join(head[head.rindex("/*"):].replace(" * ", " ").split())
    assert "replaces" in comment and "sif2.py" in comment and "MMB_EINVAL" in comment
    assert "captured into a graph" in comment and "MMB_TABLE_F32 is" in comment
    for w in words:
        assert w in comment, w


def test_argument_table_starts_from_a_supported_call():
    b = NT.BASE
    assert mmb_lib.query("mmb_mm2_stream_project_narrow_supported", b["t"], b["d"], b["a"], b["vd"], b["v"])
    F.check_arg_row("mmb_mm2_stream_project_narrow_tt", NT.ARGS, dict(b, n=0), {}, NT.OK)
    for what, change, want in NT.ARG_CASES:
        rest = {k: v for k, v in change.items() if k not in ("table_type", "frame_type")}
        if want == NT.EINVAL:
            rest.pop("n", None)  # (", n 0" rows: the rejection comes before the empty call)
            if set(rest) != {"a", "vd"}:
                assert len(rest) <= 1, what
            for k, v in rest.items():
                assert v != b[k], what
        else:
            assert set(rest) <= {"n", "table"} and rest["n"] == 0, what


def test_all_nine_pairs_and_every_table_type_are_in_the_table():
    ok = {(c[1]["table_type"], c[1]["frame_type"]) for c in NT.ARG_CASES
          if c[2] == NT.OK and "frame_type" in c[1]}
    bad = {(c[1]["table_type"], c[1]["frame_type"]) for c in NT.ARG_CASES
           if c[2] == NT.EINVAL and "frame_type" in c[1] and c[1].get("ids", 1) is None}
    nine = set(itertools.product((0, 1, 2), (0, 1, 2)))
    assert ok == nine and bad == nine
    for tn, _ in T.TABLE_TYPES:
        assert sum(c[0].startswith(f"{tn} table, ") for c in NT.ARG_CASES) >= 12 + 6
    # a 16-bit table: 1 byte off rejected (also at n == 0), 2 and 4 bytes off accepted
    for tn, _ in T.TABLE_TYPES16:
        want = {"table 1 byte off": NT.EINVAL, "table 1 byte off, n 0": NT.EINVAL,
                "table 2 bytes off, n 0": NT.OK, "table 4 bytes off, n 0": NT.OK}
        for what, w in want.items():
            assert any(c[0] == f"{tn} table, {what}" and c[2] == w for c in NT.ARG_CASES), (tn, what)
    # table_type outside 0..2, also at n == 0
    assert sum(c[1].get("table_type") in (-1, 3) for c in NT.ARG_CASES) == 4
    assert sum(c[1].get("table_type") in (-1, 3) and c[1].get("n") == 0 for c in NT.ARG_CASES) == 2


@pytest.mark.parametrize("what,change,want", NT.ARG_CASES, ids=T._ids(NT.ARG_CASES))
def test_narrow_tt_argument_table_without_gpu(what, change, want):
    F.check_arg_row("mmb_mm2_stream_project_narrow_tt", NT.ARGS, NT.BASE, change, want)


@pytest.mark.parametrize("what,change,want", NT.CACHE_ARG_CASES, ids=T._ids(NT.CACHE_ARG_CASES))
def test_text_cache_tt_argument_table_without_gpu(what, change, want):
    assert want == NT.EINVAL  # (an accepted call launches: those are the GPU file's)
    F.check_arg_row("mmb_mm2_text_cache_tt", NT.CACHE_ARGS, NT.CACHE_BASE, change, want)


def test_text_cache_table_covers_every_type_and_the_odd_address():
    for tn, _ in T.TABLE_TYPES:
        assert sum(c[0].startswith(f"{tn} table, ") for c in NT.CACHE_ARG_CASES) >= 10
    for tn, _ in T.TABLE_TYPES16:
        assert any(c[0] == f"{tn} table, table 1 byte off" for c in NT.CACHE_ARG_CASES)
    b = NT.CACHE_BASE
    assert b["d"] % 4 == 0 and b["d"] + 1 <= 304 and b["ldw"] > b["d"] and 0 < b["v"] <= 16384
    assert b["ldw"] == mmb_lib.query("mmb_mm2_ldw", b["d"])


def test_cache_gap_is_the_headers():
    """Bytes [4 * 610 v, 4 * (609 v + 32)) for v < 32 (include/mmb.h), inside the cache."""
    assert "[4 * 610 v, 4 * (609 v + 32))" in HEADER
    for v in NT.CACHE_V:
        lo, hi = NT.cache_gap(v)
        nbytes = mmb_lib.query("mmb_mm2_text_cache_bytes", v, NT.D)
        if v < 32:
            assert (lo, hi) == (4 * 610 * v, 4 * (609 * v + 32)) and hi - lo == 4 * (32 - v)
            assert 0 < lo < hi <= nbytes
        else:
            assert hi == lo
    assert {v < 32 for v in NT.CACHE_V} == {True, False} and 33 in NT.CACHE_V and 1 in NT.CACHE_V
    assert NT.CACHE_FILL16 != NT.CACHE_FILL32
    assert all(d % 4 == 0 and 256 < d < 304 for d in NT.CACHE_D)


# ---------------------------------------------------------------- the plan
def _plan(name):
    import pipeline as PL

    shape = F._shapes()[name]
    shape = {"n_total": shape["n"], **shape}
    return lambda **kw: PL.step_plan(d=300, npc=1, cus=256, **shape, **kw)


OVERRIDES = T.OVERRIDES + (dict(narrow_fused=False), dict(chunks=3), dict(gram_kind="i8"),
                            dict(narrow_frames16=True), dict(fused_table16=True), dict(stream_project=False))


@pytest.mark.parametrize("name", ["c3", "mosi", "pom", "mid"])
def test_keyword_off_every_plan_is_todays(name):
    plan = _plan(name)
    for table in ("f32", "f16", "bf16"):
        for frames in FRAMES:
            for kw in OVERRIDES:
                off = plan(table=table, frames=frames, narrow_table16=False, **kw)
                assert off == plan(table=table, frames=frames, **kw), (table, frames, kw)
                assert table == "f32" or off.front != "narrow_fused"
                # on an f32 table the keyword changes nothing either way
                if table == "f32":
                    assert plan(frames=frames, narrow_table16=True, **kw) == off, (frames, kw)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["c3", "mosi", "pom", "mid"])
def test_step_plan_with_the_narrow_table16_keyword(name, kind):
    """The front is "narrow_fused" exactly where the f32-table plan of the same
    shape and frames chooses it: mosi on f32 frames, on 16-bit frames only
    together with narrow_frames16; c3 / mid (wide frames) and pom (T > 64) keep
    the plan they have without the keyword."""
    plan = _plan(name)
    f32 = plan()
    for frames in FRAMES:
        off = plan(table=kind, frames=frames)
        on = plan(table=kind, frames=frames, narrow_table16=True)
        both = plan(table=kind, frames=frames, narrow_table16=True, narrow_frames16=True)
        if name == "mosi":
            assert f32.front == "narrow_fused" and off.front == "stream"
            assert on == plan(frames=frames)  # the f32-table plan of the same shape and frames
            assert on.front == ("narrow_fused" if frames == "f32" else "stream")
            assert both == plan(frames=frames, narrow_frames16=True) and both.front == "narrow_fused"
            assert both.project == "front" and both.split is False and both.frames == frames
            assert both._replace(frames="f32") == f32
        else:
            assert name in NT.PLAN_UNCHANGED and f32.front != "narrow_fused"
            assert on == off and both == off
        # the split stream and the wide fused front stay off whatever is asked for
        forced = plan(table=kind, frames=frames, narrow_table16=True, stream_project=True, narrow_fused=True,
                      split_stream=True, fused_frames16=True, narrow_frames16=True, split_frames16=True)
        assert forced.split is False and forced.front in ("narrow_fused", "stream")
        assert (forced.front == "narrow_fused") == (name == "mosi")
        # the caller's narrow_fused and chunks are kept
        assert plan(table=kind, frames=frames, narrow_table16=True, narrow_frames16=True, narrow_fused=False) == off
        assert plan(table=kind, frames=frames, narrow_table16=True, narrow_frames16=True, chunks=3) == \
            plan(table=kind, frames=frames, chunks=3)
        # beside fused_table16 the precedence is the f32-table plan's (the split stream aside: not opted in to)
        assert plan(table=kind, frames=frames, narrow_table16=True, fused_table16=True, narrow_frames16=True,
                    fused_frames16=True) == \
            plan(frames=frames, narrow_frames16=True, fused_frames16=True)._replace(split=False)


def test_keywords_are_opt_in_and_add_no_plan_field():
    import pipeline as PL

    for fn in (PL.step_plan, PL.FusedStep.__init__):
        pars = inspect.signature(fn).parameters
        for k in ("narrow_table16", "split_table16"):
            assert pars[k].default is False
        names = list(pars)
        i = names.index("fused_table16")
        assert names[i - 2:i] == ["narrow_table16", "split_table16"]
    sp = list(inspect.signature(PL.step_plan).parameters)
    assert sp[-2:] == ["fused_table16", "table"]
    assert PL.StepPlan._fields == ("front", "split", "gram", "project", "proj_split", "bounds", "step_rows",
                                   "s_half", "frames")
    sig = inspect.signature(PL.mm2_stream_project_narrow_tt)
    assert list(sig.parameters) == list(inspect.signature(PL.mm2_stream_project_narrow_ft).parameters)
    par = inspect.signature(PL.MMB2Projection.enable_text_cache).parameters["table16"]
    assert par.default is False and par.kind is inspect.Parameter.KEYWORD_ONLY


# ---------------------------------------------------------------- the GPU file's tables
def test_gpu_cases_are_shapes_the_narrow_kernel_takes():
    sup = lambda c: bool(mmb_lib.query("mmb_mm2_stream_project_narrow_supported", c[2], NT.D, c[0], c[1], c[4]))  # noqa: E731
    assert all(sup(c) for c in NT.KERNEL_CASES + [NT.BAD_CASE, NT.ALIGN_CASE])
    assert {c[3] for c in NT.KERNEL_CASES} == {1, 31, 3000, 8200}
    # 1 and 4 utterances per wave, a ragged last batch
    assert {NF.rows_per_wave(c[3]) for c in NT.KERNEL_CASES} >= {1, 4} and 8200 % 32 != 0
    assert NT.BAD_CASE == NF.BAD_CASES[0] and NT.SPECIAL_CASE in NF.SPECIAL_CASES
    Dc, A, Vd, T_, N, V = NT.SPECIAL_CASE
    assert Dc == NT.D and sup((A, Vd, T_, N, V)) and Dc >= 2 * max(len(v) for v in T.SPECIALS.values())
    Dc, A, Vd, T_, N, V = NT.STEP
    assert NT.STEP == NF.STEP and sup((A, Vd, T_, N, V)) and N >= Dc
