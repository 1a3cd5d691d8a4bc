"""CPU: the split stream on 16-bit frames -- the entry point's argument table,
the step plan with the `split_frames16` keyword, and the tables
tests/test_gpu_split_frames16.py rests on.

mmb_mm2_stream_split_ft reads audio / visual frames stored as fp16 or bf16 and
must give, bit for bit, what mmb_mm2_stream_split gives, with the same parts,
on the same frames upcast to f32.  Nothing here needs a device: the argument
checks and the empty call return before any launch or device query (stand-in
pointers and an explicit part count, as tests/test_lib_abi.py), and the plan
is host logic.
"""
import inspect
import itertools

import pytest

import abi_cases as ABI
import frames16_cases as F
import mmb_lib
import split_frames16_cases as SF


KINDS = list(SF.KINDS)
NAME = "mmb_mm2_stream_split_ft"


# ---------------------------------------------------------------- the entry point
def test_header_declares_and_library_exports_the_entry_point():
    assert NAME in ABI.declared_functions()
    assert hasattr(mmb_lib.load(), NAME)


def test_signature_mirrors_the_header():
    sig = mmb_lib.SIGNATURES
    assert len(sig[NAME][1]) == len(SF.ARGS)
    # mmb_mm2_stream_ft, then parts, ws, ws_bytes in front of the stream -- as mmb_mm2_stream_split
    # ends mmb_mm2_stream
    ft, split = list(sig["mmb_mm2_stream_ft"][1]), list(sig["mmb_mm2_stream_split"][1])
    assert list(sig[NAME][1]) == ft[:-1] + split[-4:]
    assert SF.ARGS[:-4] == F.ARGS[:-1] and SF.ARGS[-4:] == ABI.ENTRY_ARGS["mmb_mm2_stream_split"][-4:]
    assert sig[NAME][0] is sig["mmb_mm2_stream_split"][0]


def test_mirror_signature():
    import pipeline as PL

    sig = inspect.signature(PL.mm2_stream_split_ft)
    assert list(sig.parameters) == ("n t d a vd audio visual ids32 table wtab32 w_dense flag out s_half colmax "
                                    "colmax_ws split parts").split()
    for name in ("wtab32", "w_dense", "flag", "out", "colmax", "colmax_ws", "split"):
        assert sig.parameters[name].default is None
    assert sig.parameters["s_half"].default is True and sig.parameters["parts"].default == 0
    # mm2_stream's own names (its dense-text arguments aside), so that the step calls either alike
    stream = inspect.signature(PL.mm2_stream).parameters
    assert set(sig.parameters) == set(stream) - {"text_dense", "emb_dense"}
    for name in ("s_half", "parts", "split"):
        assert sig.parameters[name].default == stream[name].default


def test_argument_table_starts_from_a_call_the_library_takes():
    b = SF.BASE
    assert 3 * b["d"] + 2 * b["a"] + 2 * b["vd"] <= SF.FINISH_COLUMNS < 3 * 512 + 2 * b["a"] + 2 * b["vd"]
    assert b["parts"] > 0 and 0 < SF.ws_bytes() < b["ws_bytes"] and 0 < SF.ws_bytes(d=512) < b["ws_bytes"]
    assert b["n"] <= SF.MAX_BOUND_ROWS
    # the same bytes as the f32 entry point's workspace: the partials are f32
    assert mmb_lib.query("mmb_mm2_colmax_ws_bytes", b["d"]) // (4 * b["d"]) == SF.MAX_BOUND_ROWS
    whats = [w for w, _, _ in SF.ARG_CASES]
    assert len(set(whats)) == len(whats)
    for kind in ("f32", "f16", "bf16"):
        for row in ("null ids", "workspace one byte short", "parts -1", "D 512", "bounds with n 8193",
                    "n 0, no workspace"):
            assert f"{kind} {row}" in whats
    for kind in ("f16", "bf16"):
        for row in ("audio at an odd address", "visual at an odd address"):
            assert f"{kind} {row}" in whats


@pytest.mark.parametrize("what,change,want", SF.ARG_CASES, ids=[c[0].replace(" ", "_") for c in SF.ARG_CASES])
def test_stream_split_ft_argument_table_without_gpu(what, change, want):
    F.check_arg_row(NAME, SF.ARGS, SF.BASE, SF.resolve(change), want)


def test_f32_frames_need_no_even_address():
    """The odd-address rule is the 16-bit types': the f32 rows are rejected or
    taken as by mmb_mm2_stream_split (scalar rows from any 4-byte address)."""
    F.check_arg_row(NAME, SF.ARGS, SF.BASE, dict(frame_type=F.F32, n=0, audio=F.P + 4), F.OK)
    F.check_arg_row(NAME, SF.ARGS, SF.BASE, dict(frame_type=F.F16, n=0, audio=F.P + 2, visual=F.P + 6), F.OK)


# ---------------------------------------------------------------- the plan
CUS = 256


def _plan(t, n, n_total=None, **shape):
    import pipeline as PL

    shape = dict(dict(d=300, a=300, vd=300, V=7763, npc=1, cus=CUS), **shape)
    return lambda **kw: PL.step_plan(n=n, n_total=n if n_total is None else n_total, t=t, **shape, **kw)


GRID = list(itertools.product((SF.PLAN_MIN_T, SF.PLAN_MIN_T + 1), (CUS, CUS + 1), (None, 1000), (None, 1, 2),
                              (None, True, False)))


def test_the_grid_reaches_both_sides_of_every_condition():
    seen = set()
    for t, n, n_total, chunks, split_stream in GRID:
        p = _plan(t, n, n_total)(chunks=chunks, split_stream=split_stream)
        seen.add((p.front == "stream", len(p.bounds) == 1, t > SF.PLAN_MIN_T, n <= CUS, split_stream is not False,
                  p.split))
    assert {s[-1] for s in seen} == {True, False}
    # t, n and the caller's split_stream each fail alone somewhere; the fused front (t <= 64 here) and a
    # second chunk (more rows than CUs here) fail beside one of those -- the split is off in every such plan
    for i in (2, 3, 4):
        assert any(not s[i] and all(s[:i] + s[i + 1:5]) for s in seen), i
    for i in (0, 1):
        assert any(not s[i] for s in seen) and any(s[i] for s in seen), i
    assert all(s[5] == all(s[:5]) for s in seen)


@pytest.mark.parametrize("kind", KINDS)
def test_keyword_on_the_split_is_the_f32_plan_s(kind):
    for t, n, n_total, chunks, split_stream in GRID:
        plan = _plan(t, n, n_total)
        kw = dict(chunks=chunks, split_stream=split_stream)
        f32 = plan(**kw)
        on = plan(frames=kind, split_frames16=True, **kw)
        assert on.split is f32.split, (t, n, n_total, kw)
        assert on.frames == kind and on.front == "stream"
        # everything but the front kernels the keyword does not opt in to
        assert on._replace(frames="f32") == plan(stream_project=False, narrow_fused=False, **kw)
        # without the keyword: never split, the former plan
        off = plan(frames=kind, **kw)
        assert off.split is False and off == plan(frames=kind, split_frames16=False, **kw)
        assert off == on._replace(split=False)


@pytest.mark.parametrize("kind", KINDS)
def test_keyword_on_at_pom_s_shape(kind):
    shape = F._shapes()["pom"]
    assert (shape["n"], shape["t"]) == SF.POM_VALID[:2]
    import pipeline as PL

    plan = lambda **kw: PL.step_plan(d=300, npc=1, cus=CUS, n_total=shape["n"], **shape, **kw)  # noqa: E731
    f32 = plan()
    assert f32.front == "stream" and f32.split is True
    for kw in ({}, dict(split_stream=True), dict(split_stream=None)):
        assert plan(frames=kind, split_frames16=True, **kw)._replace(frames="f32") == f32
    # the caller's split_stream is kept
    assert plan(frames=kind, split_frames16=True, split_stream=False) == plan(frames=kind)
    assert plan(frames=kind, split_stream=True).split is False


@pytest.mark.parametrize("name", ["c3", "mosi", "pom", "mid"])
def test_keyword_changes_nothing_on_f32_frames(name):
    import pipeline as PL

    shape = F._shapes()[name]
    plan = lambda **kw: PL.step_plan(d=300, npc=1, cus=CUS, n_total=shape["n"], **shape, **kw)  # noqa: E731
    for kw in ({}, dict(split_stream=True), dict(split_stream=False), dict(stream_project=False), dict(chunks=3),
               dict(narrow_fused=False), dict(fused_frames16=True, narrow_frames16=True)):
        assert plan(split_frames16=True, **kw) == plan(**kw) == plan(frames="f32", split_frames16=True, **kw)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["c3", "mosi", "pom", "mid"])
def test_the_three_keywords_together_give_the_f32_plan(name, kind):
    import pipeline as PL

    shape = F._shapes()[name]
    plan = lambda **kw: PL.step_plan(d=300, npc=1, cus=CUS, n_total=shape["n"], **shape, **kw)  # noqa: E731
    all3 = dict(fused_frames16=True, narrow_frames16=True, split_frames16=True)
    for kw in ({}, dict(split_stream=True), dict(stream_project=True), dict(narrow_fused=False), dict(chunks=3)):
        f32, on = plan(**kw), plan(frames=kind, **all3, **kw)
        assert (on.front, on.split) == (f32.front, f32.split) and on._replace(frames="f32") == f32
    # the split keyword alone leaves the fused fronts off
    assert plan(frames=kind, split_frames16=True).front == "stream"


def test_keyword_is_opt_in_and_adds_no_plan_field():
    import pipeline as PL

    for fn in (PL.step_plan, PL.FusedStep.__init__):
        par = inspect.signature(fn).parameters["split_frames16"]
        assert par.default is False
    assert PL.StepPlan._fields == ("front", "split", "gram", "project", "proj_split", "bounds", "step_rows",
                                   "s_half", "frames")


# ---------------------------------------------------------------- the GPU file's tables
def test_gpu_cases_reach_what_they_are_there_for():
    assert len({c[:4] for c in SF.KERNEL_CASES}) == len(SF.KERNEL_CASES)
    for n, t, a, vd, parts, ao, vo in SF.KERNEL_CASES:
        assert 3 * SF.D + 2 * a + 2 * vd <= SF.FINISH_COLUMNS and n <= SF.MAX_BOUND_ROWS
        assert t > SF.PLAN_MIN_T and all(p >= 0 for p in parts)
    # T just past the threshold: ranges of 33 / 32 frames on 4 row slots, the one-range launch among the parts
    assert SF.KERNEL_CASES[0][:5] == (5, SF.PLAN_MIN_T + 1, 300, 300, (1, 2, 0))
    assert SF.ranges(65, 2) == [33, 32] and SF.slots(300, True) == (75, 4)
    per_slot = -(-33 // 4)  # 9 frames: the unroll's remainder runs at 8, and alone at 16
    assert per_slot == 9 and per_slot % SF.FRAME_UNROLLS[0] and per_slot < SF.FRAME_UNROLLS[1]
    # 19 / 12 units, 16 / 26 slots, a short last range; a slot gets one frame or two
    assert SF.ranges(200, 7) == [29] * 6 + [26]
    assert (SF.slots(76, True), SF.slots(48, True)) == ((19, 16), (12, 26))
    assert 16 < 29 < 2 * 16 and 26 < 29 < 2 * 26
    # one unit x 320 slots, most empty; 166 units x ONE slot: whole unrolled groups and a remainder
    assert SF.slots(4, True) == (1, 320) and SF.slots(664, True) == (166, 1)
    assert SF.ranges(130, 3) == [44, 44, 42] and 44 < 320 // 2
    assert all(44 > u and 44 % u for u in SF.FRAME_UNROLLS)
    assert 3 * SF.D + 2 * (4 + 664) <= SF.FINISH_COLUMNS < 3 * SF.D + 2 * (4 + 664 + 4)
    # scalar rows by width; by alignment (audio 2 bytes off) beside whole units 8 bytes off
    assert not SF.vector(46) and not SF.vector(37) and SF.slots(46, False) == (46, 6)
    n, t, a, vd, parts, ao, vo = SF.KERNEL_CASES[-1]
    assert (ao * 2, vo * 2) == (2, 8) and not SF.vector(a, ao) and SF.vector(vd, vo)
    assert SF.vector(a) and not SF.vector(vd, 2, fbytes=4)  # (8 bytes off is half an f32 unit)
    # more than one workgroup per modality everywhere; the guard is exact in both kinds
    import torch

    for kind, dt in SF.KINDS.items():
        assert float(torch.tensor(SF.GUARD).to(dt)) == SF.GUARD
    for n, t, a, vd, parts, ao, vo in SF.KERNEL_CASES:
        for w in (a, vd):
            g = SF.guard_elements(t, w)
            assert g % 8 == 0 and g >= 2 * t * w


def test_special_and_bad_cases():
    paths = set()
    for case, parts in SF.SPECIAL_CASES:
        D, A, Vd, T, N, V = case
        assert (D, V) == (SF.D, SF.V) and N >= 3 and T > F.SPECIAL_PADS and parts > 1
        assert T >= max(len(v) for v in F.SPECIALS.values()) and T > SF.PLAN_MIN_T
        assert 3 * D + 2 * A + 2 * Vd <= SF.FINISH_COLUMNS
        paths.add((SF.vector(A), SF.vector(Vd)))
    assert paths == {(True, True), (False, False)}
    n, t, a, vd, parts = SF.BAD_CASE
    assert t <= SF.V and n >= 6 and parts > 1  # a transcript of distinct rare words fits the table


def test_gpu_step_shapes_take_the_split():
    import pipeline as PL

    for n, t, a, vd in (SF.STEP, SF.POM_VALID):
        assert 3 * SF.D + 2 * a + 2 * vd <= SF.FINISH_COLUMNS
        for kind in KINDS:
            p = PL.step_plan(n, n, t, SF.D, a, vd, 7763, 1, CUS, frames=kind, split_frames16=True)
            assert p.split is True and p.front == "stream" and p.frames == kind
            assert PL.step_plan(n, n, t, SF.D, a, vd, 7763, 1, CUS, frames=kind).split is False
