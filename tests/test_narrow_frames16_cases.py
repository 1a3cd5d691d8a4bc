"""CPU: the narrow fused kernel on 16-bit frames -- the entry point's argument
table, the step plan with the `narrow_frames16` keyword, and the tables
tests/test_gpu_narrow_frames16.py rests on.

mmb_mm2_stream_project_narrow_ft reads audio / visual frames stored as fp16 or
bf16 and must give, bit for bit, what mmb_mm2_stream_project_narrow gives on
the same frames upcast to f32.  Nothing here needs a device: the argument
checks and the empty call return before any launch (stand-in pointers, as
tests/test_lib_abi.py), and the plan is host logic.
"""
import inspect

import pytest

import abi_cases as ABI
import frames16_cases as F
import mmb_lib
import narrow_frames16_cases as NF


KINDS = list(NF.KINDS)
NAME = "mmb_mm2_stream_project_narrow_ft"


# ---------------------------------------------------------------- the entry point
def test_header_declares_and_library_exports_the_entry_point():
    assert NAME in ABI.declared_functions()
    assert hasattr(mmb_lib.load(), NAME)


def test_signature_mirrors_the_header():
    assert len(mmb_lib.SIGNATURES[NAME][1]) == len(NF.ARGS)
    # mmb_mm2_stream_project_narrow with frame_type after the frames
    ref = list(mmb_lib.SIGNATURES["mmb_mm2_stream_project_narrow"][1])
    ft = list(mmb_lib.SIGNATURES[NAME][1])
    i = NF.ARGS.index("frame_type")
    assert ft[:i] + ft[i + 1:] == ref and ft[i] is mmb_lib.SIGNATURES["mmb_mm2_k"][1][0]
    assert mmb_lib.SIGNATURES[NAME][0] is mmb_lib.SIGNATURES["mmb_mm2_stream_project_narrow"][0]


def test_mirror_signature():
    import pipeline as PL

    sig = inspect.signature(PL.mm2_stream_project_narrow_ft)
    assert list(sig.parameters) == ("n t d a vd audio visual proj ids32 table wtab32 flag out colmax "
                                    "colmax_ws").split()
    for name in ("flag", "out", "colmax", "colmax_ws"):
        assert sig.parameters[name].default is None
    # the f32 mirror's, name for name
    assert list(sig.parameters) == list(inspect.signature(PL.mm2_stream_project_narrow).parameters)


def test_argument_table_starts_from_a_supported_call():
    b = NF.BASE
    assert mmb_lib.query("mmb_mm2_stream_project_narrow_supported", b["t"], b["d"], b["a"], b["vd"], b["v"])
    assert NF.P % 16 == 0
    whats = [w for w, _, _ in NF.ARG_CASES]
    assert len(set(whats)) == len(whats)
    for kind in ("f32", "f16", "bf16"):
        for row in ("n 0", "audio 4 bytes off", "visual 4 bytes off", "null ids", "null text cache",
                    "null wpieces", "A 128 Vd 100", "V 16385", "D 256", "D 304"):
            assert f"{kind} {row}" in whats
    for kind in ("f16", "bf16"):
        for row in ("audio 2 bytes off", "visual 2 bytes off"):
            assert f"{kind} {row}" in whats
    # the rejected shapes are rejected for the reason the row names
    sup = lambda **kw: bool(mmb_lib.query("mmb_mm2_stream_project_narrow_supported",  # noqa: E731
                                          *[dict(b, **kw)[k] for k in ("t", "d", "a", "vd", "v")]))
    assert not sup(a=128, vd=100) and sup(a=112, vd=16) and sup(a=16, vd=100)
    assert not sup(v=16385) and sup(v=16384)
    assert not sup(d=256) and sup(d=260) and not sup(d=304)


@pytest.mark.parametrize("what,change,want", NF.ARG_CASES, ids=[c[0].replace(" ", "_") for c in NF.ARG_CASES])
def test_stream_project_narrow_ft_argument_table_without_gpu(what, change, want):
    F.check_arg_row(NAME, NF.ARGS, NF.BASE, change, want)


# ---------------------------------------------------------------- the plan
def _plan(name):
    import pipeline as PL

    shape = F._shapes()[name]
    shape = {"n_total": shape["n"], **shape}
    return lambda **kw: PL.step_plan(d=300, npc=1, cus=256, **shape, **kw)


def test_the_mosi_plan_shape_is_the_issue_s():
    s = F._shapes()["mosi"]
    assert (s["a"], s["vd"], s["t"], s["V"]) == (76, 48, 20, 3016)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["c3", "mosi", "pom", "mid"])
def test_keyword_off_every_plan_is_the_former_one(name, kind):
    plan = _plan(name)
    base = plan(stream_project=False, narrow_fused=False, split_stream=False)
    for kw in ({}, dict(narrow_fused=True), dict(stream_project=True, narrow_fused=True, split_stream=True),
               dict(chunks=3), dict(gram_kind="i8"), dict(fused_frames16=True),
               dict(fused_frames16=True, narrow_fused=True)):
        assert plan(frames=kind, **kw) == plan(frames=kind, narrow_frames16=False, **kw)
    # the two-kernel plan whatever the overrides say, narrow_fused=True among them
    for kw in ({}, dict(narrow_fused=True), dict(stream_project=True, narrow_fused=True, split_stream=True)):
        got = plan(frames=kind, **kw)
        assert got.front == "stream" and got._replace(frames="f32") == base
    assert plan(frames=kind, fused_frames16=True, narrow_fused=True).front in ("fused", "stream")


@pytest.mark.parametrize("kind", KINDS)
def test_keyword_on_at_the_mosi_shape(kind):
    plan = _plan("mosi")
    f32, off = plan(), plan(frames=kind)
    assert f32.front == "narrow_fused"
    for kw in ({}, dict(narrow_fused=True), dict(narrow_fused=None)):
        on = plan(frames=kind, narrow_frames16=True, **kw)
        assert on.front == "narrow_fused" and on.project == "front" and on.frames == kind
        assert on.split is False and on.proj_split is False
        # the f32 narrow fused plan of the shape, on these frames
        assert on._replace(frames="f32") == f32
    # the caller's narrow_fused is kept
    assert plan(frames=kind, narrow_frames16=True, narrow_fused=False) == off and off.front == "stream"
    # the split stream stays forced off; a stream_project override alone opts in to nothing
    forced = plan(frames=kind, narrow_frames16=True, split_stream=True, stream_project=True)
    assert forced == plan(frames=kind, narrow_frames16=True)
    # more than one chunk asked for: the plan without the keyword
    assert plan(frames=kind, narrow_frames16=True, chunks=3) == plan(frames=kind, chunks=3)
    assert plan(frames=kind, narrow_frames16=True, chunks=3).front == "stream"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(NF.PLAN_UNCHANGED))
def test_keyword_on_at_shapes_the_narrow_kernel_does_not_take(name, kind):
    """Wide frames, T > 64: quietly the plan without the keyword."""
    plan = _plan(name)
    assert plan().front != "narrow_fused", NF.PLAN_UNCHANGED[name]
    for kw in ({}, dict(narrow_fused=True), dict(chunks=3)):
        assert plan(frames=kind, narrow_frames16=True, **kw) == plan(frames=kind, **kw)
        assert plan(frames=kind, narrow_frames16=True, **kw).front == "stream"


@pytest.mark.parametrize("kind", KINDS)
def test_keyword_on_past_the_text_cache(kind):
    """V > 16384 at MOSI's widths: unsupported, quietly the stream kernel."""
    import pipeline as PL

    shape = dict(F._shapes()["mosi"])
    shape = {"n_total": shape["n"], **shape, "V": 16385}
    plan = lambda **kw: PL.step_plan(d=300, npc=1, cus=256, **shape, **kw)  # noqa: E731
    assert plan().front == "stream"
    assert plan(frames=kind, narrow_frames16=True) == plan(frames=kind)
    assert plan(frames=kind, narrow_frames16=True).front == "stream"


@pytest.mark.parametrize("kind", KINDS)
def test_both_keywords_keep_the_f32_precedence(kind):
    import pipeline as PL

    both = dict(fused_frames16=True, narrow_frames16=True)
    # (300, 300, 300, 40): the wide fused front
    for name in ("c3", "mid"):
        plan = _plan(name)
        on = plan(frames=kind, **both)
        assert on.front == "fused" and on._replace(frames="f32") == plan()
    # MOSI: the narrow one
    plan = _plan("mosi")
    assert plan(frames=kind, **both).front == "narrow_fused"
    assert plan(frames=kind, **both)._replace(frames="f32") == plan()
    # a shape both fused kernels take (D = 260, narrow frames) with stream_project asked for:
    # the wide fused front first, as on f32 frames
    shape = dict(n=1284, n_total=1284, t=20, d=260, a=76, vd=48, V=3016, npc=1, cus=256)
    assert PL.stream_project_supported(20, 260, 76, 48) and PL.narrow_fused_supported(20, 260, 76, 48, 3016)
    f32 = PL.step_plan(**shape, stream_project=True)
    assert f32.front == "fused"
    assert PL.step_plan(**shape, stream_project=True, frames=kind, **both)._replace(frames="f32") == f32
    assert PL.step_plan(**shape, frames=kind, **both).front == "narrow_fused"


@pytest.mark.parametrize("name", ["c3", "mosi", "pom", "mid"])
def test_keyword_changes_nothing_on_f32_frames(name):
    plan = _plan(name)
    for kw in ({}, dict(stream_project=True), dict(narrow_fused=True), dict(narrow_fused=False), dict(chunks=3),
               dict(gram_kind="i8"), dict(fused_frames16=True)):
        assert plan(narrow_frames16=True, **kw) == plan(**kw) == plan(frames="f32", narrow_frames16=True, **kw)


def test_keyword_is_opt_in_and_adds_no_plan_field():
    import pipeline as PL

    for fn in (PL.step_plan, PL.FusedStep.__init__):
        par = inspect.signature(fn).parameters["narrow_frames16"]
        assert par.default is False
    assert PL.StepPlan._fields[8:] == ("frames",)
    assert PL._FRONTS_FT["narrow_fused"] is PL.mm2_stream_project_narrow_ft
    assert set(PL._FRONTS_FT) == set(PL._FRONTS)


# ---------------------------------------------------------------- the GPU file's tables
def test_gpu_cases_reach_what_they_are_there_for():
    sup = lambda T, A, Vd, V: bool(mmb_lib.query("mmb_mm2_stream_project_narrow_supported",  # noqa: E731
                                                 T, NF.D, A, Vd, V))
    assert len(set(NF.KERNEL_CASES)) == len(NF.KERNEL_CASES)
    for A, Vd, T, N, V in NF.KERNEL_CASES:
        assert sup(T, A, Vd, V) and N <= NF.MAX_ROWS
    ga, gv = NF.LOAD_GROUPS
    by = {c: c for c in NF.KERNEL_CASES}
    # MOSI: P = 3 / 5 rows per instruction, partial last groups, every frame in the first load group
    assert (NF.rows_per_instruction(76), NF.rows_per_instruction(48)) == (3, 5)
    assert 20 % 3 and 20 % 5 == 0 and NF.groups(20, 76) == 7 <= ga and NF.groups(20, 48) == 4 <= gv
    # 1, 2 and 4 utterances per wave on a 256-CU chip; a last batch of 8 rows
    assert [NF.rows_per_wave(n) for n in (3000, 6000, 8200)] == [1, 2, 4]
    assert 8200 % 32 == 8 and (76, 48, 20, 8200, 3016) in by
    assert {c[3] for c in NF.KERNEL_CASES if c[:3] == (76, 48, 20)} >= {1, 5, 31, 77, 3000, 6000, 8200}
    assert any(c[4] < 32 for c in NF.KERNEL_CASES)  # fewer words than hot slots
    # the later-group loops: more groups than the first load group holds
    assert NF.groups(64, 76) == 22 > ga and NF.groups(64, 48) > gv and (76, 48, 64, 517, 5000) in by
    # all 64 lanes live; a lone unit per row; the widest frames
    assert 64 // 4 == 16 and NF.rows_per_instruction(64) * 16 == 64 and (64, 56, 64, 517, 5000) in by
    assert NF.rows_per_instruction(4) == 64 and (4, 4, 1, 5, 3016) in by
    assert NF.rows_per_instruction(112) == 2 and not sup(40, 116, 16, 3016) and (112, 16, 40, 1001, 3016) in by
    assert any(c[4] == 16384 for c in NF.KERNEL_CASES)
    for c in NF.BAD_CASES:
        assert c in by and c[3] > 40
    for D, A, Vd, T, N, V in NF.SPECIAL_CASES:
        assert sup(T, A, Vd, V) and D == NF.D and N >= 3 and T > F.SPECIAL_PADS
        assert T >= max(len(v) for v in F.SPECIALS.values())
    assert {c[1:3] for c in NF.SPECIAL_CASES} == {(76, 48), (4, 4)}
    # the guard: a power of two exact in both kinds, whole 16-byte units either side
    for kind, dt in NF.KINDS.items():
        import torch

        assert float(torch.tensor(NF.GUARD).to(dt)) == NF.GUARD
    for A, Vd, T, N, V in NF.KERNEL_CASES:
        for w in (A, Vd):
            g = NF.guard_elements(T, w)
            assert g % 8 == 0 and g >= 2 * T * w


def test_gpu_step_is_the_issue_s():
    D, A, Vd, T, N, V = NF.STEP
    assert (D, A, Vd, T, N, V) == (300, 76, 48, 20, 3000, 3016)
    assert mmb_lib.query("mmb_mm2_stream_project_narrow_supported", T, D, A, Vd, V)
