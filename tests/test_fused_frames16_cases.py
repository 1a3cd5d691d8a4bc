"""CPU: the fused stream + projection kernel on 16-bit frames -- the entry
point's argument table, the step plan with the `fused_frames16` keyword, and
the tables tests/test_gpu_fused_frames16.py rests on.

mmb_mm2_stream_project_ft reads audio / visual frames stored as fp16 or bf16
and must give, bit for bit, what mmb_mm2_stream_project gives on the same
frames upcast to f32.  Nothing here needs a device: the argument checks and
the empty call return before any launch (stand-in pointers, as
tests/test_lib_abi.py), and the plan is host logic.
"""
import inspect

import pytest

import frames16_cases as F
import fused_frames16_cases as FF
import mmb_lib

KINDS = list(FF.KINDS)


# ---------------------------------------------------------------- the entry point
def test_signature_mirrors_the_header():
    assert len(mmb_lib.SIGNATURES["mmb_mm2_stream_project_ft"][1]) == len(FF.ARGS)
    # mmb_mm2_stream_project without text_dense, with frame_type after the frames
    ref = list(mmb_lib.SIGNATURES["mmb_mm2_stream_project"][1])
    ft = list(mmb_lib.SIGNATURES["mmb_mm2_stream_project_ft"][1])
    i = FF.ARGS.index("frame_type")
    assert ft[:i] + ft[i + 1:] == ref[:4] + ref[5:] and ft[i] is mmb_lib.SIGNATURES["mmb_mm2_k"][1][0]


def test_argument_table_starts_from_a_supported_call():
    b = FF.BASE
    assert mmb_lib.query("mmb_mm2_stream_project_supported", b["t"], b["d"], b["a"], b["vd"])
    assert FF.P % 16 == 0
    for what, change, want in FF.ARG_CASES:
        rest = {k: v for k, v in change.items() if k != "frame_type"}
        assert len(rest) <= 1, what  # one thing changed (beside the frame type the row is about)
        if want == FF.EINVAL and len(rest) == 1:
            k, v = next(iter(rest.items()))
            assert v != b[k], what
    kinds16 = [w for w, _, _ in FF.ARG_CASES if w.startswith(("f16 ", "bf16 "))]
    assert len(kinds16) == 2 * 9  # both kinds carry every row


@pytest.mark.parametrize("what,change,want", FF.ARG_CASES, ids=[c[0].replace(" ", "_") for c in FF.ARG_CASES])
def test_stream_project_ft_argument_table_without_gpu(what, change, want):
    F.check_arg_row("mmb_mm2_stream_project_ft", FF.ARGS, FF.BASE, change, want)


# ---------------------------------------------------------------- the plan
def _plan(name):
    import pipeline as PL

    shape = F._shapes()[name]
    shape = {"n_total": shape["n"], **shape}
    return lambda **kw: PL.step_plan(d=300, npc=1, cus=256, **shape, **kw)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["c3", "mosi", "pom", "mid"])
def test_step_plan_with_the_fused_frames16_keyword(name, kind):
    plan = _plan(name)
    # keyword off: today's plan, the two-kernel one whatever the overrides say
    base = plan(stream_project=False, narrow_fused=False, split_stream=False)
    off = plan(frames=kind)
    assert off == plan(frames=kind, fused_frames16=False) and off._replace(frames="f32") == base
    assert plan(frames=kind, stream_project=True, narrow_fused=True, split_stream=True) == off
    on = plan(frames=kind, fused_frames16=True)
    f32 = plan()
    if name in ("c3", "mid"):
        assert f32.front == "fused"
        assert on.front == "fused" and on.project == "front" and on.split is False and on.frames == kind
        # the f32 fused plan of the shape, on these frames
        assert on._replace(frames="f32") == f32
        assert on.proj_split is False
    else:
        # narrow frames (mosi), T > 64 (pom): the fused kernel is not the f32 plan's choice
        assert f32.front != "fused"
        assert on == off
    # the narrow fused front and the split stream stay off with the keyword set
    forced = plan(frames=kind, fused_frames16=True, narrow_fused=True, split_stream=True)
    assert forced.front in ("fused", "stream") and forced.split is False
    # the caller's stream_project is kept: off, or more than one chunk asked for
    assert plan(frames=kind, fused_frames16=True, stream_project=False) == off
    for p in (plan(frames=kind, fused_frames16=True, stream_project=False),
              plan(frames=kind, fused_frames16=True, chunks=3)):
        assert p.front == "stream" and p.frames == kind
    assert plan(frames=kind, fused_frames16=True, chunks=3) == plan(frames=kind, chunks=3)


@pytest.mark.parametrize("name", ["c3", "mosi", "pom", "mid"])
def test_keyword_changes_nothing_on_f32_frames(name):
    plan = _plan(name)
    for kw in ({}, dict(stream_project=True), dict(stream_project=False), dict(chunks=3),
               dict(narrow_fused=False), dict(gram_kind="i8")):
        assert plan(fused_frames16=True, **kw) == plan(**kw) == plan(frames="f32", fused_frames16=True, **kw)


def test_keyword_is_opt_in_and_adds_no_plan_field():
    import pipeline as PL

    for fn in (PL.step_plan, PL.FusedStep.__init__):
        par = inspect.signature(fn).parameters["fused_frames16"]
        assert par.default is False
    assert PL.StepPlan._fields[8:] == ("frames",)
    sig = inspect.signature(PL.mm2_stream_project_ft)
    assert list(sig.parameters) == ("n t d a vd audio visual proj ids32 table wtab32 w_dense flag out colmax "
                                    "colmax_ws").split()


# ---------------------------------------------------------------- the GPU file's tables
def test_gpu_cases_are_shapes_the_fused_kernel_takes():
    sup = lambda T, D, A, Vd: bool(mmb_lib.query("mmb_mm2_stream_project_supported", T, D, A, Vd))  # noqa: E731
    widths, lens, rows = set(), set(), set()
    for D, A, Vd, T, N, bad in FF.KERNEL_CASES:
        assert sup(T, D, A, Vd) and A != Vd
        widths |= {D, A, Vd}
        lens.add(T)
        rows.add(N)
    assert widths == {4, 20, 256, 260, 300, 316, 320}
    assert lens == {1, 7, 16, 17, 20, 21, 33, 40, 64} and rows == {1, 13, 49, 97, 2500}
    assert sum(c[5] for c in FF.KERNEL_CASES) == 1
    D, A, Vd, T, N = FF.LARGE
    assert sup(T, D, A, Vd) and T >= 21           # the pipelined streamer
    assert N * T * Vd * 2 > 2 ** 31 > N * T * A * 4  # 16-bit visual rows past 2^31 bytes
    # the dynamic order on 256 CUs: >= 16 rounds of 48-row batches, a 2-row last 12-row unit
    G = 256
    assert -(-N // 48) >= 16 * G
    big = max(0, N - 48 * G) // 48
    assert (N - big * 48) % 12 == 2
    for shape in FF.SPECIAL_SHAPES:
        D, A, Vd, T = shape
        assert sup(T, D, A, Vd) and FF.SPECIAL_N >= 3 and T >= 4 and T > F.SPECIAL_PADS
    assert FF.SPECIAL_SHAPES[0][3] < 21 <= FF.SPECIAL_SHAPES[1][3]


def test_gpu_step_is_one_the_family_conditions_cover():
    """The step compared with the oracle is in frames16_cases.STEP, whose
    conditions tests/test_frames16_cases.py pins on the upcast inputs."""
    assert FF.STEP in [tuple(d) for d in F.STEP]
    assert all(tuple(d) in [tuple(s) for s in F.STEP] for d in FF.STEP_UNCHANGED)
