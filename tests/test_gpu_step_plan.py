"""The step's launch sequence and stream topology, and two input guards.

FusedStep._run is one sequence chosen by step_plan().  For every
configuration the ordered C entry points, the stream each runs on and every
wait_stream / wait_event / record edge between the step's streams are pinned
here as literals: a captured graph replays exactly this topology, and a fork
joined back to another stream than it left has crashed the capture before
(StepGraph).  The lists were recorded with this recorder from the five-branch
_run that preceded the plan.

Entries: (entry point, stream) for a launch; ("wait_stream", "A<-B") for
A.wait_stream(B); ("wait_event", "A<-e1") / ("record", "e1@A") for the chunk
pipeline's events.  Streams: `caller` is the stream _run was called on,
s0, s1, ... the others in order of first appearance.
"""
import pytest
import torch

import mmb_lib as L
import models
import pipeline as P
import synth

pytestmark = pytest.mark.gpu


def _identity(t):
    return t


# name: (n, t, a, vd, V, constructor arguments, _run's fork)
CASES = {
    "narrow_fused": (64, 20, 76, 48, 3016, {}, True),
    "fused": (64, 40, 300, 300, 5000, {}, True),
    "forked_projection": (64, 40, 300, 300, 5000, dict(stream_project=False), True),
    "project_remove": (64, 40, 300, 300, 5000,
                       dict(stream_project=False, fork_projection=False), True),
    "separate_remove": (64, 40, 300, 300, 5000,
                        dict(fuse_remove=False, stream_project=False), True),
    "forked_projection_unforked": (64, 40, 300, 300, 5000, dict(stream_project=False), False),
    "chunks3": (700, 40, 300, 300, 5000, dict(chunks=3), True),
    "chunks4_side_cus": (1024, 40, 300, 300, 5000, dict(chunks=4, side_cus=96), True),
    "split_stream": (10, 80, 300, 300, 5000, {}, True),
    "direct_branch": (320, 40, 300, 300, 5000, {}, True),
    "npc2": (64, 40, 300, 300, 5000, dict(npc=2), True),
    "sharded_rows": (60, 40, 300, 300, 5000,
                     dict(allreduce=_identity, n_total=100, row0=40), True),
}

_XT = ("mmb_pc_solve_mc_xt", "caller")  # the transposed branch in one launch
_MC = ("mmb_pc_solve_mc", "caller")
_REMOVE = ("mmb_pc_remove", "caller")
_KEYS = {"mm2_prepare", "pc_solve"}

# (launch sequence, trace keys)
EXPECTED = {
    "narrow_fused": (
        [("mmb_mm2_stream_project_narrow", "caller"), ("mmb_gram", "caller"), _XT, _REMOVE],
        _KEYS | {"mm2_stream_project_narrow", "gram", "pc_remove"}),
    "fused": (
        [("mmb_mm2_stream_project", "caller"), ("mmb_gram", "caller"), _XT, _REMOVE],
        _KEYS | {"mm2_stream_project", "gram", "pc_remove"}),
    "forked_projection": (
        [("mmb_mm2_stream", "caller"),
         ("wait_stream", "s0<-caller"),
         ("mmb_mm2_project_x3_split", "s0"),
         ("mmb_gram", "caller"), _XT, _REMOVE,
         ("wait_stream", "caller<-s0")],
        _KEYS | {"mm2_stream", "mm2_project", "gram", "pc_remove"}),
    "project_remove": (
        [("mmb_mm2_stream", "caller"), ("mmb_gram", "caller"), _XT,
         ("mmb_mm2_project_x3_split", "caller")],
        _KEYS | {"mm2_stream", "gram", "mm2_project+pc_remove"}),
    "separate_remove": (
        [("mmb_mm2_stream", "caller"), ("mmb_mm2_project_x3_split", "caller"),
         ("mmb_gram", "caller"), _XT, _REMOVE],
        _KEYS | {"mm2_stream", "mm2_project+gram", "pc_remove"}),
    "forked_projection_unforked": (
        [("mmb_mm2_stream", "caller"), ("mmb_mm2_project_x3_split", "caller"),
         ("mmb_gram", "caller"), _XT, _REMOVE],
        _KEYS | {"mm2_stream", "mm2_project", "gram", "pc_remove"}),
    "chunks3": (
        [("mmb_mm2_stream", "caller"),
         ("record", "e0@caller"),
         ("wait_stream", "s0<-caller"),
         ("mmb_mm2_stream", "caller"),
         ("record", "e1@caller"),
         ("wait_event", "s0<-e0"),
         ("mmb_mm2_project_x3", "s0"), ("mmb_gram_part", "s0"),
         ("mmb_mm2_stream", "caller"),
         ("wait_event", "s0<-e1"),
         ("mmb_mm2_project_x3", "s0"), ("mmb_gram_part", "s0"),
         ("wait_stream", "caller<-s0"),
         ("mmb_mm2_project_x3", "caller"), ("mmb_gram_part", "caller"),
         ("mmb_gram_finish", "caller"), _MC, _REMOVE, _REMOVE, _REMOVE],
        _KEYS | {"mm2_stream", "mm2_project+gram", "gram_finish", "pc_start", "pc_remove"}),
    "chunks4_side_cus": (
        [("mmb_mm2_stream", "caller"),
         ("record", "e0@caller"),
         ("wait_stream", "s0<-caller"),
         ("wait_stream", "s1<-caller"),
         ("mmb_mm2_stream", "s0"),
         ("record", "e1@s0"),
         ("wait_event", "s1<-e0"),
         ("mmb_mm2_project_x3", "s1"), ("mmb_gram_part", "s1"),
         ("mmb_mm2_stream", "s0"),
         ("record", "e2@s0"),
         ("wait_event", "s1<-e1"),
         ("mmb_mm2_project_x3", "s1"), ("mmb_gram_part", "s1"),
         ("mmb_mm2_stream", "s0"),
         ("wait_event", "s1<-e2"),
         ("mmb_mm2_project_x3", "s1"), ("mmb_gram_part", "s1"),
         ("wait_stream", "caller<-s0"),
         ("wait_stream", "caller<-s1"),
         ("mmb_mm2_project_x3", "caller"), ("mmb_gram_part", "caller"),
         ("mmb_gram_finish", "caller"), _MC, _REMOVE, _REMOVE, _REMOVE, _REMOVE],
        _KEYS | {"mm2_stream", "mm2_project+gram", "gram_finish", "pc_start", "pc_remove"}),
    "split_stream": (
        [("mmb_mm2_stream_split", "caller"),
         ("wait_stream", "s0<-caller"),
         ("mmb_mm2_project_x3_split", "s0"),
         ("mmb_gram", "caller"), _XT, _REMOVE,
         ("wait_stream", "caller<-s0")],
        _KEYS | {"mm2_stream", "mm2_project", "gram", "pc_remove"}),
    "direct_branch": (
        [("mmb_mm2_stream_project", "caller"), ("mmb_gram", "caller"), _MC, _REMOVE],
        _KEYS | {"mm2_stream_project", "gram", "pc_start", "pc_remove"}),
    "npc2": (
        [("mmb_mm2_stream_project", "caller"), ("mmb_gram", "caller"), _XT, _REMOVE],
        _KEYS | {"mm2_stream_project", "gram", "pc_remove"}),
    "sharded_rows": (
        [("mmb_mm2_stream_project", "caller"), ("mmb_gram", "caller"),
         ("mmb_xt_omega", "caller"), _MC, _REMOVE],
        _KEYS | {"mm2_stream_project", "gram", "pc_start", "allreduce", "pc_remove"}),
}


class Recorder:
    """Logs libmmb launches and the step's stream edges around one _run."""

    def __init__(self, step, monkeypatch):
        self.step, self.log, self.labels = step, [], {}
        self.labels[torch.cuda.current_stream().cuda_stream] = "caller"
        call, rec = L.call, self
        wait_stream, wait_event = torch.cuda.Stream.wait_stream, torch.cuda.Stream.wait_event
        record = torch.cuda.Event.record

        def logged_call(name, *args):
            if name != "mmb_host_randn":  # (Omega's host generator on a cache miss: no launch)
                rec.log.append((name, rec.label(torch.cuda.current_stream())))
            return call(name, *args)

        def logged_wait_stream(self, other):
            rec.log.append(("wait_stream", f"{rec.label(self)}<-{rec.label(other)}"))
            return wait_stream(self, other)

        def logged_wait_event(self, ev):
            if rec.event(ev) is not None:  # (not wait_stream's own event)
                rec.log.append(("wait_event", f"{rec.label(self)}<-{rec.event(ev)}"))
            return wait_event(self, ev)

        def logged_record(self, stream=None):
            if rec.event(self) is not None:  # (not the trace's timing events)
                where = stream if stream is not None else torch.cuda.current_stream()
                rec.log.append(("record", f"{rec.event(self)}@{rec.label(where)}"))
            return record(self) if stream is None else record(self, stream)

        monkeypatch.setattr(L, "call", logged_call)
        monkeypatch.setattr(torch.cuda.Stream, "wait_stream", logged_wait_stream)
        monkeypatch.setattr(torch.cuda.Stream, "wait_event", logged_wait_event)
        monkeypatch.setattr(torch.cuda.Event, "record", logged_record)

    def label(self, stream):
        return self.labels.setdefault(stream.cuda_stream, f"s{len(self.labels) - 1}")

    def event(self, ev):
        for i, e in enumerate(self.step._events):
            if e is ev:
                return f"e{i}"
        return None


def record_case(name, dev, monkeypatch):
    n, t, a, vd, V, kw, fork = CASES[name]
    inp = synth.device_workload(n, t, V, A=a, Vd=vd, seed=7, device=dev)
    torch.manual_seed(5)
    gen = models.AudioVisualGeneratorMultimodal(300, a, vd, norm=None).to(dev)
    step = P.FusedStep(inp, gen.networks(), **kw)
    trace = {}
    with monkeypatch.context() as m:
        rec = Recorder(step, m)
        step._run(trace, fork=fork)
    torch.cuda.synchronize()
    step.check()
    return rec.log, set(trace)


@pytest.mark.parametrize("name", list(CASES))
def test_launch_sequence_and_streams(gpu, monkeypatch, name):
    log, keys = record_case(name, gpu, monkeypatch)
    want_log, want_keys = EXPECTED[name]
    assert log == want_log
    assert keys == want_keys


@pytest.mark.parametrize("split", [False, True])
def test_project_rejects_the_same_inputs_split_or_not(gpu, split):
    n = 16
    inp = synth.device_workload(n, 40, 5000, seed=8, device=gpu)
    torch.manual_seed(5)
    gen = models.AudioVisualGeneratorMultimodal(300, 300, 300, norm=None).to(gpu)
    st = P.FusedStep(inp, gen.networks(), stream_project=False, fork_projection=False)
    st.run(check=True)
    ws = P.project_split_ws(n, st.proj.kp, gpu, slices=2) if split else None
    kw = dict(split=ws, slices=2) if split else {}
    pc2 = torch.zeros((2, 300), dtype=torch.float64, device=gpu)
    with pytest.raises(L.MMBError):
        P.mm2_project(st.s, st.x, st.aux, st.proj, pc=pc2, sif_out=torch.empty_like(st.x), **kw)
    with pytest.raises(L.MMBError):
        P.mm2_project(st.s, st.x, st.aux, st.proj, pc=st.pc, **kw)


def test_unsharded_row_offset_takes_its_own_omega_rows(gpu):
    """n_total = 100, row0 = 40 on 60 rows without an all-reduce: the start
    block is X^T Omega over Omega's rows [40, 100), not [0, 60) (the one-launch
    transposed solve reads Omega from row 0, so it is not taken here)."""
    inp = synth.device_workload(60, 40, 5000, seed=9, device=gpu)
    torch.manual_seed(5)
    gen = models.AudioVisualGeneratorMultimodal(300, 300, 300, norm=None).to(gpu)
    st = P.FusedStep(inp, gen.networks(), n_total=100, row0=40)
    st.run(check=True)
    om = P.omega(100, 11, gpu)[40:100].contiguous()
    ref = P.pc_solve(st.G, P.xt_omega(st.x, None, om), 1, True)
    torch.cuda.synchronize()
    assert torch.equal(st.pc, ref)
