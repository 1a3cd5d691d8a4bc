#!/usr/bin/env python3
"""Same-process A/B of the fused stream + projection step on an f32 and on a
16-bit word table, against the two-kernel step such a table takes by default.

Variants, interleaved round by round on one workload (the 16-bit table and
frames are the f32 ones rounded; they live beside them in HBM).  A run takes
one 16-bit kind (--kind bf16 | f16).  A variant is `<table>/<frames>/<front>`:

    f32/f32/fused      the headline: mmb_mm2_stream_project
    16/f32/fused       FusedStep(fused_table16=True): mmb_mm2_stream_project_tt
    16/f32/two-kernel  what a 16-bit table runs without the opt-in:
                       mmb_mm2_stream_tt -> s in HBM -> the projection
    f32/16/fused       FusedStep(fused_frames16=True): mmb_mm2_stream_project_ft
    16/16/fused        both opt-ins: mmb_mm2_stream_project_tt
    16/16/two-kernel   mmb_mm2_stream_tt on 16-bit frames

The opted-in step is to be read against two baselines of the same process: the
two-kernel step on the same 16-bit table, and the f32-table fused step on the
same frames.  Per-phase HIP event times, median and min .. max per variant; for
the front kernel the algorithmic HBM bytes per utterance (DESIGN section 7:
rows read once, outputs written once; cached hot table rows make them
optimistic) and the fraction of the 8 TB/s peak they make.  A difference counts
only where it exceeds both variants' spread.

    python tools/fused_table16_ab.py --kind bf16     # configs[3]: 1M x 40 x 300 / 300 / 300, V = 400k
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-baselines_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import models  # noqa: E402
import pipeline as P  # noqa: E402
import synth  # noqa: E402
from table16_ab import KINDS16, PEAK, TWO_KERNEL, D, frames_to, spread, stream_bytes  # noqa: E402


def front_bytes(step) -> int:
    """Algorithmic HBM bytes per utterance of the step's front kernel: T rows
    of every modality and T ids read; x, aux and -- two-kernel: s, fused: the
    MMB2 row -- written."""
    if step.plan.front == "stream":
        return stream_bytes(step)
    fs = P.FRAME_KINDS[step.frames][0].itemsize
    ts = P.TABLE_KINDS[step.table_kind][0].itemsize
    return step.t * (ts * step.d + fs * (step.a + step.vd) + 4) + 4 * step.d + 12 + 4 * step.d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--T", type=int, default=40)
    ap.add_argument("--A", type=int, default=300)
    ap.add_argument("--Vd", type=int, default=300)
    ap.add_argument("--V", type=int, default=400_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--kind", choices=list(KINDS16), default="bf16")
    args = ap.parse_args()
    k16 = args.kind
    dev = torch.device("cuda", 0)
    inp = synth.device_workload(args.n, args.T, args.V, A=args.A, Vd=args.Vd, seed=4000, device=dev)
    torch.manual_seed(0)
    nets = models.AudioVisualGeneratorMultimodal(D, args.A, args.Vd, norm=None).to(dev).networks()
    tables = {"f32": inp["table"], k16: inp["table"].to(KINDS16[k16])}
    frames = {"f32": inp, k16: frames_to(inp, KINDS16[k16])}
    fused = dict(fused_table16=True, fused_frames16=True)
    variants = [("f32", "f32", "fused", {}), (k16, "f32", "fused", fused), (k16, "f32", "two-kernel", TWO_KERNEL),
                ("f32", k16, "fused", fused), (k16, k16, "fused", fused), (k16, k16, "two-kernel", TWO_KERNEL)]
    steps = {f"{tk}/{fk}/{front}": P.FusedStep(dict(frames[fk], table=tables[tk]), nets, **kw)
             for tk, fk, front, kw in variants}
    print(f"shape: n {args.n} T {args.T} D {D} A {args.A} Vd {args.Vd} V {args.V}; "
          f"HBM in use {torch.cuda.memory_allocated(dev) / 2 ** 30:.1f} GiB", flush=True)
    phase = {}
    for k, st in steps.items():
        st.run()
        torch.cuda.synchronize()
        st.check()
        want = "fused" if k.endswith("/fused") else "stream"
        assert st.plan.front == want and not st.plan.split and (st.s is None) == (want == "fused"), k
        phase[k] = "mm2_stream_project" if want == "fused" else "mm2_stream"
        print(f"step {k}: front {st.plan.front}, projection {st.plan.project}, gram {st.plan.gram}, "
              f"table {st.table_kind}, frames {st.plan.frames}", flush=True)
    # the fused front on a 16-bit table against the two-kernel step on the same inputs (both
    # exact on the table: they differ by the projection's sum order), and what the table's
    # rounding costs against the f32 table
    rel = lambda a, b: ((a.mmb2 - b.mmb2).abs().amax(1) / b.mmb2.abs().amax(1)).max().item()  # noqa: E731
    for fk in ("f32", k16):
        a, b, c = steps[f"{k16}/{fk}/fused"], steps[f"{k16}/{fk}/two-kernel"], steps[f"f32/{fk}/fused"]
        print(f"step {k16}/{fk}/fused: x equal to the two-kernel step's {torch.equal(a.x, b.x)}, MMB2 rows "
              f"{rel(a, b):.2e} row-relative from it, {rel(a, c):.2e} from f32/{fk}/fused (the table's rounding)",
              flush=True)
    res = {k: {} for k in steps}
    for r in range(args.rounds):
        for k, st in steps.items():
            tr = {}
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                st.run(trace=tr)
            e1.record()
            torch.cuda.synchronize()
            res[k].setdefault("step", []).append(e0.elapsed_time(e1) / args.steps)
            for ph, evs in tr.items():
                res[k].setdefault(ph, []).append(sum(x.elapsed_time(y) for x, y in evs) / args.steps)
        print(f"round {r}: " + "  ".join(f"{k} {res[k]['step'][-1]:.3f}" for k in steps) + " ms", flush=True)
    for k in steps:
        print(f"step {k}: " + ", ".join(f"{ph} {statistics.median(v):.3f}" for ph, v in res[k].items()))
    print("\n| table / frames / front | front kernel | ms, median (min .. max) | step ms, median (min .. max) | "
          "KB / utterance | of 8 TB/s |")
    print("|---|---|---|---|---|---|")
    for k, st in steps.items():
        v = res[k][phase[k]]
        b = front_bytes(st)
        frac = b * args.n / (statistics.median(v) * 1e-3) / PEAK
        print(f"| {k} | {phase[k]} | {spread(v)} | {spread(res[k]['step'])} | {b / 1e3:.1f} | {frac:.3f} |")
    # the opted-in step against its two baselines; a difference counts past both spreads
    print("\n| opted-in step | baseline | step ms (median) | difference | both spreads | counts |")
    print("|---|---|---|---|---|---|")
    for fk in ("f32", k16):
        a = f"{k16}/{fk}/fused"
        for b in (f"{k16}/{fk}/two-kernel", f"f32/{fk}/fused"):
            va, vb = res[a]["step"], res[b]["step"]
            diff = statistics.median(va) - statistics.median(vb)
            sa, sb = max(va) - min(va), max(vb) - min(vb)
            print(f"| {a} | {b} | {statistics.median(va):.3f} vs {statistics.median(vb):.3f} | {diff:+.3f} | "
                  f"{sa:.3f}, {sb:.3f} | {'yes' if abs(diff) > max(sa, sb) else 'no'} |")


if __name__ == "__main__":
    main()
