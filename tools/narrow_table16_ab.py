#!/usr/bin/env python3
"""Same-process A/B of the narrow fused step (MOSI's widths) on an f32 and on a
16-bit word table, against the two-kernel step such a table takes by default.

Variants, interleaved round by round on one workload (the 16-bit tables are
the f32 one rounded; all three live side by side in HBM).  A variant is
`<table>/<front>`, on f32 frames:

    f32/narrow_fused    mmb_mm2_stream_project_narrow
    <kind>/narrow_fused FusedStep(narrow_table16=True): mmb_mm2_stream_project_narrow_tt
                        (the f32 step's kernel on a text cache of the same bytes)
    <kind>/two-kernel   what a 16-bit table runs without the opt-in:
                        mmb_mm2_stream_tt -> s in HBM -> the projection

for both 16-bit kinds.  The opted-in step is to be read against two baselines
of the same process: the two-kernel step on the same 16-bit table, and the
f32-table narrow fused step.  Step times by HIP events, median and min .. max
per variant; a difference counts only where it exceeds both variants' spread.

    python tools/narrow_table16_ab.py     # configs[1]: 1M x 20 x 300 / 76 / 48, V = 3016
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
from table16_ab import KINDS16, TWO_KERNEL, D, spread  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--T", type=int, default=20)
    ap.add_argument("--A", type=int, default=76)
    ap.add_argument("--Vd", type=int, default=48)
    ap.add_argument("--V", type=int, default=3016)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    inp = synth.device_workload(args.n, args.T, args.V, A=args.A, Vd=args.Vd, seed=4000, device=dev)
    torch.manual_seed(0)
    nets = models.AudioVisualGeneratorMultimodal(D, args.A, args.Vd, norm=None).to(dev).networks()
    steps = {"f32/narrow_fused": P.FusedStep(inp, nets)}
    for k16, dt in KINDS16.items():
        inp16 = dict(inp, table=inp["table"].to(dt))
        steps[f"{k16}/narrow_fused"] = P.FusedStep(inp16, nets, narrow_table16=True)
        steps[f"{k16}/two-kernel"] = P.FusedStep(inp16, nets, **TWO_KERNEL)
    print(f"shape: n {args.n} T {args.T} D {D} A {args.A} Vd {args.Vd} V {args.V}; "
          f"HBM in use {torch.cuda.memory_allocated(dev) / 2 ** 30:.1f} GiB", flush=True)
    for k, st in steps.items():
        st.run()
        torch.cuda.synchronize()
        st.check()
        want = "narrow_fused" if k.endswith("/narrow_fused") else "stream"
        assert st.plan.front == want and not st.plan.split and (st.s is None) == (want == "narrow_fused"), k
        print(f"step {k}: front {st.plan.front}, projection {st.plan.project}, gram {st.plan.gram}, "
              f"table {st.table_kind}, frames {st.plan.frames}", flush=True)
    for k16 in KINDS16:
        a, b = steps[f"{k16}/narrow_fused"], steps[f"{k16}/two-kernel"]
        # the plan without the opt-in is the two-kernel plan
        assert P.FusedStep(dict(inp, table=a.table), nets).plan == b.plan
        rel = ((a.mmb2 - b.mmb2).abs().amax(1) / b.mmb2.abs().amax(1)).max().item()
        print(f"step {k16}/narrow_fused: MMB2 rows {rel:.2e} row-relative from the two-kernel step's", flush=True)
    res = {k: [] for k in steps}
    for r in range(args.rounds):
        for k, st in steps.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                st.run()
            e1.record()
            torch.cuda.synchronize()
            res[k].append(e0.elapsed_time(e1) / args.steps)
        print(f"round {r}: " + "  ".join(f"{k} {res[k][-1]:.3f}" for k in steps) + " ms", flush=True)
    print("\n| table / front | step ms, median (min .. max) |")
    print("|---|---|")
    for k in steps:
        print(f"| {k} | {spread(res[k])} |")
    # the opted-in step against its two baselines; a difference counts past both spreads
    print("\n| opted-in step | baseline | step ms (median) | difference | both spreads | counts |")
    print("|---|---|---|---|---|---|")
    for k16 in KINDS16:
        a = f"{k16}/narrow_fused"
        for b in (f"{k16}/two-kernel", "f32/narrow_fused"):
            va, vb = res[a], res[b]
            diff = statistics.median(va) - statistics.median(vb)
            sa, sb = max(va) - min(va), max(vb) - min(vb)
            print(f"| {a} | {b} | {statistics.median(va):.3f} vs {statistics.median(vb):.3f} | {diff:+.3f} | "
                  f"{sa:.3f}, {sb:.3f} | {'yes' if abs(diff) > max(sa, sb) else 'no'} |")


if __name__ == "__main__":
    main()
