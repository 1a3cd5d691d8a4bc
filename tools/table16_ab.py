#!/usr/bin/env python3
"""Same-process A/B of the SIF gather and of the two-kernel step on an f32 and
on a 16-bit word table.

Variants, interleaved round by round on one workload (the 16-bit tables and
frames are the f32 ones rounded; they live beside them in HBM).  A run takes
one 16-bit kind (--kind bf16 | f16).  A variant is `<table>/<frames>`: the
word table f32 or of the kind, each with f32 frames and with frames of the
kind:

    sif  <table>            the text-only SIF gather (weighted_sum: mmb_sif_wavg,
                            mmb_sif_wavg_tt), num and cnt written
    step <table>/<frames>   the two-kernel step (stream kernel -> s in HBM ->
                            projection; FusedStep with the fused fronts and the
                            split stream off, which is the only plan a 16-bit
                            table has): mmb_mm2_stream, mmb_mm2_stream_ft,
                            mmb_mm2_stream_tt

Every 16-bit variant is measured against the f32-table variant of the same
kernel in the same process.  Per-phase HIP event times, median and min .. max
per variant; for the gather and for the stream kernel the algorithmic HBM
bytes per utterance (rows read once, outputs written once; cached
hot table rows make them optimistic) and the fraction of the 8 TB/s peak they
make.

    python tools/table16_ab.py --kind bf16                       # configs[3]: 1M x 40 x 300 / 300 / 300, V = 400k
    python tools/table16_ab.py --kind f16 --T 20 --A 76 --Vd 48 --V 3016    # the MOSI shape
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-baselines_amd"))

import torch  # noqa: E402

import models  # noqa: E402
import pipeline as P  # noqa: E402
import synth  # noqa: E402

PEAK = 8.0e12  # HBM bytes / s
D = 300
TWO_KERNEL = dict(stream_project=False, narrow_fused=False, split_stream=False)
KINDS16 = {"bf16": torch.bfloat16, "f16": torch.float16}


def stream_bytes(step) -> int:
    """Algorithmic HBM bytes per utterance of the step's stream kernel: T rows
    of every modality and T ids read; x, aux and s written."""
    fs = P.FRAME_KINDS[step.frames][0].itemsize
    ts = P.TABLE_KINDS[step.table_kind][0].itemsize
    read = step.t * (ts * step.d + fs * (step.a + step.vd) + 4)
    return read + 4 * step.d + 12 + 4 * step.proj.kp


def sif_bytes(table, l: int) -> int:
    """The same of the SIF gather: l table rows and ids read, num and cnt written."""
    d = table.shape[1]
    return l * (table.element_size() * d + 4) + 4 * d + 4


def frames_to(inp: dict, dtype, rows: int = 1 << 16) -> dict:
    """`inp` with its frames rounded to `dtype`, converted in row chunks."""
    out = dict(inp)
    for key in ("audio", "visual"):
        src = inp[key]
        dst = torch.empty(src.shape, dtype=dtype, device=src.device)
        for r in range(0, src.shape[0], rows):
            dst[r:r + rows] = src[r:r + rows]
        out[key] = dst
    return out


def spread(v):
    return f"{statistics.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--T", type=int, default=40)
    ap.add_argument("--A", type=int, default=300)
    ap.add_argument("--Vd", type=int, default=300)
    ap.add_argument("--V", type=int, default=400_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--kind", choices=list(KINDS16), default="bf16")
    args = ap.parse_args()
    KINDS = {"f32": torch.float32, args.kind: KINDS16[args.kind]}
    dev = torch.device("cuda", 0)
    inp = synth.device_workload(args.n, args.T, args.V, A=args.A, Vd=args.Vd, seed=4000, device=dev)
    torch.manual_seed(0)
    nets = models.AudioVisualGeneratorMultimodal(D, args.A, args.Vd, norm=None).to(dev).networks()
    tables = {k: inp["table"].to(dt) for k, dt in KINDS.items()}
    frames = {"f32": inp, args.kind: frames_to(inp, KINDS16[args.kind])}
    steps = {f"{tk}/{fk}": P.FusedStep(dict(frames[fk], table=tables[tk]), nets, **TWO_KERNEL)
             for tk in KINDS for fk in KINDS}
    print(f"shape: n {args.n} T {args.T} D {D} A {args.A} Vd {args.Vd} V {args.V}; "
          f"HBM in use {torch.cuda.memory_allocated(dev) / 2 ** 30:.1f} GiB", flush=True)
    for k, st in steps.items():
        st.run()
        torch.cuda.synchronize()
        st.check()
        assert st.plan.front == "stream" and not st.plan.split, k
        print(f"step {k}: front {st.plan.front}, projection {st.plan.project}, gram {st.plan.gram}, "
              f"table {st.table_kind}, frames {st.plan.frames}", flush=True)
    # what the table's rounding costs here: the 16-bit steps' rows against the f32 table's on the same frames
    for k, st in steps.items():
        tk, fk = k.split("/")
        if tk != "f32":
            ref = steps[f"f32/{fk}"]
            rel = ((st.mmb2 - ref.mmb2).abs().amax(1) / ref.mmb2.abs().amax(1)).max().item()
            print(f"step {k}: MMB2 rows move by {rel:.2e} row-relative against f32/{fk} (the table's rounding)",
                  flush=True)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)

    def gather(tk):
        return P.weighted_sum(tables[tk], inp["ids"], wtab32=inp["wtab"], flag=flag)

    for tk in KINDS:
        gather(tk)
    torch.cuda.synchronize()
    res = {k: {} for k in steps}
    sif = {tk: [] for tk in KINDS}
    for r in range(args.rounds):
        for tk in KINDS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                gather(tk)
            e1.record()
            torch.cuda.synchronize()
            sif[tk].append(e0.elapsed_time(e1) / args.steps)
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
        print(f"round {r}: " + "  ".join(f"sif {tk} {sif[tk][-1]:.3f}" for tk in KINDS) + "  "
              + "  ".join(f"{k} {res[k]['step'][-1]:.3f}" for k in steps) + " ms", flush=True)
    for k in steps:
        print(f"step {k}: " + ", ".join(f"{ph} {statistics.median(v):.3f}" for ph, v in res[k].items()))
    print("\n| variant | kernel | ms, median (min .. max) | step ms, median (min .. max) | KB / utterance | "
          "of 8 TB/s | against the f32 table |")
    print("|---|---|---|---|---|---|---|")
    for tk in KINDS:
        b = sif_bytes(tables[tk], args.T)
        ms = statistics.median(sif[tk])
        frac = b * args.n / (ms * 1e-3) / PEAK
        print(f"| sif {tk} | mmb_sif_wavg{'' if tk == 'f32' else '_tt'} | {spread(sif[tk])} | | {b / 1e3:.1f} | "
              f"{frac:.3f} | {ms / statistics.median(sif['f32']):.3f} |")
    for k, st in steps.items():
        tk, fk = k.split("/")
        v = res[k]["mm2_stream"]
        ms = statistics.median(v)
        b = stream_bytes(st)
        frac = b * args.n / (ms * 1e-3) / PEAK
        rel = f"{ms / statistics.median(res[f'f32/{fk}']['mm2_stream']):.3f}"
        print(f"| step {k} | mm2_stream | {spread(v)} | {spread(res[k]['step'])} | {b / 1e3:.1f} | {frac:.3f} | "
              f"{rel} |")


if __name__ == "__main__":
    main()
