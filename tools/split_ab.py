#!/usr/bin/env python3
"""POM's real splits (g11: 100 x 1089, 203 x 1357 tokens): the stream phase
of the one-workgroup-per-utterance kernel (mmb_mm2_stream) against the split
path (mmb_mm2_stream_split) at several part counts, product library, HIP
events around each launch, median of --reps, alternated rounds.  Prints one
JSON line: ms per variant and the frame-byte rate as a fraction of 8 TB/s.

    python tools/split_ab.py [--reps 30]

--frames16: the split stream on 16-bit frames (mmb_mm2_stream_split_ft)
instead.  Per split and frame type, graph-timed (10 calls per graph, captured
once per variant), replays alternated variant by variant within each round:

    f32_split        the f32 split stream (automatic parts)
    <kind>_one       the 16-bit one-workgroup launch (mmb_mm2_stream_ft): what
                     16-bit frames get without the split
    <kind>_split_u8, <kind>_split_u16
                     the 16-bit split stream at 8 / 16 frames unrolled per
                     thread group (MMB_SPLIT16_UNR, tools build: make diag;
                     the product runs kSplitFU16)
    <kind>_read      a plain read of the 16-bit frame bytes (mmb_probe_read)

Prints median (min .. max) per variant, the frame-byte rate as a fraction of
8 TB/s, and the verdicts by the rule of DESIGN.md §3.1h: faster = the median
lies below the other's by more than the larger min .. max spread of the two.

    python tools/split_ab.py --frames16 [--reps 20] [--rounds 5]

--table16: the split stream on a 16-bit word table (mmb_mm2_stream_split_tt),
product library.  Per split and table type, on f32 frames, graph-timed and
alternated in the same way:

    f32_split        the f32 split stream (automatic parts)
    <kind>_one       the one-workgroup launch on the 16-bit table
                     (mmb_mm2_stream_tt): what such a table gets without the split
    <kind>_split     the split stream on the 16-bit table (automatic parts)

Prints median (min .. max) per variant and the verdicts by the same rule.

    python tools/split_ab.py --table16 [--reps 20] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "multimodal-baselines_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mmb_lib as L  # noqa: E402

# --lib PATH: an A/B clone of the product library (tools/ab_libs), loaded
# explicitly before the mirror modules bind to it
_lib = next((sys.argv[i + 1] for i, a in enumerate(sys.argv[:-1]) if a == "--lib"), None)
if _lib:
    L.load(_lib)
elif "--frames16" in sys.argv:  # the tools build (the unroll knob): explicit, never through the product loader
    L.load(os.path.join(ROOT, "tools", "diag", "libmmb_diag.so"))
import pipeline as P  # noqa: E402
import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--parts", default="0,2,3,4,6,8,12,16")
ap.add_argument("--frames16", action="store_true")
ap.add_argument("--table16", action="store_true")
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()
dev = L.require_gpu()
z = np.load(os.path.join(ROOT, "tests", "golden", "g11_pom_splits.npz"), allow_pickle=False)
splits = [synth.to_device(sp, dev) for sp in
          synth.pom_splits(z["valid_ids"], z["test_ids"], z["weights"], int(z["table_seed"]))]

UNR_KNOB = "MMB_SPLIT16_UNR"  # read per launch (at capture) by the tools build
PEAK = 8e12


def graph_of(call, n=10):
    """`n` calls captured in a graph: the GPU time per call without the host's launch gaps."""
    for _ in range(3):
        call()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g):
            for _ in range(n):
                call()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    return g


def faster(a, b):
    """a faster than b: the median lies below b's by more than the larger min .. max spread of the two."""
    ma, mb = statistics.median(a), statistics.median(b)
    return mb - ma > max(max(a) - min(a), max(b) - min(b))


def frames16_ab():
    kinds = {"bf16": torch.bfloat16, "f16": torch.float16}
    read_blocks = 1024
    sink = torch.zeros(read_blocks, dtype=torch.int32, device=dev)  # a word per block of the probe
    for si, inp in enumerate(splits):
        # every tensor a captured graph reads stays referenced while the graph is replayed: a graph holds
        # bare pointers, and the next capture empties the allocator's cache (torch.cuda.graph), which
        # unmaps whatever was freed in between
        keep = []
        n, t = inp["ids"].shape
        ws = P.split_ws(n, t, 300, 300, 300, dev)
        text = dict(table=inp["table"], wtab32=inp["wtab"])
        mk = lambda: (torch.empty((n, 300), device=dev),  # noqa: E731
                      P.s_buffer(n, P.mm2_dims(300, 300, 300)[0], True, dev), torch.empty((3, n), device=dev))
        graphs, outs = {}, {}
        outs["f32_split"] = mk()
        graphs["f32_split"] = graph_of(lambda: P.mm2_stream(n, t, 300, 300, 300, inp["audio"], inp["visual"],
                                                            ids32=inp["ids"], out=outs["f32_split"], split=ws,
                                                            **text))
        frame_bytes = {"f32_split": 2 * n * t * 300 * 4}
        for kind, dt in kinds.items():
            a16, v16 = inp["audio"].to(dt), inp["visual"].to(dt)
            keep += [a16, v16]
            os.environ.pop(UNR_KNOB, None)
            outs[f"{kind}_one"] = mk()
            graphs[f"{kind}_one"] = graph_of(lambda: P.mm2_stream(n, t, 300, 300, 300, a16, v16, ids32=inp["ids"],
                                                                  out=outs[f"{kind}_one"], **text))
            for u in (8, 16):
                os.environ[UNR_KNOB] = str(u)
                k = f"{kind}_split_u{u}"
                outs[k] = mk()
                graphs[k] = graph_of(lambda: P.mm2_stream_split_ft(n, t, 300, 300, 300, a16, v16, inp["ids"],
                                                                   out=outs[k], split=ws, **text))
            os.environ.pop(UNR_KNOB, None)

            def read(a16=a16, v16=v16):
                for buf in (a16, v16):
                    L.call("mmb_probe_read", L.ptr(buf), buf.numel() * 2 // 16 * 16, read_blocks, 1, L.ptr(sink),
                           L.stream_ptr())
            graphs[f"{kind}_read"] = graph_of(read)
            for k in (f"{kind}_one", f"{kind}_split_u8", f"{kind}_split_u16", f"{kind}_read"):
                frame_bytes[k] = 2 * n * t * 300 * 2
            # the unroll changes no sum, and the 16-bit split stream is the f32 one on the upcast frames
            for x8, x16 in zip(outs[f"{kind}_split_u8"], outs[f"{kind}_split_u16"]):
                assert torch.equal(x8, x16), (kind, "unroll")
            twin = P.mm2_stream(n, t, 300, 300, 300, a16.float(), v16.float(), ids32=inp["ids"], split=ws, **text)
            torch.cuda.synchronize()
            for x8, x32 in zip(outs[f"{kind}_split_u8"], twin):
                assert torch.equal(x8, x32), (kind, "twin")
        res = {k: [] for k in graphs}
        for _ in range(args.rounds):
            for _ in range(args.reps):
                for k, g in graphs.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    g.replay()
                    b.record()
                    b.synchronize()
                    res[k].append(a.elapsed_time(b) / 10 * 1e3)
        print(f"split{si}: {n} x {t}, automatic parts {P.split_parts(n, t)}; us per call, median (min .. max), "
              f"frame bytes / 8 TB/s", flush=True)
        for k, v in res.items():
            med = statistics.median(v)
            print(f"  {k:16s} {med:7.1f} ({min(v):.1f} .. {max(v):.1f})  {frame_bytes[k] / (med * 1e-6) / PEAK:.3f}")
        for kind in kinds:
            c8, c16 = res[f"{kind}_split_u8"], res[f"{kind}_split_u16"]
            for u, c in ((8, c8), (16, c16)):
                print(f"  {kind} split u{u}: faster than one-workgroup {faster(c, res[f'{kind}_one'])}, than the f32 "
                      f"split {faster(c, res['f32_split'])}; / read "
                      f"{statistics.median(c) / statistics.median(res[f'{kind}_read']):.2f}")
            print(f"  {kind}: u16 faster than u8 {faster(c16, c8)}, u8 faster than u16 {faster(c8, c16)}", flush=True)


def table16_ab():
    kinds = {"bf16": torch.bfloat16, "f16": torch.float16}
    for si, inp in enumerate(splits):
        keep = []  # (every tensor a captured graph reads stays referenced: see frames16_ab)
        n, t = inp["ids"].shape
        ws = P.split_ws(n, t, 300, 300, 300, dev)
        mk = lambda: (torch.empty((n, 300), device=dev),  # noqa: E731
                      P.s_buffer(n, P.mm2_dims(300, 300, 300)[0], True, dev), torch.empty((3, n), device=dev))
        au, vi, ids, wtab = inp["audio"], inp["visual"], inp["ids"], inp["wtab"]
        graphs, outs = {}, {}
        outs["f32_split"] = mk()
        graphs["f32_split"] = graph_of(lambda: P.mm2_stream(n, t, 300, 300, 300, au, vi, ids32=ids, table=inp["table"],
                                                            wtab32=wtab, out=outs["f32_split"], split=ws))
        for kind, dt in kinds.items():
            E16 = inp["table"].to(dt)
            keep.append(E16)
            outs[f"{kind}_one"] = mk()
            graphs[f"{kind}_one"] = graph_of(lambda: P.mm2_stream(n, t, 300, 300, 300, au, vi, ids32=ids, table=E16,
                                                                  wtab32=wtab, out=outs[f"{kind}_one"]))
            outs[f"{kind}_split"] = mk()
            graphs[f"{kind}_split"] = graph_of(lambda: P.mm2_stream_split_tt(n, t, 300, 300, 300, au, vi, ids, E16,
                                                                             wtab32=wtab, out=outs[f"{kind}_split"],
                                                                             split=ws))
            # the 16-bit split stream is the f32 one on the upcast table
            twin = P.mm2_stream(n, t, 300, 300, 300, au, vi, ids32=ids, table=E16.float(), wtab32=wtab, split=ws)
            torch.cuda.synchronize()
            for x16, x32 in zip(outs[f"{kind}_split"], twin):
                assert torch.equal(x16, x32), (kind, "twin")
        res = {k: [] for k in graphs}
        for _ in range(args.rounds):
            for _ in range(args.reps):
                for k, g in graphs.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    g.replay()
                    b.record()
                    b.synchronize()
                    res[k].append(a.elapsed_time(b) / 10 * 1e3)
        print(f"split{si}: {n} x {t}, automatic parts {P.split_parts(n, t)}; f32 frames; us per call, "
              f"median (min .. max)", flush=True)
        for k, v in res.items():
            print(f"  {k:16s} {statistics.median(v):7.1f} ({min(v):.1f} .. {max(v):.1f})")
        for kind in kinds:
            c = res[f"{kind}_split"]
            print(f"  {kind} split: faster than one-workgroup {faster(c, res[f'{kind}_one'])}, than the f32 split "
                  f"{faster(c, res['f32_split'])}; the f32 split faster than it {faster(res['f32_split'], c)}",
                  flush=True)


if args.frames16:
    frames16_ab()
    sys.exit(0)
if args.table16:
    table16_ab()
    sys.exit(0)
variants = ["one"] + [f"p{p}" for p in args.parts.split(",")]
res = {}
for r in range(3):
    for si, inp in enumerate(splits):
        n, t = inp["ids"].shape
        ws = P.split_ws(n, t, 300, 300, 300, dev, parts=16)
        out = (torch.empty((n, 300), device=dev), P.s_buffer(n, P.mm2_dims(300, 300, 300)[0], True, dev),
               torch.empty((3, n), device=dev))
        for v in variants:
            kw = {} if v == "one" else dict(split=ws, parts=int(v[1:]))
            call = lambda: P.mm2_stream(n, t, 300, 300, 300, inp["audio"], inp["visual"],
                                        ids32=inp["ids"], table=inp["table"], wtab32=inp["wtab"],
                                        out=out, **kw)
            for _ in range(3):
                call()
            # 10 calls captured in a graph: the GPU time per call without
            # the host's launch gaps (two ctypes launches per call)
            g = torch.cuda.CUDAGraph()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                with torch.cuda.graph(g):
                    for _ in range(10):
                        call()
            torch.cuda.synchronize()
            g.replay()
            for _ in range(args.reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                g.replay()
                b.record()
                b.synchronize()
                res.setdefault(f"split{si}_{v}", []).append(a.elapsed_time(b) / 10)
# the read ceiling at these sizes: mmb_probe_read over the split's audio and
# visual buffers (one launch each, nt loads), graph-timed like the variants
sink = torch.zeros(4096, dtype=torch.int32, device=dev)  # a word per block of the probe
for si, inp in enumerate(splits):
    for blocks in (512, 1024, 2048, 4096):
        def call(inp=inp, blocks=blocks):
            for buf in (inp["audio"], inp["visual"]):
                L.call("mmb_probe_read", L.ptr(buf), buf.numel() * 4, blocks, 1, L.ptr(sink),
                       L.stream_ptr())
        call()
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(g):
                for _ in range(10):
                    call()
        torch.cuda.synchronize()
        g.replay()
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            b.synchronize()
            res.setdefault(f"split{si}_read{blocks}", []).append(a.elapsed_time(b) / 10)
    variants_read = [f"read{b}" for b in (512, 1024, 2048, 4096)]
summary = {"auto_parts": [P.split_parts(*inp["ids"].shape) for inp in splits]}
variants = variants + variants_read
for si, inp in enumerate(splits):
    n, t = inp["ids"].shape
    frame_b = 2 * n * t * 300 * 4
    for v in variants:
        ms = statistics.median(res[f"split{si}_{v}"])
        summary[f"split{si}_{v}_ms"] = round(ms, 4)
        summary[f"split{si}_{v}_frac_frames"] = round(frame_b / (ms * 1e-3) / 8e12, 3)
print(json.dumps(summary), flush=True)
