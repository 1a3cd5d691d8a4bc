"""GPU: every kernel family on an operand past 2^31 and 2^32 bytes.

The suite pins the kernels at their smallest shapes; byte and element offsets
that no longer fit in 32 bits cannot show there.  tests/large_cases.py fixes,
per family, the smallest shape at which one operand passes 2^32 bytes (its
widest legal row, the fewest rows); tests/test_large_cases.py (CPU) pins the
size facts.  Here each case fills its inputs on the device, launches the entry
point once on the whole operand, and compares

  per-row kernels   a sample of at most 64 rows -- row 0, the last row, the
                    rows around 2^31 and 2^32 bytes of every large operand, a
                    seeded remainder -- with f64 numpy of the same operation on
                    those rows' inputs copied to the host; gathered tables
                    through ids set by hand to the table's boundary rows;
  reductions        an operand that is zero but for planted seeded rows in all
                    three regions, with the exact f64 result of those rows.

No new tolerance: every comparison uses the bar the suite holds the same
kernel to at small shapes (mmb2_cases.sum_bar / stream_reference /
project_reference, gauss_cases' bars, 2e-6 for the weighted average, 1e-13 /
2e-9 for the Grams, 2^-23 / 1e-12 for the removals), imported from where it
is defined.  Where the route does not depend on N the same entry point also
runs on a compact copy of the sampled rows and must give identical bits.

A case skips only when the device has less free memory than its buffers plus
2 GiB.  Only the product library is loaded.
"""
import numpy as np
import pytest
import torch

import gauss_cases as G
import gauss_gpu as GG       # within(): gauss_cases' bars, entry by entry
import large_cases as LC
import latent as LT
import mmb2_cases as C
import mmb2_gpu as MG        # _check_stream / _dequant: the stream outputs against mmb2_cases' bars
import mmb_lib as L
import pipeline as P
import regressor_cases as RC
import regressor_gpu as RG   # _check (regressor_cases' bounds, doubled), _launch_train
import width_cases as W
import widths_gpu as WG      # _check_gram, _check_gram_i8
import word_cases as WC      # lp_ratio, grad_ratio
from common_gpu import F32_ROW, TOL, Ledger, _dev, _flag, _frac, _networks, _unnoted
from large_gpu import _gen, _host_upcast, _projection, _rand, _randn, _stream_inputs, _weights, _word_table
from oracle import mmb2_oracle as M
from oracle import regressor_oracle as R

pytestmark = pytest.mark.gpu

_WORST = Ledger()  # (case name, what) -> [comparisons, largest error as a fraction of its bar]


def _note(case, what, frac):
    return _WORST.note((case.name, what), frac)


def _noter(case):
    """The `note` handed to a shared checker, (group, what, fraction) or (group,
    what, error, bar): recorded under the case, as a fraction of the bar."""
    def note(group, what, value, bar=None):
        _note(case, what if bar is None else f"{what} (of {bar:g})", value if bar is None else value / bar)
        return float(value)
    return note


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    by_case = {}
    for (name, what), (_, frac) in _WORST.items():
        by_case.setdefault(name, {})[what] = frac
    for name, w in by_case.items():
        c = LC.CASES[name]
        op = c.op(c.crossing)
        print(f"\nlarge {name}: {c.crossing} {op.rows} x {op.row_bytes} B = {op.nbytes} B; " +
              ", ".join(f"{k} {v:.3g} of its bar" for k, v in sorted(w.items())), end="")
    print()


@pytest.fixture(autouse=True)
def _clean():
    torch.cuda.empty_cache()
    yield
    torch.cuda.empty_cache()


def _case(name, gpu):
    """The case, after the one check that may skip it: free device memory."""
    c = LC.CASES[name]
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(gpu)
    if free < c.total_bytes + 2 * LC.GIB:
        pytest.skip(f"{name} needs {c.total_bytes} bytes + 2 GiB; {free} are free")
    return c


def _assert_sampled(c, rows):
    assert len(rows) <= LC.MAX_SAMPLE and rows[0] == 0 and rows[-1] == c.n - 1


# ------------------------------------------------------------------ 1, 2, 4: the stream kernels
def _stream_check(c, inp, out, rows, s_half, gpu, flag):
    """x, s and aux of the sampled rows against mmb2_cases.stream_reference of
    those rows' inputs (mmb2_gpu._check_stream: sum_bar)."""
    z = c.dims
    num, s, aux = out
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    ridx = torch.as_tensor(rows, device=gpu)
    ids = inp["ids"][ridx].long()
    text = _host_upcast(inp["table"][ids])          # [k, t, d] gathered on the device: the rows the kernel read
    sw = _host_upcast(inp["wtab"][ids])
    ref = C.stream_reference(text, text, sw, _host_upcast(inp["audio"][ridx]), _host_upcast(inp["visual"][ridx]))
    got = (num[ridx].cpu().numpy(), s[ridx].cpu().numpy(), aux[:, ridx].cpu().numpy(), None)
    small = (z["d"], z["a"], z["vd"], z["t"], len(rows), z["v"])
    frac = MG._check_stream(_noter(c), 0, small, got, ref, s_half)
    _note(c, "stream outputs", frac)
    print(f"{c.name}: {len(rows)} rows, largest error {frac:.3f} of its bar (mmb2_cases.sum_bar)")
    return frac


@pytest.mark.parametrize("name", LC.names(family=1) + LC.names(family=2))
def test_stream_frames_and_outputs(gpu, name):
    """The wave kernel (its narrow-frame route at s_half with D = 512) and the
    workgroup kernel (T = 65) with audio / visual / x and s past 2^32 bytes."""
    c = _case(name, gpu)
    z = c.dims
    inp = _stream_inputs(c, gpu)
    assert c.op(c.crossing).past32
    for key in ("audio", "visual"):
        assert inp[key].numel() * inp[key].element_size() == c.op(key).nbytes
    flag = _flag(gpu)
    s_half = bool(z["s_half"])
    out = P.mm2_stream(z["n"], z["t"], z["d"], z["a"], z["vd"], inp["audio"], inp["visual"], ids32=inp["ids"],
                       table=inp["table"], wtab32=inp["wtab"], flag=flag, s_half=s_half)
    assert out[0].numel() * 4 == c.op("x").nbytes and out[1].numel() * out[1].element_size() == c.op("s").nbytes
    rows = LC.sample_rows(c)
    _assert_sampled(c, rows)
    _stream_check(c, inp, out, rows, s_half, gpu, flag)


@pytest.mark.parametrize("name", LC.names(family=4))
def test_word_table(gpu, name):
    """A [V, 512] word table at 2^31 - 2048 bytes (the last the narrow-frame
    kernel's guard accepts), at 2^31 (the first it refuses: the wave kernel),
    past 2^32, and a bf16 one past 2^32: ids set by hand to the table's first,
    boundary and last rows."""
    c = _case(name, gpu)
    z = c.dims
    g = _gen(c, gpu)
    dtype = torch.float32 if z["tbytes"] == 4 else torch.bfloat16
    table = _word_table(z["v"], z["d"], g, gpu, dtype)
    assert table.numel() * table.element_size() == c.op("table").nbytes
    ids_h = LC.gather_ids(c, z["n"], z["t"])
    assert set(LC.table_rows(c)) <= set(ids_h.ravel()) and ids_h.max() == z["v"] - 1
    inp = _stream_inputs(c, gpu, table=table, ids=_dev(ids_h, gpu, torch.int32))
    rows = np.arange(z["n"])
    for s_half in (True, False):  # True with ids + wtab at D = 512, A = Vd = 4: the narrow-frame route where it is allowed
        flag = _flag(gpu)
        out = P.mm2_stream(z["n"], z["t"], z["d"], z["a"], z["vd"], inp["audio"], inp["visual"],
                           ids32=inp["ids"], table=table, wtab32=inp["wtab"], flag=flag, s_half=s_half)
        _stream_check(c, inp, out, rows, s_half, gpu, flag)


# ------------------------------------------------------------------ 3: the split stream
@pytest.mark.parametrize("name", LC.names(family=3))
def test_split_stream(gpu, name):
    """A few POM-length rows (T = 1357, A = 300: 1.6 MB of f32 audio per row)
    past 2^32 bytes, on the automatic plan (fp16 s) and on two ranges per row
    (fp32 s); the same through mmb_mm2_stream_split_ft on fp16 frames."""
    c = _case(name, gpu)
    z = c.dims
    inp = _stream_inputs(c, gpu)
    assert inp["audio"].numel() * inp["audio"].element_size() == c.op("audio").nbytes > LC.B32
    rows = LC.sample_rows(c)
    _assert_sampled(c, rows)
    dims = (z["n"], z["t"], z["d"], z["a"], z["vd"])
    for parts, s_half in zip(z["parts"], (True, False)):
        ws = P.split_ws(*dims, gpu, parts=parts)
        assert ws.numel() <= c.op("split_ws").nbytes
        flag = _flag(gpu)
        if z["frames"] == "f32":
            out = P.mm2_stream(*dims, inp["audio"], inp["visual"], ids32=inp["ids"], table=inp["table"],
                               wtab32=inp["wtab"], flag=flag, s_half=s_half, split=ws, parts=parts)
        else:
            out = P.mm2_stream_split_ft(*dims, inp["audio"], inp["visual"], inp["ids"], inp["table"],
                                        wtab32=inp["wtab"], flag=flag, s_half=s_half, split=ws, parts=parts)
        _stream_check(c, inp, out, rows, s_half, gpu, flag)


# ------------------------------------------------------------------ 5, 6: the fused kernels
def _fused_check(c, inp, out, rows, gpu, flag, what="MMB2 rows"):
    """x, count and weight sum of the sampled rows against
    mmb2_cases.stream_reference (sum_bar), their MMB2 rows against the oracle
    on those rows' inputs (1e-5 row-relative)."""
    z = c.dims
    x, aux, mmb2 = out
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    ridx = torch.as_tensor(rows, device=gpu)
    ids = inp["ids"][ridx].long()
    text, sw = _host_upcast(inp["table"][ids]), _host_upcast(inp["wtab"][ids])
    audio, visual = _host_upcast(inp["audio"][ridx]), _host_upcast(inp["visual"][ridx])
    ref = C.stream_reference(text, text, sw, audio, visual)
    a = aux[:, ridx].cpu().numpy()
    assert np.array_equal(a[0], ref["cnt"])
    fx = _note(c, "x", _frac(np.abs(x[ridx].cpu().numpy() - ref["x"]), C.sum_bar(z["t"], ref["x_abs"])))
    fw = _note(c, "weight sum", _frac(np.abs(a[1] - ref["sw"]), C.sum_bar(z["t"], ref["sw_abs"])))
    oracle = M.estimate_embedding_overall_gpu2(M.concat_inputs(text, audio, visual),
                                               C.params(z["d"], z["a"], z["vd"]), sw, text)
    got = mmb2[ridx].cpu().numpy()
    assert np.isfinite(got).all()
    fo = _note(c, what + " (of 1e-5)", M.row_rel_err(got, oracle) / TOL)
    print(f"{c.name}: {len(rows)} rows, x {fx:.3f} and weight sum {fw:.3f} of sum_bar, {what} {fo:.3f} of 1e-5")
    assert fx <= 1.0 and fw <= 1.0 and fo < 1.0


@pytest.mark.parametrize("name", ["fused_visual", "fused_audio", "fused_ft_f16_visual"])
def test_fused(gpu, name):
    """mmb_mm2_stream_project with visual / audio rows past 2^32 bytes (f32),
    and _ft with fp16 visual rows past 2^32 (52,429 and 104,858 rows: below the
    dynamic batch order's threshold)."""
    c = _case(name, gpu)
    z = c.dims
    dims = (z["n"], z["t"], z["d"], z["a"], z["vd"])
    assert P.stream_project_supported(*dims[1:])
    inp = _stream_inputs(c, gpu)
    assert inp[c.crossing].numel() * inp[c.crossing].element_size() == c.op(c.crossing).nbytes > LC.B32
    flag = _flag(gpu)
    fn = P.mm2_stream_project if z["frames"] == "f32" else P.mm2_stream_project_ft
    out = fn(*dims, inp["audio"], inp["visual"], _projection(c, gpu), ids32=inp["ids"], table=inp["table"],
             wtab32=inp["wtab"], flag=flag)
    rows = LC.sample_rows(c)
    _assert_sampled(c, rows)
    _fused_check(c, inp, out, rows, gpu, flag)


def test_fused_table_guard(gpu):
    """fused_pipe_ok: a [2^21 - 1, 256] table (2^31 - 1024 bytes) takes the
    pipelined streamer, a [2^21, 256] one (2^31 bytes) the group-at-a-time
    fallback.  The first table is the second one's rows but the last, and the
    ids reach its top rows, so the two launches gather the same rows: identical
    bits (the relation tests/test_gpu_variants.py holds the two streamers to),
    and the oracle's rows.  Then the larger table's own last row."""
    last, c = LC.CASES["fused_table_last"], _case("fused_table_refused", gpu)
    z = c.dims
    dims = (z["n"], z["t"], z["d"], z["a"], z["vd"])
    assert P.stream_project_supported(*dims[1:]) and z["t"] >= 21
    table = _word_table(z["v"], z["d"], _gen(c, gpu), gpu)
    assert table.numel() * 4 == LC.B31 and last.dims["v"] == z["v"] - 1
    ids_small = LC.gather_ids(last, z["n"], z["t"])
    assert ids_small.max() == z["v"] - 2
    inp = _stream_inputs(c, gpu, table=table, ids=_dev(ids_small, gpu, torch.int32))
    proj = _projection(c, gpu)
    rows = np.arange(z["n"])
    outs = []
    for v in (z["v"] - 1, z["v"]):
        flag = _flag(gpu)
        out = P.mm2_stream_project(*dims, inp["audio"], inp["visual"], proj, ids32=inp["ids"], table=table[:v],
                                   wtab32=inp["wtab"][:v], flag=flag)
        _fused_check(LC.CASES["fused_table_last"] if v < z["v"] else c, inp, out, rows, gpu, flag)
        outs.append(out)
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    inp["ids"] = _dev(LC.gather_ids(c, z["n"], z["t"]), gpu, torch.int32)
    assert int(inp["ids"].max()) == z["v"] - 1
    flag = _flag(gpu)
    out = P.mm2_stream_project(*dims, inp["audio"], inp["visual"], proj, ids32=inp["ids"], table=table,
                               wtab32=inp["wtab"], flag=flag)
    _fused_check(c, inp, out, rows, gpu, flag, what="MMB2 rows, last table row")


@pytest.mark.parametrize("name", LC.names(family=6))
def test_narrow_fused(gpu, name):
    """mmb_mm2_stream_project_narrow with audio past 2^32 bytes (A = 112, its
    widest frame row), with x and the MMB2 rows past 2^32 (T = 1, 3.6M rows),
    and _narrow_ft with bf16 audio past 2^32."""
    c = _case(name, gpu)
    z = c.dims
    dims = (z["n"], z["t"], z["d"], z["a"], z["vd"])
    assert P.narrow_fused_supported(*dims[1:], z["v"])
    inp = _stream_inputs(c, gpu)
    flag = _flag(gpu)
    fn = P.mm2_stream_project_narrow if z["frames"] == "f32" else P.mm2_stream_project_narrow_ft
    out = fn(*dims, inp["audio"], inp["visual"], _projection(c, gpu), inp["ids"], inp["table"], inp["wtab"],
             flag=flag)
    if c.crossing == "x":
        assert out[0].numel() * 4 == out[2].numel() * 4 == c.op("x").nbytes > LC.B32
    else:
        assert inp[c.crossing].numel() * inp[c.crossing].element_size() == c.op(c.crossing).nbytes > LC.B32
    rows = LC.sample_rows(c)
    _assert_sampled(c, rows)
    _fused_check(c, inp, out, rows, gpu, flag)


# ------------------------------------------------------------------ 7: mmb_sif_wavg
def _wavg_check(c, table, wtab, ids, got_x, got_num, got_cnt, rows, gpu):
    ridx = torch.as_tensor(rows, device=gpu)
    tok = ids[ridx].long()
    x, num, cnt = LC.wavg_reference(_host_upcast(table[tok]), _host_upcast(wtab[tok]))
    fr = []
    if got_x is not None:
        fr.append(_note(c, "x (of 2e-6)", M.row_rel_err(got_x[ridx].cpu().numpy(), x) / 2e-6))
    if got_num is not None:
        fr.append(_note(c, "num (of 2e-6)", M.row_rel_err(got_num[ridx].cpu().numpy(), num) / 2e-6))
        assert np.array_equal(got_cnt[ridx].cpu().numpy(), cnt)
    print(f"{c.name}: {len(rows)} rows, largest row-relative error {max(fr) * 2e-6:.3e} (bar 2e-6)")
    assert max(fr) < 1.0


@pytest.mark.parametrize("name", ["wavg_out_wave", "wavg_out_wg"])
def test_weighted_average_out(gpu, name):
    """x (wave route, L = 1) and num / cnt (workgroup route, L = 65) past 2^32 bytes."""
    c = _case(name, gpu)
    z = c.dims
    g = _gen(c, gpu)
    table, wtab = _word_table(z["v"], z["d"], g, gpu), _weights(z["v"], g, gpu)
    ids = torch.randint(0, z["v"], (z["n"], z["t"]), generator=g, device=gpu, dtype=torch.int32)
    rows = LC.sample_rows(c)
    _assert_sampled(c, rows)
    flag = _flag(gpu)
    if name == "wavg_out_wave":
        x = P.weighted_sum(table, ids, wtab32=wtab, flag=flag, x_out=True)
        assert x.numel() * 4 == c.op("out").nbytes > LC.B32
        _wavg_check(c, table, wtab, ids, x, None, None, rows, gpu)
        # the route does not depend on N: a compact copy of the sampled rows gives the same bits
        ridx = torch.as_tensor(rows, device=gpu)
        again = P.weighted_sum(table, ids[ridx].contiguous(), wtab32=wtab, flag=flag, x_out=True)
        assert torch.equal(again, x[ridx])
    else:
        num, cnt = P.weighted_sum(table, ids, wtab32=wtab, flag=flag)
        assert num.numel() * 4 == c.op("out").nbytes > LC.B32
        _wavg_check(c, table, wtab, ids, None, num, cnt, rows, gpu)
    assert int(flag.item()) == 0


@pytest.mark.parametrize("name", ["wavg_table", "wavg_tt_bf16"])
def test_weighted_average_table(gpu, name):
    """An f32 and a bf16 [V, 512] table past 2^32 bytes on the wave (L = 8) and
    the workgroup (L = 65) routes, ids set by hand."""
    c = _case(name, gpu)
    z = c.dims
    g = _gen(c, gpu)
    dtype = torch.float32 if z["tbytes"] == 4 else torch.bfloat16
    table = _word_table(z["v"], z["d"], g, gpu, dtype)
    assert table.numel() * table.element_size() == c.op("table").nbytes > LC.B32
    wtab = _weights(z["v"], g, gpu)
    need = LC.table_rows(c)
    for l in (z["t"], 65):
        ids_h = LC.gather_ids(c, z["n"], l)
        assert set(need) <= set(ids_h.ravel())
        ids = _dev(ids_h, gpu, torch.int32)
        flag = _flag(gpu)
        x = P.weighted_sum(table, ids, wtab32=wtab, flag=flag, x_out=True)
        num, cnt = P.weighted_sum(table, ids, wtab32=wtab, flag=flag)
        assert int(flag.item()) == 0
        _wavg_check(c, table, wtab, ids, x, num, cnt, np.arange(z["n"]), gpu)


# ------------------------------------------------------------------ 8: the Grams
def _planted(c, gpu, dtype=torch.float32, np_dtype=np.float32):
    """The case's operand on the device (zero but for the planted rows) and the planted rows."""
    z = c.dims
    rows, vals = LC.planted_values(c, z["d"], np_dtype)
    x = torch.zeros((z["n"], z["d"]), dtype=dtype, device=gpu)
    assert x.numel() * x.element_size() == c.op("x").nbytes > LC.B32
    x[torch.as_tensor(rows, device=gpu)] = _dev(vals, gpu, dtype)
    return x, rows, vals


@pytest.mark.parametrize("name", ["gram_tri", "gram_tri_cnt", "gram_generic"])
def test_gram_routes(gpu, name):
    """mmb_gram on the row-range kernel (d = 320, with and without counts) and
    the generic kernel (d = 512); gram_small_kernel takes n <= 4096 rows only."""
    c = _case(name, gpu)
    x, rows, vals = _planted(c, gpu)
    cnt = cnt_h = None
    if c.dims["cnt"]:
        cnt_h = WG._counts(len(rows), LC.seed_of(c))
        cnt = torch.ones(c.n, device=gpu)
        cnt[torch.as_tensor(rows, device=gpu)] = _dev(cnt_h, gpu)
    e = WG._check_gram(_unnoted, P.gram(x, cnt), LC.gram_reference(vals, cnt_h), name)
    _note(c, "G (of 1e-13)", e / 1e-13)
    print(f"{name}: {len(rows)} planted rows, |G - exact| / max |G| = {e:.3e} (bar 1e-13)")


def test_gram_f64(gpu):
    c = _case("gram_f64", gpu)
    x, rows, vals = _planted(c, gpu, torch.float64, np.float64)
    assert not np.array_equal(vals.astype(np.float32).astype(np.float64), vals)
    g = torch.empty((c.dims["d"],) * 2, dtype=torch.float64, device=gpu)
    ws = P.GramWorkspace(c.n, c.dims["d"], gpu)
    L.call("mmb_gram_f64", L.ptr(x), c.n, c.dims["d"], L.ptr(g), 0, L.ptr(ws.buf), L.stream_ptr())
    e = WG._check_gram(_unnoted, g, LC.gram_reference(vals), c.name)
    _note(c, "G (of 1e-13)", e / 1e-13)
    print(f"gram_f64: |G - exact| / max |G| = {e:.3e} (bar 1e-13)")


def test_gram_part_and_finish(gpu):
    """mmb_gram_part + mmb_gram_finish on the whole operand, and on two row
    blocks (the second one's rows start past 2^31 bytes) accumulated."""
    c = _case("gram_part_finish", gpu)
    n, d = c.n, c.dims["d"]
    x, rows, vals = _planted(c, gpu)
    ref = LC.gram_reference(vals)
    ws = P.GramWorkspace(n, d, gpu)
    assert ws.buf.numel() <= LC.GRAM_WS
    g = torch.empty((d, d), dtype=torch.float64, device=gpu)
    n1 = LC.B31 // (4 * d) + 7
    for blocks in ([(0, n)], [(0, n1), (n1, n)]):
        for i, (r0, r1) in enumerate(blocks):
            L.call("mmb_gram_part", L.ptr(x[r0:r1]), None, r1 - r0, n, d, int(i > 0), L.ptr(ws.buf), L.stream_ptr())
        L.call("mmb_gram_finish", n, d, L.ptr(g), 0, L.ptr(ws.buf), L.stream_ptr())
        e = WG._check_gram(_unnoted, g, ref, (c.name, len(blocks)))
        _note(c, "G (of 1e-13)", e / 1e-13)
        print(f"gram_part_finish, {len(blocks)} block(s): |G - exact| / max |G| = {e:.3e} (bar 1e-13)")


def test_gram_i8(gpu):
    """mmb_colmax + mmb_gram_i8 at d = 304, where chunk d 4 is largest."""
    c = _case("gram_i8", gpu)
    x, rows, vals = _planted(c, gpu)
    cm = P.colmax(x)
    assert np.array_equal(cm.cpu().numpy().view(np.float32), np.abs(vals).max(0).astype(np.float32))
    g = P.gram_i8(x, cm).cpu().numpy()
    WG._check_gram_i8(_noter(c), g, vals.astype(np.float32))
    exact = LC.gram_reference(vals)
    _note(c, "G vs exact (of 2e-9)", np.abs(g - exact).max() / np.abs(exact).max() / 2e-9)


# ------------------------------------------------------------------ 9: the removals
@pytest.mark.parametrize("name", LC.names(family=9))
def test_remove(gpu, name):
    """Rows in and out past 2^32 bytes: pc_remove1_kernel (d = 512, one PC, f32
    out), the general vector kernel (two PCs; f64 out), the scalar kernel
    (d = 511), and mmb_pc_remove_f64."""
    c = _case(name, gpu)
    z = c.dims
    n, d, npc = c.n, z["d"], z["npc"]
    g = _gen(c, gpu)
    f64rows = z["in_bytes"] == 8
    x = _randn((n, d), g, gpu, torch.float64 if f64rows else torch.float32, 0.3, 0.4)
    cnt = torch.randint(1, 8, (n,), generator=g, device=gpu).float() if z["cnt"] else None
    pch = W.orthonormal_rows(npc, d, seed=d + npc)
    pc = _dev(pch, gpu)
    out_dtype = torch.float64 if z["out_bytes"] == 8 else torch.float32
    out = P.remove_pc_f64(x, pc) if f64rows else P.remove_pc(x, cnt, pc, out_dtype)
    assert x.numel() * x.element_size() == c.op("x").nbytes > LC.B32
    assert out.numel() * out.element_size() == c.op("out").nbytes > LC.B32 and out.dtype == out_dtype
    rows = LC.sample_rows(c)
    _assert_sampled(c, rows)
    ridx = torch.as_tensor(rows, device=gpu)
    xs, cs = x[ridx].contiguous(), None if cnt is None else cnt[ridx].contiguous()
    ref = LC.remove_reference(xs.cpu().numpy(), None if cs is None else cs.cpu().numpy(), pch)
    got = out[ridx].cpu().numpy()
    if out_dtype == torch.float64:
        e = _note(c, "f64 out (of 1e-12)", M.row_rel_err(got, ref) / 1e-12)
    else:
        e = _note(c, "f32 out (of 2^-23 of the row's max)", LC.row_err(got, ref).max() / F32_ROW)
    print(f"{name}: {len(rows)} rows, largest error {e:.3f} of its bar")
    assert e < 1.0 if out_dtype == torch.float64 else e <= 1.0
    # the route does not depend on n: a compact copy of the sampled rows gives the same bits
    again = P.remove_pc_f64(xs, pc) if f64rows else P.remove_pc(xs, cs, pc, out_dtype)
    assert torch.equal(again, out[ridx])


# ------------------------------------------------------------------ 10: the projections
def _project_operands(c, gpu, s_half):
    """The stream kernel's own outputs at D = A = Vd = 300, T = 2 (s past 2^32
    bytes in either format), the frames freed, and the merged projection."""
    z = c.dims
    inp = _stream_inputs(c, gpu)
    flag = _flag(gpu)
    num, s, aux = P.mm2_stream(z["n"], z["t"], z["d"], z["a"], z["vd"], inp["audio"], inp["visual"],
                               ids32=inp["ids"], table=inp["table"], wtab32=inp["wtab"], flag=flag, s_half=s_half)
    torch.cuda.synchronize()
    assert int(flag.item()) == 0 and s.numel() * s.element_size() == c.op("s").nbytes > LC.B32
    proj = P.MMB2Projection(_networks((z["d"], z["a"], z["vd"]), gpu), z["d"], z["a"], z["vd"], z["t"], gpu)
    return inp, num, s, aux, proj


def _project_check(c, what, got, s_rows, num, aux, proj, ridx, x3, oracle):
    """Sampled projected rows against mmb2_cases.project_reference of the
    device's own operands (its beta bar AND the flat 1e-5) and the oracle (1e-5)."""
    z = c.dims
    K = 2 * (z["d"] + z["a"] + z["vd"])
    ref, bar = C.project_reference(s_rows, num[ridx].cpu().numpy(), aux[:, ridx].cpu().numpy(),
                                   proj.wm.cpu().numpy(), proj.c0.cpu().numpy(), z["d"], K, x3=x3)
    g = got[ridx].cpu().numpy().astype(np.float64)
    err = LC.row_err(g, ref)
    e = _note(c, what + " (of beta)", (err / bar).max())
    f = _note(c, what + " (of 1e-5)", err.max() / TOL)
    o = _note(c, what + " vs oracle (of 1e-5)", M.row_rel_err(g, oracle) / TOL)
    print(f"{c.name} {what}: {e:.3f} of beta, {f:.3f} of 1e-5, oracle {o:.3f} of 1e-5")
    assert e <= 1.0 and f < 1.0 and o < 1.0, (what, e, f, o)


def _oracle_rows(c, inp, ridx):
    z = c.dims
    ids = inp["ids"][ridx].long()
    text, sw = _host_upcast(inp["table"][ids]), _host_upcast(inp["wtab"][ids])
    data = M.concat_inputs(text, _host_upcast(inp["audio"][ridx]), _host_upcast(inp["visual"][ridx]))
    return M.estimate_embedding_overall_gpu2(data, C.params(z["d"], z["a"], z["vd"]), sw, text)


def test_project_f32(gpu):
    c = _case("project_f32", gpu)
    inp, num, s, aux, proj = _project_operands(c, gpu, False)
    rows = LC.sample_rows(c)
    _assert_sampled(c, rows)
    ridx = torch.as_tensor(rows, device=gpu)
    oracle = _oracle_rows(c, inp, ridx)
    del inp
    got = P.mm2_project(s, num, aux, proj)
    _project_check(c, "mmb_mm2_project", got, s[ridx].cpu().numpy(), num, aux, proj, ridx, False, oracle)


def test_project_x3(gpu):
    """mmb_mm2_project_x3, _x3_rmpc (sif_out on the same sample) and _x3_split
    (two slices asked for: its guard tiles nsl <= 2^31 - 1 on the accepted side)."""
    c = _case("project_x3", gpu)
    z = c.dims
    inp, num, s, aux, proj = _project_operands(c, gpu, True)
    rows = LC.sample_rows(c)
    _assert_sampled(c, rows)
    ridx = torch.as_tensor(rows, device=gpu)
    oracle = _oracle_rows(c, inp, ridx)
    del inp
    torch.cuda.empty_cache()
    s_rows = MG._dequant(s[ridx], aux[:, ridx], proj.kp)
    got = P.mm2_project(s, num, aux, proj)
    _project_check(c, "mmb_mm2_project_x3", got, s_rows, num, aux, proj, ridx, True, oracle)
    pch = W.orthonormal_rows(1, z["d"], seed=z["d"])
    pc = _dev(pch, gpu)
    xs = num[ridx].double().cpu().numpy()
    removed = xs - (xs @ pch.T) @ pch
    sif = torch.full((c.n, z["d"]), -7.0, device=gpu)
    got_pc = P.mm2_project(s, num, aux, proj, pc=pc, sif_out=sif)
    assert torch.equal(got_pc[ridx], got[ridx])  # the removal does not touch the MMB2 rows
    e = _note(c, "x3_rmpc sif_out (of 2^-23)", LC.row_err(sif[ridx].cpu().numpy(), removed).max() / F32_ROW)
    assert e <= 1.0
    del got_pc
    ws = P.project_split_ws(c.n, proj.kp, gpu, slices=z["slices"])
    assert ws is not None and ws.numel() == c.op("split_ws").nbytes
    sif.fill_(-7.0)
    got_sp = P.mm2_project(s, num, aux, proj, pc=pc, sif_out=sif, split=ws, slices=z["slices"])
    _project_check(c, "mmb_mm2_project_x3_split", got_sp, s_rows, num, aux, proj, ridx, True, oracle)
    e = _note(c, "x3_split sif_out (of 2^-23)", LC.row_err(sif[ridx].cpu().numpy(), removed).max() / F32_ROW)
    assert e <= 1.0


# ------------------------------------------------------------------ 11: the regressor
def _mlp_check(c, key, what, got, ref, bound):
    """regressor_gpu._check, its ratio noted under the case as `key`."""
    return _note(c, key, RG._check(_unnoted, "large", what, got, ref, bound))


def _mlp_params(c, gpu, seed=0):
    z = c.dims
    prm = RC.make_params(np.random.default_rng([z["d"], z["h"], z["o"], seed]), z["d"], z["h"], z["o"])
    dev = [RG._dev(p, gpu) for p in prm]
    assert dev[0].data_ptr() % 16 == 0
    return prm, dev


def test_mlp_forward_idx_and_eval_perm(gpu):
    """mmb_mlp_forward with idx and mmb_mlp_eval with perm reaching rows of a
    latents table past 2^32 bytes: regressor_cases.FwdCase(600, 56, 3, 17)'s
    rows written to the table's first, boundary and last rows."""
    c = _case("mlp_gather", gpu)
    z = c.dims
    fc = RC.FwdCase(z["d"], z["h"], z["o"], z["n"])
    assert fc in RC.FWD_CASES
    ref = RC.fwd_inputs(fc)
    g = _gen(c, gpu)
    lat = _randn((z["v"], z["d"]), g, gpu)
    lab = _rand((z["v"], z["o"]), g, gpu, lo=-3.0, hi=3.0)
    assert lat.numel() * 4 == c.op("table").nbytes > LC.B32
    rows = LC.gather_ids(c, fc.b, 1).ravel()
    assert set(LC.table_rows(c, fc.b)) == set(rows) and len(set(rows)) == fc.b and rows.max() == z["v"] - 1
    idx = _dev(rows, gpu)
    lat[idx], lab[idx] = RG._dev(ref["x"], gpu), RG._dev(ref["labels"], gpu)
    keep = [RG._dev(p, gpu) for p in ref["params"]]
    assert keep[0].data_ptr() % 16 == 0
    pp = [L.ptr(p) for p in keep]
    st = L.stream_ptr()
    y = torch.full((fc.b, fc.o), np.nan, device=gpu)
    L.call("mmb_mlp_forward", L.ptr(lat), L.ptr(idx), fc.b, fc.d, fc.h, fc.o, *pp, L.ptr(y), st)
    _mlp_check(c, "mmb_mlp_forward idx", "mmb_mlp_forward idx", RG._host64(y), ref["y"], ref["y_bound"])
    batch = 3
    bl = torch.full((-(-fc.b // batch),), np.nan, device=gpu)
    pred = torch.full((fc.b, fc.o), np.nan, device=gpu)
    L.call("mmb_mlp_eval", L.ptr(lat), L.ptr(lab), L.ptr(idx), fc.b, batch, fc.d, fc.h, fc.o, *pp, L.ptr(bl),
           L.ptr(pred), st)
    _mlp_check(c, "mmb_mlp_eval perm pred", "mmb_mlp_eval perm pred", RG._host64(pred), ref["y"], ref["y_bound"])
    # the batch losses as tests/test_gpu_regressor_widths.py derives them
    diff = np.abs(ref["y"] - ref["labels"])
    want = np.array([diff[s:s + batch].mean() for s in range(0, fc.b, batch)])
    m = np.array([diff[s:s + batch].size for s in range(0, fc.b, batch)])
    bound = np.array([ref["y_bound"][s:s + batch].mean() for s in range(0, fc.b, batch)]) + (m + 2) * RC.U32 * want
    _mlp_check(c, "mmb_mlp_eval perm batch_loss", "mmb_mlp_eval perm batch_loss", RG._host64(bl), want, bound)


@pytest.mark.parametrize("name", ["mlp_rows_x", "mlp_rows_hid"])
def test_mlp_forward_train_and_backward(gpu, name):
    """mmb_mlp_forward_train / mmb_mlp_backward with x (d = 600) or hid and dh
    (h = 2040) past 2^32 bytes: y, hid of the sampled rows; then the backward
    of a dy that is zero but for those rows -- dh and dx on them, and (x past
    2^32) the parameter gradients, sums over all rows, from those rows alone."""
    c = _case(name, gpu)
    z = c.dims
    n, d, h, o = c.n, z["d"], z["h"], z["o"]
    prm, dev = _mlp_params(c, gpu)
    pp = [L.ptr(p) for p in dev]
    g = _gen(c, gpu)
    x = _randn((n, d), g, gpu)
    y, hid = torch.empty((n, o), device=gpu), torch.empty((n, h), device=gpu)
    assert c.op(c.crossing).past32 and x.numel() * 4 == c.op("x").nbytes and hid.numel() * 4 == c.op("hid").nbytes
    st = L.stream_ptr()
    L.call("mmb_mlp_forward_train", L.ptr(x), n, d, h, o, *pp, L.ptr(y), L.ptr(hid), st)
    rows = LC.sample_rows(c)
    _assert_sampled(c, rows)
    ridx = torch.as_tensor(rows, device=gpu)
    xs = x[ridx].double().cpu().numpy()
    ry, pre, rhid = R.mlp_forward(xs, *prm)
    _mlp_check(c, "y", name + " y", RG._host64(y[ridx]), ry, R.out_bound(xs, *prm))
    _mlp_check(c, "hid", name + " hid", RG._host64(hid[ridx]), rhid, R.pre_bound(xs, *prm[:2]))
    # backward: dy planted on the sampled rows
    dys = RC.f32(np.random.default_rng(LC.seed_of(c)).standard_normal((len(rows), o)))
    dy = torch.zeros((n, o), device=gpu)
    dy[ridx] = RG._dev(dys, gpu)
    dh, dx = torch.empty((n, h), device=gpu), torch.empty((n, d), device=gpu)
    params = name == "mlp_rows_x"  # (h + 1 blocks walk all rows: at h = 2040 the row kernels alone)
    grads = {k: torch.full(s, np.nan, device=gpu) if params else None
             for k, s in (("dw1", (h, d)), ("db1", (h,)), ("dw2", (o, h)), ("db2", (o,)))}
    L.call("mmb_mlp_backward", L.ptr(x), L.ptr(hid), n, d, h, o, pp[0], pp[2], L.ptr(dy), L.ptr(dh), L.ptr(dx),
           *[L.ptr(grads[k]) for k in ("dw1", "db1", "dw2", "db2")], st)
    hid_s = RG._host64(hid[ridx])  # the activations the backward was given
    ref, bounds = RC.backward_bounds(xs, hid_s, prm[0], prm[2], dys)
    for k, t in (("dh", dh[ridx]), ("dx", dx[ridx])) + tuple((k, grads[k]) for k in grads if params):
        _mlp_check(c, k, f"{name} {k}", RG._host64(t), ref[k], bounds[k])
    others = torch.as_tensor(np.setdiff1d(LC._fill(set(), n, 5, 32), rows), device=gpu)
    assert not dh[others].cpu().numpy().any() and not dx[others].cpu().numpy().any()


def test_mlp_train_rows_past_the_boundaries(gpu):
    """mmb_mlp_train: regressor_cases.TrainCase(448, 33, 1, 32, 33, 0, 1, 0, 26)
    with its 33 rows at the first, boundary and last rows of a latents table
    past 2^32 bytes and perm drawing them there: the float64 run's bars, and
    the bits of the same run on the compact rows."""
    c = _case("mlp_train", gpu)
    z = c.dims
    tc = RC.TrainCase(z["d"], z["h"], z["o"], z["batch"], z["n"], 0, 1, 0, z["seed"])
    assert tc in RC.TRAIN_CASES
    inp, ref = RC.make_train_inputs(tc), RC.train_reference(tc)
    assert ref["margin"] >= RC.MARGIN
    g = _gen(c, gpu)
    lat = _randn((z["v"], z["d"]), g, gpu)
    lab = _rand((z["v"], z["o"]), g, gpu, lo=-3.0, hi=3.0)
    assert lat.numel() * 4 == c.op("table").nbytes > LC.B32
    rows = LC.gather_ids(c, tc.n, 1).ravel()
    assert len(set(rows)) == tc.n and rows.max() == z["v"] - 1 and (rows * z["d"] * 4 > LC.B31).sum() >= 4
    idx = _dev(rows, gpu)
    lat[idx], lab[idx] = RG._dev(inp["x"], gpu), RG._dev(inp["y"], gpu)
    prm = [RG._dev(p, gpu) for p in inp["params"]]
    perm = _dev(rows[inp["perm"]], gpu)
    spe = -(-tc.n // tc.batch)
    sl = torch.full((RC.N_EPOCHS * spe,), np.nan, device=gpu)
    flag = _flag(gpu)
    ws = RG._workspace(gpu, tc.d, tc.h)
    rc = L.query("mmb_mlp_train", L.ptr(lat), L.ptr(lab), L.ptr(perm), tc.n, RC.N_EPOCHS, tc.batch, tc.d, tc.h,
                 tc.o, RC.LR, *[L.ptr(p) for p in prm], L.ptr(sl), None, None, None, 0, 1, tc.epoch0, None,
                 L.ptr(ws), L.ptr(flag), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and int(flag.item()) == 0 and not ws[:4].any().item()
    got = {"params": [RG._host64(p) for p in prm], "step_loss": RG._host64(sl), "valid_loss": np.zeros(0)}
    env_p, env_l = RC.f32_envelope(tc)
    dev_p, dev_l = RC.rel_dev(got, ref)
    bar_p, bar_l = max(4 * env_p, RC.FLOOR), max(4 * env_l, RC.FLOOR)
    _note(c, "parameters", dev_p / bar_p)
    _note(c, "losses", dev_l / bar_l)
    print(f"mlp_train: parameters {dev_p:.2e} (bar {bar_p:.2e}), losses {dev_l:.2e} (bar {bar_l:.2e})")
    assert dev_p <= bar_p and dev_l <= bar_l
    rc2, prm2, sl2, _, flag2 = RG._launch_train(gpu, tc, inp, ws)  # the compact rows: the same bits
    assert rc2 == 0 and torch.equal(sl2, sl) and all(torch.equal(a, b) for a, b in zip(prm, prm2))


# ------------------------------------------------------------------ 12: the latent kernels
def test_word_logprob_workspace(gpu):
    """mmb_word_logprob_forward / _backward at the smallest B whose scratch
    passes 2^32 bytes: word_cases.WordCase(320, 517, 33, 5, 0)'s latents at the
    rows whose partials lie at the scratch's start, boundaries and end."""
    c = _case("word_logprob", gpu)
    z = c.dims
    n, d, v, l = c.n, z["d"], z["v"], z["t"]
    wc = WC.WordCase(d, v, z["b"], l, 0)
    assert wc in WC.WORD_CASES
    assert L.query("mmb_word_workspace_bytes", n, d, v) == c.op("ws").nbytes > LC.B32
    assert L.query("mmb_word_workspace_bytes", n - 16, d, v) <= LC.B32
    inp, lp_ref, g_ref = WC.reference(wc, False)
    rows = LC.word_rows(c)
    assert len(rows) == wc.B and rows[0] == 0 and rows[-1] == n - 1
    ridx = torch.as_tensor(rows, device=gpu)
    g = _gen(c, gpu)
    lat = _randn((n, d), g, gpu, std=0.5)
    ids = torch.randint(0, v, (n, l), generator=g, device=gpu, dtype=torch.int32)
    w, mask, up = _rand((n, l), g, gpu, lo=0.05, hi=1.0), torch.ones((n, l), device=gpu), torch.zeros(n, device=gpu)
    lat[ridx], ids[ridx] = RG._dev(inp["lat"], gpu), _dev(inp["ids"], gpu, torch.int32)
    w[ridx], mask[ridx], up[ridx] = (RG._dev(inp[k], gpu) for k in ("w", "mask", "up"))
    wt = LT.WordTable(RG._dev(inp["table"], gpu))
    x = lat.requires_grad_(True)
    lp = LT.word_log_prob(x, wt, w, mask, WC.A, ids=ids)
    (lp * up).sum().backward()
    r1 = _note(c, "lp", WC.lp_ratio(lp.detach()[ridx].cpu(), lp_ref))
    r2 = _note(c, "gradient", WC.grad_ratio(x.grad[ridx].cpu(), g_ref))
    print(f"word_logprob: lp {r1:.3f} and gradient {r2:.3f} of their bars")
    assert r1 <= 1.0 and r2 <= 1.0 and bool(torch.isfinite(lp).all())


# (the other latent kernels)
def _within(c, key, what, got, ref, bar):
    """gauss_gpu.within, its fraction noted under the case as `key`."""
    GG.within(lambda _, ratio: _note(c, key, ratio), what, got, ref, bar)


@pytest.mark.parametrize("name", ["gauss_stats_x", "gauss_stats_mask"])
def test_gauss_stats(gpu, name):
    c = _case(name, gpu)
    z = c.dims
    g = _gen(c, gpu)
    x = _rand((z["n"], z["t"], z["f"]), g, gpu)
    assert x.numel() * 4 == c.op("x").nbytes > LC.B32
    mask = None
    if z["mask"]:
        mask = torch.empty_like(x).bernoulli_(0.7, generator=g)
    st = LT.gauss_stats(x, mask)
    rows = LC.sample_rows(c)
    _assert_sampled(c, rows)
    ridx = torch.as_tensor(rows, device=gpu)
    xs, ms = x[ridx].contiguous(), None if mask is None else mask[ridx].contiguous()
    ref, bar = G.stats_reference(xs.double().cpu().numpy(), None if ms is None else ms.double().cpu().numpy())
    _within(c, "stats (gauss_cases.stats_reference)", f"large {name}", st[ridx], ref, bar)
    assert torch.equal(LT.gauss_stats(xs, ms).view(torch.int64), st[ridx].view(torch.int64))


def test_gauss_loglik_idx(gpu):
    """mmb_gauss_loglik / _backward with idx reaching rows of a stats table
    past 2^32 bytes: the frame sums of 64 utterances written to the table's
    first, boundary and last rows, the rest of it seeded noise."""
    c = _case("gauss_loglik_idx", gpu)
    z = c.dims
    b, f, ns, t = z["n"], z["f"], z["v"], 12
    g = _gen(c, gpu)
    table = _randn((ns, 3, f), g, gpu, torch.float64)
    assert table.numel() * 8 == c.op("table").nbytes > LC.B32
    idx_h = LC.gather_ids(c, b, 1).ravel()
    assert set(LC.table_rows(c)) <= set(idx_h) and len(set(idx_h)) == b
    rng = np.random.default_rng(LC.seed_of(c))
    x = G.f32(rng.uniform(-1.0, 1.0, (b, t, f)))
    mu, sigma = G.f32(0.5 * rng.standard_normal((b, f))), G.f32(rng.uniform(0.5, 1.5, (b, f)))
    up = G.f32(rng.standard_normal(b))
    idx = _dev(idx_h, gpu)
    table[idx] = LT.gauss_stats(_dev(x, gpu, torch.float32))
    mus = _dev(mu, gpu, torch.float32).requires_grad_(True)
    sgs = _dev(sigma, gpu, torch.float32).requires_grad_(True)
    lp = LT.gauss_log_prob(LT.GaussStats(text=table), ["text"], [mus], [sgs], idx=idx)
    (lp * _dev(up, gpu, torch.float32)).sum().backward()
    ref = G.normal_reference(mu, sigma, x, None, up)
    bars = G.normal_bars(mu, sigma, x, None, up, ref)
    for what, got, r, bar in zip(("lp", "dmu", "dsigma"), (lp[0], mus.grad, sgs.grad), ref, bars):
        _within(c, what, f"large gauss {what}", got, r, bar)


def _ln_inputs(c, gpu, dy=None):
    n, d = c.n, c.dims["d"]
    g = _gen(c, gpu)
    x = _randn((n, d), g, gpu, mean=0.2, std=1.5)
    var, mean = torch.var_mean(x, dim=1, unbiased=False)
    rstd = torch.rsqrt(var + G.LN_EPS)
    gamma = _rand((d,), g, gpu, lo=0.5, hi=1.5)
    if dy is None:
        dy = _randn((n, d), g, gpu)
    dx = torch.empty_like(x)
    for name, t in (("dy", dy), ("x", x), ("dx", dx)):
        assert t.numel() * 4 == c.op(name).nbytes > LC.B32
    return dy, x, mean, rstd, gamma, dx


def _ln_reference(dy, x, mean, rstd, gamma, ridx):
    a = [t[ridx].double().cpu().numpy() for t in (dy, x, mean, rstd)]
    return G.layer_norm_backward_reference(a[0], a[1], a[2], a[3], gamma.double().cpu().numpy())


def test_layer_norm_backward_dx(gpu):
    """n d past 2^32 bytes, no dgamma / dbeta (the cb = 0 launch): dx on the sample."""
    c = _case("ln_backward_dx", gpu)
    dy, x, mean, rstd, gamma, dx = _ln_inputs(c, gpu)
    L.call("mmb_layer_norm_backward", L.ptr(dy), L.ptr(x), L.ptr(mean), L.ptr(rstd), L.ptr(gamma), c.n,
           c.dims["d"], L.ptr(dx), None, None, L.stream_ptr())
    rows = LC.sample_rows(c)
    _assert_sampled(c, rows)
    ridx = torch.as_tensor(rows, device=gpu)
    ref, bars = _ln_reference(dy, x, mean, rstd, gamma, ridx)
    _within(c, "dx", "large LN dx", dx[ridx], ref[0], bars[0])


def test_layer_norm_backward_dgamma(gpu):
    """dgamma / dbeta over all rows from a dy that is zero but for planted rows
    (as many in each of the kernel's four row groups), on seeded x; dx of the
    planted rows on the way, and zero rows elsewhere."""
    c = _case("ln_backward_dgamma", gpu)
    n, d = c.n, c.dims["d"]
    rows, vals = LC.planted_values(c, d)
    assert len({int(np.sum(rows % 4 == k)) for k in range(4)}) == 1
    ridx = torch.as_tensor(rows, device=gpu)
    dy = torch.zeros((n, d), device=gpu)
    dy[ridx] = _dev(vals, gpu, torch.float32)
    dy, x, mean, rstd, gamma, dx = _ln_inputs(c, gpu, dy)
    dgamma, dbeta = torch.empty(d, device=gpu), torch.empty(d, device=gpu)
    L.call("mmb_layer_norm_backward", L.ptr(dy), L.ptr(x), L.ptr(mean), L.ptr(rstd), L.ptr(gamma), n, d,
           L.ptr(dx), L.ptr(dgamma), L.ptr(dbeta), L.stream_ptr())
    # the planted rows alone: every other row adds an exact zero to its group's sums
    ref, bars = _ln_reference(dy, x, mean, rstd, gamma, ridx)
    for what, got, r, bar in zip(("dx", "dgamma", "dbeta"), (dx[ridx], dgamma, dbeta), ref, bars):
        _within(c, what, f"large LN planted {what}", got, r, bar)
    others = torch.as_tensor(np.setdiff1d(LC.sample_rows(c), rows), device=gpu)
    assert not dx[others].cpu().numpy().any()


def test_word_normalize(gpu):
    c = _case("word_normalize", gpu)
    v, d = c.n, c.dims["d"]
    dp = L.query("mmb_word_pad", d)
    table = _word_table(v, d, _gen(c, gpu), gpu)
    wn = torch.empty((v, dp), device=gpu)
    assert table.numel() * 4 == c.op("table_in").nbytes > LC.B32 and wn.numel() * 4 == c.op("wn").nbytes
    L.call("mmb_word_normalize", L.ptr(table), v, d, L.ptr(wn), L.stream_ptr())
    rows = LC.sample_rows(c)
    _assert_sampled(c, rows)
    ridx = torch.as_tensor(rows, device=gpu)
    tab = table[ridx].contiguous()
    ref = LC.normalize_reference(tab.cpu().numpy(), dp)
    got = wn[ridx].cpu().numpy()
    # the bar of test_gpu_word_widths.test_normalised_table_is_zero_padded at this width: the norm
    # (a d-term sum of squares, (d + 1) u halved by the root), the root, the division; x2.  The
    # pad is zero, and so is row 0 (a zero table row: 0 / 1e-8)
    assert not got[:, d:].any() and not got[0].any()
    bar = 2 * ((d + 1) / 2 + 2) * C.U * np.abs(ref)
    e = _note(c, "Wn", _frac(np.abs(got - ref), bar))
    print(f"word_normalize: {len(rows)} rows, largest error {e:.3f} of its bar")
    assert e <= 1.0
    again = torch.empty((len(rows), dp), device=gpu)
    L.call("mmb_word_normalize", L.ptr(tab), len(rows), d, L.ptr(again), L.stream_ptr())
    assert torch.equal(again, wn[ridx])
