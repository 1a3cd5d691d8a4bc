"""Shared case table and f64 references of tests/test_gpu_large.py (GPU) and
tests/test_large_cases.py (CPU): every kernel family on an operand past 2^31
and 2^32 bytes.  Plain helper module: no test is collected from it.

A case fixes a shape at which exactly one named operand (`Case.crossing`) is
the smallest of its row width to pass B32 = 2^32 bytes: rows = B32 // row
bytes + 1, so bytes > B32 >= bytes - one row, and it passes B31 = 2^31 on the
way.  The row is the widest the entry point takes, so the row count stays
small.  The other operands of the launch stay small, except where the shape
itself takes a second one past a boundary (the s rows of the x-out stream
case, the removal's output, the normalised word table): those are listed too
and their boundary rows are sampled as well.  Every device buffer of a case is
an Operand, so the CPU test can add them up (<= 16 GiB per case).

Per-row kernels are checked on a sample of at most 64 rows (sample_rows): row
0, the last row, for every operand past B31 the last row wholly below the
boundary, the row holding the boundary byte and the next one (wholly above),
the same for B32 where such rows exist (at the smallest row count the row
holding B32 is the last row), and a seeded remainder.  Gathered operands (a
word table, a stats table) are reached through ids set by hand (gather_ids):
the table's sample, every row of it.

Reductions over all rows run on an operand that is zero except for planted
seeded rows (planted_rows: the boundary rows, rows of each of the three
regions, the very last row), so the exact result follows from the planted
rows alone.  wrapped_row() is what a read of a late planted row at its byte
offset taken modulo 2^31 or 2^32 would fetch: the CPU test shows that the
result then moves by more than 1e3 x the bar.
"""
from __future__ import annotations

import collections

import numpy as np

from width_cases import F32_ROW  # noqa: F401  (the removals' f32 bar, for tests/test_large_cases.py)

B31, B32 = 2 ** 31, 2 ** 32
GIB = 2 ** 30
MAX_CASE_BYTES = 16 * GIB
MAX_SAMPLE = 64


class Operand(collections.namedtuple("Operand", "name rows row_bytes index")):
    """A device buffer of a case: `rows` rows of `row_bytes` bytes.  index:
    "row" (one row per row of the launch), "table" (gathered through ids),
    "flat" (anything else: weights, workspaces)."""

    @property
    def nbytes(self):
        return self.rows * self.row_bytes

    @property
    def past31(self):
        return self.nbytes > B31

    @property
    def past32(self):
        return self.nbytes > B32


class Case(collections.namedtuple("Case", "name family entry dims crossing operands")):
    """dims: the launch's shape (a dict); crossing: the name of the operand the
    case is built around; operands: every device buffer it allocates."""

    def op(self, name):
        return next(o for o in self.operands if o.name == name)

    @property
    def n(self):
        return self.dims["n"]

    @property
    def total_bytes(self):
        return sum(o.nbytes for o in self.operands)


def rows_past(boundary, row_bytes):
    """The smallest row count whose rows pass `boundary` bytes."""
    return boundary // row_bytes + 1


def mm2_k(d, a, vd):
    return (2 * (d + a + vd) + 31) // 32 * 32


def pad16(d):
    return (d + 15) // 16 * 16


def boundary_rows(row_bytes, boundary, rows):
    """(below, at, above) of `boundary` among `rows` rows of `row_bytes`: the
    last row wholly below it, the row holding byte `boundary`, the next row
    (wholly above); None where the operand has no such row."""
    at = boundary // row_bytes
    return tuple(r if 0 <= r < rows else None for r in (at - 1, at, at + 1))


def crossing_operands(case, index="row"):
    return [o for o in case.operands if o.index == index and o.past31]


def required_rows(rows, row_bytes_list):
    """Row 0, the last row and the boundary rows of every given row width."""
    need = {0, rows - 1}
    for rb in row_bytes_list:
        for b in (B31, B32):
            if rows * rb > b:
                need.update(r for r in boundary_rows(rb, b, rows) if r is not None)
    return sorted(need)


def _fill(need, rows, seed, count):
    rng = np.random.default_rng(seed)
    need = set(need)
    assert len(need) <= count
    while len(need) < min(count, rows):
        need.add(int(rng.integers(0, rows)))
    return np.array(sorted(need), dtype=np.int64)


def sample_rows(case, count=MAX_SAMPLE):
    """The sampled launch rows of a per-row case (sorted int64)."""
    ops = crossing_operands(case, "row")
    return _fill(required_rows(case.n, [o.row_bytes for o in ops]), case.n, seed_of(case), count)


def table_rows(case, count=MAX_SAMPLE):
    """The sampled rows of a case's gathered table (sorted int64): row 0, the
    three top rows, the boundary rows, a seeded remainder."""
    t = next(o for o in case.operands if o.index == "table")
    widths = [t.row_bytes] if t.past31 else []
    need = set(required_rows(t.rows, widths)) | {max(0, t.rows - 3), max(0, t.rows - 2)}
    return _fill(sorted(need), t.rows, seed_of(case) + 1, count)


def gather_ids(case, n, l):
    """ids [n, l] int64 into the case's table: every row of table_rows() at
    least once (the boundary rows and the last row among them), the rest seeded."""
    t = next(o for o in case.operands if o.index == "table")
    need = table_rows(case, min(MAX_SAMPLE, n * l))
    rng = np.random.default_rng(seed_of(case) + 2)
    ids = rng.integers(0, t.rows, size=n * l)
    ids[rng.permutation(n * l)[:len(need)]] = need
    return ids.reshape(n, l)


def seed_of(case):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(case.name)) % (2 ** 31 - 1)


# ---------------------------------------------------------------- planted rows (reductions)
def planted_rows(case, balance=1):
    """Rows of a reduction case's operand that hold data (the rest is zero):
    the required rows of sample_rows, two more rows of each region (below B31,
    between, past B32 where the operand has them) -- sorted int64.  balance > 1
    adds seeded rows until every residue class r % balance holds as many rows
    as the fullest (LayerNorm backward: four row groups per column block)."""
    op = case.op(case.crossing)
    rb, n = op.row_bytes, op.rows
    need = set(required_rows(n, [rb]))
    r31, r32 = B31 // rb, min(B32 // rb, n - 1)
    need.update({1, r31 // 3, 2 * r31 // 3, r31 + (r32 - r31) // 3, r31 + 2 * (r32 - r31) // 3})
    rng = np.random.default_rng(seed_of(case) + 3)
    if balance > 1:
        while True:
            per = [sum(1 for r in need if r % balance == g) for g in range(balance)]
            if min(per) == max(per):
                break
            g = int(np.argmin(per))
            need.add(int(rng.integers(0, n // balance)) * balance + g)
    return np.array(sorted(need), dtype=np.int64)


def planted_values(case, d, dtype=np.float32, scale=1.0):
    """Seeded values [k, d] of the planted rows, representable in `dtype`."""
    rows = planted_rows(case, case.dims.get("balance", 1))
    rng = np.random.default_rng(seed_of(case) + 4)
    v = scale * rng.standard_normal((len(rows), d)) + 0.25
    return rows, v.astype(dtype).astype(np.float64)


def wrapped_row(rows, vals, r, esize, boundary):
    """The d values a read of row r fetches when every element's byte offset
    wraps modulo `boundary`: element e of the operand comes from element
    (e esize mod boundary) / esize -- zeros, or a piece of an early planted
    row (a row that straddles the boundary keeps its part below it)."""
    d = vals.shape[1]
    out = np.zeros(d)
    where = {int(q): i for i, q in enumerate(rows)}
    for c in range(d):
        e = (int(r) * d + c) * esize % boundary // esize
        q, col = divmod(e, d)
        if q in where:
            out[c] = vals[where[q], col]
    return out


def late_rows(rows, row_bytes, boundary):
    """The planted rows with a byte at or past `boundary`."""
    return [int(r) for r in rows if (int(r) + 1) * row_bytes > boundary]


# ---------------------------------------------------------------- f64 references
def gram_reference(x, cnt=None):
    """Exact f64 Gram of the planted rows (x = f32(num / cnt) where cnt is given)."""
    x = np.asarray(x, np.float64)
    if cnt is not None:
        x = (x.astype(np.float32) / np.asarray(cnt, np.float32)[:, None]).astype(np.float64)
    return x.T @ x


def gram_reference_2(x, cnt=None):
    """The same as a sum of row outer products in extended precision."""
    x = np.asarray(x, np.float64)
    if cnt is not None:
        x = (x.astype(np.float32) / np.asarray(cnt, np.float32)[:, None]).astype(np.float64)
    g = np.zeros((x.shape[1], x.shape[1]), np.longdouble)
    for row in x.astype(np.longdouble):
        g += np.outer(row, row)
    return g.astype(np.float64)


def remove_reference(num, cnt, pc):
    """x - (x pc^T) pc in f64 of x = f32(num / cnt) (f32 rows with a count),
    or of the f64 rows themselves (cnt None)."""
    x = np.asarray(num, np.float64)
    if cnt is not None:
        x = (np.asarray(num, np.float32) / np.asarray(cnt, np.float32)[:, None]).astype(np.float64)
    return x - (x @ pc.T) @ pc


def remove_reference_2(num, cnt, pc):
    """The same, one component at a time in extended precision."""
    x = np.asarray(num, np.longdouble)
    if cnt is not None:
        x = (np.asarray(num, np.float32) / np.asarray(cnt, np.float32)[:, None]).astype(np.longdouble)
    out = x.copy()
    for v in np.asarray(pc, np.longdouble):
        out -= np.outer(x @ v, v)
    return out.astype(np.float64)


def wavg_reference(rows, w):
    """(x, num, cnt) of mmb_sif_wavg from the gathered table rows [n, l, d]
    (f32-representable) and the gathered weights [n, l]: num = sum_t w E,
    cnt = count_nonzero(w), x = num / cnt."""
    rows, w = np.asarray(rows, np.float64), np.asarray(w, np.float64)
    num = (w[:, :, None] * rows).sum(1)
    cnt = np.count_nonzero(w, axis=1).astype(np.float64)
    return num / cnt[:, None], num, cnt


def wavg_reference_2(rows, w):
    """The same token by token in extended precision."""
    rows, w = np.asarray(rows, np.longdouble), np.asarray(w, np.longdouble)
    num = np.zeros((rows.shape[0], rows.shape[2]), np.longdouble)
    for t in range(rows.shape[1]):
        num += w[:, t, None] * rows[:, t]
    cnt = (w != 0).sum(1).astype(np.longdouble)
    return (num / cnt[:, None]).astype(np.float64), num.astype(np.float64), cnt.astype(np.float64)


def normalize_reference(w, dp):
    """mmb_word_normalize: W / max(||W||, 1e-8), zero padded to dp columns."""
    w = np.asarray(w, np.float64)
    out = np.zeros((w.shape[0], dp))
    out[:, :w.shape[1]] = w / np.maximum(np.linalg.norm(w, axis=1), 1e-8)[:, None]
    return out


def normalize_reference_2(w, dp):
    w = np.asarray(w, np.longdouble)
    n = np.sqrt((w * w).sum(1))
    out = np.zeros((w.shape[0], dp), np.longdouble)
    out[:, :w.shape[1]] = w / np.maximum(n, np.longdouble(1e-8))[:, None]
    return out.astype(np.float64)


def row_err(got, ref):
    """Per-row max |got - ref| / max |ref| (oracle.mmb2_oracle.row_rel_err without the max over rows)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref).max(axis=1) / np.abs(ref).max(axis=1)


# ---------------------------------------------------------------- the case table
def _op(name, rows, row_bytes, index="flat"):
    return Operand(name, int(rows), int(row_bytes), index)


def _case(name, family, entry, dims, crossing, operands):
    return Case(name, family, entry, dict(dims), crossing, tuple(operands))


def stream_case(name, family, entry, d, a, vd, t, crossing, fbytes=4, s_half=False, v=300, frames=None):
    """A stream launch whose `crossing` operand ("audio", "visual" or "x")
    passes B32; gathered text from a small f32 table."""
    kp = mm2_k(d, a, vd)
    width = {"audio": t * a * fbytes, "visual": t * vd * fbytes, "x": d * 4}
    n = rows_past(B32, width[crossing])
    ops = [_op("ids", n, t * 4, "row"), _op("table", v, d * 4, "table"), _op("wtab", v, 4),
           _op("audio", n, t * a * fbytes, "row"), _op("visual", n, t * vd * fbytes, "row"),
           _op("x", n, d * 4, "row"), _op("s", n, kp * 4, "row"), _op("aux", 3, n * 4)]
    frames = frames or ("f32" if fbytes == 4 else "bf16")
    return _case(name, family, entry, dict(n=n, t=t, d=d, a=a, vd=vd, v=v, kp=kp, fbytes=fbytes, s_half=s_half,
                                           frames=frames), crossing, ops)


def fused_case(name, family, entry, d, a, vd, t, crossing, fbytes=4, v=300, frames=None):
    """A fused stream + projection launch (no s rows: the sums stay on chip)
    whose `crossing` operand ("audio", "visual" or "x") passes B32; the MMB2
    rows are as wide as x."""
    width = {"audio": t * a * fbytes, "visual": t * vd * fbytes, "x": d * 4}
    n = rows_past(B32, width[crossing])
    ops = [_op("ids", n, t * 4, "row"), _op("table", v, d * 4, "table"), _op("wtab", v, 4),
           _op("audio", n, t * a * fbytes, "row"), _op("visual", n, t * vd * fbytes, "row"),
           _op("x", n, d * 4, "row"), _op("mmb2", n, d * 4, "row"), _op("aux", 3, n * 4),
           _op("weights", 1, 16 * 2 ** 20), _op("text_cache", v, 609 * 4 + 4)]
    frames = frames or ("f32" if fbytes == 4 else "bf16")
    return _case(name, family, entry, dict(n=n, t=t, d=d, a=a, vd=vd, v=v, fbytes=fbytes, frames=frames), crossing, ops)


def split_case(name, entry, fbytes=4, parts=(0, 2), frames=None):
    """The split stream on POM-length rows: T = 1357 frames of A = 300."""
    d, a, vd, t, v = 300, 300, 4, 1357, 300
    c = stream_case(name, 3, entry, d, a, vd, t, "audio", fbytes=fbytes, v=v, frames=frames)
    wsb = c.n * 3 * ((3 * d + 7) // 4 * 4 + (2 * a + 2 * vd + 3) // 4 * 4) * 4  # <= 3 parts
    return _case(name, 3, entry, dict(c.dims, parts=parts), "audio", c.operands + (_op("split_ws", 1, wsb),))


def table_case(name, family, entry, d, v, tbytes=4, n=64, t=8, a=4, vd=4, mm2=True):
    """n rows of t tokens gathered from a [v, d] word table of tbytes-byte
    elements: the table is the large operand."""
    kp = mm2_k(d, a, vd)
    ops = [_op("ids", n, t * 4, "row"), _op("table", v, d * tbytes, "table"), _op("wtab", v, 4),
           _op("x", n, d * 4, "row")]
    if mm2:
        ops += [_op("audio", n, t * a * 4, "row"), _op("visual", n, t * vd * 4, "row"),
                _op("s", n, kp * 4, "row"), _op("aux", 3, n * 4)]
    return _case(name, family, entry, dict(n=n, t=t, d=d, a=a, vd=vd, v=v, kp=kp, tbytes=tbytes), "table", ops)


def wavg_out_case(name, l):
    d, v = 512, 300
    n = rows_past(B32, d * 4)
    ops = [_op("ids", n, l * 4, "row"), _op("table", v, d * 4, "table"), _op("wtab", v, 4),
           _op("out", n, d * 4, "row"), _op("cnt", n, 4)]
    return _case(name, 7, "mmb_sif_wavg", dict(n=n, t=l, d=d, v=v), "out", ops)


GRAM_WS = 256 * 2 ** 20  # an upper bound of mmb_gram_workspace_bytes at these shapes (the CPU test checks it)


def gram_case(name, entry, d, esize=4, cnt=False):
    n = rows_past(B32, d * esize)
    ops = [_op("x", n, d * esize, "row"), _op("g", d, d * 8), _op("ws", 1, GRAM_WS)]
    if cnt:
        ops.append(_op("cnt", n, 4))
    if entry == "mmb_gram_i8":
        ops.append(_op("colmax", d, 4))
    return _case(name, 8, entry, dict(n=n, d=d, esize=esize, cnt=cnt), "x", ops)


def remove_case(name, entry, d, npc, in_bytes=4, out_bytes=4, cnt=True):
    n = rows_past(B32, d * min(in_bytes, out_bytes))
    ops = [_op("x", n, d * in_bytes, "row"), _op("out", n, d * out_bytes, "row"), _op("pc", npc, d * 8)]
    if cnt:
        ops.append(_op("cnt", n, 4))
    return _case(name, 9, entry, dict(n=n, d=d, npc=npc, in_bytes=in_bytes, out_bytes=out_bytes, cnt=cnt),
                 "x", ops)


def project_case(name, entry, s_half, split=False, rmpc=False):
    """D = A = Vd = 300: the widest s row (Kp = 1824: 7,296 bytes in either
    format).  The operands are the stream kernel's own outputs at T = 2."""
    d = a = vd = 300
    t, v = 2, 300
    kp = mm2_k(d, a, vd)
    n = rows_past(B32, kp * 4)
    ops = [_op("ids", n, t * 4, "row"), _op("table", v, d * 4, "table"), _op("wtab", v, 4),
           _op("audio", n, t * a * 4, "row"), _op("visual", n, t * vd * 4, "row"), _op("x", n, d * 4, "row"),
           _op("s", n, kp * 4, "row"), _op("aux", 3, n * 4), _op("out", n, d * 4, "row"),
           _op("weights", 1, 16 * 2 ** 20)]
    if rmpc:
        ops.append(_op("sif_out", n, d * 4, "row"))
    if split:
        ops.append(_op("split_ws", -(-n // 128) * 2, 128 * 320 * 4))
    return _case(name, 10, entry, dict(n=n, t=t, d=d, a=a, vd=vd, v=v, kp=kp, s_half=s_half, slices=2), "s", ops)


def _latent_cases():
    out = []
    # mmb_gauss_stats: x [n, t, f] (and its mask) past B32
    t, f = 64, 320
    n = rows_past(B32, t * f * 4)
    out.append(_case("gauss_stats_x", 12, "mmb_gauss_stats", dict(n=n, t=t, f=f, mask=False), "x",
                     [_op("x", n, t * f * 4, "row"), _op("stats", n, 3 * f * 8, "row")]))
    out.append(_case("gauss_stats_mask", 12, "mmb_gauss_stats", dict(n=n, t=t, f=f, mask=True), "x",
                     [_op("x", n, t * f * 4, "row"), _op("mask", n, t * f * 4, "row"),
                      _op("stats", n, 3 * f * 8, "row")]))
    # mmb_gauss_loglik / _backward: idx into a stats table past B32 (f = 320: 7,680-byte rows)
    f, b = 320, 64
    ns = rows_past(B32, 3 * f * 8)
    out.append(_case("gauss_loglik_idx", 12, "mmb_gauss_loglik", dict(n=b, f=f, v=ns), "table",
                     [_op("table", ns, 3 * f * 8, "table"), _op("idx", b, 8, "row"), _op("mu", b, f * 4, "row"),
                      _op("sigma", b, f * 4, "row"), _op("grads", 2 * b, f * 4)]))
    # mmb_layer_norm_backward: n d past B32 (dy, x, dx; d = 2048: the kernel has no width limit)
    d = 2048
    n = rows_past(B32, d * 4)
    ln = [_op("dy", n, d * 4, "row"), _op("x", n, d * 4, "row"), _op("dx", n, d * 4, "row"),
          _op("mean_rstd", 2, n * 4), _op("gamma_dgamma_dbeta", 3, d * 4)]
    out.append(_case("ln_backward_dx", 12, "mmb_layer_norm_backward", dict(n=n, d=d), "x", ln))
    out.append(_case("ln_backward_dgamma", 12, "mmb_layer_norm_backward", dict(n=n, d=d, balance=4), "x", ln))
    # mmb_word_normalize: a [v, 320] table past B32 (320: the widest the word kernels read)
    d = 320
    v = rows_past(B32, d * 4)
    out.append(_case("word_normalize", 12, "mmb_word_normalize", dict(n=v, d=d), "table_in",
                     [_op("table_in", v, d * 4, "row"), _op("wn", v, pad16(d) * 4, "row")]))
    return out


WORD_TILE_BYTES = 4 * 16 * (320 + 2) * 4  # mmb_word_logprob_forward's scratch per 16 latents at d = 320 (one split)


def _regressor_cases():
    """The regressor's kernels.  The gathers and the training run embed a small
    case of tests/regressor_cases.py (its rows written to the first, boundary
    and last rows of a latents table past B32, the rest seeded noise), so
    their float64 references and bars are that case's own."""
    out = []
    d, h, o, b = 600, 56, 3, 17  # regressor_cases.FwdCase(600, 56, 3, 17): the widest row, V4
    n = rows_past(B32, d * 4)
    small = [_op("params", 1, 4 * (h * d + h + o * h + o)), _op("outputs", 4 * b, 4 * o)]
    out.append(_case("mlp_gather", 11, "mmb_mlp_forward", dict(n=b, d=d, h=h, o=o, v=n), "table",
                     [_op("table", n, d * 4, "table"), _op("labels", n, o * 4)] + small))
    rows = lambda n, *w: [_op(name, n, 4 * k, "row") for name, k in w]
    out.append(_case("mlp_rows_x", 11, "mmb_mlp_forward_train", dict(n=n, d=d, h=h, o=o), "x",
                     rows(n, ("x", d), ("hid", h), ("y", o), ("dy", o), ("dh", h), ("dx", d)) + small))
    d, h = 4, 2040  # 8 (d + h) floats of LDS: h = 2040 is the widest hidden row beside d = 4
    n = rows_past(B32, h * 4)
    out.append(_case("mlp_rows_hid", 11, "mmb_mlp_forward_train", dict(n=n, d=d, h=h, o=o), "hid",
                     rows(n, ("x", d), ("hid", h), ("y", o), ("dy", o), ("dh", h), ("dx", d)) +
                     [_op("params", 1, 4 * (h * d + h + o * h + o))]))
    d, h, o, b = 448, 33, 1, 33  # regressor_cases.TrainCase(448, 33, 1, 32, 33, 0, 1, 0, 26): the widest trained
    n = rows_past(B32, d * 4)
    out.append(_case("mlp_train", 11, "mmb_mlp_train", dict(n=b, d=d, h=h, o=o, v=n, batch=32, seed=26), "table",
                     [_op("table", n, d * 4, "table"), _op("labels", n, o * 4),
                      _op("params_ws", 1, 4 * (h * d + h + o * h + o) + 2 ** 16)]))
    return out


def _word_case():
    """mmb_word_logprob_forward / _backward at the smallest B whose scratch
    passes B32 (d = 320, one word split: 82,432 bytes per tile of 16 latents);
    word_cases.WordCase(320, 517, 33, 5, 0) embedded in seeded latents."""
    d, v, l = 320, 517, 5
    tiles = rows_past(B32, WORD_TILE_BYTES)
    n = (tiles - 1) * 16 + 1
    per = lambda name, k: _op(name, n, 4 * k, "row")
    return _case("word_logprob", 12, "mmb_word_logprob_forward", dict(n=n, d=d, v=v, t=l, tiles=tiles, b=33), "ws",
                 [_op("ws", tiles, WORD_TILE_BYTES), _op("table", v, d * 4, "table"), _op("wn", v, d * 4),
                  per("lat", d), per("dlat", d), per("gsum", d), per("state", 4), per("cos", l), per("ids", l),
                  per("w", l), per("mask", l), per("lp_dlp", 2), per("grad", d)])


def word_rows(case):
    """The latents of the word case that are checked (the embedded small
    case's rows): row 0, the last latent, the first and last latent of every
    tile that a boundary of the scratch falls next to or into, a seeded rest."""
    n, tiles = case.n, case.dims["tiles"]
    need = {0, n - 1}
    for t in required_rows(tiles, [WORD_TILE_BYTES]):
        need.update(r for r in (16 * t, 16 * t + 15) if r < n)
    return _fill(need, n, seed_of(case), case.dims["b"])


def _build():
    two20 = 2 ** 20
    cases = [
        # 1: the wave stream kernel (D <= 256 and 320 <= D <= 512)
        stream_case("wave_audio", 1, "mmb_mm2_stream", 8, 320, 4, 64, "audio"),
        stream_case("wave_visual", 1, "mmb_mm2_stream", 8, 4, 320, 64, "visual"),
        stream_case("wave_x_s32", 1, "mmb_mm2_stream", 512, 4, 4, 1, "x", s_half=False),
        stream_case("wave_x_s16", 1, "mmb_mm2_stream", 512, 4, 4, 1, "x", s_half=True),
        stream_case("wave_ft_bf16_audio", 1, "mmb_mm2_stream_ft", 8, 320, 4, 64, "audio", fbytes=2),
        # 2: the workgroup stream kernel (T > 64): vector and scalar frame loads
        stream_case("wg_vector_audio", 2, "mmb_mm2_stream", 8, 320, 4, 65, "audio"),
        stream_case("wg_scalar_audio", 2, "mmb_mm2_stream", 8, 318, 4, 65, "audio"),
        stream_case("wg_ft_f16_audio", 2, "mmb_mm2_stream_ft", 8, 320, 4, 65, "audio", fbytes=2, frames="f16"),
        # 3: the split stream on a few POM-length rows (1.6 MB of audio per row)
        split_case("split_audio", "mmb_mm2_stream_split"),
        split_case("split_ft_f16_audio", "mmb_mm2_stream_split_ft", fbytes=2, frames="f16"),
        # 4: the word table at and past 2 GiB (D = 512: 2,048-byte rows)
        table_case("table_narrow_last", 4, "mmb_mm2_stream", 512, two20 - 1),
        table_case("table_narrow_refused", 4, "mmb_mm2_stream", 512, two20),
        table_case("table_past_b32", 4, "mmb_mm2_stream", 512, rows_past(B32, 512 * 4)),
        table_case("table_tt_bf16", 4, "mmb_mm2_stream_tt", 512, rows_past(B32, 512 * 2), tbytes=2),
        # 4 / 5: the fused kernel's table guard (fused_pipe_ok) at D = 256 (1,024-byte rows): the
        # pipelined streamer at 2^31 - 1024 bytes, the group-at-a-time fallback at 2^31
        table_case("fused_table_last", 5, "mmb_mm2_stream_project", 256, 2 ** 21 - 1, t=21),
        table_case("fused_table_refused", 5, "mmb_mm2_stream_project", 256, 2 ** 21, t=21),
        # 5: the wide fused kernel (256 <= D < 320)
        fused_case("fused_visual", 5, "mmb_mm2_stream_project", 256, 4, 320, 64, "visual"),
        fused_case("fused_audio", 5, "mmb_mm2_stream_project", 256, 320, 4, 64, "audio"),
        fused_case("fused_ft_f16_visual", 5, "mmb_mm2_stream_project_ft", 256, 4, 320, 64, "visual", fbytes=2,
                   frames="f16"),
        # 6: the narrow fused kernel (A = 112 is its widest frame row beside Vd = 4: kq(A) + kq(Vd) <= 256)
        fused_case("narrow_fused_audio", 6, "mmb_mm2_stream_project_narrow", 300, 112, 4, 64, "audio", v=3016),
        fused_case("narrow_fused_x", 6, "mmb_mm2_stream_project_narrow", 300, 4, 4, 1, "x", v=3016),
        fused_case("narrow_fused_ft_bf16_audio", 6, "mmb_mm2_stream_project_narrow_ft", 300, 112, 4, 64, "audio",
                   fbytes=2, v=3016),
        # 7: mmb_sif_wavg, wave (L <= 64) and workgroup (L = 65) routes
        wavg_out_case("wavg_out_wave", 1),
        wavg_out_case("wavg_out_wg", 65),
        table_case("wavg_table", 7, "mmb_sif_wavg", 512, rows_past(B32, 512 * 4), mm2=False),
        table_case("wavg_tt_bf16", 7, "mmb_sif_wavg_tt", 512, rows_past(B32, 512 * 2), tbytes=2, mm2=False),
        # 8: the Gram routes that a large operand can reach (gram_small_kernel takes n <= 4096 only)
        gram_case("gram_tri", "mmb_gram", 320),
        gram_case("gram_tri_cnt", "mmb_gram", 320, cnt=True),
        gram_case("gram_generic", "mmb_gram", 512),
        gram_case("gram_f64", "mmb_gram_f64", 512, esize=8),
        gram_case("gram_part_finish", "mmb_gram_part", 320),
        gram_case("gram_i8", "mmb_gram_i8", 304),
        # 9: the removals
        remove_case("remove1", "mmb_pc_remove", 512, 1),
        remove_case("remove_npc2", "mmb_pc_remove", 512, 2),
        remove_case("remove_scalar", "mmb_pc_remove", 511, 1),
        remove_case("remove_f64_out", "mmb_pc_remove", 512, 2, out_bytes=8),
        remove_case("remove_f64_rows_npc1", "mmb_pc_remove_f64", 512, 1, in_bytes=8, out_bytes=8, cnt=False),
        remove_case("remove_f64_rows_npc2", "mmb_pc_remove_f64", 512, 2, in_bytes=8, out_bytes=8, cnt=False),
        # 10: the projections
        project_case("project_f32", "mmb_mm2_project", s_half=False),
        project_case("project_x3", "mmb_mm2_project_x3", s_half=True, rmpc=True, split=True),
    ]
    cases += _regressor_cases() + _latent_cases() + [_word_case()]
    return collections.OrderedDict((c.name, c) for c in cases)


CASES = _build()


def names(family=None, entry=None):
    return [c.name for c in CASES.values()
            if (family is None or c.family == family) and (entry is None or c.entry == entry)]


# the guards of the issue's table: (guard, accepted side, refused side) as the tests that hold them
GUARDS = [
    ("narrow_ok (sif_kernels.hip): V D 4 < 2^31", "test_gpu_large::test_word_table[table_narrow_last]",
     "test_gpu_large::test_word_table[table_narrow_refused]"),
    ("fused_pipe_ok (mmb_fused.h): V D 4 < 2^31", "test_gpu_large::test_fused_table_guard (V = 2^21 - 1)",
     "test_gpu_large::test_fused_table_guard (V = 2^21)"),
    ("gram_i8l_block: chunk d 4 < 2^31", "test_gpu_large::test_gram_i8",
     "not reachable: test_large_cases::test_int8_gram_guard_is_not_reachable"),
    ("mmb_mm2_stream_project_narrow: n < 2^31 - 32", "test_gpu_large::test_narrow_fused[narrow_fused_x]",
     "test_lib_abi::mmb_mm2_stream_project_narrow-n_2^31_-_32"),
    ("split_stream: n (Pt + 2 Pf) <= 2^31 - 1", "test_gpu_large::test_split_stream",
     "test_lib_abi::mmb_mm2_stream_split-grid_past_2^31_-_1"),
    ("mmb_mm2_project_x3_split: tiles nsl <= 2^31 - 1", "test_gpu_large::test_project_x3",
     "test_lib_abi::mmb_mm2_project_x3_split-grid_past_2^31_-_1"),
    ("mmb_layer_norm_backward: rb + cb < 2^31", "test_gpu_large::test_layer_norm_backward_dgamma",
     "test_lib_abi::mmb_layer_norm_backward"),
]
