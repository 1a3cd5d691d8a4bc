"""Device-resident hot path: SIF (a1-a5) and closed-form MMB2 (a6-a8) on HBM tensors.

Every function here takes and returns torch device tensors and calls libmmb
through its C ABI on the current stream; nothing is synchronised.  The
reference-signature mirrors (`sif_functions.py`, `sif.py`, `sif2.py`) and
`bench.py` are thin layers over these.

Data layout in HBM (one utterance per row, row-major, fp32 unless noted):
  table [V, D], wtab [V] (f32 rounding of the f64 SIF weights), ids [N, L] int32,
  audio [N, T, A], visual [N, T, Vd]                                  (inputs)
  x [N, D]     a2 rows (weighted text sum / count)   s [N, Kp] frame sums   aux [3, N]
  G [D, D] f64 Gram   pc [npc, D] f64                                  (intermediates)
  sif [N, D] (f32 or f64)   mmb2 [N, D]                               (outputs)
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

import mmb_lib as L
from models import MMB2_KEYS

N_OVERSAMPLES = 10  # sklearn randomized_svd default (extmath.py:535)
N_ITER = 7          # TruncatedSVD(n_iter=7), sif_functions.py:65
PC_SEED = 0         # random_state=0, sif_functions.py:65

_omega_cache: dict = {}


def omega(rows: int, k: int, device) -> torch.Tensor:
    """RandomState(0).normal(size=(rows, k)) as f64 on `device` (cached)."""
    key = (rows, k, str(device))
    t = _omega_cache.get(key)
    if t is None:
        host = L.host_randn(PC_SEED, rows * k).reshape(rows, k)
        t = torch.from_numpy(host).to(device)
        if len(_omega_cache) > 16:
            _omega_cache.clear()
        _omega_cache[key] = t
    return t


def narrow_ids(ids: torch.Tensor) -> torch.Tensor:
    """int64 reference ids -> int32 device ids (range-checked)."""
    if ids.dtype == torch.int32:
        return ids.contiguous()
    if ids.numel():
        lo, hi = int(ids.min()), int(ids.max())
        if lo < -(2 ** 31) or hi >= 2 ** 31:
            raise IndexError("token id out of int32 range")
    return ids.to(torch.int32).contiguous()


MAX_NPC = 16 - N_OVERSAMPLES  # the device solver keeps the k = npc + 10 block in 16 columns


def check_npc(npc: int):
    if not 1 <= npc <= MAX_NPC:
        raise ValueError(f"npc={npc}: the device PC solver supports 1 <= npc <= {MAX_NPC} "
                         f"(randomized-SVD block npc + {N_OVERSAMPLES} <= 16 columns)")


def check_flag(flag: torch.Tensor, V: int, zero_weights: bool = False):
    """Raise like the reference for what the kernels reported in `flag`:
    IndexError for an id >= V (numpy fancy indexing); with `zero_weights`,
    ValueError for an utterance whose weights are all 0 -- its a2 row is
    0/0 = NaN (sif_functions.py:55) and the reference's TruncatedSVD rejects
    the split (sklearn check_array: "Input X contains NaN")."""
    check_flag_bits(int(flag.item()), V, zero_weights)


def check_flag_bits(f: int, V: int, zero_weights: bool = False):
    """check_flag on flag bits already read back."""
    if f & L.MMB_FLAG_SYNC_TIMEOUT:
        raise RuntimeError("a bounded in-kernel hand-over timed out (mmb_mm2_stream_project's "
                           "streaming / projecting waves, or mmb_pc_solve_mc's workgroups); "
                           "the step's MMB2 rows or PC are invalid")
    if f & L.MMB_FLAG_ID_RANGE:
        raise IndexError(f"token id out of bounds for a vocabulary of size {V}")
    if zero_weights and f & L.MMB_FLAG_ZERO_WEIGHTS:
        raise ValueError("Input X contains NaN: an utterance whose SIF weights are all 0 has a "
                         "0/0 weighted average (sif_functions.py:55), which the reference's "
                         "TruncatedSVD rejects (sif_functions.py:65-67)")


# status word of a checked step: the flag bits | PC_NONFINITE (FusedStep.status)
PC_NONFINITE = 1 << 16


# ------------------------------------------------------------------ a1
def seq2weight(seq32: torch.Tensor, sel: torch.Tensor | None, wtab64: torch.Tensor,
               flag: torch.Tensor | None = None) -> torch.Tensor:
    n, l = seq32.shape
    w = torch.empty((n, l), dtype=torch.float32, device=seq32.device)
    L.call("mmb_seq2weight", L.ptr(seq32, L.I32), L.ptr(sel, L.U8), n, l, L.ptr(wtab64, L.F64),
           wtab64.numel(), L.ptr(w, L.F32), L.ptr(flag, L.I32), L.stream_ptr())
    return w


# Storage types of the word table: the name step_plan and FusedStep use ->
# (torch dtype, the table_type of mmb_sif_wavg_tt / mmb_mm2_stream_tt).  The
# 16-bit kinds are read by the SIF gather, the plain stream kernels, the split
# stream, the fused stream + projection kernel and the builder of the narrow
# fused kernel's text cache (weighted_sum, sif_embeddings, mm2_stream,
# mm2_stream_split_tt, mm2_stream_project_tt, mm2_stream_project_narrow_tt with
# MMB2Projection.enable_text_cache(table16=True)); nothing here converts a table.
TABLE_KINDS = {"f32": (torch.float32, L.MMB_TABLE_F32),
               "f16": (torch.float16, L.MMB_TABLE_F16),
               "bf16": (torch.bfloat16, L.MMB_TABLE_BF16)}
_TABLE_KIND_OF = {dtype: kind for kind, (dtype, _) in TABLE_KINDS.items()}  # (one lookup on the eager paths)


def table_kind(table: torch.Tensor, who: str = "mm2_stream") -> str:
    """The TABLE_KINDS name of a word table; MMBError for a dtype the kernels
    do not read (before any launch: the C ABI takes a bare pointer and would
    read the bytes as another type, past the end of a narrower buffer)."""
    kind = _TABLE_KIND_OF.get(table.dtype)
    if kind is None:
        raise L.MMBError(f"{who}: the word table must be float32, float16 or bfloat16, not {table.dtype}")
    return kind


def _f32_table(table, who: str) -> None:
    """The check of every mirror whose kernel reads the table as f32."""
    if table is not None and table_kind(table, who) != "f32":
        raise L.MMBError(f"{who} reads a float32 word table only, not {table.dtype}: a 16-bit table "
                         f"takes mm2_stream (the two-kernel step)")


# ------------------------------------------------------------------ a1+a2
def weighted_sum(table: torch.Tensor, ids32: torch.Tensor, w: torch.Tensor | None = None,
                 wtab32: torch.Tensor | None = None, flag: torch.Tensor | None = None,
                 x_out: bool = False):
    """Returns (num [N,D], cnt [N]) or x [N,D] (= num/cnt) if x_out.  `table`
    may be float16 or bfloat16 instead of float32 (mmb_sif_wavg_tt): the
    outputs are bit for bit those of the same table upcast to float32."""
    n, l = ids32.shape
    V, D = table.shape
    dev = table.device
    kind = table_kind(table, "weighted_sum")
    # the entry point and its table arguments: a 16-bit table carries its type
    entry, tab = (("mmb_sif_wavg", (L.ptr(table, L.F32),)) if kind == "f32" else
                  ("mmb_sif_wavg_tt", (L.ptr(table, L.TABLE), TABLE_KINDS[kind][1])))
    if x_out:
        x = torch.empty((n, D), dtype=torch.float32, device=dev)
        L.call(entry, *tab, V, D, L.ptr(ids32, L.I32), n, l, L.ptr(w, L.F32), L.ptr(wtab32, L.F32),
               L.ptr(x, L.F32), None, None, L.ptr(flag, L.I32), L.stream_ptr())
        return x
    num = torch.empty((n, D), dtype=torch.float32, device=dev)
    cnt = torch.empty((n,), dtype=torch.float32, device=dev)
    L.call(entry, *tab, V, D, L.ptr(ids32, L.I32), n, l, L.ptr(w, L.F32), L.ptr(wtab32, L.F32),
           None, L.ptr(num, L.F32), L.ptr(cnt, L.F32), L.ptr(flag, L.I32), L.stream_ptr())
    return num, cnt


# ------------------------------------------------------------------ a3
class GramWorkspace:
    """Scratch for mmb_gram sized for up to `n` rows (re-used across calls)."""

    def __init__(self, n: int, d: int, device):
        nbytes = L.query("mmb_gram_workspace_bytes", n, d)
        self.buf = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=device)
        self.n, self.d = n, d

    def fits(self, n, d):
        return L.query("mmb_gram_workspace_bytes", n, d) <= self.buf.numel()


def gram(num: torch.Tensor, cnt: torch.Tensor | None, G: torch.Tensor | None = None,
         accumulate: bool = False, ws: GramWorkspace | None = None) -> torch.Tensor:
    n, d = num.shape
    if G is None:
        G = torch.empty((d, d), dtype=torch.float64, device=num.device)
    if ws is None or not ws.fits(n, d):
        ws = GramWorkspace(n, d, num.device)
    L.call("mmb_gram", L.ptr(num, L.F32), L.ptr(cnt, L.F32), n, d, L.ptr(G, L.F64), int(accumulate),
           L.ptr(ws.buf, L.BYTES), L.stream_ptr())
    return G


def colmax(x: torch.Tensor, out: torch.Tensor | None = None, accumulate: bool = False):
    """Column bounds max_i |x[i, j]| as float bits (int32 view of uint32) for
    the int8 Gram (mmb_colmax)."""
    n, d = x.shape
    L.check_grid("colmax", n, 256)
    if out is None:
        out = torch.empty((d,), dtype=torch.int32, device=x.device)
    L.call("mmb_colmax", L.ptr(x, L.F32), n, d, L.ptr(out, L.I32), int(accumulate), L.stream_ptr())
    return out


def gram_i8(x: torch.Tensor, cmax: torch.Tensor, G: torch.Tensor | None = None,
            accumulate: bool = False, ws: GramWorkspace | None = None) -> torch.Tensor:
    """G = x^T x on the int8 matrix pipe (mmb_gram_i8): 33-bit fixed point per
    column bound, ~1e-10 relative to the exact f64 Gram."""
    n, d = x.shape
    if G is None:
        G = torch.empty((d, d), dtype=torch.float64, device=x.device)
    if ws is None or not ws.fits(n, d):
        ws = GramWorkspace(n, d, x.device)
    L.call("mmb_gram_i8", L.ptr(x, L.F32), L.ptr(cmax, L.I32), n, d, L.ptr(G, L.F64), int(accumulate),
           L.ptr(ws.buf, L.BYTES), L.stream_ptr())
    return G


def xt_omega(num, cnt, omega_rows: torch.Tensor) -> torch.Tensor:
    n, d = num.shape
    k = omega_rows.shape[1]
    z0 = torch.empty((d, k), dtype=torch.float64, device=num.device)
    L.call("mmb_xt_omega", L.ptr(num, L.F32), L.ptr(cnt, L.F32), n, d, L.ptr(omega_rows, L.F64), k,
           L.ptr(z0, L.F64), L.stream_ptr())
    return z0


PC_SOLVE_MC_MAX_D = 320  # mmb_pc_solve_mc: ceil(d / 16) workgroups, k <= 16
_solve_ws: dict = {}


def solve_workspace(d: int, device) -> torch.Tensor:
    """Scratch of mmb_pc_solve_mc (the tiles exchanged between its
    workgroups), one per (d, device, current stream): a call owns it until
    it completes, and calls on one stream are ordered."""
    key = (d, str(device), L.stream_ptr())
    ws = _solve_ws.get(key)
    if ws is None:  # zeroed once: a completed solve leaves its control words zero
        ws = torch.zeros(L.query("mmb_pc_solve_mc_ws_bytes", d), dtype=torch.uint8, device=device)
        if len(_solve_ws) > 16:
            _solve_ws.clear()
        _solve_ws[key] = ws
    return ws


def pc_solve(G: torch.Tensor, z0: torch.Tensor, npc: int, transposed: bool,
             n_iter: int = N_ITER, out: torch.Tensor | None = None,
             flag: torch.Tensor | None = None, ws: torch.Tensor | None = None) -> torch.Tensor:
    """sklearn's randomized-SVD components from the Gram (a3's solve).  d <=
    320: the multi-workgroup solver (mmb_pc_solve_mc); larger d: one
    workgroup.  A hand-over timeout of the multi-workgroup solver leaves NaN
    in the PC and sets MMB_FLAG_SYNC_TIMEOUT in `flag`: a caller that passes
    its own flag (FusedStep, graph-capturable) checks it later; without one,
    this call checks a flag of its own and raises here (one host sync)."""
    d = G.shape[0]
    if z0.shape[1] > d:
        # a block wider than the space (d < npc + 10): its first d columns
        # span the same subspace -- generically all of R^d, or X's whole row
        # space in the transposed branch -- so the PC is the exact one, as
        # sklearn's is there; the kernels' k x k factors need k <= d
        z0 = z0[:, :d].contiguous()
    k = z0.shape[1]
    pc = out if out is not None else torch.empty((npc, d), dtype=torch.float64, device=G.device)
    if d <= PC_SOLVE_MC_MAX_D and k <= 16:
        if ws is None:
            ws = solve_workspace(d, G.device)
        own = flag is None
        if own:
            flag = torch.zeros(1, dtype=torch.int32, device=G.device)
        L.call("mmb_pc_solve_mc", L.ptr(G, L.F64), d, L.ptr(z0, L.F64), k, npc, n_iter, int(transposed),
               L.ptr(pc, L.F64), L.ptr(ws, L.BYTES), L.ptr(flag, L.I32), L.stream_ptr())
        if own and int(flag.item()) & L.MMB_FLAG_SYNC_TIMEOUT:
            ws[:16].zero_()  # an aborted solve leaves its control words set
            raise RuntimeError("mmb_pc_solve_mc: a bounded hand-over between the solver's "
                               "workgroups timed out; the PC is invalid (NaN)")
    else:
        L.call("mmb_pc_solve", L.ptr(G, L.F64), d, L.ptr(z0, L.F64), k, npc, n_iter, int(transposed),
               L.ptr(pc, L.F64), L.stream_ptr())
    return pc


# ------------------------------------------------------------------ a4
def remove_pc(num, cnt, pc: torch.Tensor, out_dtype=torch.float32, out=None) -> torch.Tensor:
    n, d = num.shape
    if out is None:
        out = torch.empty((n, d), dtype=out_dtype, device=num.device)
    if out.dtype not in (torch.float32, torch.float64):
        raise L.MMBError(f"remove_pc writes float32 or float64 rows, not {out.dtype}")
    L.call("mmb_pc_remove", L.ptr(num, L.F32), L.ptr(cnt, L.F32), n, d, L.ptr(pc, L.F64), pc.shape[0],
           L.ptr(out, L.F32) if out.dtype == torch.float32 else None,
           L.ptr(out, L.F64) if out.dtype == torch.float64 else None, L.stream_ptr())
    return out


# ------------------------------------------------------------------ a3/a4 on float64 X
def pc_f64(x64: torch.Tensor, npc: int) -> torch.Tensor:
    """PC of a float64 X [n, d] that is not f32-representable (the numpy
    drop-ins' general input): Gram, start block and solve all read f64 rows."""
    check_npc(npc)
    n, d = x64.shape
    G = torch.empty((d, d), dtype=torch.float64, device=x64.device)
    ws = GramWorkspace(n, d, x64.device)
    L.call("mmb_gram_f64", L.ptr(x64, L.F64), n, d, L.ptr(G, L.F64), 0, L.ptr(ws.buf, L.BYTES), L.stream_ptr())
    z0, transposed = pc_start_block(x64, None, npc, n, ops=F64Ops)
    return pc_solve(G, z0, npc, transposed)


def xt_omega_f64(x64, cnt, omega_rows: torch.Tensor) -> torch.Tensor:
    n, d = x64.shape
    k = omega_rows.shape[1]
    z0 = torch.empty((d, k), dtype=torch.float64, device=x64.device)
    L.call("mmb_xt_omega_f64", L.ptr(x64, L.F64), n, d, L.ptr(omega_rows, L.F64), k, L.ptr(z0, L.F64),
           L.stream_ptr())
    return z0


def remove_pc_f64(x64: torch.Tensor, pc: torch.Tensor) -> torch.Tensor:
    n, d = x64.shape
    out = torch.empty((n, d), dtype=torch.float64, device=x64.device)
    L.call("mmb_pc_remove_f64", L.ptr(x64, L.F64), n, d, L.ptr(pc, L.F64), pc.shape[0], L.ptr(out, L.F64),
           L.stream_ptr())
    return out


class DeviceOps:
    """The libmmb kernels global_pc() composes (tests substitute CPU doubles)."""

    gram = staticmethod(lambda num, cnt, G=None, ws=None: gram(num, cnt, G, ws=ws))
    omega = staticmethod(omega)
    xt_omega = staticmethod(xt_omega)
    pc_solve = staticmethod(pc_solve)


class F64Ops(DeviceOps):
    """The start block of pc_f64: X^T Omega from float64 rows."""

    xt_omega = staticmethod(xt_omega_f64)


def pc_start_block(num, cnt, npc: int, n_total: int, row0: int = 0, ops=DeviceOps):
    """(Z0, transposed) of sklearn's randomized SVD from this rank's rows
    [row0, row0 + n) of X = num / cnt.  Direct branch: Omega [d, k].
    Transposed branch (n_total < d): X^T Omega_n over Omega's rows of this
    shard."""
    check_npc(npc)
    n, d = num.shape
    k = npc + N_OVERSAMPLES
    if n_total >= d:
        return ops.omega(d, k, num.device), False
    om = ops.omega(n_total, k, num.device)[row0:row0 + n].contiguous()
    return ops.xt_omega(num, cnt, om), True


def global_pc(num, cnt, npc: int, n_total: int, row0: int = 0, allreduce=None, ops=DeviceOps,
              G=None, ws=None):
    """The PC of ALL utterances across ranks (a3), from this rank's rows
    [row0, row0 + n) of X = num / cnt.

    Only the Gram (d x d f64) — and, in sklearn's transposed branch (fewer
    utterances than features), the start block X^T Omega (d x k) — cross
    ranks, each as one all-reduce (sum).  Every rank then runs the same
    deterministic solve, so the PC is identical everywhere with no broadcast.
    """
    check_npc(npc)
    G = ops.gram(num, cnt, G, ws)
    z0, transposed = pc_start_block(num, cnt, npc, n_total, row0, ops)
    if allreduce is not None:
        allreduce(G)
        if transposed:
            allreduce(z0)
    return ops.pc_solve(G, z0, npc, transposed)


def sif_embeddings(table, ids, wtab32=None, w=None, npc: int = 1, out_dtype=torch.float32,
                   check_ids: bool = True, allreduce=None, n_total=None, row0: int = 0):
    """a1-a5 fused on device: weighted average, Gram (+ optional all-reduce
    across ranks), randomized-SVD PC, removal.  Returns (emb [N,D], pc).
    `table` may be float16 or bfloat16 (weighted_sum); everything after the
    gather works on the f32 rows it writes."""
    ids32 = narrow_ids(ids)
    flag = torch.zeros(1, dtype=torch.int32, device=table.device)
    num, cnt = weighted_sum(table, ids32, w=w, wtab32=wtab32, flag=flag)
    n_total = num.shape[0] if n_total is None else n_total
    pc = global_pc(num, cnt, npc, n_total, row0, allreduce)
    out = remove_pc(num, cnt, pc, out_dtype)
    if not check_ids:  # the id-range bit is then not the caller's concern
        flag.bitwise_and_(~L.MMB_FLAG_ID_RANGE)
    check_flag(flag, table.shape[0], zero_weights=True)
    check_pc_finite(pc)
    return out, pc


def check_pc_finite(pc: torch.Tensor):
    """A NaN row on ANY rank reaches every rank's PC through the Gram
    all-reduce: checking the PC makes every rank raise, not only the one that
    holds the row."""
    if not bool(torch.isfinite(pc).all()):
        raise ValueError("Input X contains NaN or infinity: the split's Gram is not finite "
                         "(an all-zero-weight utterance on some rank, or non-finite inputs), "
                         "which the reference's TruncatedSVD rejects (sif_functions.py:65-67)")


# ------------------------------------------------------------------ a7 / a8
def calc_weights(x: torch.Tensor, b_mean: torch.Tensor, b_log_sigma: torch.Tensor):
    x = x.contiguous()
    f = x.shape[-1]
    qm = torch.empty_like(x)
    qs = torch.empty_like(x)
    L.call("mmb_calc_weights", L.ptr(x, L.F32), x.numel() // f, f, L.ptr(b_mean.contiguous(), L.F32),
           L.ptr(b_log_sigma.contiguous(), L.F32), L.ptr(qm, L.F32), L.ptr(qs, L.F32), L.stream_ptr())
    return qm, qs


def mm2_dims(d, a, vd):
    return L.query("mmb_mm2_k", d, a, vd), L.query("mmb_mm2_ldw", d)


# widest merged projection of libmmb (mmb_mm2_prepare / mmb_mm2_project: MMB_EINVAL past it)
PROJECT_MAX_LDW = 384


class MMB2Projection:
    """Merged [Kp, ldw] projection of the six generators (sif2.py:167-205)."""

    def __init__(self, networks: dict, d: int, a: int, vd: int, t: int, device):
        self.d, self.a, self.vd, self.t = d, a, vd, t
        self.kp, self.ldw = mm2_dims(d, a, vd)
        if self.ldw > PROJECT_MAX_LDW:
            raise L.MMBError(f"MMB2 projection: text width d = {d} (mmb_mm2_ldw(d) = {self.ldw}) is "
                             f"past the widest merged projection libmmb takes, d <= "
                             f"{PROJECT_MAX_LDW - 1} (ldw <= {PROJECT_MAX_LDW})")
        self.wm = torch.empty((self.kp, self.ldw), dtype=torch.float32, device=device)
        self.c0 = torch.empty((self.ldw,), dtype=torch.float32, device=device)
        nbytes = L.query("mmb_mm2_split_bytes", d, a, vd)
        self.wsplit = torch.empty((nbytes + 15) // 16 * 16, dtype=torch.uint8, device=device)
        self.device = device
        self.networks = {k: networks[k] for k in MMB2_KEYS}  # KeyError like sif2.py:182
        self.refresh()

    def _live(self):
        """The generators' current parameter tensors (w_mu, b_mu, w_ls, b_ls per key)."""
        return [(mu.weight, mu.bias, ls.weight, ls.bias)
                for mu, ls in (self.networks[k] for k in MMB2_KEYS)]

    def _versions(self):
        # storage address + version counter of every parameter: an optimiser
        # step (in place) bumps the counter, `p.data = t` moves the address
        # (and of the word / weight tables behind the text cache)
        live = [t for ps in self._live() for t in ps]
        if getattr(self, "text_src", None) is not None:
            live += list(self.text_src)
        return tuple((t.data_ptr(), t._version) for t in live)

    def invalidate(self):
        """Force a re-merge at the next refresh_if_changed(): needed after
        writes that neither bump a parameter's version counter nor move its
        storage (e.g. `p.data.copy_(...)`, which bypasses autograd's counter)."""
        self._seen = None

    def refresh(self):
        self.params = [tuple(p.detach().to(device=self.device, dtype=torch.float32).contiguous()
                             for p in ps) for ps in self._live()]
        arr = lambda i: (ctypes_ptr_array([L.ptr(p[i], L.F32) for p in self.params]))
        L.call("mmb_mm2_prepare", arr(0), arr(1), arr(2), arr(3), self.d, self.a, self.vd, self.t,
               L.ptr(self.wm, L.F32), self.ldw, L.ptr(self.c0, L.F32), L.ptr(self.wsplit, L.BYTES), L.stream_ptr())
        if getattr(self, "wpieces", None) is not None:
            L.call("mmb_mm2_split_pieces", L.ptr(self.wm, L.F32), self.d, self.a, self.vd, self.ldw,
                   L.ptr(self.wpieces, L.BYTES), L.stream_ptr())
        if getattr(self, "text_cache", None) is not None:
            self._build_text_cache()
        self._seen = self._versions()

    def enable_text_cache(self, table: torch.Tensor, wtab32: torch.Tensor, *, table16: bool = False):
        """Also keep the text cache of the narrow fused step
        (mmb_mm2_text_cache: P = E Wm_t1 + E^2 Wm_t2 per word, f64 rounded
        once, and the hot-word ranks), rebuilt with every re-merge and when
        the word or weight table changes.  The narrow fused kernel reads the
        token weights from the cache's own copy, so the cache is keyed on BOTH
        tensors (identity here, storage address + version counter in
        refresh_if_changed); writes into them that bump neither (raw-pointer
        writes by other libmmb kernels, `t.data.copy_`) need invalidate().
        The cache is built from a float32 table only -- unless `table16=True`
        opts in to a float16 / bfloat16 table (mmb_mm2_text_cache_tt: the
        cache, float32 either way, is byte for byte that of the table upcast
        to float32; the mirror of mmb_mm2_stream_project_narrow_tt asks for it)."""
        if not table16 or table_kind(table, "MMB2Projection.enable_text_cache") == "f32":
            _f32_table(table, "MMB2Projection.enable_text_cache")
        src = getattr(self, "text_src", None)
        if (getattr(self, "text_cache", None) is None or src[0] is not table
                or src[1] is not wtab32):
            self.enable_pieces()
            V = table.shape[0]
            nbytes = (L.query("mmb_mm2_text_cache_bytes", V, self.d) + 15) // 16 * 16
            old = getattr(self, "text_cache", None)
            if old is None or old.numel() != nbytes or old.device != table.device:
                self.text_cache = torch.empty(nbytes, dtype=torch.uint8, device=table.device)
            self.text_src = (table, wtab32)
            self._build_text_cache()
            self._seen = self._versions()

    def _build_text_cache(self):
        table, wtab32 = self.text_src
        tkind = table_kind(table, "MMB2Projection.enable_text_cache")
        if tkind != "f32":  # (enable_text_cache(table16=True) let it in)
            L.call("mmb_mm2_text_cache_tt", L.ptr(table, L.TABLE), TABLE_KINDS[tkind][1], table.shape[0], self.d,
                   L.ptr(wtab32, L.F32), L.ptr(self.wm, L.F32), self.ldw, L.ptr(self.text_cache, L.BYTES),
                   L.stream_ptr())
            return
        L.call("mmb_mm2_text_cache", L.ptr(table, L.F32), table.shape[0], self.d, L.ptr(wtab32, L.F32),
               L.ptr(self.wm, L.F32), self.ldw, L.ptr(self.text_cache, L.BYTES), L.stream_ptr())

    def enable_pieces(self):
        """Also keep the piece-ordered split of wm (mmb_mm2_split_pieces), the
        B operand of the fused stream + projection kernel."""
        if getattr(self, "wpieces", None) is None:
            nbytes = L.query("mmb_mm2_split_pieces_bytes", self.d, self.a, self.vd)
            self.wpieces = torch.empty((nbytes + 15) // 16 * 16, dtype=torch.uint8,
                                       device=self.wm.device)
            L.call("mmb_mm2_split_pieces", L.ptr(self.wm, L.F32), self.d, self.a, self.vd, self.ldw,
                   L.ptr(self.wpieces, L.BYTES), L.stream_ptr())

    def refresh_if_changed(self) -> bool:
        """Re-merge only when a generator parameter changed since the last
        merge (torch's version counters -- an optimiser step bumps them -- or
        a parameter's storage moved), so a step over a new batch with the same
        weights skips the five prepare launches.  Writes through `p.data`
        bump no counter: call invalidate() after them.  Returns whether it
        re-merged."""
        if getattr(self, "_seen", None) == self._versions():
            return False
        self.refresh()
        return True


def ctypes_ptr_array(ptrs):
    import ctypes

    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def split_parts(n: int, t: int) -> int:
    """Token / frame ranges per utterance of the few-long-rows stream path
    (mmb_mm2_stream_split_parts: a text, an audio and a visual workgroup per
    range, about one workgroup per CU in all)."""
    return int(L.query("mmb_mm2_stream_split_parts", n, t))


def split_ws(n: int, t: int, d: int, a: int, vd: int, device, parts: int = 0) -> torch.Tensor:
    """Scratch of mmb_mm2_stream_split (its per-range partial rows)."""
    nb = int(L.query("mmb_mm2_stream_split_ws_bytes", n, t, d, a, vd, parts))
    return torch.empty(max(nb, 16), dtype=torch.uint8, device=device)


# widest modality row of the stream kernels (mmb_mm2_stream: MMB_EINVAL past it)
STREAM_MAX_VECTOR_WIDTH, STREAM_MAX_SCALAR_WIDTH = 1280, 320

# Storage types of the audio / visual frames: the name step_plan and StepPlan
# use -> (torch dtype, mmb_mm2_stream_ft's frame_type).  The 16-bit kinds are
# read by the stream kernels only (mm2_stream); nothing here converts a frame.
FRAME_KINDS = {"f32": (torch.float32, L.MMB_FRAMES_F32),
               "f16": (torch.float16, L.MMB_FRAMES_F16),
               "bf16": (torch.bfloat16, L.MMB_FRAMES_BF16)}


def frame_kind(audio: torch.Tensor, visual: torch.Tensor, who: str = "mm2_stream") -> str:
    """The FRAME_KINDS name of a pair of frame tensors; MMBError for a dtype
    the kernels do not read or a mismatched pair (before any launch: the C
    ABI takes bare pointers and would read the bytes as another type)."""
    if audio.dtype != visual.dtype:
        raise L.MMBError(f"{who}: audio is {audio.dtype} and visual {visual.dtype}; both frame "
                         f"tensors must have one dtype")
    for kind, (dtype, _) in FRAME_KINDS.items():
        if audio.dtype == dtype:
            return kind
    raise L.MMBError(f"{who}: frames must be float32, float16 or bfloat16, not {audio.dtype}")


def _stream_outputs(who: str, kind: str, n, d, a, vd, audio, visual, text_src, out, s_half: bool, colmax_ws,
                    text_kind: str = "f32"):
    """(x, s, aux) of mm2_stream and mm2_stream_split_ft -- `out` if given,
    else allocated -- after the checks both make before the call: the widths
    against the stream kernels' limits, the s buffer's dtype, the column-bound
    workspace's size.  `text_kind`: the TABLE_KINDS name of the text source."""
    # a vector row: whole 4-element units from a base aligned to one unit
    # (16 bytes of f32; 8 bytes of a 16-bit frame or table type)
    unit = 16 if kind == "f32" else 8
    text_unit = 16 if text_kind == "f32" else 8
    for what, w, src, al in (("text", d, text_src, text_unit), ("audio", a, audio, unit),
                             ("visual", vd, visual, unit)):
        vec = w % 4 == 0 and src is not None and src.data_ptr() % al == 0
        if w > (STREAM_MAX_VECTOR_WIDTH if vec else STREAM_MAX_SCALAR_WIDTH):
            raise L.MMBError(f"{who}: {what} width {w} is past the stream kernels' limit: "
                             f"{STREAM_MAX_VECTOR_WIDTH} for rows of whole float4 units (width % 4 "
                             f"== 0, 16-byte aligned; 8-byte for 16-bit frames or a 16-bit table), "
                             f"{STREAM_MAX_SCALAR_WIDTH} otherwise")
    if out is None:
        dev = audio.device
        out = (torch.empty((n, d), dtype=torch.float32, device=dev),
               s_buffer(n, mm2_dims(d, a, vd)[0], s_half, dev),
               torch.empty((3, n), dtype=torch.float32, device=dev))
    if out[1].dtype != (torch.float16 if s_half else torch.float32):
        raise L.MMBError("s buffer dtype does not match s_half")
    _check_colmax_ws(colmax_ws, d)
    return out


def mm2_stream(n, t, d, a, vd, audio, visual, ids32=None, table=None, wtab32=None,
               text_dense=None, emb_dense=None, w_dense=None, flag=None, out=None,
               s_half: bool = True, colmax=None, colmax_ws=None, split=None, parts: int = 0):
    """a6-a8 frame sums.  Returns (x, s, aux): x [n, d] the a2 rows (weighted
    text sum / count_nonzero(w)), aux [3, n] (count, total weight, row scale).
    s_half=True (default) writes s as fp16 [n, 2*kp] (hi | lo planes of the
    row-scaled sums, the x3 projection's A operand); s_half=False writes fp32
    [n, kp] for the fp32-MFMA projection.  With `colmax` ([d] int32) and
    `colmax_ws` (mmb_mm2_colmax_ws_bytes) the kernel also writes the column
    bounds max_i |x[i, j]| (float bits) for mmb_gram_i8.  With `split` (a
    split_ws scratch) every utterance's tokens / frames are cut into `parts`
    ranges (0: split_parts) summed by their own workgroups, then added in
    part order (mmb_mm2_stream_split: a few long rows, POM's splits).

    `audio` / `visual` may both be float16 or both bfloat16 instead of float32
    (mmb_mm2_stream_ft; gathered text, no `split`): the outputs are bit for bit
    those of the same frames upcast to float32 (with `split`:
    mm2_stream_split_ft).

    `table` may be float16 or bfloat16 instead of float32 (mmb_mm2_stream_tt;
    gathered text, no `split`, frames of any of the three dtypes): the outputs
    are bit for bit those of the same table upcast to float32."""
    kind = frame_kind(audio, visual)
    tkind = table_kind(table) if table is not None else "f32"
    if kind != "f32" and ids32 is None:
        raise L.MMBError(f"mm2_stream: {kind} frames go with gathered text (ids32 + table) only")
    if kind != "f32" and split is not None:
        raise L.MMBError(f"mm2_stream: the split stream reads float32 frames only, not {kind}")
    if tkind != "f32" and ids32 is None:
        raise L.MMBError(f"mm2_stream: a {tkind} word table goes with gathered text (ids32 + table) only; "
                         f"dense text is float32 and reads no table")
    if tkind != "f32" and split is not None:
        raise L.MMBError(f"mm2_stream: the split stream reads a float32 word table only, not {tkind}")
    text_src = table if ids32 is not None else text_dense
    if s_half:  # (the workgroup route's fp16 pass: a workgroup per row)
        L.check_grid("mm2_stream", n)
    num, s, aux = _stream_outputs("mm2_stream", kind, n, d, a, vd, audio, visual, text_src, out, s_half,
                                  colmax_ws, text_kind=tkind)
    V = table.shape[0] if table is not None else 0
    # the arguments the three entry points share: the gathered text's, the
    # frames', and everything from the shapes on
    # (a 16-bit table or frame type reaches only the entry points that take its `void*`)
    table_t = L.F32 if tkind == "f32" else L.TABLE
    frame_t = L.F32 if kind == "f32" else L.FRAMES
    gathered = (L.ptr(ids32, L.I32), L.ptr(table, table_t), V, L.ptr(wtab32, L.F32))
    frames = (L.ptr(audio, frame_t), L.ptr(visual, frame_t))
    tail = (n, t, d, a, vd, L.ptr(num, L.F32), L.ptr(s, L.S_BUF), int(s_half), L.ptr(aux, L.F32),
            L.ptr(flag, L.I32), L.ptr(colmax, L.I32), L.ptr(colmax_ws, L.BYTES))
    text = (*gathered, L.ptr(text_dense, L.F32), L.ptr(emb_dense, L.F32), L.ptr(w_dense, L.F32))
    if split is not None:
        L.call("mmb_mm2_stream_split", *text, *frames, *tail, int(parts), L.ptr(split, L.BYTES),
               split.numel() * split.element_size(), L.stream_ptr())
    elif tkind != "f32":
        L.call("mmb_mm2_stream_tt", gathered[0], gathered[1], TABLE_KINDS[tkind][1], V, gathered[3],
               L.ptr(w_dense, L.F32), *frames, FRAME_KINDS[kind][1], *tail, L.stream_ptr())
    elif kind != "f32":
        L.call("mmb_mm2_stream_ft", *gathered, L.ptr(w_dense, L.F32), *frames, FRAME_KINDS[kind][1], *tail,
               L.stream_ptr())
    else:
        L.call("mmb_mm2_stream", *text, *frames, *tail, L.stream_ptr())
    return num, s, aux


def mm2_stream_split_ft(n, t, d, a, vd, audio, visual, ids32, table, wtab32=None, w_dense=None,
                        flag=None, out=None, s_half: bool = True, colmax=None, colmax_ws=None,
                        split=None, parts: int = 0):
    """mm2_stream's `split` route on frames of any FRAME_KINDS dtype
    (mmb_mm2_stream_split_ft; gathered text only): `audio` / `visual` may both
    be float16 or both bfloat16 -- a modality in 4-value units from an 8-byte
    aligned base at a width % 4 == 0, in scalar loads otherwise, never from an
    odd address -- and the outputs are bit for bit those of
    mm2_stream(..., split=, parts=) on the same frames upcast to float32.
    `split` is a split_ws scratch (None: allocated here for `parts`).
    Returns (x, s, aux)."""
    kind = frame_kind(audio, visual, "mm2_stream_split_ft")
    if ids32 is None:
        raise L.MMBError("mm2_stream_split_ft: gathered text (ids32 + table) only")
    _f32_table(table, "mm2_stream_split_ft")
    num, s, aux = _stream_outputs("mm2_stream_split_ft", kind, n, d, a, vd, audio, visual, table, out, s_half,
                                  colmax_ws)
    if split is None:
        split = split_ws(n, t, d, a, vd, audio.device, parts)
    V = table.shape[0] if table is not None else 0
    L.call("mmb_mm2_stream_split_ft", L.ptr(ids32, L.I32), L.ptr(table, L.F32), V, L.ptr(wtab32, L.F32),
           L.ptr(w_dense, L.F32), L.ptr(audio, L.FRAMES), L.ptr(visual, L.FRAMES), FRAME_KINDS[kind][1],
           n, t, d, a, vd, L.ptr(num, L.F32), L.ptr(s, L.S_BUF), int(s_half), L.ptr(aux, L.F32),
           L.ptr(flag, L.I32), L.ptr(colmax, L.I32), L.ptr(colmax_ws, L.BYTES), int(parts),
           L.ptr(split, L.BYTES), split.numel() * split.element_size(), L.stream_ptr())
    return num, s, aux


def mm2_stream_split_tt(n, t, d, a, vd, audio, visual, ids32, table, wtab32=None, w_dense=None,
                        flag=None, out=None, s_half: bool = True, colmax=None, colmax_ws=None,
                        split=None, parts: int = 0):
    """mm2_stream_split_ft on a word table of any TABLE_KINDS dtype as well
    (mmb_mm2_stream_split_tt; gathered text only, all nine pairs of table and
    frame dtypes): `table` may be float16 or bfloat16 -- the text in 4-value
    units from an 8-byte aligned base at d % 4 == 0, in scalar loads
    otherwise, never from an odd address -- and the outputs are bit for bit
    those of mm2_stream_split_ft with the same `parts` on the same table
    upcast to float32 (with one range: those of mm2_stream on the 16-bit
    table).  `split` is a split_ws scratch (None: allocated here for
    `parts`).  Returns (x, s, aux)."""
    who = "mm2_stream_split_tt"
    kind = frame_kind(audio, visual, who)
    if ids32 is None or table is None:
        raise L.MMBError(f"{who}: gathered text (ids32 + table) only; dense text is float32 and reads no table")
    tkind = table_kind(table, who)
    num, s, aux = _stream_outputs(who, kind, n, d, a, vd, audio, visual, table, out, s_half, colmax_ws,
                                  text_kind=tkind)
    if split is None:
        split = split_ws(n, t, d, a, vd, audio.device, parts)
    L.call("mmb_mm2_stream_split_tt", L.ptr(ids32, L.I32), L.ptr(table, L.TABLE), TABLE_KINDS[tkind][1],
           table.shape[0], L.ptr(wtab32, L.F32), L.ptr(w_dense, L.F32), L.ptr(audio, L.FRAMES),
           L.ptr(visual, L.FRAMES), FRAME_KINDS[kind][1], n, t, d, a, vd, L.ptr(num, L.F32), L.ptr(s, L.S_BUF),
           int(s_half), L.ptr(aux, L.F32), L.ptr(flag, L.I32), L.ptr(colmax, L.I32), L.ptr(colmax_ws, L.BYTES),
           int(parts), L.ptr(split, L.BYTES), split.numel() * split.element_size(), L.stream_ptr())
    return num, s, aux


# Narrowest frame row (floats) for which the fused stream + projection step is
# the default: its 4 streaming waves per CU load every modality row as 16-B
# columns on 64 lanes, so a frame row under 256 floats leaves lanes idle and
# costs as many load round trips as a full one, while the two-kernel step's
# stream kernel (one wave per utterance, no LDS ring) keeps more loads in
# flight.  Measured (r03t, tools/step_ab.py, 500k-1M utterances, ms per
# step fused / two-kernel): A = 76, Vd = 48 at T = 20 / 40 / 64: 12.3 / 8.0,
# 8.7 / 5.8, 11.9 / 7.8 (V = 3016); 6.6 / 4.2 (V = 400k, T = 20); A = Vd = 300
# at T = 30 / 40: 10.3 / 11.0, 12.2 / 12.7 (V = 400k).
FUSED_MIN_FRAME = 256


def fused_pays(a: int, vd: int) -> bool:
    return min(a, vd) >= FUSED_MIN_FRAME


def stream_project_supported(t: int, d: int, a: int, vd: int) -> bool:
    """Shapes the fused stream + projection kernel takes (t <= 64 frames,
    256 <= d < 320, widths % 4, k <= 1920): the bench / MOSI-like configs."""
    return bool(L.query("mmb_mm2_stream_project_supported", t, d, a, vd))


def narrow_fused_supported(t: int, d: int, a: int, vd: int, v: int) -> bool:
    """Shapes of the narrow fused kernel (mmb_mm2_stream_project_narrow):
    MOSI-like frame widths (4..128, kq(A) + kq(Vd) <= 256), 256 < d < 304,
    t <= 64, a word table of <= 16384 rows (its text cache)."""
    return bool(L.query("mmb_mm2_stream_project_narrow_supported", t, d, a, vd, v))


def _stream_project(entry: str, ft: bool, cache: bool, text: tuple, n, t, d, a, vd, audio, visual,
                    proj: "MMB2Projection", ids32, table, wtab32, flag, out, colmax, colmax_ws):
    """The one body of the four fused mirrors: the call of mmb_<entry>.  `ft`:
    the entry point takes frames of any FRAME_KINDS dtype (and their
    frame_type), else float32 frames only; `cache`: it reads the projection's
    text cache, else only its weight pieces; `text`: the entry point's own
    text arguments, between wtab32 (or the text cache) and audio."""
    kind = frame_kind(audio, visual, entry)
    _f32_table(table, entry)
    if not ft and kind != "f32":
        raise L.MMBError(f"{entry} reads float32 frames only, not {audio.dtype}: 16-bit frames "
                         f"take mm2_stream (the two-kernel step)")
    if ft and not cache and ids32 is None:  # (the narrow entry points: the C side's own check)
        raise L.MMBError(f"{entry}: gathered text (ids32 + table) only")
    if cache:
        proj.enable_text_cache(table, wtab32)
    else:
        proj.enable_pieces()
    num, aux, mmb2 = _fused_outputs(n, d, audio.device, out, colmax_ws)
    V = table.shape[0] if table is not None else 0
    frame_t = L.FRAMES if ft else L.F32  # (`const void*` with a frame_type, else `const float*`)
    L.call("mmb_" + entry, L.ptr(ids32, L.I32), L.ptr(table, L.F32), V, L.ptr(wtab32, L.F32),
           *([L.ptr(proj.text_cache, L.BYTES)] if cache else []), *[L.ptr(x, L.F32) for x in text],
           L.ptr(audio, frame_t), L.ptr(visual, frame_t), *([FRAME_KINDS[kind][1]] if ft else []),
           n, t, d, a, vd, L.ptr(proj.wpieces, L.BYTES), L.ptr(proj.c0, L.F32), L.ptr(num, L.F32),
           L.ptr(aux, L.F32), L.ptr(mmb2, L.F32), L.ptr(flag, L.I32), L.ptr(colmax, L.I32),
           L.ptr(colmax_ws, L.BYTES), L.stream_ptr())
    return num, aux, mmb2


def mm2_stream_project_narrow(n, t, d, a, vd, audio, visual, proj: "MMB2Projection", ids32,
                              table, wtab32, flag=None, out=None, colmax=None, colmax_ws=None):
    """a1-a8 at narrow frame widths in ONE kernel (mmb_mm2_stream_project_narrow):
    x, aux, the MMB2 rows (and the column bounds).  Returns (x, aux, mmb2)."""
    return _stream_project("mm2_stream_project_narrow", False, True, (), n, t, d, a, vd, audio, visual,
                           proj, ids32, table, wtab32, flag, out, colmax, colmax_ws)


def mm2_stream_project_narrow_ft(n, t, d, a, vd, audio, visual, proj: "MMB2Projection", ids32,
                                 table, wtab32, flag=None, out=None, colmax=None, colmax_ws=None):
    """mm2_stream_project_narrow on frames of any FRAME_KINDS dtype
    (mmb_mm2_stream_project_narrow_ft): `audio` / `visual` may both be float16
    or both bfloat16, from an 8-byte aligned base, and the outputs are bit for
    bit those of the same frames upcast to float32.  Returns (x, aux, mmb2)."""
    return _stream_project("mm2_stream_project_narrow_ft", True, True, (), n, t, d, a, vd, audio, visual,
                           proj, ids32, table, wtab32, flag, out, colmax, colmax_ws)


def mm2_stream_project_narrow_tt(n, t, d, a, vd, audio, visual, proj: "MMB2Projection", ids32,
                                 table, wtab32, flag=None, out=None, colmax=None, colmax_ws=None):
    """mm2_stream_project_narrow_ft on a word table of any TABLE_KINDS dtype as
    well (mmb_mm2_stream_project_narrow_tt; all nine pairs of table and frame
    dtypes): `table` may be float16 or bfloat16.  The kernel takes its text
    from the projection's text cache, built here from the 16-bit table
    (enable_text_cache(table16=True): byte for byte the cache of the upcast
    table), and never reads the table itself -- the outputs are bit for bit
    those of mm2_stream_project_narrow_ft on the same table upcast to
    float32.  Returns (x, aux, mmb2)."""
    who = "mm2_stream_project_narrow_tt"
    kind = frame_kind(audio, visual, who)
    if ids32 is None or table is None:
        raise L.MMBError(f"{who}: gathered text (ids32 + table) only; dense text is float32 and reads no table")
    tkind = table_kind(table, who)
    _check_colmax_ws(colmax_ws, d)  # (before the cache is built: a rejected call launches nothing)
    proj.enable_text_cache(table, wtab32, table16=True)
    num, aux, mmb2 = _fused_outputs(n, d, audio.device, out, colmax_ws)
    L.call("mmb_mm2_stream_project_narrow_tt", L.ptr(ids32, L.I32), L.ptr(table, L.TABLE), TABLE_KINDS[tkind][1],
           table.shape[0], L.ptr(wtab32, L.F32), L.ptr(proj.text_cache, L.BYTES), L.ptr(audio, L.FRAMES),
           L.ptr(visual, L.FRAMES), FRAME_KINDS[kind][1], n, t, d, a, vd, L.ptr(proj.wpieces, L.BYTES),
           L.ptr(proj.c0, L.F32), L.ptr(num, L.F32), L.ptr(aux, L.F32), L.ptr(mmb2, L.F32),
           L.ptr(flag, L.I32), L.ptr(colmax, L.I32), L.ptr(colmax_ws, L.BYTES), L.stream_ptr())
    return num, aux, mmb2


def mm2_stream_project(n, t, d, a, vd, audio, visual, proj: "MMB2Projection", ids32=None,
                       table=None, wtab32=None, text_dense=None, w_dense=None, flag=None,
                       out=None, colmax=None, colmax_ws=None):
    """a6-a8 in ONE kernel (mmb_mm2_stream_project): x, aux (and the column
    bounds) as mm2_stream, plus the MMB2 rows of mm2_project -- the sums s
    stay in LDS.  Returns (x, aux, mmb2)."""
    return _stream_project("mm2_stream_project", False, False, (text_dense, w_dense), n, t, d, a, vd,
                           audio, visual, proj, ids32, table, wtab32, flag, out, colmax, colmax_ws)


def mm2_stream_project_ft(n, t, d, a, vd, audio, visual, proj: "MMB2Projection", ids32, table,
                          wtab32, w_dense=None, flag=None, out=None, colmax=None, colmax_ws=None):
    """mm2_stream_project on frames of any FRAME_KINDS dtype
    (mmb_mm2_stream_project_ft; gathered text only): `audio` / `visual` may
    both be float16 or both bfloat16, from an 8-byte aligned base, and the
    outputs are bit for bit those of the same frames upcast to float32.
    Returns (x, aux, mmb2)."""
    return _stream_project("mm2_stream_project_ft", True, False, (w_dense,), n, t, d, a, vd, audio, visual,
                           proj, ids32, table, wtab32, flag, out, colmax, colmax_ws)


def mm2_stream_project_tt(n, t, d, a, vd, audio, visual, proj: "MMB2Projection", ids32, table,
                          wtab32, w_dense=None, flag=None, out=None, colmax=None, colmax_ws=None):
    """mm2_stream_project_ft on a word table of any TABLE_KINDS dtype as well
    (mmb_mm2_stream_project_tt; gathered text only, all nine pairs of table
    and frame dtypes): `table` may be float16 or bfloat16, from an 8-byte
    aligned base, and the outputs are bit for bit those of the same table
    upcast to float32.  Returns (x, aux, mmb2)."""
    who = "mm2_stream_project_tt"
    kind = frame_kind(audio, visual, who)
    if ids32 is None or table is None:
        raise L.MMBError(f"{who}: gathered text (ids32 + table) only; dense text is float32 and reads no table")
    tkind = table_kind(table, who)
    proj.enable_pieces()
    num, aux, mmb2 = _fused_outputs(n, d, audio.device, out, colmax_ws)
    L.call("mmb_mm2_stream_project_tt", L.ptr(ids32, L.I32), L.ptr(table, L.TABLE), TABLE_KINDS[tkind][1],
           table.shape[0], L.ptr(wtab32, L.F32), L.ptr(w_dense, L.F32), L.ptr(audio, L.FRAMES),
           L.ptr(visual, L.FRAMES), FRAME_KINDS[kind][1], n, t, d, a, vd, L.ptr(proj.wpieces, L.BYTES),
           L.ptr(proj.c0, L.F32), L.ptr(num, L.F32), L.ptr(aux, L.F32), L.ptr(mmb2, L.F32),
           L.ptr(flag, L.I32), L.ptr(colmax, L.I32), L.ptr(colmax_ws, L.BYTES), L.stream_ptr())
    return num, aux, mmb2


def _fused_outputs(n: int, d: int, device, out, colmax_ws):
    """(x, aux, mmb2) of the fused wrappers -- `out` if given, else allocated
    -- after the workspace's size check."""
    _check_colmax_ws(colmax_ws, d)
    if out is None:
        out = (torch.empty((n, d), dtype=torch.float32, device=device),
               torch.empty((3, n), dtype=torch.float32, device=device),
               torch.empty((n, d), dtype=torch.float32, device=device))
    return out


def _check_colmax_ws(colmax_ws, d: int) -> None:
    """The C ABI takes the workspace as a bare pointer; the mirror checks its
    size (mmb_mm2_colmax_ws_bytes grew by 16 bytes in r05, include/mmb.h)."""
    if colmax_ws is None:
        return
    need = int(L.query("mmb_mm2_colmax_ws_bytes", d))
    have = colmax_ws.numel() * colmax_ws.element_size()
    if have < need:
        raise L.MMBError(f"colmax_ws holds {have} bytes; mmb_mm2_colmax_ws_bytes({d}) = {need}")


def s_buffer(n: int, kp: int, s_half: bool, device) -> torch.Tensor:
    if s_half:
        return torch.empty((n, 2 * kp), dtype=torch.float16, device=device)
    return torch.empty((n, kp), dtype=torch.float32, device=device)


def x3_supported(proj: "MMB2Projection") -> bool:
    """The x3 kernel's LDS chunk rings fit d < 320 (the D=300 configs)."""
    return proj.ldw <= 320


def project_split_ws(n: int, kp: int, device, slices: int = 0):
    """Scratch of the split-K projection (mmb_mm2_project_x3_split), or None
    where the rows alone fill the chip (one slice)."""
    if int(L.query("mmb_mm2_project_x3_split_slices", n, kp)) < 2 and slices < 2:
        return None
    nb = int(L.query("mmb_mm2_project_x3_split_ws_bytes", n, kp, slices))
    return torch.empty(max(nb, 16), dtype=torch.uint8, device=device)


def mm2_project(s, num, aux, proj: MMB2Projection, out=None, pc=None, sif_out=None, split=None,
                slices: int = 0):
    """fp16 s (s_half stream output): the fp16 hi/lo split MFMA GEMM
    (mmb_mm2_project_x3); fp32 s: the fp32-MFMA GEMM.  Same epilogue.
    With `pc` ([1, D] f64) and `sif_out` the x3 kernel also writes the
    PC-removed a2 rows (mmb_mm2_project_x3_rmpc, fp16 s only).  With `split`
    (project_split_ws) a few rows' K loop runs over several workgroups per
    row tile (mmb_mm2_project_x3_split, fp16 s)."""
    n = num.shape[0]
    L.check_grid("mm2_project", n, 128 if s.dtype == torch.float16 else 64)
    if out is None:
        out = torch.empty((n, proj.d), dtype=torch.float32, device=num.device)
    if pc is not None and (s.dtype != torch.float16 or pc.shape[0] != 1 or sif_out is None):
        raise L.MMBError("fused PC removal needs fp16 s, npc = 1 and sif_out")
    if split is not None and s.dtype == torch.float16:
        L.call("mmb_mm2_project_x3_split", L.ptr(s, L.S_BUF), L.ptr(num, L.F32), L.ptr(aux, L.F32),
               L.ptr(proj.wsplit, L.BYTES), proj.ldw, L.ptr(proj.c0, L.F32), n, proj.kp, proj.d,
               L.ptr(out, L.F32), L.ptr(pc, L.F64), L.ptr(sif_out, L.F32), int(slices),
               L.ptr(split, L.BYTES), split.numel(), L.stream_ptr())
        return out
    if pc is not None:
        L.call("mmb_mm2_project_x3_rmpc", L.ptr(s, L.S_BUF), L.ptr(num, L.F32), L.ptr(aux, L.F32),
               L.ptr(proj.wsplit, L.BYTES), proj.ldw, L.ptr(proj.c0, L.F32), n, proj.kp, proj.d,
               L.ptr(out, L.F32), L.ptr(pc, L.F64), L.ptr(sif_out, L.F32), L.stream_ptr())
        return out
    if s.dtype == torch.float32:
        L.call("mmb_mm2_project", L.ptr(s, L.F32), L.ptr(num, L.F32), L.ptr(aux, L.F32), L.ptr(proj.wm, L.F32),
               proj.ldw, L.ptr(proj.c0, L.F32), n, proj.kp, proj.d, L.ptr(out, L.F32), L.stream_ptr())
    elif s.dtype == torch.float16:
        L.call("mmb_mm2_project_x3", L.ptr(s, L.S_BUF), L.ptr(num, L.F32), L.ptr(aux, L.F32),
               L.ptr(proj.wsplit, L.BYTES), proj.ldw, L.ptr(proj.c0, L.F32), n, proj.kp, proj.d,
               L.ptr(out, L.F32), L.stream_ptr())
    else:
        raise L.MMBError(f"unsupported s dtype {s.dtype}")
    return out


class _NullSpan:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


class _EventSpan:
    """Records a timing event pair on the current stream around a block."""

    def __init__(self, sink: list):
        self.sink = sink

    def __enter__(self):
        self.a = torch.cuda.Event(enable_timing=True)
        self.a.record()
        return self

    def __exit__(self, *exc):
        b = torch.cuda.Event(enable_timing=True)
        b.record()
        self.sink.append((self.a, b))
        return False


def side_cu_set(n_cu: int, side: int, layout: str = "balanced") -> list[int]:
    """CU-mask bits for the side stream of the overlapped step.

    strided: evenly spaced bits; high: the top `side` bits; balanced: the same
    count in every block of 32 bits AND in every residue class mod 8, with the
    residues rotated from block to block -- even over the XCDs whether the
    driver deals mask bits to XCDs round-robin or in blocks of 32."""
    if layout == "strided":
        step = n_cu / side
        return sorted({int(i * step) for i in range(side)})
    if layout == "high":
        return list(range(n_cu - side, n_cu))
    if layout != "balanced":
        raise ValueError(f"unknown side CU layout {layout!r}")
    blocks = max(1, n_cu // 32)
    per = max(1, side // blocks)
    out = []
    for b in range(blocks):
        for j in range(per):
            out.append(32 * b + 8 * (j // 8) + (j + b * per) % 8)
    return sorted(set(c for c in out if c < n_cu))


# Splits below this many utterances take the exact f64 Gram (mmb_gram): at
# dataset sizes (MOSI 229-1284, POM 100-203 rows) it costs microseconds, and
# sklearn's transposed branch (n < d: a rank-n Gram) is where the int8 Gram's
# ~1e-10 relative error reached the PC at 2e-8 (r04d, real POM valid split);
# the int8 Gram pays from tens of thousands of rows up.
GRAM_I8_MIN_ROWS = 1 << 15

# Steps of at most this many rows fork the projection beside the Gram -> PC
# solve chain (FusedStep.fork): latency-bound kernels side by side.
FORK_PROJECTION_MAX_ROWS = 4096


class StepPlan(NamedTuple):
    """What one FusedStep launches, decided once from shapes (step_plan)."""

    front: str        # writes x, aux: "narrow_fused" / "fused" (and mmb2) or "stream" (and s)
    split: bool       # the stream kernel over several workgroups per utterance
    gram: str         # "i8", "f64", or "parts" (per-chunk partials + mmb_gram_finish)
    project: str      # where the projection runs: "front" (inside the front kernel), "fork"
                      # (beside Gram -> solve), "remove" (after the solve, one kernel with
                      # the removal) or "chunk" (with each chunk's Gram)
    proj_split: bool  # the projection may run split-K (a few rows)
    bounds: tuple     # row chunks ((r0, r1), ...)
    step_rows: int    # rows of a full chunk
    s_half: bool      # s as fp16 hi | lo planes (the x3 projection)
    frames: str = "f32"  # storage type of the audio / visual frames (FRAME_KINDS)

    @property
    def remove_launch(self) -> bool:
        """The removal is its own launch (mmb_pc_remove)."""
        return self.project != "remove"


def step_plan(n: int, n_total: int, t: int, d: int, a: int, vd: int, V: int, npc: int, cus: int,
              chunks: int | None = None, fuse_remove: bool = True, gram_kind: str | None = None,
              stream_project: bool | None = None, narrow_fused: bool | None = None,
              fork_projection: bool | None = None, split_stream: bool | None = None,
              split_projection: bool = True, frames: str = "f32",
              fused_frames16: bool = False, narrow_frames16: bool = False,
              split_frames16: bool = False, narrow_table16: bool = False,
              split_table16: bool = False, fused_table16: bool = False,
              table: str = "f32") -> StepPlan:
    """The plan of a step over `n` of a split's `n_total` utterances on a chip
    of `cus` CUs; the remaining arguments are FusedStep's overrides (None: by
    shape).  Precedence: the fused front kernels need one chunk ASKED for and
    the fp16 split, the wide-frame one first; fewer utterances than features
    force one chunk (the transposed branch needs X^T Omega of all rows); the
    projection forks or takes the removal only behind the plain stream kernel,
    in one chunk, at npc = 1.  16-bit `frames` ("f16" / "bf16") are read by
    the plain stream kernel only: the front is "stream" and never split,
    whatever the three overrides that allow the other fronts say -- unless
    `fused_frames16` opts in to the wide-frame fused kernel on them
    (mmb_mm2_stream_project_ft): `stream_project` then keeps the caller's
    value and the front is "fused" exactly where the f32 plan of the shape
    chooses it, "stream" everywhere else.  `narrow_frames16` is its sibling
    for the narrow fused kernel (mmb_mm2_stream_project_narrow_ft):
    `narrow_fused` then keeps the caller's value and the front is
    "narrow_fused" exactly where the f32 plan of the shape chooses it; with
    both set the precedence is the f32 plan's.  `split_frames16` is the third
    sibling, for the split stream (mmb_mm2_stream_split_ft): `split_stream`
    then keeps the caller's value and `split` is set exactly where the f32 plan
    of the shape sets it.  On f32 frames the keywords change nothing.
    A 16-bit word `table` ("f16" / "bf16", TABLE_KINDS) is read by the plain
    stream kernel only: `stream_project`, `narrow_fused` and `split_stream`
    are off whatever the overrides and the three `*_frames16` opt-ins say, so
    the plan is the two-kernel plan of the shape -- unless `fused_table16`
    opts in to the wide-frame fused kernel on it (mmb_mm2_stream_project_tt):
    `stream_project` then keeps the caller's value and the front is "fused"
    exactly where the f32-table plan of the same shape and frames chooses it
    (on 16-bit frames that still needs `fused_frames16`).  `narrow_table16`
    is its sibling for the narrow fused kernel
    (mmb_mm2_stream_project_narrow_tt, its text cache built from the 16-bit
    table): `narrow_fused` then keeps the caller's value and the front is
    "narrow_fused" exactly where the f32-table plan of the same shape and
    frames chooses it (on 16-bit frames that still needs `narrow_frames16`).
    `split_table16` is the third sibling, for the split stream
    (mmb_mm2_stream_split_tt): `split_stream` then keeps the caller's value
    and `split` is set exactly where the f32-table plan of the same shape and
    frames sets it (on 16-bit frames that still needs `split_frames16`).
    Without its opt-in a front stays off.  With "f32" the three keywords
    change nothing and every plan is as described above.  The table kind is
    not a field of the plan."""
    check_npc(npc)
    if frames not in FRAME_KINDS:
        raise ValueError(f"frames must be one of {', '.join(FRAME_KINDS)}, not {frames!r}")
    if table not in TABLE_KINDS:
        raise ValueError(f"table must be one of {', '.join(TABLE_KINDS)}, not {table!r}")
    if table != "f32":
        if not narrow_table16:
            narrow_fused = False
            narrow_frames16 = False
        if not split_table16:
            split_stream = False
            split_frames16 = False
        if not fused_table16:
            stream_project = False
            fused_frames16 = False
    if frames != "f32":
        if not split_frames16:
            split_stream = False
        if not fused_frames16:
            stream_project = False
        if not narrow_frames16:
            narrow_fused = False
    s_half = L.query("mmb_mm2_ldw", d) <= 320
    one_asked = (chunks or 1) == 1
    if stream_project is None:
        stream_project = fused_pays(a, vd)
    if narrow_fused is None:
        narrow_fused = True
    if stream_project and one_asked and s_half and stream_project_supported(t, d, a, vd):
        front = "fused"
    elif narrow_fused and one_asked and s_half and narrow_fused_supported(t, d, a, vd, V):
        front = "narrow_fused"
    else:
        front = "stream"
    if chunks is None or n_total < d:
        chunks = 1
    chunks = max(1, min(chunks, n))
    step = -(-n // chunks)
    step = -(-step // 256) * 256  # 16-byte aligned chunk starts (two-phase Gram)
    bounds = tuple((r, min(r + step, n)) for r in range(0, n, step)) or ((0, 0),)
    one = len(bounds) == 1
    # Gram of the one-chunk step: "i8" (mmb_gram_i8, int8 digits of the
    # column-bounded fixed-point x, ~1e-10 of exact; the bounds come from
    # the front kernel) or "f64" (mmb_gram, exact f64 products)
    if gram_kind is None:
        gram_kind = "i8" if n_total >= GRAM_I8_MIN_ROWS else "f64"
    if gram_kind not in ("i8", "f64"):
        raise ValueError(f"gram_kind must be 'i8' or 'f64', not {gram_kind!r}")
    if not one:
        gram = "parts" if d % 4 == 0 and d <= 320 else "f64"
    else:
        gram = "i8" if gram_kind == "i8" and d % 4 == 0 and d <= 304 else "f64"
    # small steps (the dataset splits): the projection runs on a forked
    # stream beside the Gram -> PC solve chain, and the removal is its own
    # small launch, instead of the projection waiting for the PC to fuse
    # the removal into its tail (that saves an HBM pass only at scale)
    if fork_projection is None:
        fork_projection = n <= FORK_PROJECTION_MAX_ROWS
    if front != "stream":
        project = "front"
    elif fuse_remove and one and npc == 1 and s_half:
        project = "fork" if fork_projection else "remove"
    else:
        project = "chunk"
    # a few long rows (POM's splits): every utterance's tokens and each
    # modality's frames on workgroups of their own (mmb_mm2_stream_split),
    # so 100-203 rows fill the chip instead of one workgroup each
    split = bool((split_stream is None or split_stream) and front == "stream" and one
                 and t > 64 and 0 < n <= cus)
    proj_split = bool(split_projection and front == "stream" and s_half and one)
    return StepPlan(front, split, gram, project, proj_split, bounds, step, s_half, frames)


# the fused front kernels: trace phase and mirror
_FRONTS = {"fused": ("mm2_stream_project", mm2_stream_project),
           "narrow_fused": ("mm2_stream_project_narrow", mm2_stream_project_narrow)}
# their mirrors on 16-bit frames (the same phase names)
_FRONTS_FT = {"fused": mm2_stream_project_ft, "narrow_fused": mm2_stream_project_narrow_ft}
# and on a 16-bit word table, frames of any kind (fused_table16 / narrow_table16)
_FRONTS_TT = {"fused": mm2_stream_project_tt, "narrow_fused": mm2_stream_project_narrow_tt}


class FusedStep:
    """One pass of the north-star hot path over a batch of utterances resident
    in HBM (bench 'step'): both the SIF text embedding (a1-a5, PC-removed) and
    the closed-form MMB2 embedding (a6-a8) of every utterance.

      mm2_stream   ids/table/wtab + audio + visual -> x, s, aux  (HBM-bound)
      gram         x -> G (fp64 MFMA)                  [+ RCCL all-reduce of G]
      pc_solve     G -> pc (1 workgroup)
      pc_remove    x, pc -> sif                          (HBM-bound)
      mm2_prepare  generator weights -> Wm, c0, fp16 hi/lo split
      mm2_project  s, x, aux, Wm -> mmb2 (fp16-split MFMA + fused normalisation;
                   the weighted text sum is x * count)

    With one chunk, npc = 1 and the fp16 split (the bench shape) the order is
    stream, Gram, PC solve, then ONE projection kernel that also writes the
    PC-removed rows (mmb_mm2_project_x3_rmpc): the removal re-reads x from
    cache instead of a separate HBM pass (`fuse_remove=False` keeps the
    separate pc_remove kernel).

    x is the a2 row (weighted text sum / count, the exact f32 division of
    sif_functions.py:55) written once by the stream kernel, so the Gram and
    the removal read it without dividing.

    With `chunks` > 1 the utterances are cut into row chunks (multiples of 256
    rows) and pipelined: chunk 0's stream kernel runs on every CU; then chunk
    c's stream kernel runs on the main stream while chunk c-1's projection and
    Gram partials (mmb_gram_part) run on a side stream; the last chunk's
    projection runs on every CU again, one mmb_gram_finish sums the partials,
    and the PC solve and removal follow.  `side_cus` > 0 puts the two streams
    on disjoint CU sets (CU-masked HIP streams; grid-stride kernels size their
    grids from the mask).  Measured on MI355X (1M utterances)
    the overlap does not pay: beside the MFMA-bound kernels the HBM-bound
    stream kernel slows by about what the projection hides (8 chunks, shared
    CUs / 64 balanced side CUs / 96 'high' side CUs: 28.5 / 30.7 / 28.8 ms per
    step against 28.6 ms unpipelined), so the default is one chunk.

    Small steps (the dataset splits, r06): `split_stream` cuts
    a few long rows over workgroups (mmb_mm2_stream_split), `split_projection`
    runs the projection split-K (mmb_mm2_project_x3_split; K summed in another
    f32 order than the one-pass kernel), and `fork_projection` runs it on a
    side stream beside Gram -> PC solve; each is chosen by shape when left at
    its default.

    16-bit frames (float16 / bfloat16 `audio` and `visual`) take the
    two-kernel step; `fused_frames16=True` opts in to the fused stream +
    projection kernel on them where the f32 plan of the shape would choose it
    (mm2_stream_project_ft: no s buffer, the same rows bit for bit as on the
    upcast frames), `narrow_frames16=True` to the narrow fused kernel in the
    same way (mm2_stream_project_narrow_ft; MOSI's widths), and
    `split_frames16=True` to the split stream of the two-kernel step
    (mm2_stream_split_ft; POM's long transcripts).

    A 16-bit word table (float16 / bfloat16 `inputs["table"]`, `self.table_kind`)
    takes the two-kernel step (mmb_mm2_stream_tt: the same rows bit for bit as
    on the upcast table), with frames of any of the three dtypes;
    `fused_table16=True` opts in to the fused stream + projection kernel on it
    where the f32-table plan of the shape and frames would choose it
    (mm2_stream_project_tt: no s buffer, the same rows bit for bit; on 16-bit
    frames together with `fused_frames16`), `narrow_table16=True` to the
    narrow fused kernel in the same way (mm2_stream_project_narrow_tt: the
    text cache is built from the 16-bit table, byte for byte that of the
    upcast table; on 16-bit frames together with `narrow_frames16`), and
    `split_table16=True` to the split stream of the two-kernel step
    (mm2_stream_split_tt; on 16-bit frames together with `split_frames16`).

    Which of these a step takes is decided once, by step_plan() (`self.plan`);
    _run is one sequence over it: front kernel, chunk pipeline, projection
    (unless the front kernel or the removal carries it), Gram, PC solve,
    removal.
    """

    def __init__(self, inputs: dict, networks: dict, npc: int = 1, allreduce=None,
                 n_total: int | None = None, row0: int = 0, chunks: int | None = None,
                 side_cus: int = 0, side_layout: str = "balanced", fuse_remove: bool = True,
                 gram_kind: str | None = None, stream_project: bool | None = None,
                 narrow_fused: bool | None = None, check_each_run: bool = False,
                 fork_projection: bool | None = None, split_stream: bool | None = None,
                 split_projection: bool = True, fused_frames16: bool = False,
                 narrow_frames16: bool = False, split_frames16: bool = False,
                 narrow_table16: bool = False, split_table16: bool = False,
                 fused_table16: bool = False):
        self.inp = inputs
        self.check_each_run = check_each_run
        self.ids = inputs["ids"]
        self.n, self.t = self.ids.shape
        self.table = inputs["table"]
        self.V, self.d = self.table.shape
        self.a = inputs["audio"].shape[-1]
        self.vd = inputs["visual"].shape[-1]
        dev = self.table.device
        self.npc = npc
        self.allreduce = allreduce
        self.n_total = self.n if n_total is None else n_total
        self.row0 = row0
        # the frames' storage type, checked here: a step never launches on a
        # dtype its kernels would read as another
        self.frames = frame_kind(inputs["audio"], inputs["visual"], "FusedStep")
        # the word table's, likewise: a 16-bit table takes the two-kernel step
        # (or, with fused_table16 / narrow_table16 / split_table16, the `_tt`
        # mirror of the front the f32-table plan chooses)
        self.table_kind = table_kind(self.table, "FusedStep")
        # and the ids' and the weight table's: int64 ids would be read as
        # pairs of int32, float64 weights as pairs of float32
        for what, t, dtype in (("ids", self.ids, torch.int32), ("wtab", inputs["wtab"], torch.float32)):
            if t is not None and t.dtype != dtype:
                raise L.MMBError(f"FusedStep: inputs[{what!r}] must be {dtype}, not {t.dtype}")
        self.plan = p = step_plan(self.n, self.n_total, self.t, self.d, self.a, self.vd, self.V, npc,
                                  L.cu_count(dev), chunks=chunks, fuse_remove=fuse_remove,
                                  gram_kind=gram_kind, stream_project=stream_project,
                                  narrow_fused=narrow_fused, fork_projection=fork_projection,
                                  split_stream=split_stream, split_projection=split_projection,
                                  frames=self.frames, fused_frames16=fused_frames16,
                                  narrow_frames16=narrow_frames16, split_frames16=split_frames16,
                                  narrow_table16=narrow_table16, split_table16=split_table16,
                                  fused_table16=fused_table16, table=self.table_kind)
        self.proj = MMB2Projection(networks, self.d, self.a, self.vd, self.t, dev)
        kp = self.proj.kp
        self.x = torch.empty((self.n, self.d), dtype=torch.float32, device=dev)
        self.s = s_buffer(self.n, kp, p.s_half, dev) if p.front == "stream" else None
        if p.front == "fused":
            self.proj.enable_pieces()
        if p.front == "narrow_fused":
            # (a 16-bit table gets here with narrow_table16 only)
            self.proj.enable_text_cache(self.table, inputs["wtab"], table16=self.table_kind != "f32")
        self.G = torch.empty((self.d, self.d), dtype=torch.float64, device=dev)
        self.pc_buf = torch.empty((npc, self.d), dtype=torch.float64, device=dev)
        self.solve_ws = (torch.zeros(L.query("mmb_pc_solve_mc_ws_bytes", self.d), dtype=torch.uint8,
                                     device=dev) if self.d <= PC_SOLVE_MC_MAX_D else None)
        self.sif = torch.empty((self.n, self.d), dtype=torch.float32, device=dev)
        self.mmb2 = torch.empty((self.n, self.d), dtype=torch.float32, device=dev)
        self.flag = torch.zeros(1, dtype=torch.int32, device=dev)
        # aux is planar per chunk: chunk [r0, r1) owns flat[3 r0 : 3 r1] as [3][r1 - r0]
        self.aux_flat = torch.empty((3 * self.n,), dtype=torch.float32, device=dev)
        if p.gram == "i8":
            self.colmax = torch.zeros((self.d,), dtype=torch.int32, device=dev)
            nb = L.query("mmb_mm2_colmax_ws_bytes", self.d)
            self.colmax_ws = torch.empty((nb + 15) // 16 * 16, dtype=torch.uint8, device=dev)
        else:
            self.colmax = self.colmax_ws = None
        self.split = split_ws(self.n, self.t, self.d, self.a, self.vd, dev) if p.split else None
        self.fork = torch.cuda.Stream(device=dev) if p.project == "fork" else None
        # (None where the rows alone fill the chip)
        self.proj_split = project_split_ws(self.n, kp, dev) if p.proj_split else None
        self.gws = GramWorkspace(max(r1 - r0 for r0, r1 in p.bounds), self.d, dev)
        self.side = torch.cuda.Stream(device=dev) if len(p.bounds) > 1 else None
        self.main = None
        self._cu_streams = []
        self._events = [torch.cuda.Event() for _ in p.bounds]
        if side_cus and self.side is not None:
            # disjoint CU sets: the stream kernel on `main`, the projection +
            # Gram of the previous chunk on `side`
            n_cu = L.cu_count(dev)
            side_set = side_cu_set(n_cu, side_cus, side_layout)
            main_set = [c for c in range(n_cu) if c not in set(side_set)]
            self._cu_streams = [L.CUStream(main_set, dev), L.CUStream(side_set, dev)]
            self.main, self.side = self._cu_streams[0].torch, self._cu_streams[1].torch

    # the plan, under the names the step has always answered to
    stream_project = property(lambda self: self.plan.front == "fused")
    narrow_fused = property(lambda self: self.plan.front == "narrow_fused")
    gram_i8 = property(lambda self: self.plan.gram == "i8")
    gram_parts = property(lambda self: self.plan.gram == "parts")
    fused_remove = property(lambda self: not self.plan.remove_launch)
    bounds = property(lambda self: self.plan.bounds)
    step_rows = property(lambda self: self.plan.step_rows)
    s_half = property(lambda self: self.plan.s_half)

    def check(self):
        """Raise what the reference would have raised for the last step(s):
        IndexError for a token id >= V, ValueError for an utterance whose SIF
        weights are all 0 (the PC step of the split is then undefined),
        RuntimeError if the fused kernel's hand-over timed out.  Reads the flag
        word (one device sync); the flag accumulates until `reset()`.

        Sharded (an `allreduce` given), the three flag bits are summed over
        the ranks first -- one small all-reduce, only here -- so EVERY rank
        raises the same error for a bad utterance on any rank (a rank that
        raised alone would leave the others waiting in the next step's Gram
        all-reduce).  A NaN row reaches every rank's PC through the Gram anyway
        (check_pc_finite)."""
        flag = self.flag
        if self.allreduce is not None:
            bits = (L.MMB_FLAG_ID_RANGE, L.MMB_FLAG_ZERO_WEIGHTS, L.MMB_FLAG_SYNC_TIMEOUT)
            t = torch.stack([(flag[0] & b) != 0 for b in bits]).to(torch.int32)
            self.allreduce(t)
            flag = sum((t[i] > 0).to(torch.int32) * b for i, b in enumerate(bits)).reshape(1)
        self.raise_status(int(self.status(flag).item()))  # the one device sync

    def status(self, flag=None, out=None) -> torch.Tensor:
        """[1] int32 on the device: the flag bits | PC_NONFINITE when the last
        step's PC is not finite -- what check() reads back, formed without a
        sync (StepGraph captures it into the graph)."""
        flag = self.flag if flag is None else flag
        pc = getattr(self, "pc", None)
        if pc is None:
            return torch.add(flag, 0, out=out)
        if out is None:
            out = torch.empty(1, dtype=torch.int32, device=flag.device)
        # one launch (mmb_step_status): eight elementwise torch kernels here
        # were ~40 us of every dataset split's graph (r06 kernel trace)
        L.call("mmb_step_status", L.ptr(flag, L.I32), L.ptr(pc, L.F64), pc.numel(), PC_NONFINITE,
               L.ptr(out, L.I32), L.stream_ptr())
        return out

    def raise_status(self, v: int):
        """check()'s verdict on a status word read back (status())."""
        if self.solve_ws is not None and v & (L.MMB_FLAG_SYNC_TIMEOUT | PC_NONFINITE):
            # an aborted solve leaves its control words set (and a NaN PC):
            # hand the next launch a zeroed workspace again
            self.solve_ws[:16].zero_()
        check_flag_bits(v & (PC_NONFINITE - 1), self.V, zero_weights=True)
        if v & PC_NONFINITE:
            raise ValueError("Input X contains NaN or infinity: the split's Gram is not finite "
                             "(an all-zero-weight utterance on some rank, or non-finite inputs), "
                             "which the reference's TruncatedSVD rejects (sif_functions.py:65-67)")

    def reset(self):
        self.flag.zero_()

    def aux_of(self, c: int) -> torch.Tensor:
        r0, r1 = self.bounds[c]
        return self.aux_flat[3 * r0:3 * r1].view(3, r1 - r0)

    @property
    def aux(self) -> torch.Tensor:
        """[3, N] planar aux (count, total weight, row scale) of a one-chunk step."""
        if len(self.bounds) != 1:
            raise ValueError("aux is planar per chunk when chunks > 1; use aux_of(c)")
        return self.aux_of(0)

    def _stream_chunk(self, c: int):
        r0, r1 = self.bounds[c]
        inp = self.inp
        # the split stream on a 16-bit table (split_table16) or on 16-bit
        # frames (split_frames16) has its own mirror
        stream = mm2_stream
        if self.split is not None and self.table_kind != "f32":
            stream = mm2_stream_split_tt
        elif self.split is not None and self.frames != "f32":
            stream = mm2_stream_split_ft
        stream(r1 - r0, self.t, self.d, self.a, self.vd, inp["audio"][r0:r1],
               inp["visual"][r0:r1], ids32=self.ids[r0:r1], table=self.table,
               wtab32=inp["wtab"], flag=self.flag, s_half=self.s_half,
               out=(self.x[r0:r1], self.s[r0:r1], self.aux_of(c)),
               colmax=self.colmax, colmax_ws=self.colmax_ws, split=self.split)

    def _project(self, c: int, pc=None):
        """Chunk c's MMB2 rows; with `pc` also its PC-removed rows."""
        r0, r1 = self.bounds[c]
        mm2_project(self.s[r0:r1], self.x[r0:r1], self.aux_of(c), self.proj, out=self.mmb2[r0:r1],
                    pc=pc, sif_out=None if pc is None else self.sif[r0:r1],
                    split=self.proj_split)  # (None past one chunk)

    def _gram(self, c: int):
        """Chunk c's rows into G (or into the partials of mmb_gram_finish)."""
        r0, r1 = self.bounds[c]
        if self.gram_parts:
            L.call("mmb_gram_part", L.ptr(self.x[r0:r1], L.F32), None, r1 - r0,
                   self.step_rows, self.d, int(c > 0), L.ptr(self.gws.buf, L.BYTES), L.stream_ptr())
        elif self.gram_i8:  # one chunk
            gram_i8(self.x, self.colmax, self.G, ws=self.gws)
        else:
            gram(self.x[r0:r1], None, self.G, accumulate=c > 0, ws=self.gws)

    def _pipeline_chunks(self, mark):
        """Chunks 1 .. nb-1 streamed on `main` while the chunk before each is
        projected and its Gram partial formed on `side`; chunk 0 is streamed
        and the last chunk is left to the caller's stream."""
        nb = len(self.bounds)
        caller = torch.cuda.current_stream(self.table.device)
        main = self.main if self.main is not None else caller
        side = self.side
        ev = self._events
        ev[0].record(caller)
        if main is not caller:
            main.wait_stream(caller)
        side.wait_stream(caller)
        for c in range(1, nb):
            with torch.cuda.stream(main):
                with mark("mm2_stream"):
                    self._stream_chunk(c)
                if c < nb - 1:
                    ev[c].record(main)
            with torch.cuda.stream(side):
                side.wait_event(ev[c - 1])
                with mark("mm2_project+gram"):
                    self._project(c - 1)
                    self._gram(c - 1)
        if main is not caller:
            caller.wait_stream(main)
        caller.wait_stream(side)

    def _solve(self, mark):
        """G (this rank's rows) -> pc: Omega, RCCL all-reduce of G, the solve."""
        d, k = self.d, self.npc + N_OVERSAMPLES
        if (self.n_total < d and self.allreduce is None and self.row0 == 0
                and self.n_total == self.n and self.solve_ws is not None and k <= min(16, d)):
            # the transposed branch over all of Omega's rows, unsharded: X^T
            # Omega and the squared matrix in one launch in front of the
            # solve (mmb_pc_solve_mc_xt)
            om = omega(self.n_total, k, self.table.device)
            with mark("pc_solve"):
                L.call("mmb_pc_solve_mc_xt", L.ptr(self.G, L.F64), d, L.ptr(self.x, L.F32), self.n,
                       L.ptr(om, L.F64), k, self.npc, N_ITER, L.ptr(self.pc_buf, L.F64),
                       L.ptr(self.solve_ws, L.BYTES), L.ptr(self.flag, L.I32), L.stream_ptr())
            return self.pc_buf
        with mark("pc_start"):
            z0, transposed = pc_start_block(self.x, None, self.npc, self.n_total, self.row0)
        if self.allreduce is not None:
            with mark("allreduce"):
                self.allreduce(self.G)
                if transposed:
                    self.allreduce(z0)
        with mark("pc_solve"):
            return pc_solve(self.G, z0, self.npc, transposed, out=self.pc_buf, flag=self.flag,
                            ws=self.solve_ws)

    def run(self, trace: dict | None = None, check: bool | None = None):
        """One step.  With `trace` (a dict), HIP events are recorded on the
        stream each phase runs on: trace[phase] gets (start, end) pairs.
        With `check` (default: the constructor's `check_each_run`) the step
        ends with check() -- one device sync -- and raises like the
        reference; without it the step never synchronises and the caller
        calls check() when it wants the verdict (bench.py: once, after the
        timed steps)."""
        out = self._run(trace)
        if self.check_each_run if check is None else check:
            self.check()
        return out

    def _run(self, trace, fork: bool = True):
        def mark(name):
            if trace is None:
                return _NullSpan()
            return _EventSpan(trace.setdefault(name, []))

        p = self.plan
        last = len(p.bounds) - 1
        with mark("mm2_prepare"):
            self.proj.refresh_if_changed()
        if p.front == "stream":
            with mark("mm2_stream"):
                self._stream_chunk(0)  # every CU
        else:
            phase, front = _FRONTS[p.front]
            if p.frames != "f32":  # the fused kernels on 16-bit frames (fused_frames16 / narrow_frames16)
                front = _FRONTS_FT[p.front]
            if self.table_kind != "f32":  # on a 16-bit table (fused_table16 / narrow_table16), any frames
                front = _FRONTS_TT[p.front]
            with mark(phase):
                front(self.n, self.t, self.d, self.a, self.vd, self.inp["audio"],
                      self.inp["visual"], self.proj, ids32=self.ids, table=self.table,
                      wtab32=self.inp["wtab"], flag=self.flag,
                      out=(self.x, self.aux_of(0), self.mmb2), colmax=self.colmax,
                      colmax_ws=self.colmax_ws)
        if last > 0:
            self._pipeline_chunks(mark)
        if p.project == "fork":
            # the projection beside the Gram -> solve chain; with fork=False
            # (inside a concurrent StepGraph) the same kernels in one stream,
            # so the rows are the forked step's bit for bit
            caller = torch.cuda.current_stream(self.table.device)
            side = self.fork if fork else caller
            if fork:
                side.wait_stream(caller)
            with torch.cuda.stream(side):
                with mark("mm2_project"):
                    self._project(0)
        with mark("mm2_project+gram" if p.project == "chunk" else "gram"):
            if p.project == "chunk":
                self._project(last)  # every CU
            self._gram(last)
        if p.gram == "parts":
            with mark("gram_finish"):
                L.call("mmb_gram_finish", p.step_rows, self.d, L.ptr(self.G, L.F64), 0,
                       L.ptr(self.gws.buf, L.BYTES), L.stream_ptr())
        pc = self._solve(mark)
        if p.remove_launch:
            with mark("pc_remove"):
                for r0, r1 in p.bounds:
                    remove_pc(self.x[r0:r1], None, pc, out=self.sif[r0:r1])
        else:
            with mark("mm2_project+pc_remove"):
                self._project(0, pc=pc)
        if p.project == "fork" and fork:
            caller.wait_stream(side)
        self.pc = pc
        return self.sif, self.mmb2


class StepGraph:
    """One or more FusedSteps' device work captured ONCE as a HIP graph and
    replayed: the per-split call pattern of the reference (SIF once per split,
    each split with its own PC: simplesif.py:296-311) pays the host launch
    cost of ~10 kernels per split on every call; a replay is one launch.

    `concurrent=True` captures every step on its own stream (fork / join
    branches of the graph), so independent splits overlap on the chip -- the
    PC solves of different splits (each ceil(d/16) workgroups) run side by
    side instead of back to back.  Steps are warmed up eagerly first (weight
    merge, Omega upload, workspaces); a later in-place update of a generator
    parameter is re-merged eagerly before the replay (the merge writes the
    buffers the graph reads).  No host sync unless `check`."""

    def __init__(self, steps, concurrent: bool = False, warmup: int = 1):
        self.steps = list(steps) if isinstance(steps, (list, tuple)) else [steps]
        dev = self.steps[0].table.device
        caller = torch.cuda.current_stream(dev)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(caller)
        with torch.cuda.stream(side):
            for _ in range(warmup):
                for st in self.steps:
                    st.run()
        caller.wait_stream(side)
        torch.cuda.synchronize(dev)
        for st in self.steps:
            # the warm-up's verdict first: a flag (or an aborted solve's NaN
            # PC) raises here instead of being cleared by reset() and leaving
            # every replay to run on a dirty workspace
            st.check()
            st.reset()
        self._branches = ([torch.cuda.Stream(device=dev) for _ in self.steps]
                          if concurrent and len(self.steps) > 1 else None)
        # every step's status word (FusedStep.status) is formed inside the
        # graph, so a checked replay reads ONE small tensor back (one sync for
        # all steps; check() per step took up to four)
        self._status = torch.zeros(len(self.steps), dtype=torch.int32, device=dev)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            cap = torch.cuda.current_stream(dev)
            if self._branches is None:
                self.outs = [st._run(None) for st in self.steps]
            else:
                self.outs = []
                # the steps run WITHOUT their forked projection here: the
                # splits' branches already overlap, and with the forks the
                # replay ran the branches one after the other (POM's two
                # splits 0.505 ms concurrent vs 0.503 serial; without 0.436,
                # r06 tools/pom_graph_ab.py); a fork joined back to its
                # branch stream also segfaulted the capture
                # (tools/dbg/fork_graph_probe.py)
                for st, br in zip(self.steps, self._branches):
                    br.wait_stream(cap)
                    with torch.cuda.stream(br):
                        self.outs.append(st._run(None, fork=False))
                for br in self._branches:
                    cap.wait_stream(br)
            for i, st in enumerate(self.steps):
                if st.allreduce is None:
                    st.status(out=self._status[i:i + 1])

    def run(self, check: bool = False):
        for st in self.steps:
            st.proj.refresh_if_changed()
        self.graph.replay()
        if check:
            words = self._status.tolist()  # the one sync
            for st, v in zip(self.steps, words):
                if st.allreduce is not None:
                    st.check()  # (its flag bits cross ranks: check()'s all-reduce)
                else:
                    st.raise_status(v)
        return self.outs if len(self.steps) > 1 else self.outs[0]
