"""GPU: the mirrors on the dtypes, layouts and devices the reference takes.

Every drop-in below is run on a baseline (float32 / int64, contiguous; numpy C
order, or torch on the GPU) that is held to the float64 oracle at the bar the
drop-in's own test module uses, and then on every presentation of
tests/presentation_cases.py that applies to each of its arguments, one
argument at a time.  The values are float32-representable, so a presentation
must return the baseline's result bit for bit, with its dtype and shape (and
on the caller's device where the mirror documents that), must not raise, and
must leave its input as it was.  A gradient that reaches a float64 or strided
leaf is the baseline's bit for bit after the cast to the leaf's dtype, with the
leaf's shape and device; a broadcast leaf (T4) gets the sum over the broadcast
axis, held to the oracle.

Also here: latent.word_table follows a table's current values (a rewritten
numpy array under torch.from_numpy, a float64 device table rewritten through
.data), and every pipeline mirror refuses an operand of another element type
before anything is launched (only types at least as wide as the expected one
are tried, so even an unchecked mirror would read inside the buffer).

The module prints, per drop-in, how many presentations ran.
"""
import functools

import numpy as np
import pytest
import torch

import gauss_cases as G
import gauss_gpu
import latent as LT
import losses
import mmb_lib as L
import pipeline as P
import presentation_cases as PC
import regressor_cases as RC
import regressor_gpu as RG
import sentiment_model as SM
import sif
import sif2
import sif_functions as SF
import word_cases as W
import mmb2_cases as C
from common_gpu import TOL, Ledger, _networks, _untouched
from mmb2_gpu import _check_step, _device_inputs
from common_gpu import _dev32 as _dev  # float32 unless told otherwise
from oracle import latent_oracle as LO
from oracle import mmb2_oracle as M
from oracle import sif_oracle as O
from width_cases import EMB_TOL, PC_BAR

pytestmark = pytest.mark.gpu

_WORST = Ledger()   # baseline against the oracle, as a fraction of the bar
_COUNT = {}         # drop-in -> presentations run


def _note(what, ratio):
    return _WORST.note(what, ratio)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for what, (n, r) in sorted(_WORST.items()):
        print(f"\npresentations, baseline {what}: {n} comparisons, largest {r:.3f} of its bar", end="")
    for what, n in sorted(_COUNT.items()):
        print(f"\npresentations run, {what}: {n}", end="")
    print()


def _within(what, got, ref, bar):
    gauss_gpu.within(_note, what, got, ref, bar)


def _results(r):
    return r if isinstance(r, (tuple, list)) else (r,)


def _sweep(name, fn, args, spec, base, device=None):
    """Run fn(**args) with one argument at a time replaced by each of its
    presentations (spec: argument -> [(id, builder)]) and hold every result to
    `base` bit for bit.  Collects every miss and fails once, naming them."""
    bad = []
    for arg, forms in spec.items():
        for pid, build in forms:
            shown = build(args[arg])
            snap = PC.snapshot(shown)
            try:
                got = fn(**{**args, arg: shown})
            except Exception as e:  # a presentation the reference accepts must not raise
                bad.append(f"{arg} as {pid}: raised {type(e).__name__}: {e}")
                continue
            finally:
                _COUNT[name] = _COUNT.get(name, 0) + 1
            for k, (g, b) in enumerate(zip(_results(got), _results(base))):
                if not PC.same_result(g, b):
                    bad.append(f"{arg} as {pid}: result {k} differs from the baseline's "
                               f"({getattr(g, 'dtype', None)} {tuple(getattr(g, 'shape', ()))})")
                elif device is not None and torch.is_tensor(g) and g.device.type != device(arg, pid, shown):
                    bad.append(f"{arg} as {pid}: result on {g.device}")
            if not PC.unchanged(shown, snap):
                bad.append(f"{arg} as {pid}: the input was modified")
    assert not bad, f"{name}:\n  " + "\n  ".join(bad)


def _tforms(t, **kw):
    return [(k, PC.TORCH_FORMS[k]) for k in PC.torch_forms(t, **kw)]


def _grad_sweep(name, run, args, leaves, base_grads):
    """`run(args)` returns a scalar to differentiate.  For each leaf argument
    and each T2 / T3 presentation of it, the gradient that reaches the
    presented leaf is the baseline's bit for bit after the cast to the leaf's
    dtype, with the leaf's shape and device."""
    bad = []
    for arg in leaves:
        for pid, build in _tforms(args[arg]):
            leaf = build(args[arg]).detach().requires_grad_(True)
            run({**args, arg: leaf}).backward()
            _COUNT[name + " (gradients)"] = _COUNT.get(name + " (gradients)", 0) + 1
            g, want = leaf.grad, base_grads[arg].to(leaf.dtype)
            if g is None or g.shape != leaf.shape or g.device != leaf.device or g.dtype != leaf.dtype:
                bad.append(f"{arg} as {pid}: gradient {None if g is None else (g.dtype, tuple(g.shape), g.device)}")
            elif not np.array_equal(PC.bits(g), PC.bits(want)):
                bad.append(f"{arg} as {pid}: the gradient differs from the baseline's")
    assert not bad, f"{name} gradients:\n  " + "\n  ".join(bad)


# ================================================================ numpy drop-ins
class _Params:
    def __init__(self, rmpc):
        self.rmpc = rmpc


def _nforms(a, **kw):
    return PC.numpy_forms(a, **kw)


def test_seq2weight_presentations(gpu):
    z = PC.sif_inputs()
    args = dict(seq=z.ids, mask=z.mask, weight4ind=z.weights)
    base = SF.seq2weight(**args)
    assert base.dtype == np.float32 and np.array_equal(base, O.seq2weight(z.ids, z.mask, z.weights))
    spec = {"seq": _nforms(z.ids, ids=True), "mask": _nforms(z.mask) + list(PC.MASK_FORMS.items()),
            "weight4ind": [(k, f) for k, f in _nforms(z.weights) if k != "N1"] +
            [("N1-float32", lambda a: a.astype(np.float32))]}
    _sweep("sif_functions.seq2weight", SF.seq2weight, args, spec, base)
    # sif.get_sentence_word_weights: the same kernel under an all-ones mask
    args = dict(text=z.ids, weights=z.weights)
    base = sif.get_sentence_word_weights(**args)
    assert np.array_equal(base, O.seq2weight(z.ids, np.ones(z.ids.shape), z.weights))
    _sweep("sif.get_sentence_word_weights", sif.get_sentence_word_weights, args,
           {"text": _nforms(z.ids, ids=True), "weights": [(k, f) for k, f in _nforms(z.weights) if k != "N1"]}, base)


def test_weighted_average_presentations(gpu):
    z = PC.sif_inputs()
    args = dict(We=z.We, x=z.ids, w=z.w)
    base = SF.get_weighted_average(**args)
    ref = O.get_weighted_average(z.We, z.ids, z.w)
    assert base.dtype == np.float64 and _note("get_weighted_average", M.row_rel_err(base, ref) / PC.WAVG_TOL) < 1.0
    spec = {"We": _nforms(z.We), "x": _nforms(z.ids, ids=True), "w": _nforms(z.w)}
    _sweep("sif_functions.get_weighted_average", SF.get_weighted_average, args, spec, base)


@pytest.mark.parametrize("rmpc", [0, 1])
def test_sif_embedding_presentations(gpu, rmpc):
    z = PC.sif_inputs()
    fn = lambda We, x, w: SF.SIF_embedding(We, x, w, _Params(rmpc))  # noqa: E731
    args = dict(We=z.We, x=z.ids, w=z.w)
    base = fn(**args)
    ref = O.SIF_embedding(z.We, z.ids, z.w, rmpc)
    assert base.dtype == np.float64 and _note(f"SIF_embedding rmpc={rmpc}", M.row_rel_err(base, ref) / EMB_TOL) < 1.0
    spec = {"We": _nforms(z.We), "x": _nforms(z.ids, ids=True), "w": _nforms(z.w)}
    _sweep(f"sif_functions.SIF_embedding rmpc={rmpc}", fn, args, spec, base)


def test_sentence_embeddings_presentations(gpu):
    z = PC.sif_inputs()
    args = dict(word_embeddings=z.We, weights=z.weights, text=z.ids)
    base = sif.get_sentence_embeddings(**args)
    ref = O.get_sentence_embeddings(z.We, z.weights, z.ids)
    assert base.dtype == np.float64 and _note("get_sentence_embeddings", M.row_rel_err(base, ref) / EMB_TOL) < 1.0
    spec = {"word_embeddings": _nforms(z.We), "text": _nforms(z.ids, ids=True),
            "weights": [(k, f) for k, f in _nforms(z.weights) if k != "N1"]}
    _sweep("sif.get_sentence_embeddings", sif.get_sentence_embeddings, args, spec, base)


@pytest.mark.parametrize("shape", PC.PC_SHAPES, ids=["direct", "transposed"])
def test_pc_presentations(gpu, shape):
    X = PC.pc_rows(*shape)
    for name, fn, ref, tol in (("compute_pc", SF.compute_pc, O.compute_pc, PC_BAR[1]),
                               ("remove_pc", SF.remove_pc, O.remove_pc, PC.REMOVE_TOL)):
        base = fn(X, 1)
        want = ref(X.astype(np.float64), 1)
        err = np.abs(base - want).max() if name == "compute_pc" else M.row_rel_err(base, want)
        assert base.dtype == np.float64 and _note(f"{name} {shape}", err / tol) < 1.0
        _sweep(f"sif_functions.{name}", lambda X: fn(X, 1), dict(X=X), {"X": _nforms(X)}, base)  # noqa: B023


@pytest.mark.parametrize("shape", PC.PC_SHAPES, ids=["direct", "transposed"])
def test_pc_float64_rows_presentations(gpu, shape):
    """A float64 X that is not float32-representable takes the f64 kernels;
    its presentations are float64 too (N1 does not apply)."""
    X = PC.pc_rows(*shape, f32_representable=False)
    forms = [(k, f) for k, f in _nforms(X) if k != "N1"]
    for name, fn, ref in (("compute_pc", SF.compute_pc, O.compute_pc), ("remove_pc", SF.remove_pc, O.remove_pc)):
        base = fn(X, 1)
        want = ref(X, 1)
        err = np.abs(base - want).max() if name == "compute_pc" else M.row_rel_err(base, want)
        assert _note(f"{name} f64 rows {shape}", err / PC.F64_ROUTE_TOL) < 1.0
        _sweep(f"sif_functions.{name} (f64 rows)", lambda X: fn(X, 1), dict(X=X), {"X": forms}, base)  # noqa: B023


# ================================================================ the word likelihood
WORD = W.WordCase(16, 33, 17, 5, 0)


@functools.lru_cache(maxsize=None)
def _word_table_reference():
    """get_word_log_prob_angular's own float64 reference: per-token weights
    gathered from a weight table [V] (the inputs and cosines are the case's)."""
    z = W.make_inputs(WORD)
    wv = W.f32(np.random.default_rng(33).uniform(0.05, 1.0, WORD.V))
    t = {k: torch.tensor(v) for k, v in z.items()}
    x = t["lat"].clone().requires_grad_(True)
    mask3 = t["mask"][:, :, None].expand(WORD.B, WORD.L, WORD.D)
    lp = LO.word_log_prob_angular2(x, t["table"], torch.tensor(wv)[t["ids"]], t["table"][t["ids"]], mask3, W.A)
    (lp * t["up"]).sum().backward()
    return z, wv, lp.detach().numpy(), x.grad.numpy()


def _word_baseline(name, fn, args, up, lp_ref, g_ref):
    """(lp, d lp / d latents) of the baseline, held to the oracle at lp_ratio / grad_ratio."""
    with torch.no_grad():
        lp0 = fn(**args)
    x = args["latents"].clone().requires_grad_(True)
    lp = fn(**{**args, "latents": x})
    (lp * up).sum().backward()
    assert PC.same_result(lp.detach(), lp0)
    assert _note(f"{name} lp", W.lp_ratio(lp0.cpu(), lp_ref)) <= 1.0
    assert _note(f"{name} gradient", W.grad_ratio(x.grad.cpu(), g_ref)) <= 1.0
    return lp0, x.grad


def _broadcast_weight_row(name, fn, args, arg, z, dense):
    """T4: one weight row [1, L] expanded over the batch (row stride 0).  The
    result is that of the materialised rows bit for bit, and those meet the
    float64 oracle on the same weights at lp_ratio."""
    row = args[arg][:1].clone()
    shown = row.expand(WORD.B, WORD.L)
    assert shown.stride(0) == 0
    snap = PC.snapshot(row)
    with torch.no_grad():
        base = fn(**{**args, arg: shown.contiguous()})
        got = fn(**{**args, arg: shown})
    _COUNT[name] = _COUNT.get(name, 0) + 1
    assert PC.same_result(got, base) and PC.unchanged(row, snap)
    t = {k: torch.tensor(v) for k, v in z.items()}
    sent = t["dense"] if dense else t["table"][t["ids"]]
    mask3 = t["mask"][:, :, None].expand(WORD.B, WORD.L, WORD.D)
    ref = LO.word_log_prob_angular2(t["lat"], t["table"], t["w"][:1].expand(WORD.B, WORD.L), sent, mask3, W.A)
    assert _note(f"{name}, one weight row over the batch, lp", W.lp_ratio(base.cpu(), ref.numpy())) <= 1.0


def test_word_log_prob_angular_presentations(gpu):
    z, wv, lp_ref, g_ref = _word_table_reference()
    a = W.A
    fn = lambda latents, weights, word_embeddings, data, mask: losses.get_word_log_prob_angular(  # noqa: E731
        latents, weights, word_embeddings, data, mask, a)
    args = dict(latents=_dev(z["lat"], gpu), weights=_dev(wv, gpu), word_embeddings=_dev(z["table"], gpu),
                data=_dev(z["ids"], gpu, torch.int64), mask=_dev(z["mask"], gpu))
    up = _dev(z["up"], gpu)
    lp0, g0 = _word_baseline("get_word_log_prob_angular", fn, args, up, lp_ref, g_ref)
    spec = {"latents": _tforms(args["latents"]), "weights": _tforms(args["weights"], cpu=True),
            "word_embeddings": _tforms(args["word_embeddings"], cpu=True),
            "data": _tforms(args["data"], cpu=True, ids=True), "mask": _tforms(args["mask"], cpu=True)}
    with torch.no_grad():
        _sweep("losses.get_word_log_prob_angular", fn, args, spec, lp0, device=lambda *_: "cuda")
        # T5: a requires_grad leaf into a no-grad call
        leaf = args["latents"].clone().requires_grad_(True)
        assert PC.same_result(fn(**{**args, "latents": leaf}), lp0)
    _grad_sweep("losses.get_word_log_prob_angular", lambda kw: (fn(**kw) * up).sum(), args, ["latents"],
                {"latents": g0})


def test_word_log_prob_angular2_presentations(gpu):
    z, lp_ref, g_ref = W.reference(WORD, True)
    a = W.A
    fn = lambda latents, word_embeddings, word_weights, sent_embeddings, mask: \
        losses.get_word_log_prob_angular2(latents, word_embeddings, word_weights, sent_embeddings, mask, a)  # noqa: E731
    mask2 = _dev(z["mask"], gpu)
    mask3 = mask2[:, :, None].expand(WORD.B, WORD.L, WORD.D)
    args = dict(latents=_dev(z["lat"], gpu), word_embeddings=_dev(z["table"], gpu), word_weights=_dev(z["w"], gpu),
                sent_embeddings=_dev(z["dense"], gpu), mask=mask3.contiguous())
    up = _dev(z["up"], gpu)
    lp0, g0 = _word_baseline("get_word_log_prob_angular2", fn, args, up, lp_ref, g_ref)
    spec = {k: _tforms(args[k]) for k in ("latents", "word_weights", "sent_embeddings", "mask")}
    spec["word_embeddings"] = _tforms(args["word_embeddings"], cpu=True)
    # T4: the reference's mask, [B, L, 1] expanded over the features (stride 0)
    assert mask3.stride(2) == 0
    spec["mask"] = spec["mask"] + [("T4", lambda t: mask3)]
    with torch.no_grad():
        _sweep("losses.get_word_log_prob_angular2", fn, args, spec, lp0, device=lambda *_: "cuda")
    _grad_sweep("losses.get_word_log_prob_angular2", lambda kw: (fn(**kw) * up).sum(), args, ["latents"],
                {"latents": g0})
    _broadcast_weight_row("losses.get_word_log_prob_angular2", fn, args, "word_weights", z, True)


@pytest.mark.parametrize("dense", [False, True], ids=["ids", "dense"])
def test_latent_word_log_prob_presentations(gpu, dense):
    z, lp_ref, g_ref = W.reference(WORD, dense)
    wt = LT.WordTable(_dev(z["table"], gpu))
    tok = "sent_dense" if dense else "ids"
    args = dict(latents=_dev(z["lat"], gpu), w=_dev(z["w"], gpu), mask=_dev(z["mask"], gpu))
    args[tok] = _dev(z["dense"], gpu) if dense else _dev(z["ids"], gpu, torch.int64)
    fn = lambda latents, w, mask, **t: LT.word_log_prob(latents, wt, w, mask, W.A, **t)  # noqa: E731
    up = _dev(z["up"], gpu)
    lp0, g0 = _word_baseline(f"latent.word_log_prob {tok}", fn, args, up, lp_ref, g_ref)
    spec = {"latents": _tforms(args["latents"]), "w": _tforms(args["w"], cpu=True),
            "mask": _tforms(args["mask"], cpu=True), tok: _tforms(args[tok], cpu=True, ids=not dense)}
    with torch.no_grad():
        _sweep(f"latent.word_log_prob {tok}", fn, args, spec, lp0, device=lambda *_: "cuda")
    _grad_sweep(f"latent.word_log_prob {tok}", lambda kw: (fn(**kw) * up).sum(), args, ["latents"], {"latents": g0})
    _broadcast_weight_row(f"latent.word_log_prob {tok}", fn, args, "w", z, dense)


# ---------------------------------------------------------------- word_table follows the table's values
def _fresh_table(seed):
    z = W.make_inputs(WORD, seed)
    return z["table"].astype(np.float32)


def _table_lp(z, table64):
    """The float64 oracle's lp for the case's inputs on another table."""
    t = {k: torch.tensor(v) for k, v in z.items()}
    tab = torch.tensor(table64)
    mask3 = t["mask"][:, :, None].expand(WORD.B, WORD.L, WORD.D)
    return LO.word_log_prob_angular2(t["lat"], tab, t["w"], tab[t["ids"]], mask3, W.A).numpy()


def _angular_on(z, gpu, table):
    w = _dev(z["w"], gpu)
    ids = _dev(z["ids"], gpu, torch.int64)
    with torch.no_grad():
        return LT.word_log_prob(_dev(z["lat"], gpu), LT.word_table(table), w, _dev(z["mask"], gpu), W.A, ids=ids)


def test_word_table_follows_a_rewritten_numpy_array(gpu):
    """A CPU float32 table over a numpy array, rewritten in place: the fresh
    torch.from_numpy tensor has the same address and _version 0, and the
    second call must see the new values."""
    z = W.make_inputs(WORD)
    arr = _fresh_table(0).copy()
    assert np.array_equal(arr.astype(np.float64), z["table"])
    first_t = torch.from_numpy(arr)
    first = _angular_on(z, gpu, first_t)
    assert W.lp_ratio(first.cpu(), _table_lp(z, arr.astype(np.float64))) <= 1.0
    new = _fresh_table(1)
    assert W.max_abs_cos({**z, "table": new.astype(np.float64)}) <= W.MAX_COS
    arr[...] = new
    second_t = torch.from_numpy(arr)
    assert second_t.data_ptr() == first_t.data_ptr() and second_t._version == 0 == first_t._version
    second = _angular_on(z, gpu, second_t)
    r = _note("word_table after a numpy rewrite, lp", W.lp_ratio(second.cpu(), _table_lp(z, new.astype(np.float64))))
    assert r <= 1.0, f"the second call is {r:.1f} of the bar from the oracle on the NEW table"
    assert not torch.equal(first, second)
    # and through the drop-in itself
    lat, mask = _dev(z["lat"], gpu), _dev(z["mask"], gpu)
    wv = _dev(_word_table_reference()[1], gpu)
    ids = _dev(z["ids"], gpu, torch.int64)
    with torch.no_grad():
        a = losses.get_word_log_prob_angular(lat, wv, torch.from_numpy(arr), ids, mask, W.A)
        arr[...] = _fresh_table(0)
        b = losses.get_word_log_prob_angular(lat, wv, torch.from_numpy(arr), ids, mask, W.A)
    assert W.lp_ratio(b.cpu(), _word_table_reference()[2]) <= 1.0 and not torch.equal(a, b)


def test_word_table_follows_a_float64_table_rewritten_through_data(gpu):
    z = W.make_inputs(WORD)
    table = _dev(z["table"], gpu, torch.float64)
    first = _angular_on(z, gpu, table)
    new = _fresh_table(1).astype(np.float64)
    version = table._version
    table.data.copy_(_dev(new, gpu, torch.float64))
    assert table._version == version  # (a write through .data moves no version counter)
    second = _angular_on(z, gpu, table)
    r = _note("word_table after a .data rewrite, lp", W.lp_ratio(second.cpu(), _table_lp(z, new)))
    assert r <= 1.0, f"the second call is {r:.1f} of the bar from the oracle on the NEW table"
    assert not torch.equal(first, second)


def test_word_table_still_caches_a_float32_device_table(gpu):
    """The fix keeps the cache where it is sound: a float32 contiguous device
    table is normalised once, and an in-place edit (a version bump) is seen."""
    table = _dev(W.make_inputs(WORD)["table"], gpu)
    a = LT.word_table(table)
    assert LT.word_table(table) is a and a.table.data_ptr() == table.data_ptr()
    table.mul_(2.0)
    assert LT.word_table(table) is not a
    # a strided view at a cached tensor's address, shape and version is another table
    big = _dev(np.arange(2 * WORD.V * WORD.D).reshape(2 * WORD.V, WORD.D) % 7 + 1.0, gpu)
    head = LT.word_table(big[:WORD.V])
    view = LT.word_table(big[::2])
    assert big[::2].data_ptr() == big[:WORD.V].data_ptr() and view is not head
    assert torch.equal(view.table, big[::2]) and torch.equal(head.table, big[:WORD.V])
    sq = _dev(np.arange(WORD.D * WORD.D).reshape(WORD.D, WORD.D) % 5 + 1.0, gpu)
    assert LT.word_table(sq.t()) is not LT.word_table(sq) and torch.equal(LT.word_table(sq.t()).table, sq.t())


# ================================================================ the Gaussians
KEYS2 = next(c for c in G.FAMILY_C if len(c.keys) == 2)  # the smallest two-key case


def _normal_args(gpu):
    z, refs, bars = G.key_reference(KEYS2)
    key = KEYS2.keys[0]
    (mod, _), = G.key_segments(KEYS2, key)
    args = dict(mu=_dev(z["mu"][0], gpu), sigma=_dev(z["sigma"][0], gpu), values=_dev(z["x"][mod], gpu),
                mask=_dev(z["mask"][mod], gpu))
    return z, refs[0], bars[0], args, _dev(z["up"][0], gpu)


def _normal(mu, sigma, values, mask):
    """losses.get_normal_log_prob on [B, F] mu / sigma handed over as the reference's [B, 1, F]."""
    return losses.get_normal_log_prob(mu[:, None, :], sigma[:, None, :], values, mask)


def test_normal_log_prob_presentations(gpu):
    z, ref, bar, args, up = _normal_args(gpu)
    assert z["idx"] is None
    with torch.no_grad():
        lp0 = _normal(**args)
    leaves = {k: args[k].clone().requires_grad_(True) for k in ("mu", "sigma")}
    lp = _normal(**{**args, **leaves})
    (lp * up).sum().backward()
    assert PC.same_result(lp.detach(), lp0)
    _within("get_normal_log_prob lp", lp0, ref[0], bar[0])
    _within("get_normal_log_prob dmu", leaves["mu"].grad, ref[1], bar[1])
    _within("get_normal_log_prob dsigma", leaves["sigma"].grad, ref[2], bar[2])
    with torch.no_grad():
        _sweep("losses.get_normal_log_prob", _normal, args, {k: _tforms(v) for k, v in args.items()}, lp0,
               device=lambda *_: "cuda")
        leaf = args["mu"].clone().requires_grad_(True)  # T5
        assert PC.same_result(_normal(**{**args, "mu": leaf}), lp0)
    _grad_sweep("losses.get_normal_log_prob", lambda kw: (_normal(**kw) * up).sum(), args, ["mu", "sigma"],
                {k: v.grad for k, v in leaves.items()})


def _broadcast_reference(z, mod, row, which=("mu", "sigma")):
    """normal_reference with row `row` of mu / sigma broadcast over the batch,
    and the bar of the broadcast leaves' gradients: the per-row bars summed (the
    errors of the rows add) plus the float32 sum of B rows, (B - 1) u sum |g_b|."""
    B = KEYS2.B
    mu, sg = z["mu"][0], z["sigma"][0]
    if "mu" in which:
        mu = np.broadcast_to(mu[row:row + 1], mu.shape)
    if "sigma" in which:
        sg = np.broadcast_to(sg[row:row + 1], sg.shape)
    x, mask, up = z["x"][mod], z["mask"][mod], z["up"][0]
    ref = G.normal_reference(mu, sg, x, mask, up)
    bar = G.normal_bars(mu, sg, x, mask, up, ref)
    gsum = [r.sum(0, keepdims=True) for r in ref[1:]]
    gbar = [b.sum(0, keepdims=True) + (B - 1) * G.U32 * np.abs(r).sum(0, keepdims=True)
            for r, b in zip(ref[1:], bar[1:])]
    return mu, sg, ref[0], bar[0], gsum, gbar


def test_normal_log_prob_broadcast_mu_and_sigma(gpu):
    """T4: mu / sigma [1, 1, F] expanded over the batch (row stride 0), as the
    reference's expression broadcasts.  The result is that of the materialised
    rows bit for bit; the leaves' gradients are the sums over the batch."""
    z, _, _, args, up = _normal_args(gpu)
    (mod, _), = G.key_segments(KEYS2, KEYS2.keys[0])
    B, F = args["mu"].shape
    mu_b, sg_b, lp_ref, lp_bar, gsum, gbar = _broadcast_reference(z, mod, 3)
    full = dict(args, mu=_dev(mu_b, gpu), sigma=_dev(sg_b, gpu))
    with torch.no_grad():
        lp0 = _normal(**full)
    _within("get_normal_log_prob broadcast lp", lp0, lp_ref, lp_bar)
    for which in (("mu",), ("sigma",), ("mu", "sigma")):
        leaves = {k: full[k][:1].reshape(1, 1, F).clone().requires_grad_(True) for k in which}
        shown = {k: v.expand(B, 1, F) for k, v in leaves.items()}
        assert all(v.stride(0) == 0 for v in shown.values())
        snaps = {k: PC.snapshot(v) for k, v in leaves.items()}
        rest = {k: full[k][:, None, :] for k in ("mu", "sigma") if k not in which}
        lp = losses.get_normal_log_prob(values=args["values"], mask=args["mask"], **shown, **rest)
        _COUNT["losses.get_normal_log_prob"] = _COUNT.get("losses.get_normal_log_prob", 0) + 1
        assert PC.same_result(lp.detach(), lp0), which
        (lp * up).sum().backward()
        for k, leaf in leaves.items():
            assert leaf.grad.shape == leaf.shape and leaf.grad.device == leaf.device
            j = ("mu", "sigma").index(k)
            _within(f"get_normal_log_prob broadcast d{k}", leaf.grad.reshape(1, F), gsum[j], gbar[j])
            assert PC.unchanged(leaf, snaps[k])


def test_gauss_log_prob_presentations(gpu):
    """latent.gauss_log_prob over both keys, with idx: mu / sigma of one key at
    a time in every form; idx on the CPU, as int32 and as a stepped view."""
    c = KEYS2
    z, refs, bars = G.key_reference(c)
    st = {m: None if z["x"][m] is None else LT.gauss_stats(_dev(z["x"][m], gpu), _dev(z["mask"][m], gpu))
          for m in G.MODS}
    stats = LT.GaussStats(**st)
    keys = list(c.keys)
    up = _dev(z["up"], gpu)
    args = {"idx": torch.arange(c.B, device=gpu)}
    for k in range(2):
        args[f"mu{k}"], args[f"sigma{k}"] = _dev(z["mu"][k], gpu), _dev(z["sigma"][k], gpu)
    fn = lambda idx, mu0, mu1, sigma0, sigma1: LT.gauss_log_prob(stats, keys, [mu0, mu1], [sigma0, sigma1],  # noqa: E731
                                                                idx=idx)
    floats = [k for k in args if k != "idx"]
    leaves = {k: args[k].clone().requires_grad_(True) for k in floats}
    lp = fn(**{**args, **leaves})
    (lp * up).sum().backward()
    with torch.no_grad():
        lp0 = fn(**args)
        assert PC.same_result(lp0, LT.gauss_log_prob(stats, keys, [args["mu0"], args["mu1"]],
                                                     [args["sigma0"], args["sigma1"]]))  # idx = 0 .. B
    assert PC.same_result(lp.detach(), lp0)
    for k in range(2):
        _within("gauss_log_prob lp", lp0[k], refs[k][0], bars[k][0])
        _within("gauss_log_prob dmu", leaves[f"mu{k}"].grad, refs[k][1], bars[k][1])
        _within("gauss_log_prob dsigma", leaves[f"sigma{k}"].grad, refs[k][2], bars[k][2])
    spec = {k: _tforms(args[k]) for k in floats}
    spec["idx"] = [("T1", PC.t_cpu), ("T3b", PC.t_stepped), ("T6-int32", PC.t_int32)]
    with torch.no_grad():
        _sweep("latent.gauss_log_prob", fn, args, spec, lp0, device=lambda *_: "cuda")
    _grad_sweep("latent.gauss_log_prob", lambda kw: (fn(**kw) * up).sum(), args, floats,
                {k: v.grad for k, v in leaves.items()})
    # T4 on one key, the other contiguous: bit for bit the materialised rows
    F0 = args["mu0"].shape[1]
    row = args["mu0"][:1].clone().requires_grad_(True)
    mat = row.detach().expand(c.B, F0).contiguous()
    got = fn(**{**args, "mu0": row.expand(c.B, F0)})
    assert PC.same_result(got.detach(), fn(**{**args, "mu0": mat}).detach())
    (got * up).sum().backward()
    assert row.grad.shape == row.shape and row.grad.device == row.device
    # the leaf's gradient is the batch sum of the materialised rows' dmu, held to the oracle's
    (mod, _), = G.key_segments(c, keys[0])
    _, _, lp_ref, lp_bar, gsum, gbar = _broadcast_reference(z, mod, 0, which=("mu",))
    _within("gauss_log_prob broadcast lp", got[0], lp_ref, lp_bar)
    _within("gauss_log_prob broadcast dmu", row.grad, gsum[0], gbar[0])
    _COUNT["latent.gauss_log_prob"] += 1


def test_layer_norm_presentations(gpu):
    c = G.LNCase(5, 65, "wide")
    z, _, _ = G.ln_case(c)
    x, dy, gamma = _dev(z["x"], gpu), _dev(z["dy"], gpu), _dev(z["gamma"], gpu)
    beta = _dev(np.linspace(-1.0, 1.0, c.d), gpu)

    def run(x, gamma, beta):
        return LT.layer_norm(x, gamma, beta, G.LN_EPS)

    leaves = {"x": x.clone().requires_grad_(True), "gamma": gamma.clone().requires_grad_(True),
              "beta": beta.clone().requires_grad_(True)}
    y = run(**leaves)
    (y * dy).sum().backward()
    _, mean, rstd = torch.native_layer_norm(x, [c.d], gamma, beta, G.LN_EPS)
    ref, bars = G.layer_norm_backward_reference(z["dy"], z["x"], mean.reshape(-1).cpu().numpy().astype(np.float64),
                                                rstd.reshape(-1).cpu().numpy().astype(np.float64), z["gamma"])
    for name, leaf, r, b in zip(("dx", "dgamma", "dbeta"), leaves.values(), ref, bars):
        _within(f"layer_norm {name}", leaf.grad, r, b)
    args = dict(x=x, gamma=gamma, beta=beta)
    y0 = run(**args).detach()
    assert PC.same_result(y.detach(), y0)
    # float64 is not a presentation here: the reference's LayerNorm rejects a float64 input beside
    # float32 parameters (RuntimeError, mixed dtypes) and so does the mirror (MMBError is one)
    with pytest.raises(RuntimeError):
        torch.nn.functional.layer_norm(x.double(), [c.d], gamma, beta, G.LN_EPS)
    with pytest.raises(RuntimeError):
        run(x.double(), gamma, beta)
    t3 = lambda t: [(k, f) for k, f in _tforms(t) if k != "T2"]  # noqa: E731
    with torch.no_grad():
        _sweep("latent.layer_norm", run, args, {k: t3(v) for k, v in args.items()}, y0, device=lambda *_: "cuda")
    bad = []
    for arg in args:
        for pid, build in t3(args[arg]):
            leaf = build(args[arg]).detach().requires_grad_(True)
            (run(**{**args, arg: leaf}) * dy).sum().backward()
            _COUNT["latent.layer_norm (gradients)"] = _COUNT.get("latent.layer_norm (gradients)", 0) + 1
            want = leaves[arg].grad
            if leaf.grad.shape != leaf.shape or not np.array_equal(PC.bits(leaf.grad), PC.bits(want)):
                bad.append(f"{arg} as {pid}")
    assert not bad, bad


# ================================================================ the whole objective
def test_log_prob_matrix_presentations(gpu):
    """losses.get_log_prob_matrix on the generator's own outputs (column blocks
    of its fused linear's result): the data and mask tensors of the Gaussians
    and of the word model in every form; strided latents' gradients."""
    c = G.FAMILY_F[0]
    z, total_r, dlat_r, _ = G.matrix_reference(c)
    gen = G.make_generator(c).to(gpu)
    t, data, masks = G.matrix_data(z, list(gen.embed2out), lambda a: _dev(a, gpu))

    def wfn(latents, word_weights, sent, mask):
        return losses.get_word_log_prob_angular2(latents, t["table"], word_weights, sent, mask, G.WORD_A)

    def total_of(x, **over):
        d, m = dict(data), dict(masks)
        for k, v in over.items():
            kind, key = k.split(":")
            (d if kind == "data" else m)[key] = v
        return losses.get_log_prob_matrix(G.ARGS, x, gen(x), d, m, wfn)

    x = t["lat"].clone().requires_grad_(True)
    total = total_of(x)
    (-total).mean().backward()
    _within("get_log_prob_matrix total", total, total_r, G.LP_RTOL * np.abs(total_r) + G.LP_ATOL)
    _within("get_log_prob_matrix dlat", x.grad, dlat_r,
            np.broadcast_to(G.GRAD_TOL * np.abs(dlat_r).max(1, keepdims=True), dlat_r.shape))
    assert masks["text"].stride(2) == 0  # (T4: the reference's text mask is an expand)
    keys = list(gen.embed2out)
    shown = ["text", "text_weights", keys[0], keys[-1]]
    args = {f"data:{k}": data[k].contiguous() for k in shown}
    args.update({f"mask:{k}": masks[k].contiguous() for k in ("text", keys[0], keys[-1])})
    with torch.no_grad():
        base = total_of(t["lat"])
        assert PC.same_result(base, total.detach())
        _sweep("losses.get_log_prob_matrix", lambda **kw: total_of(t["lat"], **kw), args,
               {k: _tforms(v) for k, v in args.items()}, base, device=lambda *_: "cuda")
    # float64 latents are no presentation here: the reference's generator is torch modules with float32
    # parameters, which reject them (RuntimeError: mixed dtypes), and so does the mirror's
    with pytest.raises(RuntimeError):
        torch.nn.Sequential(torch.nn.LayerNorm(c.D), torch.nn.Linear(c.D, 4)).to(gpu)(t["lat"].double())
    with pytest.raises(RuntimeError):
        total_of(t["lat"].double())
    bad = []
    for pid, build in [f for f in _tforms(t["lat"]) if f[0] != "T2"]:
        leaf = build(t["lat"]).detach().requires_grad_(True)
        (-total_of(leaf)).mean().backward()
        _COUNT["losses.get_log_prob_matrix (gradients)"] = _COUNT.get("losses.get_log_prob_matrix (gradients)", 0) + 1
        if leaf.grad.shape != leaf.shape or not np.array_equal(PC.bits(leaf.grad), PC.bits(x.grad)):
            bad.append(pid)
    assert not bad, bad


# ================================================================ the regressor
def _regressor(gpu, o):
    c = RC.FwdCase(PC.REGRESSOR["d"], PC.REGRESSOR["h"], o, PC.REGRESSOR["b"])
    z = RC.fwd_inputs(c)
    m = SM.SentimentModel(c.d, c.h, c.o)
    with torch.no_grad():
        for p, v in zip((m.hidden1.weight, m.hidden1.bias, m.out.weight, m.out.bias), z["params"]):
            p.copy_(torch.as_tensor(np.array(v), dtype=torch.float32))
    return c, z, m.to(gpu)


@pytest.mark.parametrize("o", [1, 2])
def test_sentiment_model_presentations(gpu, o):
    c, z, m = _regressor(gpu, o)
    x = _dev(z["x"], gpu)
    dy = _dev(z["dy"], gpu)
    with torch.no_grad():
        y0 = m(x)
    RG._check(lambda g, what, r: _note(what, r), "", f"SentimentModel o={o} no-grad",
              RG._host64(y0).reshape(c.b, c.o), z["y"], z["y_bound"])
    for p in m.parameters():
        p.requires_grad_(False)
    fn = lambda inputs: m(inputs)  # noqa: E731
    with torch.no_grad():  # (the result comes back on the caller's device)
        _sweep(f"SentimentModel.forward no-grad o={o}", fn, dict(inputs=x), {"inputs": _tforms(x, cpu=True)}, y0,
               device=lambda arg, pid, shown: shown.device.type)
    # T5: a requires_grad leaf under no_grad takes the no-grad kernel; the result is the same
    with torch.no_grad():
        assert PC.same_result(m(x.clone().requires_grad_(True)), y0)
    _COUNT[f"SentimentModel.forward no-grad o={o}"] += 1
    # the differentiable path
    leaf = x.clone().requires_grad_(True)
    y = m(leaf)
    assert y.requires_grad and y.shape == y0.shape
    (y.reshape(c.b, c.o) * dy).sum().backward()
    RG._check(lambda g, what, r: _note(what, r), "", f"SentimentModel o={o} autograd y",
              RG._host64(y.detach()).reshape(c.b, c.o), z["y"], z["y_bound"])
    for pid, build in _tforms(x):
        shown = build(x).detach().requires_grad_(True)
        assert PC.same_result(m(shown).detach(), y.detach()), pid
    _grad_sweep(f"SentimentModel.forward autograd o={o}", lambda kw: (m(kw["inputs"]).reshape(c.b, c.o) * dy).sum(),
                dict(inputs=x), ["inputs"], {"inputs": leaf.grad})


@pytest.mark.parametrize("o", [1, 2])
def test_predict_sentiment_presentations(gpu, o):
    from torch.utils.data import DataLoader

    c, z, m = _regressor(gpu, o)
    labels = z["labels"][:, 0] if o == 1 else z["labels"]
    loader = DataLoader(SM.SentimentData(np.array(labels), gpu), batch_size=32, shuffle=True)

    def fn(latents):
        torch.manual_seed(5)  # the loader's order comes from the global RNG
        return SM.predict_sentiment(loader, m, latents)

    lat = _dev(z["x"], gpu)
    pred0, y0 = fn(lat)
    torch.manual_seed(5)
    order = torch.cat(SM._epoch_batches(loader)).numpy()
    RG._check(lambda g, what, r: _note(what, r), "", f"predict_sentiment o={o}",
              pred0.astype(np.float64).reshape(c.b, c.o), z["y"][order], z["y_bound"][order])
    assert np.array_equal(y0.reshape(c.b, c.o), z["labels"][order].astype(np.float32)[:, :c.o])
    _sweep(f"sentiment_model.predict_sentiment o={o}", fn, dict(latents=lat), {"latents": _tforms(lat, cpu=True)},
           (pred0, y0))


# ================================================================ sif2.calc_weights
def test_calc_weights_presentations(gpu):
    rng = np.random.default_rng(52)
    data = W.f32(rng.standard_normal((5, 7, 12)))
    bm, bls = W.f32(rng.standard_normal(12)), W.f32(0.3 * rng.standard_normal(12))
    args = dict(data=_dev(data, gpu), b_mean=_dev(bm, gpu), b_log_sigma=_dev(bls, gpu))
    fn = lambda data, b_mean, b_log_sigma: sif2.calc_weights(data, b_mean, b_log_sigma, None)  # noqa: E731
    qm0, qs0 = fn(**args)
    rm, rs = M.calc_weights(data, bm, bls)
    # (the bars of tests/test_gpu_mmb2.py::test_calc_weights)
    np.testing.assert_allclose(qm0.cpu().numpy(), rm, rtol=2e-6, atol=1e-6)
    np.testing.assert_allclose(qs0.cpu().numpy(), rs, rtol=2e-6, atol=1e-5)
    spec = {k: _tforms(v, cpu=True) for k, v in args.items()}
    _sweep("sif2.calc_weights", fn, args, spec, (qm0, qs0),
           device=lambda arg, pid, shown: shown.device.type if arg == "data" else "cuda")
    # T5: requires_grad leaves into the no-grad drop-in, outside torch.no_grad()
    assert torch.is_grad_enabled()
    for k in args:
        leaf = args[k].clone().requires_grad_(True)
        got = fn(**{**args, k: leaf})
        _COUNT["sif2.calc_weights"] += 1
        assert all(PC.same_result(g, b) and not g.requires_grad for g, b in zip(got, (qm0, qs0))), k


# ================================================================ the pipeline mirrors refuse another element type
def _wrong(t):
    """The operand in another element type at least as wide as the expected
    one: float32 as float64, int32 as int64, and float64 as int64 (the same
    width) -- even an unchecked mirror would read inside the buffer."""
    if t.dtype == torch.float64:
        return t.to(torch.int64)
    return t.double() if t.is_floating_point() else t.to(torch.int64)


REFUSALS = "pipeline mirrors, mistyped operand refused"


def _refused(call, outs=()):
    """`call` raises MMBError naming a dtype before anything is launched: the
    sentinel-filled outputs the caller owns are untouched."""
    for o in outs:
        o.fill_(-7.0)
    with pytest.raises(L.MMBError, match="torch"):
        call()
    assert _untouched(outs)
    _COUNT[REFUSALS] = _COUNT.get(REFUSALS, 0) + 1


def _each_wrong(fn, args, operands, outs=()):
    """fn(**args) with one operand at a time handed over in a wrong type."""
    for k in operands:
        _refused(lambda: fn(**{**args, k: _wrong(args[k])}), outs)  # noqa: B023


def test_pipeline_mirrors_refuse_mistyped_operands(gpu):
    z = PC.sif_inputs()
    table, ids32, w = _dev(z.We, gpu), _dev(z.ids, gpu, torch.int32), _dev(z.w, gpu)
    wtab32, wtab64 = _dev(z.weights, gpu), _dev(z.weights, gpu, torch.float64)
    n, d = PC.SIF_N, PC.SIF_D
    x = P.weighted_sum(table, ids32, w=w, x_out=True)
    num, cnt = P.weighted_sum(table, ids32, w=w)
    x64 = x.double()
    torch.cuda.synchronize()
    # seq2weight: seq and wtab64
    _each_wrong(P.seq2weight, dict(seq32=ids32, sel=None, wtab64=wtab64), ("seq32", "wtab64"))
    # weighted_sum: w, wtab32, ids32, on both output routes
    for x_out in (False, True):
        _each_wrong(P.weighted_sum, dict(table=table, ids32=ids32, w=w, x_out=x_out), ("w", "ids32"))
        _each_wrong(P.weighted_sum, dict(table=table, ids32=ids32, wtab32=wtab32, x_out=x_out), ("wtab32",))
    # gram / xt_omega / remove_pc: num and cnt; omega_rows; pc
    G64 = torch.empty((d, d), dtype=torch.float64, device=gpu)
    _each_wrong(P.gram, dict(num=num, cnt=cnt, G=G64), ("num", "cnt"), [G64])
    om = P.omega(n, 11, gpu).contiguous()
    _each_wrong(P.xt_omega, dict(num=num, cnt=cnt, omega_rows=om), ("num", "cnt", "omega_rows"))
    _each_wrong(P.xt_omega_f64, dict(x64=x64, cnt=None, omega_rows=om), ("x64", "omega_rows"))
    pc = torch.zeros((1, d), dtype=torch.float64, device=gpu)
    pc[0, 0] = 1.0
    for out in (torch.empty((n, d), dtype=torch.float32, device=gpu),
                torch.empty((n, d), dtype=torch.float64, device=gpu)):
        _each_wrong(P.remove_pc, dict(num=num, cnt=cnt, pc=pc, out=out), ("num", "cnt", "pc"), [out])
    _each_wrong(P.remove_pc_f64, dict(x64=x64, pc=pc), ("x64", "pc"))
    _refused(lambda: P.pc_f64(_wrong(x64), 1))
    # colmax / gram_i8: x and cmax
    cm = torch.zeros(d, dtype=torch.int32, device=gpu)
    _refused(lambda: P.colmax(_wrong(x), cm))
    assert not cm.any().item()
    cm = P.colmax(x)
    _each_wrong(P.gram_i8, dict(x=x, cmax=cm, G=G64), ("x", "cmax"), [G64])
    # pc_solve: G and z0, on the multi-workgroup solver (d <= 320) and past it
    for dd in (d, P.PC_SOLVE_MC_MAX_D + 4):
        Gd = torch.eye(dd, dtype=torch.float64, device=gpu)
        z0 = P.omega(dd, 11, gpu).contiguous()
        pco = torch.empty((1, dd), dtype=torch.float64, device=gpu)
        _each_wrong(P.pc_solve, dict(G=Gd, z0=z0, npc=1, transposed=False, out=pco), ("G", "z0"), [pco])
    # mm2_stream's text operands, gathered and dense, on both s layouts
    A, Vd, T = 8, 12, PC.SIF_L
    rng = np.random.default_rng(7)
    audio, visual = _dev(rng.standard_normal((n, T, A)), gpu), _dev(rng.standard_normal((n, T, Vd)), gpu)
    kp = P.mm2_dims(d, A, Vd)[0]
    text = _dev(rng.standard_normal((n, T, d)), gpu)
    for s_half in (True, False):
        outs = (torch.empty((n, d), device=gpu), P.s_buffer(n, kp, s_half, gpu), torch.empty((3, n), device=gpu))
        head = dict(n=n, t=T, d=d, a=A, vd=Vd, audio=audio, visual=visual, out=outs, s_half=s_half)
        _each_wrong(P.mm2_stream, dict(head, ids32=ids32, table=table, wtab32=wtab32), ("ids32", "wtab32"),
                    [outs[0], outs[2]])
        _each_wrong(P.mm2_stream, dict(head, ids32=ids32, table=table, w_dense=w), ("w_dense",), [outs[0], outs[2]])
        _each_wrong(P.mm2_stream, dict(head, text_dense=text, emb_dense=text, w_dense=w),
                    ("text_dense", "emb_dense", "w_dense"), [outs[0], outs[2]])


def test_stream_family_refuses_mistyped_text_operands(gpu):
    """The rest of the mm2_stream* family, at a shape every fused entry point
    supports: the split route, mm2_stream_split_ft, the four fused mirrors and
    mm2_stream_project_tt, each with ids32 / wtab32 / w_dense / text_dense in a
    wider type.  Every call raises at the hand-over, before its launch."""
    case = C.NARROW_FUSED[1]  # (260, 76, 48, 20) at 31 rows, V = 3016
    D, A, Vd, T, N, V = case
    assert P.stream_project_supported(T, D, A, Vd) and P.narrow_fused_supported(T, D, A, Vd, V)
    inp = _device_inputs(case, gpu)
    z = C.inputs(case)
    ids32, table, wtab32 = inp["ids"], inp["table"], inp["wtab"]
    w, text = _dev(z["sw"], gpu), _dev(z["text"], gpu)
    proj = P.MMB2Projection(_networks(case, gpu), D, A, Vd, T, gpu)
    kp = proj.kp
    shape = dict(n=N, t=T, d=D, a=A, vd=Vd, audio=inp["audio"], visual=inp["visual"])
    # the split route of mm2_stream, and mm2_stream_split_ft
    outs = (torch.empty((N, D), device=gpu), P.s_buffer(N, kp, True, gpu), torch.empty((3, N), device=gpu))
    split = dict(shape, out=outs, split=P.split_ws(N, T, D, A, Vd, gpu, 2), parts=2)
    keep = [outs[0], outs[2]]
    _each_wrong(P.mm2_stream, dict(split, ids32=ids32, table=table, wtab32=wtab32), ("ids32", "wtab32"), keep)
    _each_wrong(P.mm2_stream, dict(split, text_dense=text, emb_dense=text, w_dense=w),
                ("text_dense", "emb_dense", "w_dense"), keep)
    _each_wrong(P.mm2_stream_split_ft, dict(split, ids32=ids32, table=table, wtab32=wtab32), ("ids32", "wtab32"), keep)
    _each_wrong(P.mm2_stream_split_ft, dict(split, ids32=ids32, table=table, w_dense=w), ("w_dense",), keep)
    # the fused mirrors: (x, aux, mmb2) are the caller's
    fused = (torch.empty((N, D), device=gpu), torch.empty((3, N), device=gpu), torch.empty((N, D), device=gpu))
    head = dict(shape, proj=proj, out=fused)
    gathered = dict(head, ids32=ids32, table=table, wtab32=wtab32)
    for mirror in (P.mm2_stream_project_narrow, P.mm2_stream_project_narrow_ft):
        _each_wrong(mirror, gathered, ("ids32", "wtab32"), fused)
    for mirror in (P.mm2_stream_project, P.mm2_stream_project_ft, P.mm2_stream_project_tt):
        _each_wrong(mirror, gathered, ("ids32", "wtab32"), fused)
        _each_wrong(mirror, dict(head, ids32=ids32, table=table, wtab32=None, w_dense=w), ("w_dense",), fused)
    _each_wrong(P.mm2_stream_project, dict(head, text_dense=text, w_dense=w), ("text_dense", "w_dense"), fused)
    # float32-only entry points state float32 for the frames as well
    half = dict(gathered, audio=inp["audio"].half(), visual=inp["visual"].half())
    for mirror in (P.mm2_stream_project, P.mm2_stream_project_narrow):
        _refused(lambda: mirror(**half), fused)  # noqa: B023
    # and the family still runs on well-typed operands after the refusals
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    x, aux, mmb2 = P.mm2_stream_project_narrow(**gathered, flag=flag)
    assert int(flag.item()) == 0
    assert M.row_rel_err(mmb2.cpu().numpy(), C.oracle_rows(case)) < TOL


def test_fused_step_checks_ids_and_wtab_at_construction(gpu):
    """FusedStep states the ids' and the weight table's element type once, beside
    frame_kind and table_kind: int64 ids would be read as pairs of int32."""
    dims = C.STEP[0]
    case = C.case_of(dims[:4], dims[4])
    inputs, nets = _device_inputs(case, gpu), _networks(case, gpu)
    with pytest.raises(L.MMBError, match=r"inputs\['ids'\] must be torch.int32, not torch.int64"):
        P.FusedStep({**inputs, "ids": inputs["ids"].long()}, nets)
    with pytest.raises(L.MMBError, match=r"inputs\['wtab'\] must be torch.float32, not torch.float64"):
        P.FusedStep({**inputs, "wtab": inputs["wtab"].double()}, nets)
    step = P.FusedStep(inputs, nets)
    sif_rows, mm2 = step.run(check=True)
    _check_step(lambda g, what, r: _note(what, r), case, step, sif_rows, mm2)


# ================================================================ sif2.estimate_embedding_overall_gpu2
MMB2 = C.case_of((52, 8, 12, 7))  # tests/test_mmb2_cases.py pins its conditions


@pytest.mark.parametrize("own_text", [True, False], ids=["embeddings-is-text", "separate"])
def test_estimate_embedding_presentations(gpu, own_text):
    D, A, Vd, T, N, V = MMB2
    z = C.inputs(MMB2)
    host = M.concat_inputs(z["text"], z["audio"], z["visual"])
    data = {k: _dev(v, gpu) for k, v in host.items()}
    nets = _networks(MMB2, gpu)
    masks = {k: None for k in data}
    sw = _dev(z["sw"], gpu)

    def fn(sentence_weights, embeddings=None, **mods):
        d = {**data, **mods}
        emb = d["text"] if embeddings is None else embeddings
        with torch.no_grad():
            return sif2.estimate_embedding_overall_gpu2(d, masks, nets, sentence_weights, emb)

    args = dict(sentence_weights=sw, text=data["text"], audio=data["audio"], visual=data["visual"])
    if not own_text:
        args["embeddings"] = data["text"].clone()
    base = fn(**args)
    ref = M.estimate_embedding_overall_gpu2(host, C.params(D, A, Vd), z["sw"], z["text"])
    assert base.dtype == torch.float32 and base.shape == (N, D)
    assert _note("estimate_embedding_overall_gpu2", M.row_rel_err(base.cpu().numpy(), ref) / TOL) < 1.0
    # the modalities and the combination tensors in every form; a combination as a real torch.cat result
    # (the baseline) and as a view (T3a / T3b / T3c of it)
    spec = {k: _tforms(v, cpu=True) for k, v in args.items()}
    home = "text" if own_text else "embeddings"  # (the result comes back on the embeddings' device)
    _sweep(f"sif2.estimate_embedding_overall_gpu2 ({'text' if own_text else 'separate'} embeddings)", fn, args, spec,
           base, device=lambda arg, pid, shown: shown.device.type if arg == home else "cuda")
    # T5: requires_grad leaves into the no-grad drop-in, outside torch.no_grad()
    assert torch.is_grad_enabled()
    for k in args:
        leaf = args[k].clone().requires_grad_(True)
        d = {**data, **{m: (leaf if m == k else args[m]) for m in ("text", "audio", "visual")}}
        sw_, emb = (leaf if k == "sentence_weights" else sw), (leaf if k == "embeddings" else args.get("embeddings"))
        got = sif2.estimate_embedding_overall_gpu2(d, masks, nets, sw_, d["text"] if emb is None else emb)
        _COUNT["sif2.estimate_embedding_overall_gpu2 (T5)"] = _COUNT.get("sif2.estimate_embedding_overall_gpu2 (T5)", 0) + 1
        assert PC.same_result(got, base) and not got.requires_grad, k
    combos = {k: data[k] for k in ("audiovisual", "textaudiovisual")}
    _sweep("sif2.estimate_embedding_overall_gpu2 (combination tensors)", lambda **kw: fn(**args, **kw), combos,
           {k: _tforms(v) for k, v in combos.items()}, base)


def test_estimate_embedding_other_length_presentations(gpu):
    """L = 9 != T: the weighted text average over the embeddings' own length."""
    D, A, Vd, T, N, V = MMB2
    z = C.inputs(MMB2)
    Lw = 9
    ids = synth_ids(N, Lw, V)
    emb_h, sw_h = z["E"][ids], z["wt32"][ids]
    host = M.concat_inputs(z["text"], z["audio"], z["visual"])
    data = {k: _dev(v, gpu) for k, v in host.items()}
    nets = _networks(MMB2, gpu)
    masks = {k: None for k in data}

    def fn(sentence_weights, embeddings):
        with torch.no_grad():
            return sif2.estimate_embedding_overall_gpu2(data, masks, nets, sentence_weights, embeddings)

    args = dict(sentence_weights=_dev(sw_h, gpu), embeddings=_dev(emb_h, gpu))
    base = fn(**args)
    ref = M.estimate_embedding_overall_gpu2(host, C.params(D, A, Vd), sw_h, emb_h)
    assert _note("estimate_embedding_overall_gpu2, L != T", M.row_rel_err(base.cpu().numpy(), ref) / TOL) < 1.0
    _sweep("sif2.estimate_embedding_overall_gpu2 (L != T)", fn, args, {k: _tforms(v, cpu=True) for k, v in args.items()},
           base, device=lambda arg, pid, shown: shown.device.type if arg == "embeddings" else "cuda")


def synth_ids(n, l, v):
    ids = np.random.default_rng([n, l, v]).integers(1, v, size=(n, l))
    ids[:, -2:] = 0  # pads weigh like any word here (the reference ignores the masks)
    return ids
