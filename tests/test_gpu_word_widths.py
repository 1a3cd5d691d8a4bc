"""GPU parity of the word log-likelihood kernels at table widths other than 300.

latent.word_log_prob (losses.get_word_log_prob_angular* under it) reaches
word_zsum_kernel<NT> of csrc/latent_kernels.hip, instantiated per 16-column
tile count NT = pad16(D) / 16 = 1..20; every other test uses a 300-d table
(NT 19, 4 padded columns).  The table of tests/word_cases.py holds widths
from 4 to 320 -- GloVe's 50 / 100 / 200 among them -- with fewer words than
one tile, fewer tiles than waves and ragged latent tiles; the reference is
oracle.latent_oracle.word_log_prob_angular2 in float64.  Tokens by id and
dense, with and without gradient.

Bars (the ones tests/test_gpu_latent.py states):
  lp        |y - y_ref| <= 2e-5 |y_ref| + 1e-4
  gradient  per row, max |g - g_ref| <= 2e-4 max |g_ref|

tests/test_word_cases.py (CPU) pins that no cosine of a case passes 0.99 (the
gradient holds 1 / sqrt(1 - cos^2)).  D = 321 is rejected (MMBError) with
nothing launched.

Measured on MI355X (the module prints these at its end): 96 lp comparisons,
largest 0.004 of the bar; 48 gradients, largest 0.003 of the bar.  Before the
kernels wrote (1 - alpha) / Z as a alpha, the gradient at (D 15, V 1), dense
tokens, was 1.18 of its bar: 1.f - alpha loses 2^-24 / (a Z) of itself, 1.2e-4
where one word makes a Z = 5e-4.
"""
import numpy as np
import pytest
import torch

import latent as LT
import mmb_lib as L
import word_cases as W
from common_gpu import Ledger
from common_gpu import _dev32 as _dev  # float32 unless told otherwise
from word_cases import grad_ratio, lp_ratio

pytestmark = pytest.mark.gpu

_WORST = Ledger()
_note = _WORST.note  # (what, ratio)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for what, (n, r) in sorted(_WORST.items()):
        print(f"\nword widths {what}: {n} comparisons, largest {r:.3f} of its bar", end="")
    print()


@pytest.mark.parametrize("dense", [False, True], ids=["ids", "dense"])
@pytest.mark.parametrize("c", W.WORD_CASES, ids=[W.word_id(c) for c in W.WORD_CASES])
def test_word_log_prob_vs_float64(gpu, c, dense):
    z, lp_ref, g_ref = W.reference(c, dense)
    assert W.max_abs_cos(z) <= W.MAX_COS
    wt = LT.WordTable(_dev(z["table"], gpu))
    assert wt.Dp == -(-c.D // 16) * 16 and wt.wn.shape == (c.V, wt.Dp)
    w, mask, up = _dev(z["w"], gpu), _dev(z["mask"], gpu), _dev(z["up"], gpu)
    tok = {"sent_dense": _dev(z["dense"], gpu)} if dense else {"ids": _dev(z["ids"], gpu, torch.int64)}
    with torch.no_grad():  # want_grad = 0: no G product, no state
        lp0 = LT.word_log_prob(_dev(z["lat"], gpu), wt, w, mask, W.A, **tok)
    assert not lp0.requires_grad
    r = _note("lp, no gradient", lp_ratio(lp0.cpu(), lp_ref))
    assert r <= 1.0, f"lp (no gradient) {r:.3f} of the bar"
    x = _dev(z["lat"], gpu).requires_grad_(True)
    lp = LT.word_log_prob(x, wt, w, mask, W.A, **tok)
    (lp * up).sum().backward()
    r = _note("lp, with gradient", lp_ratio(lp.detach().cpu(), lp_ref))
    assert r <= 1.0, f"lp {r:.3f} of the bar"
    assert torch.equal(lp.detach(), lp0)  # the same Z whether or not G is accumulated
    assert np.abs(g_ref).max(1).min() > 0
    r = _note("gradient", grad_ratio(x.grad.cpu(), g_ref))
    assert r <= 1.0, f"gradient {r:.3f} of the bar"


def test_normalised_table_is_zero_padded(gpu):
    """The MFMA tiles read pad16(D) columns: the normalised table's pad is zero
    and its rows are unit (GloVe 50: 14 padded columns)."""
    c = next(c for c in W.WORD_CASES if c.D == 50 and c.V == 517)
    z = W.make_inputs(c)
    wt = LT.WordTable(_dev(z["table"], gpu))
    wn = wt.wn.cpu().numpy().astype(np.float64)
    assert wn.shape == (517, 64) and not wn[:, 50:].any()
    ref = z["table"] / np.linalg.norm(z["table"], axis=1, keepdims=True)
    # the norm: a 50-term sum of squares ((D + 1) u, halved by the root), the root, the division; x2
    assert (np.abs(wn[:, :50] - ref) <= 2 * ((50 + 1) / 2 + 2) * 2.0 ** -24 * np.abs(ref)).all()


@pytest.mark.parametrize("dense", [False, True], ids=["ids", "dense"])
def test_width_321_is_rejected(gpu, dense):
    """One past the widest instantiation: MMB_EINVAL from the forward and from
    the backward, before any launch (lp and dlat keep their sentinel)."""
    D, V, B, Lt = 321, 17, 3, 2
    rng = np.random.default_rng(321)
    table = _dev(rng.standard_normal((V, D)), gpu)
    wt = LT.WordTable(table)  # the normalisation serves any width
    lat = _dev(rng.standard_normal((B, D)), gpu)
    w, mask = torch.ones(B, Lt, device=gpu), torch.ones(B, Lt, device=gpu)
    tok = {"sent_dense": _dev(rng.standard_normal((B, Lt, D)), gpu)} if dense else \
        {"ids": _dev(rng.integers(0, V, (B, Lt)), gpu, torch.int64)}
    with pytest.raises(L.MMBError):
        LT.word_log_prob(lat.clone().requires_grad_(True), wt, w, mask, W.A, **tok)
    with pytest.raises(L.MMBError):
        with torch.no_grad():
            LT.word_log_prob(lat, wt, w, mask, W.A, **tok)
    # the C entry points themselves, every buffer at full size
    ids = tok["ids"].to(torch.int32) if not dense else None
    sent = tok["sent_dense"] if dense else None
    ws = torch.zeros(max(L.query("mmb_word_workspace_bytes", B, D, V), 16), dtype=torch.uint8, device=gpu)
    lp = torch.full((B,), np.nan, device=gpu)
    state, gsum = torch.full((B, 4), np.nan, device=gpu), torch.full((B, wt.Dp), np.nan, device=gpu)
    cosv, dlat = torch.full((B, Lt), np.nan, device=gpu), torch.full((B, D), np.nan, device=gpu)
    rc = L.query("mmb_word_logprob_forward", L.ptr(lat), B, D, L.ptr(wt.wn), V, L.ptr(ids),
                 L.ptr(wt.table) if ids is not None else None, L.ptr(sent), Lt, L.ptr(w), L.ptr(mask), W.A, 1,
                 L.ptr(ws), L.ptr(lp), L.ptr(state), L.ptr(gsum), L.ptr(cosv), L.stream_ptr())
    assert rc == -1
    st_in, g_in = torch.ones(B, 4, device=gpu), torch.zeros(B, wt.Dp, device=gpu)
    cos_in, dlp = torch.zeros(B, Lt, device=gpu), torch.ones(B, device=gpu)
    rc = L.query("mmb_word_logprob_backward", L.ptr(lat), B, D, V, L.ptr(ids),
                 L.ptr(wt.table) if ids is not None else None, L.ptr(sent), Lt, L.ptr(w), L.ptr(mask), W.A,
                 L.ptr(st_in), L.ptr(g_in), L.ptr(cos_in), L.ptr(dlp), L.ptr(dlat), L.stream_ptr())
    assert rc == -1
    torch.cuda.synchronize()
    for t in (lp, state, gsum, cosv, dlat):
        assert torch.isnan(t).all()
    assert not ws.any().item()
