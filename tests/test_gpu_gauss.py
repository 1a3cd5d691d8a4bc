"""GPU: the Gaussian likelihood and LayerNorm kernels of csrc/latent_kernels.hip
(gauss_stats_kernel, gauss_loglik_kernel, gauss_backward_kernel,
ln_backward_kernel) against float64 references, at bars built from each
case's own terms (tests/gauss_cases.py states them; tests/test_gauss_cases.py
pins on the CPU what they rest on, and that they have teeth).

  A  one key through losses.get_normal_log_prob: widths on both sides of the
     block's 256 threads, T = 1357, the eight unit / non-unit shapes of the
     reference's .squeeze(), no / 0-1 / fractional / broadcast masks, negative
     sigma, and the two empty calls B = 0 and T = 0
  B  features 30 to 1000 spreads from zero, where q = M2 - 2 mu M1 + mu^2 M0
     cancels: only float64 frame sums and a float64 q pass
  C  key sets through latent.gauss_log_prob (key_feature's modality walk at
     kMaxKeys = 8 keys, idx with repeats and B > N, unused modalities without
     stats, the generator's strided layout, gradients for some inputs only)
     and through mmb_gauss_*_strided with padded rows
  D  mmb_gauss_stats alone, past one trip of its grid-stride loop
  E  mmb_layer_norm_backward from given f32 row statistics, with both, one
     and neither of dgamma / dbeta (the cb = 0 launch of a frozen generator)
  F  losses.get_log_prob_matrix end to end against the float64 oracle on a
     .double() copy of the generator, at the bars tests/test_gpu_latent.py
     states (torch's f32 GEMMs are in this path: the derived bars do not apply)

Also: lp is the same bits with and without gradients requested, from a second
launch, and from the strided layout and contiguous copies.

Two findings of these tests, fixed with them: a negative sigma gave NaN
(-log(s) where the reference has log(1 / sqrt(2 pi s^2))), and B = 0 / T = 0
raised MMBError (null data pointers of empty tensors failed the entry points'
pointer checks before their empty-call returns).

Measured on MI355X (the module prints these at its end), comparisons and the
largest fraction of the bar (77 tests, 5 s):
  A  lp / dmu / dsigma            24 each   0.484 / 0.496 / 0.496
  B  lp / dmu / dsigma             4 each   0.459 / 0.491 / 0.479
  C  lp / dmu / dsigma         74 / 55 / 50  0.471 / 0.497 / 0.499
  D  stats                         6        0.149
  E  dx / dgamma / dbeta       28 / 14 / 14  0.035 / 0.155 / 0.124
  F  total / dlat / parameters   2 / 2 / 36  0.009 / 0.007 / 0.010
The Gaussian figures are the one f32 rounding of the result (half of the
doubled 2^-23 |ref|): the float64 route itself adds nothing visible.  With the
library of the commit before these tests the three negative-sigma cases and the
two empty calls fail (NaN; MMBError) and the other 72 pass; with M2 alone
accumulated in float in gauss_stats_kernel 42 of the 77 fail, every case of
family B among them.
"""
import ctypes

import numpy as np
import pytest
import torch

import gauss_cases as G
import latent as LT
import losses
import gauss_gpu
import mmb_lib as L
from common_gpu import Ledger
from common_gpu import _dev32 as _dev  # float32 unless told otherwise

pytestmark = pytest.mark.gpu

_WORST = Ledger()
_note = _WORST.note  # (what, ratio)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for what, (n, r) in sorted(_WORST.items()):
        print(f"\ngauss {what}: {n} comparisons, largest {r:.3f} of its bar", end="")
    print()


def within(what, got, ref, bar):
    """gauss_gpu.within, noted in this module's report."""
    gauss_gpu.within(_note, what, got, ref, bar)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


# ---------------------------------------------------------------- A and B
AB = G.FAMILY_A + G.FAMILY_B


@pytest.mark.parametrize("c", AB, ids=[G.gauss_id(c) for c in AB])
def test_normal_log_prob_vs_float64(gpu, c):
    z, ref, bar = G.gauss_reference(c)
    fam = "B" if c in G.FAMILY_B else "A"
    x, mask, up = _dev(z["x"], gpu), _dev(z["mask"], gpu), _dev(z["up"], gpu)
    mu0, sg0 = _dev(z["mu"], gpu), _dev(z["sigma"], gpu)
    with torch.no_grad():
        lp0 = losses.get_normal_log_prob(mu0[:, None], sg0[:, None], x, mask)
    assert not lp0.requires_grad
    mu, sg = mu0.clone().requires_grad_(True), sg0.clone().requires_grad_(True)
    lp = losses.get_normal_log_prob(mu[:, None], sg[:, None], x, mask)
    assert tuple(lp.shape) == ref["lp"].shape  # [B], or 0-d where the reference's squeeze drops the batch
    (lp * (up[0] if lp.dim() == 0 else up)).sum().backward()
    within(f"{fam} lp", lp, ref["lp"], bar["lp"])
    assert torch.equal(_bits(lp), _bits(lp0))  # with and without gradients requested
    again = losses.get_normal_log_prob(mu[:, None], sg[:, None], x, mask)
    assert torch.equal(_bits(again), _bits(lp))  # fixed reduction order
    within(f"{fam} dmu", mu.grad, ref["dmu"], bar["dmu"])
    within(f"{fam} dsigma", sg.grad, ref["dsigma"], bar["dsigma"])


@pytest.mark.parametrize("shape", G.EMPTY_SHAPES, ids=str)
def test_empty_calls_return_zeros(gpu, shape):
    """B = 0 and T = 0: the oracle's shape ([B]) and value (zeros), gradients
    of the inputs' shapes, zero."""
    B, T, F = shape
    mu = torch.zeros(B, 1, F, device=gpu, requires_grad=True)
    sg = torch.full((B, 1, F), 1.5, device=gpu, requires_grad=True)
    x, mask = torch.ones(B, T, F, device=gpu), torch.ones(B, T, F, device=gpu)
    lp = losses.get_normal_log_prob(mu, sg, x, mask)
    assert tuple(lp.shape) == (B,) and not lp.detach().cpu().numpy().any()
    lp.sum().backward()
    for t in (mu, sg):
        assert t.grad.shape == t.shape and not t.grad.cpu().numpy().any()
    st = LT.gauss_stats(x, None)
    assert tuple(st.shape) == (B, 3, F) and not st.cpu().numpy().any()


# ---------------------------------------------------------------- C
def _key_stats(c, z, gpu):
    st = {m: None if z["x"][m] is None else LT.gauss_stats(_dev(z["x"][m], gpu), _dev(z["mask"][m], gpu))
          for m in G.MODS}
    idx = None if z["idx"] is None else torch.as_tensor(z["idx"]).to(gpu)
    return LT.GaussStats(**st), idx


def _key_operands(c, z, gpu, layout):
    """mu / sigma per key as contiguous [B, F_k] tensors, or as the column
    blocks of one [B, 2 F] (mu) and one [B, F] (sigma) buffer."""
    mus, sgs = [_dev(m, gpu) for m in z["mu"]], [_dev(s, gpu) for s in z["sigma"]]
    if layout == "gen":
        widths = [m.shape[1] for m in mus]
        f = sum(widths)
        y = torch.zeros(c.B, 2 * f, device=gpu)
        y[:, :f] = torch.cat(mus, 1)
        mus, sgs = y[:, :f].split(widths, 1), torch.cat(sgs, 1).split(widths, 1)
        assert mus[-1].stride(0) == 2 * f and sgs[-1].stride(0) == f and len(c.keys) > 1
    flags = [G.wants_grad(c, k) for k in range(len(c.keys))]
    return ([m.detach().requires_grad_(w[0]) for m, w in zip(mus, flags)],
            [s.detach().requires_grad_(w[1]) for s, w in zip(sgs, flags)])


def _key_run(c, z, gpu, stats, idx, layout):
    mus, sgs = _key_operands(c, z, gpu, layout)
    lp = LT.gauss_log_prob(stats, list(c.keys), mus, sgs, idx=idx)
    (lp * _dev(z["up"], gpu)).sum().backward()
    return lp.detach(), [t.grad for t in mus], [t.grad for t in sgs], (mus, sgs)


@pytest.mark.parametrize("c", G.FAMILY_C, ids=[G.key_id(c) for c in G.FAMILY_C])
def test_key_sets_vs_float64(gpu, c):
    z, refs, bars = G.key_reference(c)
    stats, idx = _key_stats(c, z, gpu)
    assert [s is None for s in stats.stats] == [z["x"][m] is None for m in G.MODS]
    lp, dmu, dsg, (mus, sgs) = _key_run(c, z, gpu, stats, idx, c.layout)
    assert tuple(lp.shape) == (len(c.keys), c.B)
    for k in range(len(c.keys)):
        within("C lp", lp[k], refs[k][0], bars[k][0])
        for name, g, j in (("C dmu", dmu[k], 0), ("C dsigma", dsg[k], 1)):
            if G.wants_grad(c, k)[j]:
                within(name, g, refs[k][j + 1], bars[k][j + 1])
            else:
                assert g is None  # the kernel's null dmu[k] / dsigma[k]
    with torch.no_grad():
        lp0 = LT.gauss_log_prob(stats, list(c.keys), mus, sgs, idx=idx)
    assert torch.equal(_bits(lp0), _bits(lp))
    if c.layout == "gen":  # the strided kernels and the same kernels on contiguous copies
        lp_c, dmu_c, dsg_c, _ = _key_run(c, z, gpu, stats, idx, "rows")
        assert torch.equal(_bits(lp_c), _bits(lp))
        for a, b in zip(dmu + dsg, dmu_c + dsg_c):
            assert (a is None) == (b is None) and (a is None or torch.equal(_bits(a), _bits(b)))


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[0 if t is None else t.data_ptr() for t in ts])


@pytest.mark.parametrize("c", G.FAMILY_C_PADDED, ids=[G.key_id(c) for c in G.FAMILY_C_PADDED])
def test_strided_entry_points_leave_the_pad_alone(gpu, c):
    """mmb_gauss_loglik_strided / mmb_gauss_backward_strided with rows F_k + 3
    apart: the three pad columns of mu / sigma hold NaN (nothing may read
    them), those of dmu / dsigma a poison word that must come back as it was."""
    z, refs, bars = G.key_reference(c)
    stats, idx = _key_stats(c, z, gpu)
    K, B = len(c.keys), c.B
    widths = [G.key_width(c, k) for k in c.keys]

    def padded(a):
        t = torch.full((B, a.shape[1] + G.PAD), float("nan"), device=gpu)
        t[:, :a.shape[1]] = _dev(a, gpu)
        return t

    def poison(w):
        return torch.full((B, w + G.PAD), G.POISON_BITS, dtype=torch.int32, device=gpu).view(torch.float32)

    mus, sgs = [padded(m) for m in z["mu"]], [padded(s) for s in z["sigma"]]
    flags = [G.wants_grad(c, k) for k in range(K)]
    dmu = [poison(w) if f[0] else None for w, f in zip(widths, flags)]
    dsg = [poison(w) if f[1] else None for w, f in zip(widths, flags)]
    lp = torch.full((K, B), float("nan"), device=gpu)
    head = [_ptrs(stats.stats), (ctypes.c_int * 3)(*stats.fm), L.ptr(idx), B, K,
            (ctypes.c_int * K)(*[LT.key_mods(k) for k in c.keys]), _ptrs(mus),
            (ctypes.c_int64 * K)(*[w + G.PAD for w in widths]), _ptrs(sgs),
            (ctypes.c_int64 * K)(*[w + G.PAD for w in widths])]
    L.call("mmb_gauss_loglik_strided", *head, L.ptr(lp), L.stream_ptr())
    L.call("mmb_gauss_backward_strided", *head, L.ptr(_dev(z["up"], gpu)), _ptrs(dmu), _ptrs(dsg),
           L.stream_ptr())
    torch.cuda.synchronize()
    for k, w in enumerate(widths):
        within("C lp", lp[k], refs[k][0], bars[k][0])
        for name, g, j in (("C dmu", dmu[k], 1), ("C dsigma", dsg[k], 2)):
            if g is not None:
                assert (_bits(g)[:, w:] == G.POISON_BITS).all().item(), (name, k)
                within(name, g[:, :w], refs[k][j], bars[k][j])


# ---------------------------------------------------------------- D
@pytest.mark.parametrize("c", G.FAMILY_D, ids=[G.stats_id(c) for c in G.FAMILY_D])
def test_gauss_stats_vs_float64(gpu, c):
    x, mask, st, bar = G.stats_case(c)
    xd, md = _dev(x, gpu), _dev(mask, gpu)
    got = LT.gauss_stats(xd, md)
    assert got.dtype == torch.float64 and tuple(got.shape) == (c.N, 3, c.F)
    within("D stats", got, st, bar)
    assert torch.equal(LT.gauss_stats(xd, md).view(torch.int64), got.view(torch.int64))
    if c.mask != "frac":
        assert np.array_equal(got[:, 0].cpu().numpy(), st[:, 0])  # counts are exact


# ---------------------------------------------------------------- E
@pytest.mark.parametrize("outs", G.LN_OUTS)
@pytest.mark.parametrize("c", G.FAMILY_E, ids=[G.ln_id(c) for c in G.FAMILY_E])
def test_layer_norm_backward_vs_float64(gpu, c, outs):
    z, ref, bars = G.ln_case(c)
    t = {k: _dev(v, gpu) for k, v in z.items()}

    def run():
        out = [torch.full((w + 1,), G.POISON_BITS, dtype=torch.int32, device=gpu).view(torch.float32)
               if on else None for w, on in ((c.n * c.d, True), (c.d, outs in ("both", "dgamma")),
                                             (c.d, outs in ("both", "dbeta")))]
        L.call("mmb_layer_norm_backward", L.ptr(t["dy"]), L.ptr(t["x"]), L.ptr(t["mean"]), L.ptr(t["rstd"]),
               L.ptr(t["gamma"]), c.n, c.d, L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]), L.stream_ptr())
        torch.cuda.synchronize()
        return out

    first, second = run(), run()
    for name, a, b, r, bar in zip(("E dx", "E dgamma", "E dbeta"), first, second, ref, bars):
        if a is None:
            continue
        assert _bits(a)[-1].item() == G.POISON_BITS, name  # the word after the output
        within(name, a[:-1].view(r.shape), r, bar)
        assert torch.equal(_bits(a), _bits(b)), name


# ---------------------------------------------------------------- F
@pytest.mark.parametrize("c", G.FAMILY_F, ids=[G.matrix_id(c) for c in G.FAMILY_F])
def test_log_prob_matrix_vs_float64(gpu, c):
    z, total_r, dlat_r, grads_r = G.matrix_reference(c)
    gen = G.make_generator(c).to(gpu)
    t, data, masks = G.matrix_data(z, list(gen.embed2out), lambda a: _dev(a, gpu))

    def wfn(latents, word_weights, sent, mask):
        return losses.get_word_log_prob_angular2(latents, t["table"], word_weights, sent, mask, G.WORD_A)

    x = t["lat"].clone().requires_grad_(True)
    total = losses.get_log_prob_matrix(G.ARGS, x, gen(x), data, masks, wfn)
    (-total).mean().backward()
    within("F total", total, total_r, G.LP_RTOL * np.abs(total_r) + G.LP_ATOL)
    within("F dlat", x.grad, dlat_r, np.broadcast_to(G.GRAD_TOL * np.abs(dlat_r).max(1, keepdims=True), dlat_r.shape))
    assert set(grads_r) == {n for n, _ in gen.named_parameters()}
    for n, p in gen.named_parameters():
        within("F parameters", p.grad, grads_r[n], np.full(grads_r[n].shape, G.GRAD_TOL * np.abs(grads_r[n]).max()))
