"""CPU: what the bars of tests/test_gpu_gauss.py rest on (tests/gauss_cases.py).

  * the float64 references agree with oracle.latent_oracle.normal_log_prob run
    in float64 (values, gradients, the squeeze shapes) and, on the zero-offset
    family, with it run in float32 within the bar the suite already holds the
    Gaussian kernels to (2e-5 |y| + 1e-4);
  * every derived lp bar is below that bar and every gradient bar below 1e-5
    of its row's largest entry, so nothing is compared more loosely than in
    tests/test_gpu_latent.py;
  * the kernels' own route (frame sums, q = M2 - 2 mu M1 + mu^2 M0) restated
    in float64 numpy stays below 1e-3 of the lp bar: the rewrite is sound in
    float64 on every case;
  * teeth: the same route with the three frame sums kept in f32 misses the
    bar by more than 100x on every offset case, and with an f32 accumulator
    over the features it misses the bar somewhere in the table;
  * the C entry points' argument checks, which return before any launch.
"""
import ctypes

import numpy as np
import pytest
import torch

import gauss_cases as G
import mmb_lib
from oracle import latent_oracle as LO

AB = G.FAMILY_A + G.FAMILY_B
OFFSET_CASES = [c for c in G.FAMILY_B if c.offset > 0]


def _oracle(c, dtype):
    z, _, _ = G.gauss_reference(c)
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    mu, sg = t(z["mu"]).requires_grad_(True), t(z["sigma"]).requires_grad_(True)
    mask = torch.ones(c.B, c.T, c.F, dtype=dtype) if z["mask"] is None else t(z["mask"])
    lp = LO.normal_log_prob(mu[:, None], sg[:, None], t(z["x"]), mask)
    up = t(z["up"])
    (lp * (up[0] if lp.dim() == 0 else up)).sum().backward()
    return lp.detach().numpy(), mu.grad.numpy(), sg.grad.numpy()


@pytest.mark.parametrize("c", AB, ids=[G.gauss_id(c) for c in AB])
def test_reference_agrees_with_oracle_in_float64(c):
    _, ref, bar = G.gauss_reference(c)
    lp, dmu, dsigma = _oracle(c, torch.float64)
    assert lp.shape == ref["lp"].shape == (() if G.squeezed((c.B, c.T, c.F)) else (c.B,))
    # (two float64 evaluations: a dsigma entry whose two terms cancel keeps the
    # rounding of the terms, 1e-12 of the tensor's largest entry at the most)
    for got, name in ((lp, "lp"), (dmu, "dmu"), (dsigma, "dsigma")):
        slack = 1e-12 * np.abs(ref[name]).max() if ref[name].size else 0.0
        assert (np.abs(got - ref[name]) <= 1e-3 * bar[name] + slack).all(), name


@pytest.mark.parametrize("c", G.FAMILY_A, ids=[G.gauss_id(c) for c in G.FAMILY_A])
def test_reference_agrees_with_oracle_in_float32(c):
    _, ref, _ = G.gauss_reference(c)
    lp, _, _ = _oracle(c, torch.float32)
    assert (np.abs(lp - ref["lp"]) <= G.LP_RTOL * np.abs(ref["lp"]) + G.LP_ATOL).all()


@pytest.mark.parametrize("shape", G.SQUEEZE_SHAPES + G.EMPTY_SHAPES, ids=str)
def test_squeeze_table_is_the_oracles(shape):
    B, T, F = shape
    out = LO.normal_log_prob(torch.zeros(B, 1, F, dtype=torch.float64), torch.ones(B, 1, F, dtype=torch.float64),
                             torch.ones(B, T, F, dtype=torch.float64), torch.ones(B, T, F, dtype=torch.float64))
    assert tuple(out.shape) == (() if G.squeezed(shape) else (B,))
    if 0 in shape:
        assert not G.squeezed(shape) and not out.numpy().any()  # an empty call: zeros [B]


def _gauss_bars():
    for c in AB:
        _, ref, bar = G.gauss_reference(c)
        yield G.gauss_id(c), ref["lp"], bar["lp"], [(ref["dmu"], bar["dmu"]), (ref["dsigma"], bar["dsigma"])]
    for c in G.FAMILY_C + G.FAMILY_C_PADDED:
        _, refs, bars = G.key_reference(c)
        for k, (r, b) in enumerate(zip(refs, bars)):
            yield f"{G.key_id(c)}-key{k}", r[0], b[0], [(r[1], b[1]), (r[2], b[2])]


def test_bars_are_below_the_bars_already_held():
    worst_lp = worst_g = 0.0
    for name, lp, lp_bar, grads in _gauss_bars():
        held = G.LP_RTOL * np.abs(lp) + G.LP_ATOL
        assert (lp_bar <= held).all(), name
        worst_lp = max(worst_lp, float((lp_bar / held).max()))
        for g, g_bar in grads:
            row = np.abs(g).max(1, keepdims=True)
            assert (g_bar <= 1e-5 * row).all(), name
            worst_g = max(worst_g, float((g_bar / np.where(row > 0, row, 1.0)).max()))
    print(f"lp bar at most {worst_lp:.3f} of 2e-5 |y| + 1e-4; gradient bars at most {worst_g:.2e} of the row")


@pytest.mark.parametrize("c", AB, ids=[G.gauss_id(c) for c in AB])
def test_kernel_route_in_float64_is_far_inside_the_bar(c):
    z, ref, bar = G.gauss_reference(c)
    lp = G.kernel_route_lp(z["mu"], z["sigma"], z["x"], z["mask"])
    assert (np.abs(lp - ref["lp_rows"]) <= 1e-3 * bar["lp_rows"]).all()


@pytest.mark.parametrize("c", OFFSET_CASES, ids=[G.gauss_id(c) for c in OFFSET_CASES])
def test_f32_frame_sums_miss_the_bar(c):
    """M0, M1, M2 kept in f32: the cancellation of q at features tens to a
    thousand spreads from zero; more than 100 bars on every offset case."""
    z, ref, bar = G.gauss_reference(c)
    lp = G.kernel_route_lp(z["mu"], z["sigma"], z["x"], z["mask"], stat_dtype=np.float32)
    ok = bar["lp_rows"] > 0  # (a row without frames: lp = 0 exactly)
    r = np.abs(lp - ref["lp_rows"])[ok] / bar["lp_rows"][ok]
    print(f"{G.gauss_id(c)}: f32 frame sums at {r.max():.3g} of the lp bar")
    assert r.max() >= 100.0


def test_f32_feature_sum_misses_the_bar():
    """gauss_loglik_kernel's block sum with a float accumulator (the terms and
    frame sums still float64) is out of the lp bar somewhere in the table."""
    for how in (True, "loop"):  # the block's own order | a plain running sum
        worst = {}
        for c in AB:
            z, ref, bar = G.gauss_reference(c)
            lp = G.kernel_route_lp(z["mu"], z["sigma"], z["x"], z["mask"], feat_f32=how)
            ok = bar["lp_rows"] > 0
            worst[G.gauss_id(c)] = float((np.abs(lp - ref["lp_rows"])[ok] / bar["lp_rows"][ok]).max())
        print(how, {k: round(v, 2) for k, v in worst.items()})
        assert max(worst.values()) > 1.0


def test_stats_reference_accumulates_in_extended_precision():
    assert np.finfo(np.longdouble).nmant >= 63
    for c in G.FAMILY_D[:4]:
        x, mask, st, bar = G.stats_case(c)
        m = np.ones(x.shape) if mask is None else np.broadcast_to(mask, x.shape)
        plain = np.stack([m.sum(1), (m * x).sum(1), (m * x * x).sum(1)], 1)
        assert st.shape == (c.N, 3, c.F) and (np.abs(plain - st) <= bar).all()
        assert np.array_equal(st[:, 0], m.sum(1)) or c.mask == "frac"  # M0 is exact for 0/1 masks
    big = G.FAMILY_D[-1]
    assert G.STATS_THREADS < big.N * big.F < G.STATS_THREADS + 8192  # a second trip for a few elements


@pytest.mark.parametrize("c", G.FAMILY_E, ids=[G.ln_id(c) for c in G.FAMILY_E])
def test_layer_norm_reference_is_torchs_backward(c):
    """With the exact float64 row statistics the reference's formulas are
    torch's float64 layer_norm backward; with the f32 ones it stays within the
    statistics' own rounding of it."""
    z, _, _ = G.ln_case(c)
    x = torch.tensor(z["x"]).requires_grad_(True)
    w, b = torch.tensor(z["gamma"]).requires_grad_(True), torch.zeros(c.d, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.layer_norm(x, [c.d], w, b, G.LN_EPS).backward(torch.tensor(z["dy"]))
    mean, rstd = z["x"].mean(1), 1.0 / np.sqrt(z["x"].var(1) + G.LN_EPS)
    (dx, dg, db), _ = G.layer_norm_backward_reference(z["dy"], z["x"], mean, rstd, z["gamma"])
    for got, want in ((dx, x.grad), (dg, w.grad), (db, b.grad)):
        want = want.numpy()
        assert np.abs(got - want).max() <= 1e-9 * max(np.abs(want).max(), 1.0)
    assert np.abs(z["mean"] - mean).max() <= G.U32 * np.abs(mean).max()
    assert (np.abs(z["rstd"] - rstd) <= G.U32 * rstd).all()


def test_case_tables_reach_the_edges():
    assert len(G.ALL8) == 8 and len(set(G.ALL8)) == 7  # kMaxKeys; every combination; one repeat
    widths = {G.key_width(c, k) for c in G.FAMILY_C for k in c.keys}
    assert 424 in widths and 1 in widths and max(widths) > 256
    assert {c.idx for c in G.FAMILY_C} == {"none", "perm", "wrap"}
    assert any(c.B > c.N for c in G.FAMILY_C) and any(c.layout == "gen" for c in G.FAMILY_C)
    for c in G.FAMILY_C + G.FAMILY_C_PADDED:
        z = G.make_key_inputs(c)
        if z["idx"] is not None:  # in range, with a repeat: no test passes a row the stats do not have
            assert z["idx"].min() >= 0 and z["idx"].max() < c.N and len(set(z["idx"])) < c.B
    assert G.make_key_inputs(G.FAMILY_C[3])["x"]["text"] is None
    assert {c.F for c in G.FAMILY_A} >= {1, 37, 255, 256, 257, 421}
    assert {(c.B, c.T, c.F) for c in G.FAMILY_A} >= set(G.SQUEEZE_SHAPES)
    for c in G.FAMILY_A:
        if c.neg:
            s = G.make_gauss_inputs(c)["sigma"]
            assert 0.2 < (s < 0).mean() < 0.5


# ---------------------------------------------------------------- argument checks
# Stand-ins for device pointers, never dereferenced: every call below returns
# before a launch (tests/test_lib_abi.py does the same for the stream kernels).
P = 0x7F0000001000
FM = (300, 76, 48)
MODS3 = (2, 4, 6)  # audio, visual, audiovisual
W3 = (76, 48, 124)


def _arr(ctype, vals):
    return (ctype * max(len(vals), 1))(*vals)


def _gauss(entry, *, stats=(None, P, P), fm=FM, b=4, nkeys=None, mods=MODS3, mu=None, sigma=None, ld_mu=W3,
           ld_sigma=W3, out=P):
    n = len(mods)
    mu = [P] * n if mu is None else mu
    sigma = [P] * n if sigma is None else sigma
    head = [_arr(ctypes.c_void_p, stats), _arr(ctypes.c_int, fm), None, b, n if nkeys is None else nkeys,
            _arr(ctypes.c_int, mods), _arr(ctypes.c_void_p, mu),
            None if ld_mu is None else _arr(ctypes.c_int64, ld_mu), _arr(ctypes.c_void_p, sigma),
            None if ld_sigma is None else _arr(ctypes.c_int64, ld_sigma)]
    if entry == "mmb_gauss_loglik_strided":
        return mmb_lib.call(entry, *head, out, None)
    return mmb_lib.call(entry, *head, out, _arr(ctypes.c_void_p, [P] * n), _arr(ctypes.c_void_p, [None] * n), None)


GAUSS_REJECTED = {
    "nkeys 0": dict(nkeys=0),
    "nkeys 9": dict(nkeys=9, mods=(2,) * 9, ld_mu=(76,) * 9, ld_sigma=(76,) * 9),
    "mods 0": dict(mods=(2, 0, 6)),
    "mods 8": dict(mods=(2, 8, 6)),
    "used modality without stats": dict(stats=(None, P, None)),
    "used modality of width 0": dict(fm=(300, 0, 48)),
    "text key without text stats": dict(mods=(2, 4, 1), ld_mu=(76, 48, 300), ld_sigma=(76, 48, 300)),
    "ld_mu one short": dict(ld_mu=(76, 48, 123)),
    "ld_sigma one short": dict(ld_sigma=(75, 48, 124)),
    "null mu[k]": dict(mu=[P, None, P]),
    "null sigma[k]": dict(sigma=[P, P, None]),
}


@pytest.mark.parametrize("entry", ["mmb_gauss_loglik_strided", "mmb_gauss_backward_strided"])
@pytest.mark.parametrize("what", list(GAUSS_REJECTED), ids=[w.replace(" ", "_") for w in GAUSS_REJECTED])
def test_gauss_argument_checks(entry, what):
    with pytest.raises(mmb_lib.MMBError, match=r"code -1 \(invalid argument\)"):
        _gauss(entry, **GAUSS_REJECTED[what])


@pytest.mark.parametrize("entry", ["mmb_gauss_loglik_strided", "mmb_gauss_backward_strided"])
def test_gauss_empty_batch_returns_before_any_launch(entry):
    assert _gauss(entry, b=0) == 0
    assert _gauss(entry, b=0, ld_mu=None, ld_sigma=None) == 0
    # an empty batch's tensors have null data pointers (losses.get_normal_log_prob at B = 0)
    assert _gauss(entry, b=0, stats=(None, None, None), mu=[None] * 3, sigma=[None] * 3, out=None) == 0
    with pytest.raises(mmb_lib.MMBError, match=r"code -1 \(invalid argument\)"):
        _gauss(entry, b=0, ld_mu=(76, 48, 123))  # the shape checks hold at b = 0 too
    with pytest.raises(mmb_lib.MMBError, match=r"code -1 \(invalid argument\)"):
        _gauss(entry, b=-1)


def test_gauss_stats_and_layer_norm_argument_checks():
    bad = r"code -1 \(invalid argument\)"
    with pytest.raises(mmb_lib.MMBError, match=bad):
        mmb_lib.call("mmb_gauss_stats", P, None, 4, 3, 0, P, None)       # f = 0
    with pytest.raises(mmb_lib.MMBError, match=bad):
        mmb_lib.call("mmb_gauss_stats", P, None, 4, -1, 5, P, None)
    with pytest.raises(mmb_lib.MMBError, match=bad):
        mmb_lib.call("mmb_gauss_stats", None, None, 4, 3, 5, P, None)    # frames to read, no x
    with pytest.raises(mmb_lib.MMBError, match=bad):
        mmb_lib.call("mmb_gauss_stats", P, None, 4, 3, 5, None, None)
    assert mmb_lib.call("mmb_gauss_stats", P, None, 0, 3, 5, P, None) == 0
    assert mmb_lib.call("mmb_gauss_stats", None, None, 0, 3, 5, None, None) == 0  # [0, T, F]: null pointers
    with pytest.raises(mmb_lib.MMBError, match=bad):
        mmb_lib.call("mmb_layer_norm_backward", P, P, P, P, None, 4, 300, P, P, P, None)  # no gamma
    with pytest.raises(mmb_lib.MMBError, match=bad):
        mmb_lib.call("mmb_layer_norm_backward", P, P, P, P, P, 4, 0, P, P, P, None)       # d = 0
    with pytest.raises(mmb_lib.MMBError, match=bad):
        mmb_lib.call("mmb_layer_norm_backward", P, P, P, P, P, 4, 300, None, P, P, None)  # no dx
    assert mmb_lib.call("mmb_layer_norm_backward", None, None, None, None, P, 0, 300, None, None, None, None) == 0
