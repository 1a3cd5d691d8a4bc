"""GPU parity of the sentiment regressor's kernels at widths other than 300.

csrc/mlp_kernels.hip dispatches on the width: mlp_train_mc_kernel<NTD> per
32-feature tile count (NTD <= 8: only NTD waves hold a tile; above: two tiles
a wave), P = ceil(h / 32) workgroups, and mlp_fwd_rows_kernel<V4> staged /
scalar by d % 4, w1's alignment and whether W1 fits in LDS.  The tables of
tests/regressor_cases.py hold the smallest shapes at which each instantiation,
partial tile and threshold is reached; every comparison is against the plain
float64 reference of oracle/regressor_oracle.py.

  a stateless entry points   element by element, |err| <= 2 (terms + 1) 2^-24 sum |terms|
                             of the dot products involved (the first layer's bound pushed
                             through |W2|; dh's through the sums over it): derived, not tuned
  b mmb_mlp_train            step_loss, valid_loss and the four parameter tensors against the
                             float64 run, relative to each loss / each tensor's largest entry.
                             The bar per case is 4x what the SAME algorithm run in float32 on
                             the CPU deviates from the float64 run (the device sums in another
                             order -- MFMA K order, P shares in tile order -- over sums of the
                             same length), and not below 8 x 2^-24.  Flag 0, control words left
                             zero, a second launch on the same workspace bit-identical.
  c limits                   the next multiple of 4 past the largest width, d % 4 != 0, h = 513,
                             n_out = 17, batch = 33: MMB_EINVAL, parameters and step_loss untouched
  d the Python mirror        SentimentModel at d = 100 and 50 (bars of a) and
                             train_sentiment_for_latents for 3 epochs against
                             oracle.regressor_oracle.train_for_latents (bars of b)

tests/test_regressor_cases.py (CPU) pins that every training case keeps 2
float32 bounds clear of the ReLU's and the L1 sign's kinks at every step.

Measured on MI355X (the module prints these at its end), as the largest
fraction of its bar any comparison reached:
  a  forward: 208 arrays over 26 shapes, y 0.005 (all three entry points), hid 0.24,
     batch_loss 0.08; backward: 338 arrays, dh 0.31, dx 0.20, dw1 0.23, db1 0.12,
     dw2 0.22, db2 0.13
  b  31 cases.  The float32 CPU run's own deviation from the float64 run is
     6.6e-8 .. 5.1e-7 on parameters and 1.1e-8 .. 4.3e-7 on losses; the device's is
     6.6e-8 .. 4.4e-7 and 3.3e-8 .. 4.6e-7.  Parameters reach 0.31 of their bar.  The
     losses reach 0.97 at (28, 512, 1): its last batch is one row whose loss, 0.26, is
     what is left of a sum of |terms| 2.8, so 4.6e-7 of the loss is 0.7 x 2^-24 of that
     sum (the CPU run happens to land 1.3e-8 from it there; the bar is the 8 x 2^-24
     floor); every other case stays at or below 0.25.
  d  SentimentModel 0.07 (dw1); train_sentiment_for_latents 0.25 / 0.20
     (parameters / losses; device 1.8e-7 and 3.3e-7 beside the CPU run's 1.8e-7 and 3.3e-7)
This file and tests/test_gpu_word_widths.py take 7 s together.

Only the product library is loaded.
"""
import numpy as np
import pytest
import torch

import mmb_lib as L
import regressor_cases as C
import regressor_gpu as RG
import sentiment_model as SM
from common_gpu import Ledger
from oracle import regressor_oracle as R
from regressor_cases import FLOOR
from regressor_gpu import _dev, _host64, _launch_train, _workspace

pytestmark = pytest.mark.gpu

MMB_EINVAL = -1

_WORST = Ledger()  # (group, what) -> [comparisons, largest error / bar]


def _note(group, what, ratio):
    return _WORST.note((group, what), ratio)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for (group, what), (n, r) in sorted(_WORST.items()):
        print(f"\nregressor widths group {group} {what}: {n} comparisons, largest {r:.3f} of its bar", end="")
    print()


def _check(group, what, got, ref, bound):
    """regressor_gpu._check, noted in this module's report."""
    return RG._check(_note, group, what, got, ref, bound)


FWD_IDS = [C.fwd_id(c) for c in C.FWD_CASES]


# ------------------------------------------------------------------ a: stateless entry points
@pytest.mark.parametrize("c", C.FWD_CASES, ids=FWD_IDS)
def test_forward_entry_points(gpu, c):
    """mmb_mlp_forward (with and without idx), mmb_mlp_eval (with and without
    perm, ragged last batches; pred_out and batch_loss) and
    mmb_mlp_forward_train (y and hid), each against the float64 forward."""
    z = C.fwd_inputs(c)
    x, lab = _dev(z["x"], gpu), _dev(z["labels"], gpu)
    P = [_dev(p, gpu) for p in z["params"]]
    assert P[0].data_ptr() % 16 == 0
    pp = [L.ptr(p) for p in P]
    st = L.stream_ptr()
    y = torch.full((c.b, c.o), np.nan, device=gpu)
    L.call("mmb_mlp_forward", L.ptr(x), None, c.b, c.d, c.h, c.o, *pp, L.ptr(y), st)
    _check("a", "mmb_mlp_forward", _host64(y), z["y"], z["y_bound"])
    rng = np.random.default_rng(c.b)
    perm = rng.permutation(c.b)
    idx = _dev(perm, gpu, torch.int64)
    y = torch.full((c.b, c.o), np.nan, device=gpu)
    L.call("mmb_mlp_forward", L.ptr(x), L.ptr(idx), c.b, c.d, c.h, c.o, *pp, L.ptr(y), st)
    _check("a", "mmb_mlp_forward idx", _host64(y), z["y"][perm], z["y_bound"][perm])

    y = torch.full((c.b, c.o), np.nan, device=gpu)
    hid = torch.full((c.b, c.h), np.nan, device=gpu)
    L.call("mmb_mlp_forward_train", L.ptr(x), c.b, c.d, c.h, c.o, *pp, L.ptr(y), L.ptr(hid), st)
    _check("a", "mmb_mlp_forward_train y", _host64(y), z["y"], z["y_bound"])
    _check("a", "mmb_mlp_forward_train hid", _host64(hid), z["hid"], z["pre_bound"])

    for order, batch, p_dev in ((np.arange(c.b), 4, None), (perm, 3, idx)):
        nb = -(-c.b // batch)
        bl = torch.full((nb,), np.nan, device=gpu)
        pred = torch.full((c.b, c.o), np.nan, device=gpu)
        L.call("mmb_mlp_eval", L.ptr(x), L.ptr(lab), L.ptr(p_dev), c.b, batch, c.d, c.h, c.o, *pp,
               L.ptr(bl), L.ptr(pred), st)
        what = "mmb_mlp_eval" + (" perm" if p_dev is not None else "")
        _check("a", what + " pred", _host64(pred), z["y"][order], z["y_bound"][order])
        diff = np.abs(z["y"] - z["labels"])[order]
        ref = np.array([diff[s:s + batch].mean() for s in range(0, c.b, batch)])
        # each |y - label| carries y's bound and one rounding; the sum of m terms m more, the division one
        m = np.array([diff[s:s + batch].size for s in range(0, c.b, batch)])
        bound = np.array([z["y_bound"][order][s:s + batch].mean() for s in range(0, c.b, batch)]) \
            + (m + 2) * C.U32 * ref
        _check("a", what + " batch_loss", _host64(bl), ref, bound)


@pytest.mark.parametrize("want", ["all", "no_dx", "no_params"])
@pytest.mark.parametrize("c", C.FWD_CASES, ids=FWD_IDS)
def test_backward_entry_point(gpu, c, want):
    """mmb_mlp_backward against the float64 gradients for an upstream dy, given
    the float64 forward's activations rounded to f32: every output wanted, dx
    null, the parameter gradients null."""
    z = C.fwd_inputs(c)
    hid32 = C.f32(z["hid"])
    w1, _, w2, _ = z["params"]
    g, bounds = C.backward_bounds(z["x"], hid32, w1, w2, z["dy"])
    x, hid, dy = _dev(z["x"], gpu), _dev(hid32, gpu), _dev(z["dy"], gpu)
    out = {k: torch.full(g[k].shape, np.nan, device=gpu) for k in g}
    if want == "no_dx":
        out["dx"] = None
    if want == "no_params":
        for k in ("dw1", "db1", "dw2", "db2"):
            out[k] = None
    w1d, w2d = _dev(w1, gpu), _dev(w2, gpu)
    L.call("mmb_mlp_backward", L.ptr(x), L.ptr(hid), c.b, c.d, c.h, c.o, L.ptr(w1d), L.ptr(w2d),
           L.ptr(dy), *[L.ptr(out[k]) for k in ("dh", "dx", "dw1", "db1", "dw2", "db2")], L.stream_ptr())
    for k, t in out.items():
        if t is not None:
            _check("a", "mmb_mlp_backward " + k, _host64(t), g[k], bounds[k])


# ------------------------------------------------------------------ b: mmb_mlp_train
def _launch_train(gpu, c, z, ws):
    """One mmb_mlp_train launch of a case from its initial parameters; returns
    (rc, params, step_loss, valid_loss, flag) as device tensors."""
    d, h, o, batch = c.d, c.h, c.o, c.batch
    x, y = _dev(z["x"], gpu), _dev(z["y"], gpu)
    P = [_dev(p, gpu) for p in z["params"]]
    perm = _dev(z["perm"], gpu, torch.int64)
    spe = -(-c.n // batch)
    sl = torch.full((C.N_EPOCHS * spe,), np.nan, device=gpu)
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    vl, keep = None, []
    vargs = (None, None, None, 0, 1, c.epoch0, None)
    if z["valid"] is not None:
        xv, yv, vperm, every, epoch0 = z["valid"]
        keep = [_dev(xv, gpu), _dev(yv, gpu), _dev(vperm, gpu, torch.int64)]
        vl = torch.full((max(C.n_validations(c), 1) * -(-c.nv // batch),), np.nan, device=gpu)
        vargs = (*[L.ptr(t) for t in keep], c.nv, every, epoch0, L.ptr(vl))
    rc = L.query("mmb_mlp_train", L.ptr(x), L.ptr(y), L.ptr(perm), c.n, C.N_EPOCHS, batch, d, h, o,
                 C.LR, *[L.ptr(p) for p in P], L.ptr(sl), *vargs, L.ptr(ws), L.ptr(flag), L.stream_ptr())
    torch.cuda.synchronize()
    return rc, P, sl, vl, flag


def _workspace(gpu, d, h, slack=1):
    return torch.zeros(slack * (L.query("mmb_mlp_workspace_bytes", d, h) // 4 + 4), dtype=torch.int32,
                       device=gpu)


@pytest.mark.parametrize("c", C.TRAIN_CASES, ids=[C.train_id(c) for c in C.TRAIN_CASES])
def test_train_vs_float64_run(gpu, c):
    z = C.make_train_inputs(c)
    ref = C.train_reference(c)
    assert ref["margin"] >= C.MARGIN
    env_p, env_l = C.f32_envelope(c)
    ws = _workspace(gpu, c.d, c.h)
    runs = []
    for _ in range(2):  # the second launch: the same workspace, the same initial parameters
        rc, P, sl, vl, flag = _launch_train(gpu, c, z, ws)
        assert rc == 0
        assert int(flag.item()) == 0
        assert not ws[:4].any().item(), "control words left non-zero"
        runs.append(P + [sl] + ([vl] if vl is not None else []))
    for a, b in zip(*runs):
        assert torch.equal(a, b), "second launch on the same workspace differs"
    nvl = C.n_validations(c) * -(-c.nv // c.batch) if c.nv else 0
    got = {"params": [_host64(p) for p in P], "step_loss": _host64(sl),
           "valid_loss": _host64(vl)[:nvl] if nvl else np.zeros(0)}
    assert all(np.isfinite(a).all() for a in got["params"]) and np.isfinite(got["step_loss"]).all()
    dev_p, dev_l = C.rel_dev(got, ref)
    bar_p, bar_l = max(4 * env_p, FLOOR), max(4 * env_l, FLOOR)
    print(f"{C.train_id(c)}: parameters device {dev_p:.2e} (CPU f32 {env_p:.2e}, bar {bar_p:.2e}); "
          f"losses device {dev_l:.2e} (CPU f32 {env_l:.2e}, bar {bar_l:.2e})")
    _note("b", "parameters", RG._ratio(dev_p, bar_p))
    _note("b", "losses", RG._ratio(dev_l, bar_l))
    assert dev_p <= bar_p
    assert dev_l <= bar_l


# ------------------------------------------------------------------ c: limits
@pytest.mark.parametrize("what,d,h,o,batch", [
    ("next multiple of 4 past 448", 452, 33, 1, 32),
    ("next multiple of 4 past 448 at 13 outputs", 452, 33, 13, 32),
    ("next multiple of 4 past 416 at 14 outputs", 420, 33, 14, 32),
    ("next multiple of 4 past 416 at 16 outputs", 420, 33, 16, 32),
    ("the old documented limit", 512, 33, 1, 32),
    ("d % 4 != 0", 50, 33, 1, 32),
    ("d % 4 != 0", 301, 33, 2, 5),
    ("h = 513", 36, 513, 1, 32),
    ("n_out = 17", 36, 33, 17, 32),
    ("batch = 33", 36, 33, 1, 33),
])
def test_train_rejects_past_its_limits(gpu, what, d, h, o, batch):
    """MMB_EINVAL before any launch: parameters and step_loss untouched, bit
    for bit (every buffer has the full size of the requested shape)."""
    c = C.TrainCase(d, h, o, batch, 35, 9, 1, 0, 0)
    z = C.make_train_inputs(c)
    ws = _workspace(gpu, d, h, slack=2)
    rc, P, sl, vl, flag = _launch_train(gpu, c, z, ws)
    assert rc == MMB_EINVAL, what
    for p, p0 in zip(P, z["params"]):
        assert np.array_equal(p.cpu().numpy(), p0.astype(np.float32))
    assert torch.isnan(sl).all() and torch.isnan(vl).all()
    assert int(flag.item()) == 0 and not ws.any().item()


def test_largest_widths_are_accepted(gpu):
    """The limit is exactly mmb_mlp_train_max_d: the widths the rejection test
    steps past are the ones part b trains at."""
    assert L.query("mmb_mlp_train_max_d", 1) == L.query("mmb_mlp_train_max_d", 13) == 448
    assert L.query("mmb_mlp_train_max_d", 14) == L.query("mmb_mlp_train_max_d", 16) == 416
    assert any(c.d == 448 and c.o == 13 for c in C.TRAIN_CASES)
    assert any(c.d == 416 and c.o == 16 for c in C.TRAIN_CASES)


# ------------------------------------------------------------------ d: the Python mirror
MIRROR = [(100, 64, 3, 9), (50, 33, 1, 17)]


@pytest.mark.parametrize("d,h,o,b", MIRROR)
def test_sentiment_model_forward_and_autograd(gpu, d, h, o, b):
    """SentimentModel(d, h, o): the no-grad forward (mmb_mlp_forward) and the
    forward under autograd with backward() (mmb_mlp_forward_train /
    mmb_mlp_backward) against torch's own module in float64."""
    ref = torch.nn.Sequential(torch.nn.Linear(d, h), torch.nn.ReLU(), torch.nn.Linear(h, o)).double()
    torch.manual_seed(d + h)
    m = SM.SentimentModel(d, h, o)
    with torch.no_grad():
        for p, q in zip(ref.parameters(), m.parameters()):
            p.copy_(q.double())
    m = m.to(gpu)
    x = torch.randn(b, d)
    dy = torch.randn(b, o)
    params = [p.detach().numpy() for p in ref.parameters()]
    xr = x.double().requires_grad_(True)
    yr = ref(xr)
    yr.backward(dy.double())
    xn, dyn = x.double().numpy(), dy.double().numpy()
    y_bound, pre_b = R.out_bound(xn, *params), R.pre_bound(xn, *params[:2])
    pre = xn @ params[0].T + params[1]
    assert (np.abs(pre) >= 2 * pre_b).all(), "a hidden unit sits on the ReLU's kink: choose another seed"
    with torch.no_grad():
        y = m(x.to(gpu))
    assert not y.requires_grad and y.shape == yr.squeeze().shape
    _check("d", "SentimentModel no-grad", _host64(y).reshape(b, o), yr.detach().numpy(), y_bound)
    xg = x.to(gpu).requires_grad_(True)
    y = m(xg)
    assert y.requires_grad
    _check("d", "SentimentModel autograd y", _host64(y.detach()).reshape(b, o), yr.detach().numpy(), y_bound)
    y.reshape(b, o).backward(dy.to(gpu))
    hid = np.maximum(pre, 0)
    g, bounds = C.backward_bounds(xn, hid, params[0], params[2], dyn)
    bounds["dw2"] = bounds["dw2"] + np.abs(dyn).T @ pre_b   # the device's own hid carries pre's bound
    got = {"dx": xg.grad, "dw1": m.hidden1.weight.grad, "db1": m.hidden1.bias.grad,
           "dw2": m.out.weight.grad, "db2": m.out.bias.grad}
    want = {"dx": xr.grad, "dw1": ref[0].weight.grad, "db1": ref[0].bias.grad, "dw2": ref[2].weight.grad,
            "db2": ref[2].bias.grad}
    for k in got:
        np.testing.assert_allclose(g[k], want[k].numpy(), rtol=0, atol=1e-12)  # the oracle is torch's autograd
        _check("d", "SentimentModel autograd " + k, _host64(got[k]), want[k].numpy(), bounds[k])


def mirror_case(d, seed):
    """Latents / labels (train 70, valid 20, test 10) and the args of a 3-epoch run."""
    rng = np.random.default_rng([d, seed])
    lat = tuple(rng.standard_normal((n, d)).astype(np.float32) for n in (70, 20, 10))
    lab = tuple(rng.uniform(-3, 3, n).astype(np.float32) for n in (70, 20, 10))
    args = {"sentiment_hidden_size": 33, "n_sentiment_epochs": 3, "sentiment_lr": 0.05,
            "early_stopping": False, "dataset": "mosi", "lr_decay": 0.5}
    return args, lat, lab


def mirror_reference(d, seed, dtype):
    args, lat, lab = mirror_case(d, seed)
    torch.manual_seed(seed)
    return R.train_for_latents(args, lat, lab, dtype=dtype)


def mirror_margin(d, seed):
    """The margin (regressor_cases.MARGIN) of the float64 train_for_latents run:
    its own initial weights and sample orders replayed by sgd_run."""
    args, lat, lab = mirror_case(d, seed)
    r = mirror_reference(d, seed, torch.float64)
    init = [r["init"][k].numpy() for k in ("hidden1.weight", "hidden1.bias", "out.weight", "out.bias")]
    run = R.sgd_run(lat[0], lab[0][:, None], torch.cat(r["order"]).numpy(), 3, 32, args["sentiment_lr"],
                    init, margins=True)
    np.testing.assert_allclose(run["params"][0], r["state"]["hidden1.weight"].numpy(), rtol=0, atol=1e-13)
    return run["margin"]


MIRROR_SEEDS = {100: 0, 50: 0}  # torch seeds whose float64 run keeps the margin (searched once)


@pytest.mark.parametrize("d", [100, 50])
def test_train_sentiment_for_latents_vs_oracle(gpu, d):
    """train_sentiment_for_latents for 3 epochs (d = 50: no multiple of 4, the
    mirror pads) against oracle.regressor_oracle.train_for_latents from the
    same torch seed, computed in float64; bar: 4x the float32 oracle run's own
    deviation from it, not below 8 x 2^-24."""
    seed = MIRROR_SEEDS[d]
    assert mirror_margin(d, seed) >= C.MARGIN
    r64, r32 = mirror_reference(d, seed, torch.float64), mirror_reference(d, seed, torch.float32)
    args, lat, lab = mirror_case(d, seed)
    captured = {}
    orig = SM.train_sentiment

    def spy(*a, **k):
        tl, vl = orig(*a, **k)
        captured["train"], captured["valid"] = tl, vl
        captured["state"] = {kk: v.detach().cpu().numpy() for kk, v in a[1].state_dict().items()}
        return tl, vl

    SM.train_sentiment = spy
    try:
        torch.manual_seed(seed)
        SM.train_sentiment_for_latents(args, tuple(torch.tensor(l) for l in lat), lab, gpu)
    finally:
        SM.train_sentiment = orig

    def as_run(state, tl, vl):
        return {"params": [np.asarray(state[k], np.float64) for k in
                           ("hidden1.weight", "hidden1.bias", "out.weight", "out.bias")],
                "step_loss": np.asarray(tl, np.float64), "valid_loss": np.asarray(vl, np.float64)}

    ref = as_run({k: v.numpy() for k, v in r64["state"].items()}, r64["train_losses"], r64["valid_losses"])
    cpu = as_run({k: v.numpy() for k, v in r32["state"].items()}, r32["train_losses"], r32["valid_losses"])
    got = as_run(captured["state"], captured["train"], captured["valid"])
    assert len(got["step_loss"]) == 3 and len(got["valid_loss"]) == 1
    (env_p, env_l), (dev_p, dev_l) = C.rel_dev(cpu, ref), C.rel_dev(got, ref)
    bar_p, bar_l = max(4 * env_p, FLOOR), max(4 * env_l, FLOOR)
    print(f"d {d}: parameters device {dev_p:.2e} (CPU f32 {env_p:.2e}, bar {bar_p:.2e}); "
          f"losses device {dev_l:.2e} (CPU f32 {env_l:.2e}, bar {bar_l:.2e})")
    _note("d", "train_sentiment_for_latents parameters", RG._ratio(dev_p, bar_p))
    _note("d", "train_sentiment_for_latents losses", RG._ratio(dev_l, bar_l))
    assert dev_p <= bar_p
    assert dev_l <= bar_l
