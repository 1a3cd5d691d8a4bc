"""GPU parity: the sentiment regressor (a10-a12) vs the reference's recorded runs.

* one SGD step (forward, L1 backward, update) vs torch autograd + optim.SGD;
* a 20-epoch train_sentiment_for_latents run from the same torch seed: the
  same mini-batch order (global RNG consumed identically), so loss curves and
  final weights track the reference's to fp32 rounding.
"""
import json
import os

import numpy as np
import pytest
import torch

import mmb_lib as L
import sentiment_model as SM

pytestmark = pytest.mark.gpu


def _train_steps(gpu, x, y, w1, b1, w2, b2, lr, perm=None, epochs=1, batch=32):
    n = x.shape[0]
    lat = torch.tensor(x, device=gpu)
    lab = torch.tensor(y, device=gpu).reshape(n, -1).contiguous()
    o = lab.shape[1]
    h, d = w1.shape
    P = [torch.tensor(a, device=gpu).contiguous() for a in (w1, b1, w2, b2)]
    if perm is None:
        perm = np.tile(np.arange(n), epochs)
    perm = torch.as_tensor(perm, dtype=torch.int64, device=gpu)
    spe = (n + batch - 1) // batch
    sl = torch.empty(spe * epochs, dtype=torch.float32, device=gpu)
    ws = torch.zeros(L.query("mmb_mlp_workspace_bytes", d, h) // 4 + 4, device=gpu)
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    L.call("mmb_mlp_train", L.ptr(lat), L.ptr(lab), L.ptr(perm), n, epochs, batch, d, h, o,
           float(lr), *[L.ptr(p) for p in P], L.ptr(sl), None, None, None, 0, 1, 0, None,
           L.ptr(ws), L.ptr(flag), L.stream_ptr())
    assert int(flag.item()) == 0
    return [p.cpu().numpy() for p in P], sl.cpu().numpy()


@pytest.mark.parametrize("h,o,every", [(100, 1, 2), (150, 3, 1)])
def test_in_launch_validation_equals_eval_kernel(gpu, h, o, every):
    """mmb_mlp_train's validation passes (the weights of that moment, its own
    sample order per validation) equal mmb_mlp_eval run between separate
    training launches; the parameters after the one launch equal the
    chained launches' bit for bit."""
    rng = np.random.default_rng(h + o)
    n, nv, d, B, epochs, lr = 130, 71, 300, 32, 4, 0.05
    x = torch.tensor(rng.standard_normal((n, d)).astype(np.float32), device=gpu)
    y = torch.tensor(rng.uniform(-3, 3, (n, o)).astype(np.float32), device=gpu)
    xv = torch.tensor(rng.standard_normal((nv, d)).astype(np.float32), device=gpu)
    yv = torch.tensor(rng.uniform(-3, 3, (nv, o)).astype(np.float32), device=gpu)
    torch.manual_seed(h)
    init = [p.detach() for p in SM.SentimentModel(d, h, o).parameters()]
    perm = torch.cat([torch.randperm(n) for _ in range(epochs)]).to(gpu)
    nval = len([e for e in range(epochs) if e % every == 0])
    vperm = torch.cat([torch.randperm(nv) for _ in range(nval)]).to(gpu)
    spe, nbv = -(-n // B), -(-nv // B)
    ws = torch.zeros(L.query("mmb_mlp_workspace_bytes", d, h) // 4 + 4, device=gpu)
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    P1 = [p.clone().to(gpu).contiguous() for p in init]
    sl1 = torch.empty(spe * epochs, device=gpu)
    vl1 = torch.empty(nval * nbv, device=gpu)
    L.call("mmb_mlp_train", L.ptr(x), L.ptr(y), L.ptr(perm), n, epochs, B, d, h, o, float(lr),
           *[L.ptr(p) for p in P1], L.ptr(sl1), L.ptr(xv), L.ptr(yv), L.ptr(vperm), nv, every, 0,
           L.ptr(vl1), L.ptr(ws), L.ptr(flag), L.stream_ptr())
    P2 = [p.clone().to(gpu).contiguous() for p in init]
    sl2, vl2 = [], []
    k = 0
    for e in range(epochs):
        s = torch.empty(spe, device=gpu)
        L.call("mmb_mlp_train", L.ptr(x), L.ptr(y), L.ptr(perm[e * n:(e + 1) * n].contiguous()), n,
               1, B, d, h, o, float(lr), *[L.ptr(p) for p in P2], L.ptr(s), None, None, None, 0, 1,
               0, None, L.ptr(ws), L.ptr(flag), L.stream_ptr())
        sl2.append(s)
        if e % every == 0:
            bl = torch.empty(nbv, device=gpu)
            L.call("mmb_mlp_eval", L.ptr(xv), L.ptr(yv), L.ptr(vperm[k * nv:(k + 1) * nv].contiguous()),
                   nv, B, d, h, o, *[L.ptr(p) for p in P2], L.ptr(bl), None, L.stream_ptr())
            vl2.append(bl)
            k += 1
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    for a, b in zip(P1, P2):
        assert torch.equal(a, b)
    assert torch.equal(sl1, torch.cat(sl2))
    np.testing.assert_allclose(vl1.cpu().numpy(), torch.cat(vl2).cpu().numpy(), rtol=2e-6, atol=1e-7)


def test_one_sgd_step(gpu, golden):
    z = golden("g5_senti_step")
    (w1, b1, w2, b2), sl = _train_steps(gpu, z["x"], z["y"], z["w1"], z["b1"], z["w2"], z["b2"], 0.1)
    assert abs(sl[0] - float(z["loss"])) < 1e-6 * max(1.0, abs(float(z["loss"])))
    np.testing.assert_allclose(w1, z["nw1"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(b1, z["nb1"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(w2, z["nw2"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(b2, z["nb2"], rtol=1e-5, atol=1e-6)


def test_forward(gpu, golden):
    z = golden("g5_senti_step")
    m = SM.SentimentModel(300, 100, 1).to(gpu)
    with torch.no_grad():
        m.hidden1.weight.copy_(torch.tensor(z["w1"]))
        m.hidden1.bias.copy_(torch.tensor(z["b1"]))
        m.out.weight.copy_(torch.tensor(z["w2"]))
        m.out.bias.copy_(torch.tensor(z["b2"]))
    x = torch.tensor(z["x"], device=gpu)
    with torch.no_grad():
        y = m(x)  # mmb_mlp_forward
    assert y.shape == (32,) and not y.requires_grad
    np.testing.assert_allclose(y.cpu().numpy(), z["pred"], rtol=1e-5, atol=1e-6)
    y = m(x)  # autograd recording (the e2e objective): differentiable device path
    assert y.shape == (32,) and y.requires_grad
    np.testing.assert_allclose(y.detach().cpu().numpy(), z["pred"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("h,o,n", [(150, 1, 77), (100, 7, 64), (60, 3, 33)])
def test_multi_step_vs_torch(gpu, h, o, n):
    """Several epochs incl. a ragged last batch, other widths, multi-output heads."""
    rng = np.random.default_rng(h + o)
    x = rng.standard_normal((n, 300)).astype(np.float32)
    y = rng.uniform(-3, 3, (n, o)).astype(np.float32)
    torch.manual_seed(h)
    ref = torch.nn.Sequential(torch.nn.Linear(300, h), torch.nn.ReLU(), torch.nn.Linear(h, o))
    init = [p.detach().numpy().copy() for p in ref.parameters()]
    perm = np.concatenate([rng.permutation(n) for _ in range(3)])
    opt = torch.optim.SGD(ref.parameters(), lr=0.05)
    losses = []
    for e in range(3):
        order = perm[e * n:(e + 1) * n]
        for s in range(0, n, 32):
            idx = order[s:s + 32]
            opt.zero_grad()
            out = ref(torch.tensor(x[idx]))
            loss = torch.nn.L1Loss(reduction="none")(out, torch.tensor(y[idx])).mean()
            loss.backward()
            opt.step()
            losses.append(loss.item())
    (w1, b1, w2, b2), sl = _train_steps(gpu, x, y if o > 1 else y[:, 0], *init, 0.05, perm=perm,
                                        epochs=3)
    np.testing.assert_allclose(sl, losses, rtol=1e-4, atol=1e-5)
    got = [w1, b1, w2, b2]
    for g, r in zip(got, ref.parameters()):
        np.testing.assert_allclose(g, r.detach().numpy(), rtol=1e-4, atol=1e-5)


def test_train_for_latents_matches_reference_run(gpu, golden):
    z = golden("g5_senti_train")
    with open(os.path.join(os.path.dirname(__file__), "golden", "g5_senti_train_metrics.json")) as f:
        ref_metrics = json.load(f)
    args = {"sentiment_hidden_size": 100, "n_sentiment_epochs": 20, "sentiment_lr": 0.1,
            "early_stopping": False, "dataset": "mosi", "lr_decay": 0.5}
    lat = tuple(torch.tensor(z[k]) for k in ("lat_train", "lat_valid", "lat_test"))
    labels = (z["y_train"], z["y_valid"], z["y_test"])
    captured = {}
    orig = SM.train_sentiment

    def spy(*a, **k):
        tl, vl = orig(*a, **k)
        captured["train"], captured["valid"] = tl, vl
        captured["model"] = {kk: v.detach().cpu().numpy() for kk, v in a[1].state_dict().items()}
        return tl, vl

    SM.train_sentiment = spy
    try:
        torch.manual_seed(int(z["seed"]))
        results = SM.train_sentiment_for_latents(args, lat, labels, gpu)
    finally:
        SM.train_sentiment = orig
    np.testing.assert_allclose(captured["train"], z["train_losses"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(captured["valid"], z["valid_losses"], rtol=1e-4, atol=1e-6)
    for k, v in captured["model"].items():
        np.testing.assert_allclose(v, z["final_" + k.replace(".", "_")], rtol=1e-3, atol=1e-5)
    after = ref_metrics["after"]
    assert abs(results["mae"] - after["mae"]) < 1e-4
    assert abs(results["corr"] - after["corr"]) < 1e-4
    assert results["accuracy"] == after["accuracy"]


def _rel_dev(a, ref):
    n = min(len(a), len(ref))
    a, ref = np.asarray(a[:n], np.float64), np.asarray(ref[:n], np.float64)
    return float(np.max(np.abs(a - ref) / np.abs(ref)))


@pytest.mark.parametrize("case", ["g5_full", "g5_full_es"])
def test_full_size_run_matches_reference(gpu, tmp_path, case, capsys):
    """BASELINE configs[4]: MOSI-sized splits (1284 / 229 / 686), H = 100, 400
    epochs against the reference's own recorded runs
    (tests/golden/make_goldens_regressor.py).  g5_full_es takes the
    early-stopping branch end to end: reloads of the best checkpoint with lr
    decay at epochs 100 and 200, the early stop at 300, and the reference's
    quirk of evaluating the un-reloaded model afterwards
    (sentiment_model.py:132-160, 243-250).

    Bars.  16,400 fp32 SGD steps on an L1 loss amplify rounding: the
    REFERENCE ITSELF, run in float64 or on latents nudged by one ulp, leaves
    its recorded loss curve by up to ~20 % after epoch ~30 (the fixture's
    `envelope`).  So: the first 20 epochs within 1e-4; the early-stopping
    events, epoch count and files exactly; the loss curves and final metrics
    within 1.5x the reference's own rounding envelope."""
    from regressor_cases import full_case

    args, lat, lab, z, meta = full_case(case)
    captured = {}
    orig = SM.train_sentiment

    def spy(*a, **k):
        tl, vl = orig(*a, **k)
        captured["train"], captured["valid"] = tl, vl
        captured["model"] = {kk: v.detach().cpu().numpy() for kk, v in a[1].state_dict().items()}
        return tl, vl

    SM.train_sentiment = spy
    try:
        torch.manual_seed(int(z["seed"]))
        results = SM.train_sentiment_for_latents(args, tuple(torch.tensor(l) for l in lat),
                                                 tuple(lab), gpu, model_save_path=str(tmp_path))
    finally:
        SM.train_sentiment = orig
    out = capsys.readouterr().out
    ev = meta["events"]
    assert out.count("reloading model and decaying") == ev["reloads"]
    assert ("early stopping..." in out) == ev["early_stop"]
    assert sorted(os.listdir(tmp_path)) == meta["files"]
    tl, vl = captured["train"], captured["valid"]
    assert len(tl) == len(z["train_losses"]) and len(vl) == len(z["valid_losses"])
    np.testing.assert_allclose(tl[:20], z["train_losses"][:20], rtol=1e-4)
    np.testing.assert_allclose(vl[:2], z["valid_losses"][:2], rtol=1e-4)
    env = meta["envelope"]
    for kind in env:  # the perturbed reference runs took the same branch decisions
        assert env[kind]["events"]["reloads"] == ev["reloads"]
    env_train = max(_rel_dev(e["train_losses"], z["train_losses"]) for e in env.values())
    env_valid = max(_rel_dev(e["valid_losses"], z["valid_losses"]) for e in env.values())
    assert _rel_dev(tl, z["train_losses"]) <= 1.5 * env_train + 1e-3
    assert _rel_dev(vl, z["valid_losses"]) <= 1.5 * env_valid + 1e-3
    after = meta["after"]
    for key in ("mae", "corr", "accuracy"):
        band = max(abs(e["after"][key] - after[key]) for e in env.values())
        assert abs(results[key] - after[key]) <= 1.5 * band + 0.01, (key, results[key], after[key], band)
    if ev["early_stop"]:
        # after each reload the epoch-0 checkpoint is back: the next validation
        # is again above the first one, like the reference's
        assert all(v > vl[0] for v in vl[1:])


@pytest.mark.parametrize("b,h,o", [(64, 100, 1), (4, 150, 1), (33, 100, 7)])
def test_differentiable_forward_backward_vs_torch(gpu, b, h, o):
    """The e2e objective's regressor term under autograd goes through
    mmb_mlp_forward_train / mmb_mlp_backward: outputs and the gradients to the
    inputs and every parameter equal torch autograd of the reference module
    (sentiment_model.py:36-41) on the same device, within fp32 sum order."""
    torch.manual_seed(b + h + o)
    m = SM.SentimentModel(300, h, o).to(gpu)
    ref = torch.nn.Sequential(torch.nn.Linear(300, h), torch.nn.ReLU(), torch.nn.Linear(h, o)).to(gpu)
    with torch.no_grad():
        ref[0].weight.copy_(m.hidden1.weight); ref[0].bias.copy_(m.hidden1.bias)
        ref[2].weight.copy_(m.out.weight); ref[2].bias.copy_(m.out.bias)
    x = torch.randn(b, 300, device=gpu, requires_grad=True)
    x2 = x.detach().clone().requires_grad_(True)
    y = m(x)
    yr = ref(x2).squeeze()
    assert y.shape == yr.shape
    np.testing.assert_allclose(y.detach().cpu().numpy(), yr.detach().cpu().numpy(), rtol=1e-5, atol=1e-5)
    g = torch.randn_like(yr)
    y.backward(g)
    yr.backward(g)
    pairs = [(x.grad, x2.grad), (m.hidden1.weight.grad, ref[0].weight.grad),
             (m.hidden1.bias.grad, ref[0].bias.grad), (m.out.weight.grad, ref[2].weight.grad),
             (m.out.bias.grad, ref[2].bias.grad)]
    for got, want in pairs:
        np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=1e-4, atol=1e-5)
