"""CPU restatement of the sentiment regressor loop (a10/a11) — TEST INFRASTRUCTURE ONLY.

Follows `/root/reference/sentiment_model.py`:
  SentimentModel            :29-41   squeeze(out(relu(hidden1(x))))
  predict_sentiment         :52-74   one shuffled pass, L1 sums
  train_sentiment           :76-163  SGD on mean L1 over shuffled batches of 32,
                                      validation every 10 epochs, early stopping
                                      (patience 10, 3 trials, lr decay, best reload)
  train_sentiment_for_latents :165-265 init, test predictions before/after,
                                      the reload-best quirk (:243-250: a NEW model
                                      is built -- consuming the torch RNG -- and
                                      then not used)

torch on the CPU, consuming the global torch RNG in the reference's order (model
init, then each DataLoader pass draws its iterator base seed and its sampler
permutation), so with the same `torch.manual_seed` the same rows meet the same
weights.  The best-model checkpoint is kept in memory (a torch.save / torch.load
round trip of a state dict is exact).  Used by the CPU tests (against the
reference fixtures g5_*) and as bench.py's regressor cpu_baseline.
"""
from __future__ import annotations

import copy

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.utils.data import DataLoader, Dataset


class _Labels(Dataset):
    def __init__(self, y, dtype=torch.float32):
        self.y = torch.as_tensor(y, dtype=torch.float32).to(dtype)

    def __len__(self):
        return self.y.shape[0]

    def __getitem__(self, i):
        return i, self.y[i]


class Regressor(nn.Module):
    def __init__(self, d, h, o):
        super().__init__()
        self.hidden1 = nn.Linear(d, h)
        self.out = nn.Linear(h, o)

    def forward(self, x):
        return self.out(F.relu(self.hidden1(x))).squeeze()


def predict(loader, model, lat):
    preds, ys = [], []
    with torch.no_grad():
        for j, y in loader:
            preds.append(model(lat[j]))
            ys.append(y)
    return torch.cat(preds).numpy(), torch.cat(ys).numpy()


def train(args, model, train_loader, train_lat, valid_loader, valid_lat, valid_niter=10, order=None):
    """sentiment_model.py:76-163; returns (train_losses, valid_losses, events).
    `order` (a list) collects the row indices of every training step."""
    lr = args["sentiment_lr"]
    patience, n_trials = 10, 3
    opt = torch.optim.SGD(model.parameters(), lr=lr)
    train_losses, valid_losses = [], []
    n_bad = n_bad_trials = 0
    best = None
    events = {"reloads": 0, "early_stop": False}
    for i in range(args["n_sentiment_epochs"]):
        epoch_loss = torch.zeros((), dtype=next(model.parameters()).dtype)
        nb = 0
        for j, y in train_loader:
            nb += 1
            if order is not None:
                order.append(j.clone())
            model.zero_grad()
            loss = (model(train_lat[j]) - y).abs()
            epoch_loss = epoch_loss + loss.mean()
            loss.mean().backward()
            opt.step()
        train_losses.append(float(epoch_loss / nb))
        if i % valid_niter == 0:
            vl = torch.zeros((), dtype=epoch_loss.dtype)
            vb = 0
            with torch.no_grad():
                for j, y in valid_loader:
                    vl = vl + (model(valid_lat[j]) - y).abs().mean()
                    vb += 1
            v = float(vl / vb)
            is_better = len(valid_losses) == 0 or v < min(valid_losses)
            valid_losses.append(v)
            if args["early_stopping"]:
                if is_better:
                    n_bad = 0
                    best = (copy.deepcopy(model.state_dict()), copy.deepcopy(opt.state_dict()))
                else:
                    n_bad += 1
                    if n_bad >= patience:
                        n_bad_trials += 1
                        if n_bad_trials < n_trials:
                            model.load_state_dict(best[0])
                            opt.load_state_dict(best[1])
                            events["reloads"] += 1
                            lr = lr * args["lr_decay"]
                            for g in opt.param_groups:
                                g["lr"] = lr
                            n_bad = 0
                        else:
                            events["early_stop"] = True
                            break
    return train_losses, valid_losses, events


def train_for_latents(args, latents, labels, batch=32, dtype=torch.float32):
    """sentiment_model.py:165-265 with metrics left to the caller: returns
    dict(before=(pred, y), after=(pred, y), train_losses, valid_losses,
    state, init, order, events; order: the row indices of every training
    step).  Call `torch.manual_seed(s)` first, like the reference run.
    dtype=torch.float64 computes the same run -- the float32 initial weights,
    the same sample orders -- in float64."""
    tr, va, te = (torch.as_tensor(l, dtype=torch.float32).to(dtype) for l in latents)
    ytr, yva, yte = labels
    n_out = 1 if ytr.ndim == 1 else ytr.shape[-1]
    model = Regressor(tr.shape[-1], args["sentiment_hidden_size"], n_out).to(dtype)
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    loaders = [DataLoader(_Labels(y, dtype), batch_size=batch, shuffle=True) for y in (ytr, yva, yte)]
    model.eval()
    before = predict(loaders[2], model, te)
    model.train()
    order = []
    tl, vl, events = train(args, model, loaders[0], tr, loaders[1], va, order=order)
    if args["early_stopping"]:
        Regressor(tr.shape[-1], args["sentiment_hidden_size"], n_out)  # :244, RNG only
    model.eval()
    after = predict(loaders[2], model, te)
    return {"before": before, "after": after, "train_losses": tl, "valid_losses": vl,
            "state": {k: v.detach().clone() for k, v in model.state_dict().items()},
            "init": init, "order": order, "events": events}


# ---------------------------------------------------------------- plain numpy
# The regressor's arithmetic restated without torch, in a chosen precision:
# the float64 reference of the kernel tests at widths other than 300
# (tests/regressor_cases.py) and, run in float32, the measure of what float32
# rounding alone does to an SGD run.
U32 = 2.0 ** -24  # unit roundoff of float32


def mlp_forward(x, w1, b1, w2, b2):
    """(y [b, o], pre [b, h], hid [b, h]) of y = relu(x W1^T + b1) W2^T + b2."""
    pre = x @ w1.T + b1
    hid = np.maximum(pre, 0)
    return hid @ w2.T + b2, pre, hid


def mlp_backward(x, hid, w1, w2, dy):
    """Gradients of mlp_forward for an upstream dy [b, o], given the post-ReLU
    activations: dict(dh, dx, dw1, db1, dw2, db2)."""
    dh = (dy @ w2) * (hid > 0)
    return {"dh": dh, "dx": dh @ w1, "dw1": dh.T @ x, "db1": dh.sum(0), "dw2": dy.T @ hid,
            "db2": dy.sum(0)}


def pre_bound(x, w1, b1):
    """Worst-case float32 rounding of pre [b, h] for any summation order:
    (d + 1) 2^-24 (|b1| + sum_d |w1 x|)."""
    return (x.shape[1] + 1) * U32 * (np.abs(b1) + np.abs(x) @ np.abs(w1).T)


def out_bound(x, w1, b1, w2, b2):
    """The same for y [b, o]: the second layer's own (h + 1) 2^-24 term plus the
    first layer's bound pushed through |W2| (ReLU is 1-Lipschitz)."""
    _, _, hid = mlp_forward(x, w1, b1, w2, b2)
    own = (w1.shape[0] + 1) * U32 * (np.abs(b2) + hid @ np.abs(w2).T)
    return own + pre_bound(x, w1, b1) @ np.abs(w2).T


def l1_batches(x, y, perm, batch, params):
    """Per-batch mean L1 over consecutive slices of perm (the last one ragged)
    and the predictions in perm order."""
    losses, preds = [], []
    for s in range(0, len(perm), batch):
        idx = perm[s:s + batch]
        out = mlp_forward(x[idx], *params)[0]
        preds.append(out)
        losses.append(np.abs(out - y[idx]).mean(dtype=out.dtype))
    return np.array(losses), np.concatenate(preds)


def sgd_run(x, y, perm, n_epochs, batch, lr, params, valid=None, dtype=np.float64, margins=False):
    """sentiment_model.py:98-127 on given sample orders: mean L1 over
    rows * n_out, its sign gradient, p -= lr grad; mini-batches are consecutive
    slices of perm[e * n:(e + 1) * n] with a ragged last one.  valid = (xv, yv,
    vperm, valid_every, epoch0): after every epoch e with (epoch0 + e) %
    valid_every == 0 the per-batch mean L1 of the k-th slice of vperm with the
    weights of that moment.  Everything is computed in `dtype`.

    Returns dict(params, step_loss, valid_loss, margin); with margins=True,
    margin = the smallest, over every training step and row, of
    |pre| / pre_bound and |y - label| / out_bound: how far the run stays from
    the kinks of the ReLU and of the L1 sign, in units of the float32 bound."""
    x, y = np.asarray(x, dtype), np.asarray(y, dtype)
    w1, b1, w2, b2 = (np.array(p, dtype) for p in params)
    lr = dtype(lr)
    n = x.shape[0]
    step_loss, valid_loss, k = [], [], 0
    margin = np.inf
    for e in range(n_epochs):
        order = perm[e * n:(e + 1) * n]
        for s in range(0, n, batch):
            idx = order[s:s + batch]
            xb, yb = x[idx], y[idx]
            out, pre, hid = mlp_forward(xb, w1, b1, w2, b2)
            diff = out - yb
            if margins:
                margin = min(margin, float((np.abs(pre) / pre_bound(xb, w1, b1)).min()),
                             float((np.abs(diff) / out_bound(xb, w1, b1, w2, b2)).min()))
            step_loss.append(np.abs(diff).mean(dtype=dtype))
            g = mlp_backward(xb, hid, w1, w2, np.sign(diff) / dtype(diff.size))
            w1, b1 = w1 - lr * g["dw1"], b1 - lr * g["db1"]
            w2, b2 = w2 - lr * g["dw2"], b2 - lr * g["db2"]
        if valid is not None and (valid[4] + e) % valid[3] == 0:
            xv, yv, vperm = np.asarray(valid[0], dtype), np.asarray(valid[1], dtype), valid[2]
            nv = xv.shape[0]
            valid_loss.extend(l1_batches(xv, yv, vperm[k * nv:(k + 1) * nv], batch,
                                         (w1, b1, w2, b2))[0])
            k += 1
    return {"params": (w1, b1, w2, b2), "step_loss": np.array(step_loss, dtype),
            "valid_loss": np.array(valid_loss, dtype), "margin": margin}
