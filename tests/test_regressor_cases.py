"""CPU: the case tables of tests/regressor_cases.py keep the GPU bars of
tests/test_gpu_regressor_widths.py meaningful.

A training step is discontinuous where a hidden unit's pre-activation or an
output's residual crosses zero: a flipped branch moves W1 by ~1e-3 relative
and says nothing about the kernel.  So every line of TRAIN_CASES must keep
its float64 run clear of both kinks, at every step and for every row, by
MARGIN = 2 worst-case float32 rounding bounds (the bound holds for any
summation order; the weights the device carries into a step differ from the
reference's by far less than the bound).  The stored seeds were found by
search at 4 bounds when the table was written; here they are only checked.
Someone who edits the table into a case that sits on a kink fails here, on
the CPU, instead of chasing a GPU failure that no kernel caused.

Also pinned: the table still reaches every dispatch edge it exists for, and
the LDS arithmetic behind the width limit of mmb_mlp_train.
"""
import numpy as np
import pytest

import mmb_lib
import regressor_cases as C
from oracle import regressor_oracle as R


def test_train_table_is_the_issue_table():
    cs = C.TRAIN_CASES
    assert 28 <= len(cs) <= 34 and len(set(c[:-1] for c in cs)) == len(cs)
    assert {4, 28, 32, 36, 100, 200, 252, 256, 260, 288, 300, 320, 416, 448} <= {c.d for c in cs}
    assert {c.h for c in cs} == {1, 31, 32, 33, 40, 64, 100, 512}
    assert {1, 2, 16} <= {c.o for c in cs} and {c.batch for c in cs} == {1, 5, 32}
    for c in cs:
        assert c.d % 4 == 0 and c.d <= C.train_max_d(c.o)
        assert -(-c.n // c.batch) <= 3                       # at most 3 mini-batches an epoch
        assert c.h <= 40 and c.n <= 35 if c.d >= 250 else True   # the pairing rule
        assert c.d <= 36 if c.h == 512 else True
    assert any(c.n < c.batch for c in cs)
    assert any(c.n % c.batch == 0 and c.n > c.batch for c in cs)
    assert any(c.n % c.batch == 1 and c.n > c.batch > 1 for c in cs)
    assert any(c.nv and c.nv % c.batch for c in cs) and any(not c.nv for c in cs)
    assert {(c.every, c.epoch0) for c in cs if c.nv} == {(1, 0), (3, 0), (1, 2), (3, 2)}
    # the largest accepted width at both ends of n_out
    assert any(c.d == C.train_max_d(1) for c in cs)
    assert any(c.d == C.train_max_d(16) and c.o == 16 for c in cs)
    # a validation that is not after the first epoch, and one that is skipped
    assert any(c.nv and C.n_validations(c) == 1 and (c.epoch0 % c.every) for c in cs)


def test_width_limit_is_the_lds_arithmetic():
    """mmb_mlp_train accepts d <= 32 nTd for the largest nTd whose LDS fits in
    156 KB: 448 up to 13 outputs, 416 for 14 to 16 -- the library's own
    answer, this module's arithmetic and the documented figures agree."""
    for o in range(1, 17):
        want = 448 if o <= 13 else 416
        assert C.train_max_d(o) == want
        assert mmb_lib.query("mmb_mlp_train_max_d", o) == want
        assert C.train_lds_bytes(want // 32, o) <= C.TRAIN_LDS_MAX < C.train_lds_bytes(want // 32 + 1, o)
    assert mmb_lib.query("mmb_mlp_train_max_d", 0) == 0
    assert mmb_lib.query("mmb_mlp_train_max_d", 17) == 0
    header = open(mmb_lib.HERE + "/../include/mmb.h").read()
    assert "448 for n_out <= 13, 416 for n_out = 14..16" in header


def test_inputs_are_f32_representable_and_seeded_by_the_case():
    c = C.TRAIN_CASES[1]
    z, z2 = C.make_train_inputs(c), C.make_train_inputs(c)
    for a in (z["x"], z["y"], *z["params"], z["valid"][0], z["valid"][1]):
        assert a.dtype == np.float64 and np.array_equal(C.f32(a), a)
    assert np.array_equal(z["x"], z2["x"]) and np.array_equal(z["perm"], z2["perm"])
    assert not np.array_equal(C.make_train_inputs(c, seed=c.seed + 1)["x"], z["x"])
    assert sorted(z["perm"][:c.n]) == list(range(c.n)) and len(z["perm"]) == C.N_EPOCHS * c.n
    assert len(z["valid"][2]) == C.n_validations(c) * c.nv


@pytest.mark.parametrize("c", C.TRAIN_CASES, ids=[C.train_id(c) for c in C.TRAIN_CASES])
def test_training_case_keeps_clear_of_the_kinks(c):
    ref = C.train_reference(c)
    spe = -(-c.n // c.batch)
    assert len(ref["step_loss"]) == C.N_EPOCHS * spe
    assert len(ref["valid_loss"]) == C.n_validations(c) * -(-c.nv // c.batch)
    print(f"{C.train_id(c)}: margin {ref['margin']:.2f} bounds")
    assert ref["margin"] >= C.MARGIN


def test_reference_run_is_torch_autograd_sgd():
    """The plain-numpy run is the reference's algorithm: torch autograd of
    L1(reduction='none').mean() and optim.SGD in float64 give the same run."""
    import torch

    c = next(c for c in C.TRAIN_CASES if c.d == 100 and c.nv)
    z = C.make_train_inputs(c)
    ref = C.train_reference(c)
    m = torch.nn.Sequential(torch.nn.Linear(c.d, c.h), torch.nn.ReLU(), torch.nn.Linear(c.h, c.o)).double()
    with torch.no_grad():
        for p, a in zip(m.parameters(), z["params"]):
            p.copy_(torch.tensor(a))
    opt = torch.optim.SGD(m.parameters(), lr=C.LR)
    x, y = torch.tensor(z["x"]), torch.tensor(z["y"])
    xv, yv, vperm, every, epoch0 = z["valid"]
    sl, vl, k = [], [], 0
    for e in range(C.N_EPOCHS):
        order = z["perm"][e * c.n:(e + 1) * c.n]
        for s in range(0, c.n, c.batch):
            idx = order[s:s + c.batch]
            opt.zero_grad()
            loss = (m(x[idx]) - y[idx]).abs().mean()
            loss.backward()
            opt.step()
            sl.append(loss.item())
        if (epoch0 + e) % every == 0:
            with torch.no_grad():
                vo = vperm[k * c.nv:(k + 1) * c.nv]
                for s in range(0, c.nv, c.batch):
                    idx = vo[s:s + c.batch]
                    vl.append((m(torch.tensor(xv[idx])) - torch.tensor(yv[idx])).abs().mean().item())
            k += 1
    np.testing.assert_allclose(ref["step_loss"], sl, rtol=1e-13)
    np.testing.assert_allclose(ref["valid_loss"], vl, rtol=1e-13)
    for a, p in zip(ref["params"], m.parameters()):
        np.testing.assert_allclose(a, p.detach().numpy(), rtol=0, atol=1e-14)


def test_backward_reference_is_torch_autograd():
    c = C.FwdCase(50, 33, 3, 5)
    rng = np.random.default_rng(0)
    import torch

    x = torch.tensor(rng.standard_normal((c.b, c.d)), requires_grad=True)
    ps = [torch.tensor(a, requires_grad=True) for a in C.make_params(rng, c.d, c.h, c.o)]
    dy = rng.standard_normal((c.b, c.o))
    hid = torch.relu(x @ ps[0].T + ps[1])
    (hid @ ps[2].T + ps[3]).backward(torch.tensor(dy))
    g, bounds = C.backward_bounds(x.detach().numpy(), hid.detach().numpy(), ps[0].detach().numpy(),
                                  ps[2].detach().numpy(), dy)
    for k, t in (("dx", x), ("dw1", ps[0]), ("db1", ps[1]), ("dw2", ps[2]), ("db2", ps[3])):
        np.testing.assert_allclose(g[k], t.grad.numpy(), rtol=0, atol=1e-13)
        assert bounds[k].shape == g[k].shape and (bounds[k] >= 0).all()


def test_f32_envelope_is_rounding_sized():
    """The float32 CPU run of every case stays within a few 1e-6 of the float64
    one (the GPU bar is 4x this, per case): no case amplifies rounding."""
    worst = (0.0, 0.0)
    for c in C.TRAIN_CASES:
        p, l = C.f32_envelope(c)
        worst = (max(worst[0], p), max(worst[1], l))
        assert p < 2e-5 and l < 2e-6, (C.train_id(c), p, l)
    print(f"f32 CPU run vs f64: parameters up to {worst[0]:.2e}, losses up to {worst[1]:.2e}")


def test_fwd_table_reaches_both_row_kernels_and_their_edges():
    cs = C.FWD_CASES
    assert {1, 3, 4, 5, 50, 100, 255, 256, 257, 300, 301, 512, 600} == {c.d for c in cs}
    assert {1, 100, 127, 128, 129, 257, 300} <= {c.h for c in cs}
    assert {1, 3, 4, 5, 8, 9, 17} == {c.b for c in cs} and {1, 3, 16} == {c.o for c in cs}
    v4 = {(c.d, c.h) for c in cs if C.takes_v4(c.d, c.h)}
    sc = {(c.d, c.h) for c in cs if not C.takes_v4(c.d, c.h)}
    # both sides of the LDS threshold at three widths, and of d % 4
    for d, h in ((300, 122), (512, 68), (600, 56)):
        assert (d, h) in v4 and (d, h + 1) in sc
    assert any(d % 4 for d, _ in sc) and any(h > 128 for _, h in v4) and any(h > 256 for _, h in sc)
    assert C.mlp_wld(300) == 308 and C.mlp_wld(512) == 532 and all(
        C.mlp_wld(d) % 32 == 20 and 0 <= C.mlp_wld(d) - d < 36 for d in range(1, 700))
