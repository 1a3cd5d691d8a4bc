"""Shared case tables, inputs and float64 references of
tests/test_gpu_regressor_widths.py (GPU) and tests/test_regressor_cases.py
(CPU): the sentiment regressor's kernels (csrc/mlp_kernels.hip) at widths
other than 300; tests/regressor_gpu.py, tests/test_gpu_scratch.py and
tests/test_gpu_large.py read the same tables.  Plain helper module: no test
is collected from it.

Inputs are seeded from the case alone, rounded to f32 and widened back, so the
device sees exactly what the float64 reference sees: rows N(0, 1), labels
U(-3, 3), parameters U(+-1/sqrt(fan_in)) like nn.Linear's.

A training step is discontinuous at pre = 0 (ReLU) and y = label (the L1
sign), so a training case means something only while the float64 run stays
clear of both: `margin` of oracle.regressor_oracle.sgd_run, at least MARGIN
float32 bounds at every step and row.  The seeds in TRAIN_CASES were searched
for that when the table was written (search_seed, at twice that margin; never
at test time) and tests/test_regressor_cases.py asserts it.
"""
from __future__ import annotations

import collections
import functools
import importlib.util
import json
import os

import numpy as np

from oracle import regressor_oracle as R

MARGIN = 2.0
N_EPOCHS = 2
LR = float(np.float32(0.05))
U32 = R.U32
FLOOR = 8 * 2.0 ** -24  # the training bars (4x the float32 CPU run's own deviation) are not below this

# LDS of mlp_train_mc_kernel (csrc/mlp_kernels.hip, train_lds_bytes): what
# decides the largest width mmb_mlp_train accepts for a number of outputs
TRAIN_LDS_MAX = 156 * 1024


def train_lds_bytes(ntd, o):
    return 4 * (6 * 32 + 2 * 32 * (32 * ntd + 1) + 2 * 32 * o + 8 * 32 * 32 + 32 * 32 + 32 * o +
                o * 32 + 32 + o + 8)


def train_max_d(o):
    return 32 * max(t for t in range(0, 17) if t == 0 or train_lds_bytes(t, o) <= TRAIN_LDS_MAX)


TrainCase = collections.namedtuple("TrainCase", "d h o batch n nv every epoch0 seed")

# d, h, n_out, batch, n, n_valid (0: no validation), valid_every, epoch0, seed
TRAIN_CASES = [
    # NTD 1 and 2: fewer feature tiles than waves (nwu < 8)
    TrainCase(4, 1, 1, 1, 3, 0, 1, 0, 0),          # the smallest of everything; batch 1
    TrainCase(4, 32, 2, 5, 11, 7, 1, 0, 0),        # last batch of one row; ragged validation
    TrainCase(4, 100, 16, 32, 33, 40, 1, 0, 0),    # P = 4 at NTD 1, 16 outputs
    TrainCase(8, 512, 1, 32, 64, 0, 1, 0, 0),      # P = 16; n a multiple of the batch
    TrainCase(28, 31, 1, 32, 20, 0, 1, 0, 0),      # partial tile both ways; n < batch
    TrainCase(28, 512, 1, 32, 33, 0, 1, 0, 1),     # P = 16, last batch of one row
    TrainCase(32, 33, 16, 32, 64, 40, 3, 0, 0),    # one full tile; h one past the tile; every 3
    TrainCase(32, 64, 1, 5, 15, 0, 1, 0, 0),
    TrainCase(32, 31, 1, 1, 3, 2, 1, 0, 0),        # batch 1 with validation
    TrainCase(36, 512, 2, 5, 12, 9, 1, 2, 0),      # NTD 2, P = 16, epoch0 2
    TrainCase(36, 1, 16, 1, 2, 3, 3, 2, 0),        # every 3 from epoch0 2: validates after the 2nd epoch only
    TrainCase(36, 100, 1, 32, 65, 0, 1, 0, 0),
    # GloVe widths
    TrainCase(100, 31, 1, 32, 65, 33, 1, 0, 1),
    TrainCase(100, 64, 2, 5, 12, 0, 1, 0, 0),
    TrainCase(100, 100, 16, 32, 32, 0, 1, 0, 0),
    TrainCase(200, 33, 1, 32, 40, 0, 1, 0, 1),
    TrainCase(200, 64, 2, 5, 15, 8, 1, 0, 0),
    # NTD 8 (the last width with one tile per wave) and 9 (the first with two)
    TrainCase(252, 32, 1, 32, 33, 0, 1, 0, 4),
    TrainCase(256, 33, 2, 5, 11, 0, 1, 0, 0),
    TrainCase(260, 33, 2, 5, 12, 0, 1, 0, 0),
    TrainCase(260, 31, 1, 32, 32, 20, 1, 0, 3),
    TrainCase(288, 32, 16, 32, 33, 0, 1, 0, 0),
    TrainCase(300, 40, 1, 32, 35, 0, 1, 0, 14),    # the control width
    TrainCase(300, 33, 1, 5, 11, 6, 3, 2, 0),
    TrainCase(320, 1, 1, 32, 35, 0, 1, 0, 0),
    TrainCase(320, 33, 2, 32, 20, 0, 1, 0, 0),
    # the largest accepted widths: 448 for n_out <= 13, 416 for n_out = 14..16
    TrainCase(448, 33, 1, 32, 33, 0, 1, 0, 26),
    TrainCase(448, 32, 2, 5, 11, 7, 1, 0, 0),
    TrainCase(448, 1, 13, 1, 3, 0, 1, 0, 0),
    TrainCase(416, 40, 16, 32, 33, 0, 1, 0, 54),
    TrainCase(416, 32, 16, 5, 12, 6, 1, 0, 3),
]


def train_id(c):
    v = f"-v{c.nv}e{c.every}s{c.epoch0}" if c.nv else ""
    return f"d{c.d}-h{c.h}-o{c.o}-B{c.batch}-n{c.n}{v}"


def f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def make_params(rng, d, h, o):
    k1, k2 = 1 / np.sqrt(d), 1 / np.sqrt(h)
    return (f32(rng.uniform(-k1, k1, (h, d))), f32(rng.uniform(-k1, k1, h)),
            f32(rng.uniform(-k2, k2, (o, h))), f32(rng.uniform(-k2, k2, o)))


def n_validations(c):
    return sum(1 for e in range(N_EPOCHS) if (c.epoch0 + e) % c.every == 0) if c.nv else 0


def make_train_inputs(c, seed=None):
    """dict(x, y, perm, params, valid) of a training case: f32-representable
    float64; valid = (xv, yv, vperm, every, epoch0) or None."""
    key = [c.d, c.h, c.o, c.batch, c.n, c.nv, c.every, c.epoch0, c.seed if seed is None else seed]
    rng = np.random.default_rng(key)
    z = {"x": f32(rng.standard_normal((c.n, c.d))), "y": f32(rng.uniform(-3, 3, (c.n, c.o))),
         "params": make_params(rng, c.d, c.h, c.o),
         "perm": np.concatenate([rng.permutation(c.n) for _ in range(N_EPOCHS)]), "valid": None}
    if c.nv:
        xv, yv = f32(rng.standard_normal((c.nv, c.d))), f32(rng.uniform(-3, 3, (c.nv, c.o)))
        vperm = np.concatenate([rng.permutation(c.nv) for _ in range(max(n_validations(c), 1))])
        z["valid"] = (xv, yv, vperm, c.every, c.epoch0)
    return z


def run_reference(c, dtype=np.float64, seed=None, margins=False):
    z = make_train_inputs(c, seed)
    return R.sgd_run(z["x"], z["y"], z["perm"], N_EPOCHS, c.batch, LR, z["params"], z["valid"],
                     dtype=dtype, margins=margins)


@functools.lru_cache(maxsize=None)
def train_reference(c):
    """The float64 run of a case (with its margin), computed once."""
    return run_reference(c, margins=True)


def rel_dev(got, ref):
    """Deviation of a run from the float64 one: parameters relative to each
    tensor's largest entry, losses relative to each loss.  (params, losses)."""
    p = max(float(np.abs(np.asarray(g, np.float64) - r).max() / np.abs(r).max())
            for g, r in zip(got["params"], ref["params"]))
    ls = [np.abs(np.asarray(got[k], np.float64) - ref[k]) / np.abs(ref[k])
          for k in ("step_loss", "valid_loss") if len(ref[k])]
    return p, max(float(a.max()) for a in ls)


@functools.lru_cache(maxsize=None)
def f32_envelope(c):
    """(params, losses): how far the same algorithm run in float32 on the CPU
    lands from the float64 run."""
    return rel_dev(run_reference(c, dtype=np.float32), train_reference(c))


def search_seed(c, margin=MARGIN, tries=200):
    """The first seed whose float64 run keeps `margin` (table-writing time only)."""
    for s in range(tries):
        if run_reference(c, seed=s, margins=True)["margin"] >= margin:
            return s
    return None


# ------------------------------------------------------------------ stateless entry points
FwdCase = collections.namedtuple("FwdCase", "d h o b")

# d, h, n_out, rows: mmb_mlp_forward / _eval / _forward_train / _backward
FWD_CASES = [
    FwdCase(1, 1, 1, 1),          # the smallest of everything; scalar path
    FwdCase(3, 100, 3, 3),        # d % 4 != 0: scalar
    FwdCase(4, 127, 1, 4),        # V4 at one float4 per row; h one below the V4 stride
    FwdCase(5, 128, 16, 5),       # scalar; h = the V4 stride
    FwdCase(4, 129, 3, 8),        # V4, h one past its stride; a full 8-row block
    FwdCase(50, 100, 1, 9),       # GloVe 50 (scalar: 50 % 4 = 2); one row past a block
    FwdCase(100, 100, 3, 17),     # GloVe 100, V4; three blocks, the last of one row
    FwdCase(100, 257, 1, 5),      # V4, h one past the scalar stride of 256
    FwdCase(255, 257, 3, 3),      # scalar path with h past its stride of 256
    FwdCase(256, 128, 16, 4),     # V4; half an 8-row block (the second half empty)
    FwdCase(256, 129, 1, 5),      # V4; one row in the second half
    FwdCase(257, 127, 3, 8),      # scalar at d past 256
    FwdCase(300, 100, 1, 17),     # the control: V4
    FwdCase(300, 122, 1, 4),      # the last h whose staged W1 fits in LDS at d = 300
    FwdCase(300, 123, 1, 4),      # the first past it: scalar
    FwdCase(300, 127, 16, 9),     # scalar by the LDS fallback
    FwdCase(300, 128, 3, 8),
    FwdCase(300, 300, 1, 1),      # h past the scalar stride of 256
    FwdCase(301, 129, 3, 4),      # scalar, d % 4 = 1
    FwdCase(512, 1, 1, 3),        # V4 at d = 512
    FwdCase(512, 68, 3, 5),       # the last h on V4 at d = 512
    FwdCase(512, 69, 3, 5),       # the first past it
    FwdCase(512, 100, 16, 8),     # scalar by the LDS fallback
    FwdCase(600, 56, 3, 17),      # the widest: the last h on V4
    FwdCase(600, 57, 3, 4),       # the first past it
    FwdCase(600, 257, 1, 9),      # scalar
]


def fwd_id(c):
    return f"d{c.d}-h{c.h}-o{c.o}-b{c.b}"


def mlp_wld(d):
    """Row stride of the W1 staged in LDS (csrc/mlp_kernels.hip, mlp_wld)."""
    r = (d + 3) // 4 * 4
    return r + (20 - r % 32) % 32


def takes_v4(d, h):
    """mmb_mlp_forward_train's dispatch for a 16-byte aligned w1."""
    return d % 4 == 0 and 4 * (8 * (d + h) + h * mlp_wld(d)) <= 160 * 1024


@functools.lru_cache(maxsize=None)
def fwd_inputs(c):
    """x, params, dy, labels of a stateless case (f32-representable float64) and
    the float64 forward, computed once and read-only."""
    rng = np.random.default_rng([c.d, c.h, c.o, c.b])
    z = {"x": f32(rng.standard_normal((c.b, c.d))), "params": make_params(rng, c.d, c.h, c.o),
         "dy": f32(rng.standard_normal((c.b, c.o))), "labels": f32(rng.uniform(-3, 3, (c.b, c.o)))}
    z["y"], z["pre"], z["hid"] = R.mlp_forward(z["x"], *z["params"])
    z["pre_bound"] = R.pre_bound(z["x"], *z["params"][:2])
    z["y_bound"] = R.out_bound(z["x"], *z["params"])
    for v in list(z.values()):
        for a in (v if isinstance(v, tuple) else (v,)):
            a.setflags(write=False)
    return z


def backward_bounds(x, hid, w1, w2, dy):
    """Worst-case float32 rounding (any summation order) of every output of
    mlp_backward, (terms + 1) 2^-24 sum |terms| per dot product; the sums over
    dh carry dh's own bound through as well."""
    g = R.mlp_backward(x, hid, w1, w2, dy)
    b, o = dy.shape
    h = w1.shape[0]
    e_dh = (o + 1) * U32 * (np.abs(dy) @ np.abs(w2)) * (hid > 0)
    a_dh = np.abs(g["dh"])
    return g, {
        "dh": e_dh,
        "dx": (h + 1) * U32 * (a_dh @ np.abs(w1)) + e_dh @ np.abs(w1),
        "dw1": (b + 1) * U32 * (a_dh.T @ np.abs(x)) + e_dh.T @ np.abs(x),
        "db1": (b + 1) * U32 * a_dh.sum(0) + e_dh.sum(0),
        "dw2": (b + 1) * U32 * (np.abs(dy).T @ np.abs(hid)),
        "db2": (b + 1) * U32 * np.abs(dy).sum(0),
    }


# ---------------------------------------------------------------- the recorded full-size runs
# (tests/test_regressor_oracle.py on the CPU, tests/test_gpu_regressor.py on the device)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _gen():
    spec = importlib.util.spec_from_file_location(
        "make_goldens_regressor", os.path.join(GOLDEN, "make_goldens_regressor.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def full_case(name):
    """(args, latents, labels, fixture, meta) of a g5_full* fixture, inputs
    regenerated from the recorded seed and checked by checksum."""
    g = _gen()
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        meta = json.load(f)
    lat, lab = g.latents_and_labels(int(z["seed"]), noise=meta["noise"],
                                    flip_valid=meta["flip_valid"])
    assert np.allclose([g.checksum(l) for l in lat], z["lat_checksums"], rtol=0, atol=1e-9)
    assert np.allclose([g.checksum(l) for l in lab], z["label_checksums"], rtol=0, atol=1e-9)
    return dict(meta["args"]), lat, lab, z, meta
