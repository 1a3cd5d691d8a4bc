"""What the GPU tests on operands past 2^31 and 2^32 bytes share
(tests/test_gpu_large.py, tests/test_gpu_fused_table16.py): the seeded device
generator of a case of tests/large_cases.py, fills made on the device in the
storage type itself, the stream kernels' inputs, the case's projection, and
host copies of sampled rows.  Plain helper module: no test is collected from
it.
"""
import numpy as np
import torch

import large_cases as LC
import pipeline as P
import synth
from common_gpu import _dev, _networks

FRAME_DTYPE = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def _gen(c, gpu):
    g = torch.Generator(device=gpu)
    g.manual_seed(LC.seed_of(c))
    return g


def _rand(shape, g, gpu, dtype=torch.float32, lo=-1.0, hi=1.0):
    """U(lo, hi) filled on the device, in the storage type itself."""
    return torch.empty(shape, dtype=dtype, device=gpu).uniform_(lo, hi, generator=g)


def _randn(shape, g, gpu, dtype=torch.float32, mean=0.0, std=1.0):
    return torch.empty(shape, dtype=dtype, device=gpu).normal_(mean, std, generator=g)


def _host_upcast(t):
    return t.float().cpu().numpy() if t.dtype in (torch.float16, torch.bfloat16) else t.cpu().numpy()


def _word_table(v, d, g, gpu, dtype=torch.float32):
    """synth.word_table's family on the device: 0.4 N(0, 1) + 0.3 g, row 0 zero."""
    table = _randn((v, d), g, gpu, dtype, 0.0, 0.4)
    table.add_((0.3 * torch.randn(d, generator=g, device=gpu)).to(dtype))
    table[0].zero_()
    return table


def _weights(v, g, gpu):
    """SIF weights of a small vocabulary (synth.sif_weights); seeded U(0.05, 1) of a large one."""
    if v <= 2 ** 16:
        return _dev(synth.sif_weights(v, w0=1.0).astype(np.float32), gpu)
    return _rand((v,), g, gpu, lo=0.05, hi=1.0)


def _stream_inputs(c, gpu, table=None, ids=None):
    z = c.dims
    g = _gen(c, gpu)
    ft = FRAME_DTYPE[z.get("frames", "f32")]
    if table is None:
        table = _word_table(z["v"], z["d"], g, gpu)
    if ids is None:
        ids = torch.randint(0, z["v"], (z["n"], z["t"]), generator=g, device=gpu, dtype=torch.int32)
    return {"table": table, "wtab": _weights(z["v"], g, gpu), "ids": ids,
            "audio": _rand((z["n"], z["t"], z["a"]), g, gpu, ft),
            "visual": _rand((z["n"], z["t"], z["vd"]), g, gpu, ft)}


def _projection(c, gpu):
    z = c.dims
    return P.MMB2Projection(_networks((z["d"], z["a"], z["vd"]), gpu), z["d"], z["a"], z["vd"], z["t"], gpu)
