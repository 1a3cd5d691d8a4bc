"""CPU: bench.py's contract pieces that need no GPU.

* `bench.py --gpus 2` outside torchrun starts the ranks itself (a child
  torch.distributed.run), here in --launch-check mode: both ranks join a gloo
  group and all-reduce a one, rank 0 reports what it saw.
* the algorithmic byte counts the roofline divides by.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", [2, 3])
def test_bench_self_launches_n_ranks(n):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n),
                        "--launch-check"], capture_output=True, text=True, timeout=300, env=env,
                       cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout  # rank 0 only
    out = json.loads(lines[0])
    assert out["ranks_seen"] == n and out["allreduce_sum"] == n
    assert out["pid"] != os.getpid()
    assert "launching %d ranks" % n in r.stderr


def test_single_rank_launch_check_runs_in_process():
    env = {k: v for k, v in os.environ.items() if k != "WORLD_SIZE"}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--launch-check"],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1])["ranks_seen"] == 1
    assert "launching" not in r.stderr


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path):
    """--dump-outputs: float32 / float64 .npy files, the same seeded rows on
    every call, at most 64 MB at the bench shape (300-d rows), every row of a
    split no larger than the sample."""
    import types

    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import bench

    assert 2 * bench.DUMP_SAMPLE_ROWS * 300 * 4 + bench.DUMP_SAMPLE_ROWS * 8 <= 64 << 20
    n = bench.DUMP_SAMPLE_ROWS + 1000
    sif = torch.arange(n, dtype=torch.float32)[:, None].repeat(1, 3)
    mmb2 = -sif
    step = types.SimpleNamespace(n=n)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, 0, 1, 0, step, sif, mmb2)
    bench.dump_outputs(b, 0, 1, 0, step, sif, mmb2)
    assert sorted(os.listdir(a)) == ["mmb2.npy", "rows.npy", "sif.npy"]
    za = {f: np.load(os.path.join(a, f)) for f in os.listdir(a)}
    for f, arr in za.items():
        assert arr.dtype in (np.float32, np.float64), f
        assert np.array_equal(arr, np.load(os.path.join(b, f))), f
    rows = za["rows.npy"]
    assert rows.shape == (bench.DUMP_SAMPLE_ROWS,) and np.all(np.diff(rows) > 0)
    assert rows[0] >= 0 and rows[-1] < n
    assert np.array_equal(za["sif.npy"][:, 0], rows)
    assert np.array_equal(za["mmb2.npy"], -za["sif.npy"])
    # a small split whole; a rank's rows are numbered in the split and named by rank
    small = types.SimpleNamespace(n=10)
    c = str(tmp_path / "c")
    bench.dump_outputs(c, 1, 2, 40, small, sif[:10], mmb2[:10])
    assert sorted(os.listdir(c)) == ["mmb2_rank1.npy", "rows_rank1.npy", "sif_rank1.npy"]
    assert np.array_equal(np.load(os.path.join(c, "rows_rank1.npy")), np.arange(40.0, 50.0))
    assert np.array_equal(np.load(os.path.join(c, "sif_rank1.npy")), sif[:10].numpy())


def test_algorithmic_bytes_match_survey():
    sys.path.insert(0, ROOT)
    import bench

    assert bench.path_bytes(40, 300, 300, 300) == 149_120  # SURVEY §8d B_utt at configs[3]
    assert bench.stream_kernel_bytes(40, 300, 300, 300) == 152_728
    # ragged: id-0 pad rows counted once per utterance (text_rows = n_tok + 1)
    assert bench.path_bytes(64, 300, 300, 300, text_rows=41) == 8 * 64 + 1200 * 41 + 2400 * 64 + 4800
