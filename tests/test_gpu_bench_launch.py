"""bench.py --gpus N on the GPU box.

With fewer than N GPUs visible, `bench.py --gpus N` must refuse before any
rank starts (exit 2, no JSON line) -- never print a P = 1 line under an
N-GPU request.  With N GPUs visible (a multi-GPU node) it starts N ranks
over RCCL; that run is the driver's, so only the refusal is tested here.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def test_bench_plain_run_dumps_last_step(tmp_path, oracle):
    """a plain `--gpus 1` run on libknn: one line without the --full legs, and
    --dump-outputs holds the last timed step's neighbours, bit-exact to the
    oracle on the seeded corpus (2000 rows: several workgroups, a part tile)"""
    import numpy as np
    from mpiknn import synth
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "KNN_BENCH_TEST_ENGINE")}
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--m", "2000", "--steps", "2",
                        "--warmup", "1", "--dump-outputs", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = lines[0]
    assert line["steps"] == 2 and line["n_gpus"] == 1 and line["ms_per_step"] > 0
    assert line["roofline"] is None and line["check"] is None and line["cpu_baseline"] is None
    assert "secondary" not in line
    idx, dist = np.load(out / "idx.npy"), np.load(out / "distance.npy")
    assert idx.dtype == np.float64 and dist.dtype == np.float64 and idx.shape == (2000, 30)
    ref = oracle.knn(synth.mnist_like(2000, 784)[0], 30)
    assert np.array_equal(idx, ref["idx"].astype(np.float64))
    assert np.array_equal(dist.view(np.uint64), ref["distance"].view(np.uint64))


def test_bench_gpus_more_than_visible_refuses():
    import torch
    n = torch.cuda.device_count()
    want = n + 1
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "KNN_BENCH_TEST_ENGINE")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(want), "--steps", "1",
                        "--warmup", "0", "--secondary-steps", "0", "--no-cpu-baseline"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert "visible GPUs" in r.stderr
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]
