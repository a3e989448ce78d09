"""bench.py --gpus N: the rank launcher and the world-size guards (CPU).

VERDICT r05 item 1: `python bench.py --gpus N` with no launcher must run N
ranks (one per GPU) and print ONE rank-0 line with n_gpus = N, or exit
non-zero -- never a P = 1 line.  The multi-rank path runs here under gloo
with the CPU stand-in engine (tests/bench_standin.py, via
KNN_BENCH_TEST_ENGINE); the GPU box's refusal when fewer than N GPUs are
visible is tests/test_gpu_bench_launch.py.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
BENCH = os.path.join(ROOT, "bench.py")
SMALL = ["--m", "240", "--n", "784", "--steps", "2", "--warmup", "1", "--full", "--secondary-steps", "0",
         "--check", "8"]


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK",
                                                              "LOCAL_WORLD_SIZE", "MASTER_PORT")}
    env["KNN_BENCH_TEST_ENGINE"] = "bench_standin:make"
    env.update(kw)
    return env


def _lines(out):
    return [json.loads(l) for l in out.splitlines() if l.startswith("{")]


@pytest.mark.parametrize("gpus,schedule", [(2, "direct"), (3, "ring")])
def test_bench_gpus_n_runs_n_ranks(gpus, schedule):
    r = subprocess.run([sys.executable, BENCH, "--gpus", str(gpus)] + SMALL, cwd=ROOT, capture_output=True,
                       text=True, timeout=300, env=_env(KNN_RING_SCHEDULE=schedule))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = _lines(r.stdout)
    assert len(lines) == 1, r.stdout          # rank 0 only
    line = lines[0]
    assert line["n_gpus"] == gpus
    assert line["config"]["parallelism"] == "ring%d" % gpus
    assert line["launcher"] == "bench.py"
    assert line["rccl_world"] is None         # gloo stand-in, not RCCL
    assert line["check"]["mismatches"] == 0   # rank 0's rows against the oracle
    assert np.isclose(line["value"], 240 / (line["ms_per_step"] * 1e-3))
    assert line["cpu_baseline"] is None       # P > 1: no CPU leg


def test_bench_plain_run_dumps_last_step(tmp_path):
    """a plain run (no --full) times --steps steps, leaves the legs beside the
    headline out of the line, and --dump-outputs writes the last step's
    neighbour records as float64 arrays: the oracle's on the seeded corpus"""
    sys.path.insert(0, os.path.join(ROOT, "mpi-knn_amd"))
    import oracle
    from mpiknn import synth
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--m", "240", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300,
                       env=_env())
    assert r.returncode == 0, r.stderr[-3000:]
    lines = _lines(r.stdout)
    assert len(lines) == 1, r.stdout
    line = lines[0]
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "queries/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert np.isclose(line["value"], 240 / (line["ms_per_step"] * 1e-3))
    for leg in ("check", "check_all_rows", "roofline", "cpu_baseline"):
        assert line[leg] is None, leg
    assert "secondary" not in line
    assert sorted(p.name for p in out.iterdir()) == ["distance.npy", "idx.npy"]
    idx, dist = np.load(out / "idx.npy"), np.load(out / "distance.npy")
    assert idx.dtype == np.float64 and dist.dtype == np.float64
    ref = oracle.knn(synth.mnist_like(240, 784)[0], 30)
    assert np.array_equal(idx, ref["idx"].astype(np.float64))
    assert np.array_equal(dist.view(np.uint64), ref["distance"].view(np.uint64))


def test_bench_dump_samples_large_results():
    """above its byte budget the dump is a fixed seeded sample of the rows"""
    import importlib.util
    import tempfile
    spec = importlib.util.spec_from_file_location("knn_bench", BENCH)
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    import oracle
    k = 64
    nq = bench.DUMP_BUDGET_BYTES // (16 * k) + 1000
    nb = np.zeros((nq, k), dtype=oracle.NB_DTYPE)
    nb["idx"] = np.arange(nq, dtype=np.int32)[:, None]
    picks = []
    for _ in range(2):
        with tempfile.TemporaryDirectory() as d:
            bench.dump_outputs(d, nb, 0, 1)
            files = {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
        assert sorted(files) == ["distance.npy", "idx.npy", "rows.npy"]
        assert sum(a.nbytes for a in files.values()) <= 64 << 20
        assert np.array_equal(files["idx.npy"][:, 0], files["rows.npy"])
        picks.append(files["rows.npy"])
    assert np.array_equal(picks[0], picks[1]) and np.all(np.diff(picks[0]) > 0)


def test_bench_world_size_must_match_gpus():
    """under a launcher, --gpus and WORLD_SIZE must agree"""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2"] + SMALL, cwd=ROOT, capture_output=True,
                       text=True, timeout=120, env=_env(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"))
    assert r.returncode != 0
    assert "WORLD_SIZE" in r.stderr
    assert not _lines(r.stdout)


def test_bench_refuses_more_ranks_than_gpus():
    """no stand-in: the launcher counts the visible GPUs (none here) and
    refuses before starting any rank"""
    env = _env()
    env.pop("KNN_BENCH_TEST_ENGINE")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2"] + SMALL, cwd=ROOT, capture_output=True,
                       text=True, timeout=120, env=env)
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert "visible GPUs" in r.stderr
    assert not _lines(r.stdout)


def test_bench_failed_rank_fails_the_job():
    """a rank that dies ends the launch with a non-zero exit (its peers are
    stopped, no line is printed)"""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2"] + SMALL, cwd=ROOT, capture_output=True,
                       text=True, timeout=300, env=_env(KNN_BENCH_TEST_ENGINE="bench_standin:nosuch"))
    assert r.returncode != 0
    assert not _lines(r.stdout)
