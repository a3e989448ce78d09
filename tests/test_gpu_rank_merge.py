"""The rank merge of int8 lane lists as a P = 1 search's only merge
(knn_launch_merge_rank, fin && first_step): k_merge_rank16 when a query has
at most 16 lists (lists a split x KNN_SPLITS), k_merge_rank -- finalizing,
without a state -- above.  The split count is set on either side of that
boundary and far above it (more than 32 lanes holding lists):

  KNN_I8_KL   lists a split   KNN_SPLITS -> lists a query -> kernel
  12          2               8 -> 16 -> k_merge_rank16;  9 -> 18, 24 -> 48 -> k_merge_rank
  17          4               4 -> 16 -> k_merge_rank16;  5 -> 20 -> k_merge_rank

Every run is compared with the oracle (index AND distance bits, 8-bit
contraction), and the runs of a case with each other, byte for byte.  With
KNN_FORCE_RESCAN=1 every query misses the certificate (force_fail): the
merges publish the whole fail list and the rescan pass rewrites the records."""
import numpy as np
import pytest

import datasets
from test_gpu_h16 import run_engine

pytestmark = pytest.mark.gpu

SPLITS = {"12": (8, 9, 24), "17": (4, 5)}


def _ints(seed, hi, m, n):
    return np.random.default_rng(seed).integers(0, hi, (m, n)).astype(np.float64)


# name -> (rows, k, dtype)
CASES = {
    "mnist": (lambda: datasets.mnist_like(2500, 64, seed=51)[0], 30, "f64"),
    # fp32: the published bound is rounded up to a float
    "sift_f32": (lambda: datasets.sift_like(3000, 128, clusters=16, seed=3), 32, "f32"),
    # the index half of the key decides
    "ties": (lambda: _ints(8, 4, 2000, 24), 30, "f64"),
    # the tighter-bound pass finds its k + 1 head entries nearly always
    "k1": (lambda: datasets.mnist_like(2500, 64, seed=51)[0], 1, "f64"),
    "k2": (lambda: datasets.mnist_like(2500, 64, seed=51)[0], 2, "f64"),
    # fewer than k + 1 candidates: no tighter bound, padding records, the
    # fallback
    "m40": (lambda: _ints(12, 256, 40, 50), 30, "f64"),
    "m20": (lambda: _ints(13, 256, 20, 50), 30, "f64"),
    # a partial last group of 16 queries and a partial last wave of 4
    "m777": (lambda: datasets.mnist_like(777, 64, seed=52)[0], 30, "f64"),
}

_cache = {}


def _case(oracle, name):
    """(rows, k, dtype, the oracle's result): computed once, never changed"""
    if name not in _cache:
        make, k, dtype = CASES[name]
        X = make()
        ref = oracle.knn(X.astype(np.float32).astype(np.float64) if dtype == "f32" else X, k)
        _cache[name] = (X, k, dtype, ref)
    return _cache[name]


@pytest.mark.parametrize("rescan", [False, True], ids=["certified", "force_rescan"])
@pytest.mark.parametrize("kl", ["12", "17"])
@pytest.mark.parametrize("name", list(CASES))
def test_rank_merge_list_boundary(oracle, monkeypatch, name, kl, rescan):
    X, k, dtype, ref = _case(oracle, name)
    monkeypatch.setenv("KNN_I8_KL", kl)
    splits = SPLITS[kl]
    if rescan:
        monkeypatch.setenv("KNN_FORCE_RESCAN", "1")
        splits = splits[:2]   # the boundary pair
    first = None
    for s in splits:
        monkeypatch.setenv("KNN_SPLITS", str(s))
        got, bits = run_engine(X, k, dtype)
        assert bits == 8
        assert np.array_equal(got["idx"], ref["idx"]), s
        assert np.array_equal(got["distance"].view(np.uint64), ref["distance"].view(np.uint64)), s
        if first is None:
            first = got.tobytes()
        assert got.tobytes() == first, s
