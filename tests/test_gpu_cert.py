"""Soundness of the GEMM-mode certificate where it decides: data whose
common offset makes |q|^2 + |c|^2 >> d^2, so the cancellation in qn + cn -
2 q.c lifts the filter's error to the gap between the k-th neighbour and the
first dropped candidate, and E (knn_cert_E) -- not the data's slack -- is
what keeps a wrong neighbour from being certified.  Every comparison is idx
equal and distance equal bit for bit against the CPU oracle (fp32 blocks: the
oracle on the fp32-rounded points).  tests/test_cert_cpu.py shows from the
numpy model of tests/cert_ref.py that each sweep here crosses the
transition; the unresolved counts printed here ("cert-u" lines) are the
measurement DESIGN.md tabulates next to that model."""
import functools

import numpy as np
import pytest

import cert_ref as cr
from query_ref import query_ref, same
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

GEMM = 1


def run_engine(X, k, config, monkeypatch, split=None):
    """One-block search of the stored points X through begin / step / end /
    rescan on the filter of `config` (split: override the config's filter);
    asserts the filter and the mode that ran.  Returns (result, unresolved)."""
    import torch
    import mpiknn.ring as ring
    dtype, _, no_split = cr.CONFIGS[config]
    if split is not None:
        no_split = not split
    if no_split:
        monkeypatch.setenv("KNN_NO_SPLIT", "1")
    else:
        monkeypatch.delenv("KNN_NO_SPLIT", raising=False)
    m, n = X.shape
    src = np.ascontiguousarray(X.astype(np.float32) if dtype == "f32" else X)
    e = ring.GpuEngine(torch, 0, n, m, m, k, dtype=dtype)
    e.pack(torch.from_numpy(src).to(torch.device("cuda", 0)), layout_col=False, elements=True)
    e.begin(0)
    assert e.ctx.split() == (0 if no_split else 1), "not the intended filter"
    e.step(e.qb, m, 0)
    u = e.end()
    assert e.ctx.info()[0] == GEMM, "expected GEMM mode"
    if u:
        e.step(e.qb, m, 0, rescan=True)
        e.rescan_end()
    monkeypatch.delenv("KNN_NO_SPLIT", raising=False)
    return e.result(), u


def check(X, k, config, monkeypatch, oracle, what):
    """exact against the oracle; on the split filter also the bytes of the
    MFMA filter's result.  Returns the unresolved count."""
    ref = oracle.knn(X, k)
    got, u = run_engine(X, k, config, monkeypatch)
    print("cert-u %s %s k=%d: %d of %d unresolved" % (what, config, k, u, len(X)))
    assert_same(got, ref, "%s %s k=%d" % (what, config, k))
    if not cr.CONFIGS[config][2]:
        base, _ = run_engine(X, k, config, monkeypatch, split=False)
        assert got.tobytes() == base.tobytes(), what
    return u


# ---- a. offset sweep through the transition --------------------------------

@pytest.mark.parametrize("config,n,k", cr.SWEEPS)
def test_offset_sweep(knn, oracle, monkeypatch, config, n, k):
    m = cr.M_SWEEP
    us = []
    for off in cr.offsets_for(cr.CONFIGS[config][1]):
        X = cr.sweep_points(config, n, off)
        us.append(check(X, k, config, monkeypatch, oracle, "sweep n=%d off=%g" % (n, off)))
    # the sweep lives on both sides of the transition
    assert us[0] <= m // 10, us
    assert us[-1] >= m // 2, us


@pytest.mark.parametrize("config,n", sorted(cr.MID))
def test_mid_transition_ragged_and_long_rows(knn, oracle, monkeypatch, config, n):
    off = cr.MID[(config, n)]
    check(cr.sweep_points(config, n, off), 30, config, monkeypatch, oracle, "mid n=%d off=%g" % (n, off))


# ---- b. exact ties under cancellation --------------------------------------

@pytest.mark.parametrize("config", sorted(cr.CONFIGS))
def test_exact_ties_lower_index_wins(knn, oracle, monkeypatch, config):
    """tie sets of 19 or 20 rows across rank 30 (S a few sixty-fourths,
    exact at every offset): the oracle's order -- the lower index -- through
    the certified path (first offset) and the exact rescan (second)"""
    dtype, filt, _ = cr.CONFIGS[config]
    Z = cr.tie_data()
    m = len(Z)
    us = [check(Z + off, 30, config, monkeypatch, oracle, "ties off=%g" % off) for off in cr.TIE_OFFSETS[filt]]
    assert us[0] <= m // 10 and us[1] >= m // 2, us


# ---- c. near-duplicate crowds at a large offset ----------------------------

@functools.lru_cache(maxsize=None)
def _crowd_queries(off):
    """corpus, queries: every 9th corpus row (zero distances, duplicates
    among them) and 70 fresh rows one grid step off a corpus row"""
    X = cr.crowd_data() + off
    rng = np.random.default_rng(8)
    fresh = X[5::40] + rng.integers(-1, 2, (70, X.shape[1])) * 2.0 ** -11
    return X, np.vstack([X[::9], fresh])


@pytest.mark.parametrize("config,k", [("f64-mfma", 30), ("f32-mfma", 30), ("f32-mfma", 100),
                                      ("f32-split", 30), ("f32-split", 100), ("f64-split", 30)])
def test_crowds_negative_filter_values(knn, oracle, monkeypatch, config, k):
    """Every GEMM-form d^2 inside a crowd is noise of either sign (S <
    E / 100): negative keys in the lane lists, the shared bound, the merge's
    zero window and its rk >= KP fallback.  As a search (zeros dropped), then
    as queries under both zero rules, one block and 384-row blocks with
    128-row query tiles (the bound crosses steps)."""
    dtype, filt, no_split = cr.CONFIGS[config]
    X, Q = _crowd_queries(cr.CROWD_OFFSET[filt])
    check(X, k, config, monkeypatch, oracle, "crowds")
    if no_split:
        monkeypatch.setenv("KNN_NO_SPLIT", "1")
    for keep_zero in (False, True):
        ref = query_ref(X, Q, k, keep_zero, dtype=dtype)
        got, _ = knn.query(X, Q, k, dtype=dtype, keep_zero=keep_zero)
        assert same(got, ref), "crowd queries %s keep_zero=%s" % (config, keep_zero)
        monkeypatch.setenv("KNN_QUERY_BLOCK", "384")
        monkeypatch.setenv("KNN_QUERY_TILE", "128")
        got, _ = knn.query(X, Q, k, dtype=dtype, keep_zero=keep_zero)
        assert same(got, ref), "crowd queries %s keep_zero=%s, blocks and tiles" % (config, keep_zero)
        monkeypatch.delenv("KNN_QUERY_BLOCK")
        monkeypatch.delenv("KNN_QUERY_TILE")


# ---- d. one outlier row owns MAXNORM and maxabs ----------------------------

@pytest.mark.parametrize("scale", [2.0 ** 10, 2.0 ** 20])
@pytest.mark.parametrize("config", sorted(cr.CONFIGS))
def test_outlier_row(knn, oracle, monkeypatch, config, scale):
    """the zero-offset data with one row scaled: E of every query follows that
    row's norm, and the split pre-scale pushes the other rows' lo halves to
    fp16 subnormals or zero.  Then the reverse: the outlier as a query."""
    dtype, _, no_split = cr.CONFIGS[config]
    Z = cr.sweep_points(config, 64, 0.0)
    X = cr.stored(cr.with_outlier(Z, scale), dtype)
    check(X, 30, config, monkeypatch, oracle, "outlier 2^%d" % int(np.log2(scale)))
    if no_split:
        monkeypatch.setenv("KNN_NO_SPLIT", "1")
    Q = np.vstack([X[17], Z[:40], X[17] * 0.5])
    for keep_zero in (False, True):
        got, _ = knn.query(Z, Q, 30, dtype=dtype, keep_zero=keep_zero)
        assert same(got, query_ref(Z, Q, 30, keep_zero, dtype=dtype)), (config, scale, keep_zero)


# ---- e. the mid-transition offset as a P = 3 block rotation ----------------

@pytest.mark.parametrize("config", sorted(cr.RING_MID))
def test_mid_transition_ring_blocks(knn, oracle, monkeypatch, config):
    """blocks rotated as in the ring (simulated on one GPU, P = 3), the meta
    max-reduced across the blocks; each rank against its rows of the
    one-search oracle result"""
    import torch
    import mpiknn.ring as ring
    dtype, _, no_split = cr.CONFIGS[config]
    if no_split:
        monkeypatch.setenv("KNN_NO_SPLIT", "1")
    X = cr.sweep_points(config, 64, cr.RING_MID[config])
    m, n = X.shape
    k = 30
    full = oracle.knn(X, k)
    Xd = torch.from_numpy(X).to(torch.device("cuda", 0))
    if dtype == "f32":
        Xd = Xd.float()
    P = 3
    R, blocks = ring.partition(m, P)
    engines = []
    for g in range(P):
        base, rows = blocks[g]
        e = ring.GpuEngine(torch, 0, n, R, rows, k, dtype=dtype)
        e.pack(Xd[base:base + rows], layout_col=False, elements=True)
        engines.append(e)
    meta = torch.stack([e.meta for e in engines]).max(dim=0).values
    total = 0
    for g, e in enumerate(engines):
        e.meta.copy_(meta)
        base, rows = blocks[g]
        e.begin(base)
        assert e.ctx.split() == (0 if no_split else 1)
        for s in range(P):
            b = (g - s) % P
            e.step(engines[b].qb, blocks[b][1], blocks[b][0])
        u = e.end()
        assert e.ctx.info()[0] == GEMM
        total += u
        if u:
            for s in range(P):
                b = (g - s) % P
                e.step(engines[b].qb, blocks[b][1], blocks[b][0], rescan=True)
            e.rescan_end()
        assert_same(e.result(), full[base:base + rows], "%s ring rank %d" % (config, g))
    print("cert-u ring off=%g %s k=%d: %d of %d unresolved" % (cr.RING_MID[config], config, k, total, m))
