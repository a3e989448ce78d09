"""knn_index_remove / mpiknn.Index.remove on the GPU: an index that forgot rows
answers exactly as the numpy restatement of tests/query_ref.py on the
surviving rows, and as knn_query on them -- idx equal once mapped through the
live ids, distance equal bit for bit -- on every path, for every removal
pattern, through a remove / add / remove lifecycle, with fewer than k rows
left, on real-valued corpora, with labels, into a device buffer, from every
source type, and after refused calls.  Rows keep their ids: X is indexed by id
throughout.  (Inputs and make_queries as tests/test_gpu_index_add.py.)"""
import ctypes
import functools

import numpy as np
import pytest

import datasets
from query_ref import query_ref, same, vote_ref

pytestmark = pytest.mark.gpu

M = 1524                                    # six blocks of KNN_QUERY_BLOCK=256, the last one partial
BLOCK = "256"
ENVS = [{}, {"KNN_NO_I8": "1"}, {"KNN_NO_I8": "1", "KNN_NO_H16": "1"}, {"KNN_FORCE_RESCAN": "1"}]
PATTERNS = {
    "first": [1],
    "last": [M],
    "boundary": [127, 128, 129],
    "block2": list(range(257, 513)),
    "random": sorted(np.random.default_rng(11).choice(np.arange(1, M + 1), M // 10, replace=False).tolist()),
}


def make_queries(X, nq, nfresh, fresh, rng_seed=5):
    """tests/test_gpu_index_add.py's make_queries restated; also returns the
    rows that appear three times: (corpus, queries, [(row, twin, twin)])"""
    X = X.copy()
    m = len(X)
    rng = np.random.default_rng(rng_seed)
    ncopy = (nq - nfresh) // 2
    rows = rng.permutation(m)
    single = rows[:ncopy]
    trip = rows[ncopy:2 * ncopy]
    a, b = rows[2 * ncopy:3 * ncopy], rows[3 * ncopy:4 * ncopy]
    X[a] = X[trip]
    X[b] = X[trip]
    Q = np.vstack([fresh[:nfresh], X[single], X[trip]])
    return X, Q, list(zip(trip.tolist(), a.tolist(), b.tolist()))


def mapped(rec, live):
    """records over the rows X[live - 1] with idx as the ids `live`"""
    out = rec.copy()
    ok = rec["idx"] > 0
    out["idx"][ok] = live[rec["idx"][ok] - 1]
    return out


def expected(X, live, Q, k, keep_zero, dtype="f64"):
    return mapped(query_ref(X[live - 1], Q, k, keep_zero, dtype=dtype), live)


def one_call(knn, X, live, Q, k, keep_zero, dtype="f64"):
    got, _ = knn.query(X[live - 1], Q, k, keep_zero=keep_zero, dtype=dtype)
    return mapped(got, live)


def without(live, ids):
    return live[~np.isin(live, np.asarray(ids))]


@pytest.fixture(scope="module")
def int_data():
    X, y = datasets.mnist_like(M + 300)
    F, _ = datasets.mnist_like(160, seed=77)
    X0, Q, trips = make_queries(X[:M], 200, 160, F)
    X = np.vstack([X0, X[M:]])              # ids M+1 ..: rows for the adds
    all_ids = np.arange(1, M + 1)

    @functools.lru_cache(None)
    def ref(pattern, keep_zero):
        return expected(X, without(all_ids, PATTERNS[pattern]), Q, 30, keep_zero)
    return X, y, Q, ref, trips


@pytest.fixture(scope="module")
def real_data():
    X, y = datasets.mnist_real(1000)
    F, _ = datasets.mnist_real(120, seed=77)
    X, Q, _ = make_queries(X, 160, 120, F)
    return X, Q


# ------------------------------------------- 1. removal patterns, every path

@pytest.mark.parametrize("keep_zero", [False, True])
@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("env", ENVS, ids=["i8", "h16", "f64int", "rescan"])
def test_remove_int(knn, int_data, monkeypatch, env, pattern, keep_zero):
    X, y, Q, ref, _ = int_data
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    ids = PATTERNS[pattern]
    live = without(np.arange(1, M + 1), ids)
    with knn.Index(X[:M]) as ix:
        ix.query(Q[:8], 30)                                   # a context and tile buffers from before the removal
        assert ix.info().nblocks == 6
        assert ix.remove(ids) == len(ids)
        info = ix.info()
        assert info.m == ix.m == len(live) and ix.last_id == M
        assert info.nblocks == (5 if pattern == "block2" else 6)
        got, secs = ix.query(Q, 30, keep_zero=keep_zero)
        bits = ix.info().last_bits
    assert same(got, ref(pattern, keep_zero))
    assert same(got, one_call(knn, X, live, Q, 30, keep_zero))
    assert secs > 0.0 and not np.isin(got["idx"], ids).any()
    if "KNN_NO_I8" not in env:
        assert bits == 8
    else:
        assert bits == (64 if "KNN_NO_H16" in env else 16)


# -------------------------------------------------------------- 2. triplicates

def test_remove_one_of_three(knn, int_data, monkeypatch):
    X, y, Q, ref, trips = int_data
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    all_ids = np.arange(1, M + 1)
    for which in range(3):
        t = trips[which]
        three = sorted(r + 1 for r in t)
        assert (X[t[1]] == X[t[0]]).all() and (X[t[2]] == X[t[0]]).all()
        gone = three[which]
        rest = [i for i in three if i != gone]
        q = X[[t[0]]]
        with knn.Index(X[:M]) as ix:
            before, _ = ix.query(q, 30, keep_zero=True)
            assert before["idx"][0, :3].tolist() == three and (before["distance"][0, :3] == 0.0).all()
            assert ix.remove([gone]) == 1
            got, _ = ix.query(q, 30, keep_zero=True)
            drop, _ = ix.query(q, 30, keep_zero=False)
        assert got["idx"][0, :2].tolist() == rest and (got["distance"][0, :2] == 0.0).all()
        assert got["distance"][0, 2] > 0.0
        live = without(all_ids, [gone])
        assert same(got, expected(X, live, q, 30, True)) and same(drop, expected(X, live, q, 30, False))
        assert (drop["distance"] > 0.0).all()


# ---------------------------------------------------------------- 3. lifecycle

def test_lifecycle(knn, int_data, monkeypatch):
    X, y, Q, ref, _ = int_data
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    Qs = Q[:96]
    m0 = 1000
    live = np.arange(1, m0 + 1)
    seen_gone = []

    def check(ix, live, last_id, rules=(True,)):
        info = ix.info()
        assert info.m == ix.m == len(live) and ix.last_id == last_id
        assert info.nblocks == (len(live) + 255) // 256
        for kz in rules:
            got, _ = ix.query(Qs, 30, keep_zero=kz)
            assert same(got, expected(X, live, Qs, 30, kz))
            assert np.isin(got["idx"], live).all() and not np.isin(got["idx"], seen_gone).any()
            for row in got["idx"]:
                assert len(set(row.tolist())) == 30           # no id twice
        assert ix.info().last_bits == 8
        return got

    with knn.Index(X[:m0]) as ix:
        check(ix, live, m0)
        gone = [3, 300, 256, 257, 999, 1000]
        assert ix.remove(gone) == 6
        seen_gone += gone
        live = without(live, gone)
        check(ix, live, m0)
        # added rows take last_id + 1 .., never an id that was given up
        first = ix.add(X[m0:m0 + 300])
        assert first == m0 + 1
        live = np.concatenate([live, np.arange(m0 + 1, m0 + 301)])
        got = check(ix, live, m0 + 300)
        # a query equal to an added row finds it first, at 0.0, under its id
        # (the last added row that make_queries gave no twin)
        row = next(r for r in range(m0 + 299, m0, -1) if (X[live - 1] == X[r]).all(axis=1).sum() == 1)
        me, _ = ix.query(X[[row]], 30, keep_zero=True)
        assert me["idx"][0, 0] == row + 1 and me["distance"][0, 0] == 0.0
        gone = [1001, 5, 1200, 3, 1300] + list(range(600, 900))
        assert ix.remove(gone) == len(gone) - 1               # 3 went before
        seen_gone += gone
        live = without(live, gone)
        check(ix, live, m0 + 300, rules=(True, False))
        first = ix.add(X[m0 + 300:m0 + 310].astype(np.uint8))
        assert first == m0 + 301
        live = np.concatenate([live, np.arange(m0 + 301, m0 + 311)])
        check(ix, live, m0 + 310)
        # only trailing rows: nothing moves, and an add fills the freed rows
        assert ix.remove(np.arange(m0 + 306, m0 + 311)) == 5
        seen_gone += list(range(m0 + 306, m0 + 311))
        live = without(live, np.arange(m0 + 306, m0 + 311))
        check(ix, live, m0 + 310)


# ------------------------------------------------------- 4. fewer than k left

@pytest.mark.parametrize("keep_zero", [False, True])
def test_fewer_than_k_left(knn, int_data, monkeypatch, keep_zero):
    X, y, Q, ref, _ = int_data
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    m0 = 600
    live = np.array([2, 3, 128, 129, 255, 256, 257, 258, 300, 301, 400, 511, 512, 513, 514, 590, 597, 598, 599, 600])
    with knn.Index(X[:m0]) as ix:
        assert ix.remove(without(np.arange(1, m0 + 1), live)) == m0 - 20
        assert ix.info().m == 20 and ix.info().nblocks == 1
        got, _ = ix.query(Q[:64], 30, keep_zero=keep_zero)
    assert same(got, expected(X, live, Q[:64], 30, keep_zero))
    assert np.isinf(got["distance"][:, 20:]).all() and not got["idx"][:, 20:].any() and not got["label"].any()
    assert (got["idx"][:, :19] > 0).all()


# ------------------------------------------------------- 5. real-valued data

def real_gone():
    rng = np.random.default_rng(3)
    return sorted(set(rng.choice(np.arange(1, 1001), 100, replace=False).tolist()) | {1, 256, 257, 1000})


@pytest.mark.parametrize("keep_zero", [False, True])
def test_remove_real_f64(knn, real_data, monkeypatch, keep_zero):
    X, Q = real_data
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    gone = real_gone()
    live = without(np.arange(1, 1001), gone)
    with knn.Index(X) as ix:
        assert ix.remove(gone) == len(gone)
        got, _ = ix.query(Q, 30, keep_zero=keep_zero)
        assert ix.info().last_bits != 8
    assert same(got, expected(X, live, Q, 30, keep_zero)) and same(got, one_call(knn, X, live, Q, 30, keep_zero))


@pytest.mark.parametrize("keep_zero", [False, True])
@pytest.mark.parametrize("no_split", [False, True])
def test_remove_f32_k100(knn, real_data, monkeypatch, no_split, keep_zero):
    X, Q = real_data
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    if no_split:
        monkeypatch.setenv("KNN_NO_SPLIT", "1")
    gone = real_gone()
    live = without(np.arange(1, 1001), gone)
    with knn.Index(X, dtype="f32") as ix:
        assert ix.remove(gone) == len(gone)
        got, _ = ix.query(Q, 100, keep_zero=keep_zero)
    assert same(got, expected(X, live, Q, 100, keep_zero, dtype="f32"))
    assert same(got, one_call(knn, X, live, Q, 100, keep_zero, dtype="f32"))


# ------------------------------------------------------------ 6. labels, vote

@pytest.mark.parametrize("rule", [0, 1, 2])
def test_remove_labels_and_vote(knn, int_data, monkeypatch, rule):
    X, y, Q, ref, _ = int_data
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    with knn.Index(X[:M], labels=y[:M]) as ix:
        assert ix.remove(PATTERNS["random"]) == len(PATTERNS["random"])
        ix.add(X[M:M + 40], labels=y[M:M + 40])
        got, _ = ix.query(Q, 30)
    live = np.concatenate([without(np.arange(1, M + 1), PATTERNS["random"]), np.arange(M + 1, M + 41)])
    assert same(got, expected(X, live, Q, 30, True))
    ok = got["idx"] > 0
    assert ok.all() and (got["label"] == y[got["idx"] - 1]).all()    # labels stay indexed by id
    yq = ((np.arange(len(Q)) % 10) + 1).astype(np.float64)
    pred, matches = knn.classify_query(got, y[:M + 40], yq, 10, rule)
    pred_r, matches_r = vote_ref(got, y[:M + 40], yq, 10, rule)
    assert np.array_equal(pred, pred_r) and matches == matches_r


# ------------------------------------------------- 7. device output, sources

def test_remove_device_out(knn, int_data, monkeypatch):
    import torch
    X, y, Q, ref, _ = int_data
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    dev = torch.device("cuda", 0)
    with knn.Index(X[:M]) as ix:
        ix.remove(PATTERNS["random"])
        host, _ = ix.query(Q, 30)
        buf = torch.zeros(len(Q) * 30 * 16, dtype=torch.uint8, device=dev)
        out, _ = ix.query(Q, 30, out=buf)
        torch.cuda.synchronize()
        rec = out.cpu().numpy().view(knn.NB_DTYPE).reshape(len(Q), 30)
    assert same(rec, host) and same(rec, ref("random", True)) and not rec["label"].any()


def test_remove_sources(knn, int_data, monkeypatch):
    import torch
    X, y, Q, ref, _ = int_data
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    dev = torch.device("cuda", 0)
    want = ref("random", True)
    sizes = set()
    for name, kw, cast in (("f64", {}, lambda a: a), ("torch-u8", {}, lambda a: torch.from_numpy(a.astype(np.uint8)).to(dev)),
                           ("col", {"layout": "col"}, lambda a: a)):
        with knn.Index(cast(X[:M]), **kw) as ix:
            ix.query(Q, 30)
            off = ix.info().device_bytes                  # never removed: no id map on the device
            assert ix.remove(PATTERNS["random"]) == len(PATTERNS["random"])
            got, _ = ix.query(cast(Q), 30)
            assert ix.info().last_bits == 8, name
            sizes.add((off, ix.info().device_bytes))
        assert same(got, want), name
    assert len(sizes) == 1                                # equal across source types, before and after
    off, on = sizes.pop()
    assert on == off + 4 * (M - len(PATTERNS["random"]))  # six blocks still; the id map is what came


def test_off_state_device_bytes(knn, int_data, monkeypatch):
    """an index that never removed holds what it always held; the first
    removal adds the id map and nothing else (the last row: nothing moves)"""
    X, y, Q, ref, _ = int_data
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    with knn.Index(X[:M]) as ix:
        ix.query(Q[:64], 30)
        off = ix.info().device_bytes
        ctx_and_tiles = off - 6 * (knn.block_bytes(256, 784) + knn.s8_block_bytes(256, 784)) - 64 \
            - 64 * 30 * knn.NB_DTYPE.itemsize
        assert ctx_and_tiles > 0
        assert ix.remove([M]) == 1
        assert ix.info().device_bytes == off + 4 * (M - 1)
    with knn.Index(X[:M].astype(np.uint8)) as ix:
        ix.query(Q[:64].astype(np.uint8), 30)
        assert ix.info().device_bytes == off


# ------------------------------------------------ 8. refused and skipped ids

def test_refused_calls_leave_the_index_alone(knn, int_data, monkeypatch):
    X, y, Q, ref, _ = int_data
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    Qs = Q[:64]
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def raw(ix, ids, count=None, flags=0):
        a = np.ascontiguousarray(ids, dtype=np.int32)
        n = ctypes.c_size_t(99)
        rc = knn.lib.knn_index_remove(ix._h, p(a), len(a) if count is None else count, flags, ctypes.byref(n))
        return rc, n.value

    with knn.Index(X[:M], labels=y[:M]) as ix:
        assert ix.remove([10, 700]) == 2                      # (a map exists from here on)
        want, _ = ix.query(Qs, 30)
        state = ix.info()[:4], ix.last_id

        def unchanged():
            got, _ = ix.query(Qs, 30)
            assert np.array_equal(got, want) and (ix.info()[:4], ix.last_id) == state and ix.m == M - 2

        assert raw(ix, [0]) == (knn.ERR_INVALID, 99)
        assert raw(ix, [5, M + 1]) == (knn.ERR_INVALID, 99)
        assert raw(ix, [-1]) == (knn.ERR_INVALID, 99)
        assert raw(ix, [5], flags=1) == (knn.ERR_INVALID, 99)
        assert raw(ix, [5], count=0) == (knn.ERR_INVALID, 99)
        assert raw(ix, np.arange(1, M + 1)) == (knn.ERR_INVALID, 99)      # every live row (and two stale ids)
        assert knn.lib.knn_index_remove(ix._h, None, 1, 0, None) == knn.ERR_INVALID
        unchanged()
        for bad in ([0], [M + 1], [], list(range(1, M + 1)), [2 ** 31]):
            with pytest.raises(knn.KnnError) as e:
                ix.remove(bad)
            assert e.value.status == knn.ERR_INVALID
        with pytest.raises(ValueError):
            ix.remove([1.5])
        unchanged()
        # stale and repeated ids are skipped, and `removed` says so
        assert raw(ix, [10, 700, 10]) == (knn.OK, 0)
        unchanged()
        assert raw(ix, [10, 11, 11, 700, 12, 11]) == (knn.OK, 2)
        assert ix.info().m == M - 4
        got, _ = ix.query(Qs, 30)
        live = without(np.arange(1, M + 1), [10, 11, 12, 700])
        assert same(got, expected(X, live, Qs, 30, True))
        assert (got["label"] == y[got["idx"] - 1]).all()
    with knn.Index(X[:300]) as ix:                            # no map yet: the same refusals
        want, _ = ix.query(Qs, 30)
        assert raw(ix, [0]) == (knn.ERR_INVALID, 99) and raw(ix, [301]) == (knn.ERR_INVALID, 99)
        assert raw(ix, np.arange(1, 301)) == (knn.ERR_INVALID, 99)
        got, _ = ix.query(Qs, 30)
        assert np.array_equal(got, want) and ix.info().m == 300 and ix.last_id == 300
    with pytest.raises(ValueError):
        ix.remove([1])                                        # closed
    with pytest.raises(ValueError):
        ix.last_id
