"""knn_index_update / mpiknn.Index.update on the GPU: an index whose rows were
given new coordinates in place answers exactly as the numpy restatement of
tests/query_ref.py on the updated corpus, and as one knn_query on it -- idx and
distance equal bit for bit -- on every path, for every update pattern, with
the byte path kept (8-bit updates) and dropped (a 300.5), with ties on both
sides, through a remove / update / add / update lifecycle, on real-valued
fp32 data, with labels, from device sources into device records, and after
refused calls.  Rows keep their ids and positions: X is indexed by id
throughout.  (Inputs and make_queries as tests/test_gpu_index_remove.py.)"""
import ctypes
import functools

import numpy as np
import pytest

import datasets
from query_ref import query_ref, same

pytestmark = pytest.mark.gpu

M = 700                                     # three blocks of KNN_QUERY_BLOCK=256, the last one partial
BLOCK = "256"
K = 30
ENVS = [{}, {"KNN_NO_I8": "1"}, {"KNN_NO_I8": "1", "KNN_NO_H16": "1"}, {"KNN_FORCE_RESCAN": "1"}]
PATTERNS = {
    "first": [1],
    "last": [M],
    "boundary": [257, 256, 258],
    "block2": list(range(257, 513)),
    "random": np.random.default_rng(11).permutation(np.arange(1, M + 1))[:M // 10].tolist(),
}


def make_queries(X, nq, nfresh, fresh, rng_seed=5):
    """tests/test_gpu_index_remove.py's make_queries restated: fresh rows,
    copies of corpus rows, and rows that appear three times in the corpus"""
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


def updated(X, ids, U):
    Y = X.copy()
    Y[np.asarray(ids) - 1] = U[:len(ids)]
    return Y


@pytest.fixture(scope="module")
def int_data():
    X, y = datasets.mnist_like(M + 60)
    F, _ = datasets.mnist_like(160, seed=77)
    X0, Q, trips = make_queries(X[:M], 200, 160, F)
    X = np.vstack([X0, X[M:]])              # ids M+1 ..: rows for the adds
    # the new coordinates: fresh rows, the first ones equal to queries (so the update shows at distance 0)
    U, _ = datasets.mnist_like(256, seed=99)
    U[:3] = Q[[0, 1, 170]]
    all_ids = np.arange(1, M + 1)

    @functools.lru_cache(None)
    def ref(pattern, keep_zero):
        return expected(updated(X[:M], PATTERNS[pattern], U), all_ids, Q, K, keep_zero)
    return X, y, Q, U, ref


# -------------------------------------------- 1. update patterns, every path

@pytest.mark.parametrize("keep_zero", [False, True])
@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("env", ENVS, ids=["i8", "h16", "f64int", "rescan"])
def test_update_int(knn, int_data, monkeypatch, env, pattern, keep_zero):
    X, y, Q, U, ref = int_data
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    ids = PATTERNS[pattern]
    Y = updated(X[:M], ids, U)
    with knn.Index(X[:M]) as ix:
        before, _ = ix.query(Q, K, keep_zero=keep_zero)       # a context and tile buffers from before the update
        state = ix.info()[:4], ix.last_id, ix.m
        assert state[0][2] == 3
        assert ix.update(ids, U[:len(ids)]) is None
        assert (ix.info()[:4], ix.last_id, ix.m) == state     # m, blocks, capacity, device bytes, ids: as they were
        got, secs = ix.query(Q, K, keep_zero=keep_zero)
        bits = ix.info().last_bits
    assert same(got, ref(pattern, keep_zero))
    one, _ = knn.query(Y, Q, K, keep_zero=keep_zero)
    assert same(got, one)
    assert secs > 0.0
    if keep_zero:                                             # U[0] == Q[0]: the update shows
        assert got["idx"][0, 0] == ids[0] and got["distance"][0, 0] == 0.0 and before["distance"][0, 0] > 0.0
    if "KNN_NO_I8" not in env:
        assert bits == 8
    else:
        assert bits == (64 if "KNN_NO_H16" in env else 16)


# ------------------------------------------------- 2. the byte path, kept / dropped

def test_byte_path_kept(knn, int_data, monkeypatch):
    X, y, Q, U, ref = int_data
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    with knn.Index(X[:M].astype(np.uint8)) as ix:
        ix.query(Q[:8].astype(np.uint8), K)
        size = ix.info().device_bytes
        ix.update(PATTERNS["random"], U[:M // 10].astype(np.uint8))
        got, _ = ix.query(Q.astype(np.uint8), K)
        assert ix.info().last_bits == 8
        ix.update(PATTERNS["block2"], U.astype(np.float32))   # on top: other rows, another source type
        got2, _ = ix.query(Q, K, keep_zero=False)
        assert ix.info().last_bits == 8 and ix.info().device_bytes >= size
    assert same(got, ref("random", True))
    Y = updated(updated(X[:M], PATTERNS["random"], U), PATTERNS["block2"], U)
    assert same(got2, expected(Y, np.arange(1, M + 1), Q, K, False))


def test_byte_path_dropped(knn, int_data, monkeypatch):
    X, y, Q, U, ref = int_data
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    all_ids = np.arange(1, M + 1)
    ids = [300, 5, 699]
    V = U[:3].copy()
    V[1, 17] = 300.5                                          # neither 8-bit nor an integer
    Y = updated(X[:M], ids, V)
    with knn.Index(X[:M]) as ix:
        ix.query(Q, K)
        assert ix.info().last_bits == 8
        size = ix.info().device_bytes
        ix.update(ids, V)
        assert ix.info().device_bytes == size - 3 * knn.s8_block_bytes(256, 784)   # (the tiles' byte forms stay)
        got, _ = ix.query(Q, K)
        info = ix.info()
        assert info.last_bits != 8                            # (the element path's context holds other buffers)
        drop, _ = ix.query(Q, K, keep_zero=False)
        # integers again, the 300.5 overwritten: the byte blocks do not come back
        ix.update([5, 1], U[10:12])
        again, _ = ix.query(Q, K)
        assert ix.info().last_bits != 8 and ix.info().device_bytes == info.device_bytes
    assert same(got, expected(Y, all_ids, Q, K, True)) and same(drop, expected(Y, all_ids, Q, K, False))
    assert same(got, knn.query(Y, Q, K)[0])
    assert same(again, expected(updated(Y, [5, 1], U[10:12]), all_ids, Q, K, True))


# ------------------------------------------------------------------- 3. ties

def test_ties_come_lower_id_first(knn, int_data, monkeypatch):
    X, y, Q, U, ref = int_data
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    _, inv, cnt = np.unique(X[:M], axis=0, return_inverse=True, return_counts=True)
    once = np.flatnonzero(cnt[inv.reshape(-1)] == 1).tolist()
    lo, hi = once[0] + 1, once[-1] + 1                        # ids of two rows nothing else equals
    mid = [i + 1 for i in once if 256 <= i < 512][:2]
    assert lo < mid[0] < mid[1] < hi
    all_ids = np.arange(1, M + 1)
    for target, twin in ((hi, mid[0]), (lo, mid[1])):         # the updated row's id is the higher / the lower one
        Y = updated(X[:M], [target], X[[twin - 1]])
        q = X[[twin - 1]]
        with knn.Index(X[:M]) as ix:
            b4, _ = ix.query(q, K, keep_zero=True)
            assert b4["idx"][0, 0] == twin and b4["distance"][0, 1] > 0.0
            ix.update([target], X[[twin - 1]])
            got, _ = ix.query(q, K, keep_zero=True)
            drop, _ = ix.query(q, K, keep_zero=False)
        assert got["idx"][0, :2].tolist() == sorted([target, twin]) and (got["distance"][0, :2] == 0.0).all()
        assert got["distance"][0, 2] > 0.0 and (drop["distance"] > 0.0).all()
        assert same(got, expected(Y, all_ids, q, K, True)) and same(drop, expected(Y, all_ids, q, K, False))


# -------------------------------------------------------------- 4. lifecycle

def test_lifecycle(knn, int_data, monkeypatch):
    X, y, Q, U, ref = int_data
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    Y = X.copy()                                              # by id, as the index holds it
    live = np.arange(1, M + 1)

    def check(ix, last_id):
        assert ix.info().m == ix.m == len(live) and ix.last_id == last_id
        for kz in (True, False):
            got, _ = ix.query(Q, K, keep_zero=kz)
            assert same(got, expected(Y, live, Q, K, kz))
        assert ix.info().last_bits == 8

    with knn.Index(X[:M]) as ix:
        gone = [3, 200, 256, 257, 600]
        assert ix.remove(gone) == 5
        live = live[~np.isin(live, gone)]
        # by surviving ids, through the id map: their positions moved by up to 5, across the block boundaries
        ids = [700, 1, 258, 259, 260, 261, 262, 255, 512, 513, 514, 515, 516, 517, 4]
        ix.update(ids, U[:len(ids)])
        Y[np.asarray(ids) - 1] = U[:len(ids)]
        check(ix, M)
        first = ix.add(X[M:M + 60])
        assert first == M + 1
        live = np.concatenate([live, np.arange(M + 1, M + 61)])
        check(ix, M + 60)
        ids = [M + 60, 2, M + 1, M + 30]                      # added rows, and an old one
        ix.update(ids, U[100:104].astype(np.uint8))
        Y[np.asarray(ids) - 1] = U[100:104]
        check(ix, M + 60)
        for dead in gone:
            with pytest.raises(knn.KnnError):
                ix.update([dead], U[:1])
        check(ix, M + 60)


# ------------------------------------------------------------ 5. real-valued

@pytest.mark.parametrize("keep_zero", [False, True])
def test_update_real_f32(knn, monkeypatch, keep_zero):
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    X, _ = datasets.mnist_real(600)
    F, _ = datasets.mnist_real(120, seed=77)
    X, Q, _ = make_queries(X, 160, 120, F)
    U, _ = datasets.mnist_real(80, seed=99)
    U[0] = Q[0]
    ids = np.random.default_rng(3).permutation(np.arange(1, 601))[:77]
    ids[:3] = [1, 600, 256]
    ids = np.unique(ids)[::-1].copy()
    Y = updated(X, ids, U)
    with knn.Index(X.astype(np.float32), dtype="f32") as ix:
        ix.query(Q[:8].astype(np.float32), K)
        ix.update(ids, U[:len(ids)].astype(np.float32))
        got, _ = ix.query(Q.astype(np.float32), K, keep_zero=keep_zero)
        assert ix.info().last_bits != 8
    assert same(got, expected(Y, np.arange(1, 601), Q, K, keep_zero, dtype="f32"))
    assert same(got, knn.query(Y, Q, K, keep_zero=keep_zero, dtype="f32")[0])


# ----------------------------------------------------------------- 6. labels

def test_labels_replaced_and_left(knn, int_data, monkeypatch):
    X, y, Q, U, ref = int_data
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    ids = PATTERNS["random"]
    ynew = y[:M].copy()
    with knn.Index(X[:M], labels=y[:M]) as ix:
        ix.update(ids[:40], U[:40], labels=np.full(40, 7.0))
        ynew[np.asarray(ids[:40]) - 1] = 7.0
        ix.update(ids[40:], U[40:len(ids)])                   # labels left as they are
        got, _ = ix.query(Q, K)
        with pytest.raises(ValueError):
            ix.update(ids[:2], U[:2], labels=[1.0])
    assert same(got, ref("random", True))
    assert np.isin(got["idx"], ids[:40]).any()
    assert (got["label"] == ynew[got["idx"] - 1]).all()


# ----------------------------------------------------------- 7. device paths

def test_device_source_and_records(knn, int_data, monkeypatch):
    import torch
    X, y, Q, U, ref = int_data
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    dev = torch.device("cuda", 0)
    ids = PATTERNS["random"]
    for cast, kw in ((lambda a: torch.from_numpy(a.astype(np.uint8)).to(dev), {}),
                     (lambda a: torch.from_numpy(a).to(dev), {}),
                     (lambda a: torch.from_numpy(a.astype(np.float32)).to(dev), {"layout": "col"})):
        with knn.Index(cast(X[:M]), **kw) as ix:
            ix.query(cast(Q[:8]), K)
            ix.update(ids, cast(U[:len(ids)]))
            buf = torch.zeros(len(Q) * K * 16, dtype=torch.uint8, device=dev)
            out, _ = ix.query(cast(Q), K, out=buf)
            torch.cuda.synchronize()
            rec = out.cpu().numpy().view(knn.NB_DTYPE).reshape(len(Q), K)
            assert ix.info().last_bits == 8
        assert same(rec, ref("random", True)) and not rec["label"].any()


# ----------------------------------------------------------- 8. refused calls

def test_refused_calls_leave_the_index_alone(knn, int_data, monkeypatch):
    X, y, Q, U, ref = int_data
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    Qs = Q[:64]
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rows = np.ascontiguousarray(U[:4])

    def raw(ix, ids, count=None, layout=1, src=0, labels=None, flags=0, X=rows):
        a = np.ascontiguousarray(ids, dtype=np.int32)
        return knn.lib.knn_index_update(ix._h, p(a), len(a) if count is None else count, None if X is None else p(X),
                                        layout, src, None if labels is None else p(labels), flags)

    for with_map in (False, True):
        with knn.Index(X[:M]) as ix:
            if with_map:
                assert ix.remove([10, 300]) == 2
            want, _ = ix.query(Qs, K)
            state = ix.info()[:4], ix.last_id, ix.m

            def unchanged():
                got, _ = ix.query(Qs, K)
                assert np.array_equal(got, want) and (ix.info()[:4], ix.last_id, ix.m) == state

            assert raw(ix, [0]) == knn.ERR_INVALID
            assert raw(ix, [5, M + 1]) == knn.ERR_INVALID                 # last_id + 1
            assert raw(ix, [-1]) == knn.ERR_INVALID
            assert raw(ix, [5, 6, 5]) == knn.ERR_INVALID                  # a repeat
            assert raw(ix, [5], labels=np.ones(1)) == knn.ERR_INVALID     # labels on a label-less index
            assert raw(ix, [5], count=0) == knn.ERR_INVALID
            assert raw(ix, [5], layout=2) == knn.ERR_INVALID
            assert raw(ix, [5], flags=1) == knn.ERR_INVALID
            assert raw(ix, [5], flags=4) == knn.ERR_INVALID               # KNN_INDEX_DEVICE_OUT: not here
            assert raw(ix, [5], X=None) == knn.ERR_INVALID
            assert raw(ix, [5], src=3) == knn.ERR_UNSUPPORTED
            assert knn.lib.knn_index_update(ix._h, None, 1, p(rows), 1, 0, None, 0) == knn.ERR_INVALID
            if with_map:
                assert raw(ix, [5, 300]) == knn.ERR_INVALID               # no longer live
                assert raw(ix, [10]) == knn.ERR_INVALID
            unchanged()
            for bad in ([0], [M + 1], [7, 7], [2 ** 31]) + (([300],) if with_map else ()):
                with pytest.raises(knn.KnnError) as e:
                    ix.update(bad, U[:len(bad)])
                assert e.value.status == knn.ERR_INVALID
            with pytest.raises(knn.KnnError) as e:
                ix.update([5], U[:1], labels=[1.0])
            assert e.value.status == knn.ERR_INVALID
            with pytest.raises(ValueError):
                ix.update([1.5], U[:1])
            with pytest.raises(ValueError):
                ix.update([1, 2], U[:3])                                  # one row a listed id
            with pytest.raises(ValueError):
                ix.update([1], U[:1, :100])
            unchanged()
    with pytest.raises(ValueError):
        ix.update([1], U[:1])                                             # closed
