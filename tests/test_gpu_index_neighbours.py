"""knn_index_neighbours / mpiknn.Index.neighbours on the GPU: the k nearest
OTHER live rows of resident rows, by id, equal bit for bit (idx and distance)
to the numpy restatement of tests/query_ref.py on the live rows -- under flags
0 query_ref with zero distances dropped, under keep-zero query_ref at k + 1
with the row itself deleted -- on every path, for the whole corpus (ids=None)
and for a shuffled list with repeats across the block boundaries; equal to
knn_search and the committed golden records on digits and digits_real; equal
to knn_index_query of the same rows under flags 0; through a remove / add /
update lifecycle with ids reported; on real-valued fp32 data at k = 100; into
device records; over several query tiles; for a small batch behind a large one
(stale tile rows); at the k limits; and after refused calls.

The corpus (tests/test_gpu_index_update.py's shapes: M = 700 mnist_like rows,
KNN_QUERY_BLOCK=256 for three blocks with the last one partial, K = 30) holds
rows that occur three times (make_queries' triples), so the two zero rules
differ, and one group of K + 4 identical rows, so the group's last rows are
absent from their own k + 1 records: the branch a "query, then strip the first
record" would get wrong."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import datasets
from query_ref import NB_DTYPE, query_ref, same

pytestmark = pytest.mark.gpu

M = 700
BLOCK = "256"
K = 30
GROUP = K + 4
ENVS = [{}, {"KNN_NO_I8": "1"}, {"KNN_NO_I8": "1", "KNN_NO_H16": "1"}, {"KNN_FORCE_RESCAN": "1"}]
ENV_IDS = ["i8", "h16", "f64int", "rescan"]
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def make_queries(X, nq, nfresh, fresh, rng_seed=5):
    """tests/test_gpu_index_update.py's make_queries restated: rows that appear three times in the corpus"""
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


def expected(X, live, ids, k, keep_zero, dtype="f64"):
    """X by id; live: the live ids, ascending; ids: the listed ids (None: all).
    Flags 0: query_ref with zeros dropped.  Keep-zero: query_ref at k + 1 with
    the row itself deleted (absent: the first k)."""
    live = np.asarray(live)
    Xl = X[live - 1]
    pos = np.arange(len(live)) if ids is None else np.searchsorted(live, np.asarray(ids))
    if not keep_zero:
        return mapped(query_ref(Xl, Xl[pos], k, False, dtype=dtype), live)
    wide = query_ref(Xl, Xl[pos], k + 1, True, dtype=dtype)
    rec = np.zeros((len(pos), k), dtype=NB_DTYPE)
    for i, p in enumerate(pos):
        rec[i] = wide[i][wide["idx"][i] != p + 1][:k]
    return mapped(rec, live)


@pytest.fixture(scope="module")
def int_data():
    X, y = datasets.mnist_like(M + 60)
    F, _ = datasets.mnist_like(160, seed=77)
    X0, _, trips = make_queries(X[:M], 200, 160, F)
    # one group of GROUP identical rows, outside the triples, in every block
    free = np.setdiff1d(np.arange(M), np.asarray(trips).reshape(-1))
    group = np.sort(np.random.default_rng(21).choice(free, GROUP, replace=False))
    assert group[0] < 256 and group[-1] >= 512
    X0[group] = X0[group[0]]
    X = np.vstack([X0, X[M:]])              # ids M+1 ..: rows for the add
    all_ids = np.arange(1, M + 1)

    @functools.lru_cache(None)
    def ref(keep_zero):
        return expected(X, all_ids, None, K, keep_zero)
    return X, y, trips, group + 1, ref


def the_list(group_ids, trips):
    """shuffled, with repeats, across the block boundaries, with group and triple rows"""
    rng = np.random.default_rng(8)
    lst = [256, 257, 258, 1, M, 257] + group_ids[-3:].tolist() + [group_ids[0]] + [t + 1 for t in trips[0]] + \
        rng.permutation(np.arange(1, M + 1))[:60].tolist()
    lst = np.asarray(lst + lst[3:9])
    return lst[np.random.default_rng(9).permutation(len(lst))]


# ------------------------------------------------ 1. every path, both rules

@pytest.mark.parametrize("keep_zero", [False, True])
@pytest.mark.parametrize("env", ENVS, ids=ENV_IDS)
def test_every_path(knn, int_data, monkeypatch, env, keep_zero):
    X, y, trips, group, ref = int_data
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    lst = the_list(group, trips)
    with knn.Index(X[:M]) as ix:
        assert ix.info().nblocks == 3
        graph, secs = ix.neighbours(None, K, keep_zero=keep_zero)
        bits = ix.info().last_bits
        some, _ = ix.neighbours(lst, K, keep_zero=keep_zero)
    want = ref(keep_zero)
    assert graph.shape == (M, K) and secs > 0.0
    assert same(graph, want)
    assert same(some, want[lst - 1])
    if "KNN_NO_I8" not in env:
        assert bits == 8
    else:
        assert bits == (64 if "KNN_NO_H16" in env else 16)
    # no row is its own neighbour
    assert not (graph["idx"] == np.arange(1, M + 1)[:, None]).any()
    t, a, b = (i + 1 for i in trips[0])
    late = group[K + 1:]                                      # rows with K + 1 duplicates of lower id
    if keep_zero:
        # the two other copies of a triple, lower id first
        assert graph["idx"][t - 1, :2].tolist() == sorted([a, b]) and (graph["distance"][t - 1, :2] == 0.0).all()
        assert graph["distance"][t - 1, 2] > 0.0
        # absent from their own k + 1 records: K duplicates at distance 0.0, lower ids first
        assert len(late) >= 2
        for g in late:
            assert graph["idx"][g - 1].tolist() == group[:K].tolist() and (graph["distance"][g - 1] == 0.0).all()
        # and a row inside the first K + 1: every other of them
        g = group[3]
        assert graph["idx"][g - 1].tolist() == [i for i in group[:K + 1] if i != g]
    else:
        assert (graph["distance"] > 0.0).all()
        assert not np.isin(graph["idx"][t - 1], [a, b]).any()
        assert not np.isin(graph["idx"][group - 1], group).any()


def test_rules_differ(int_data):
    X, y, trips, group, ref = int_data
    assert not same(ref(True), ref(False))


# ------------------------------------------------------ 2. against knn_search

def check_digits(nb, g):
    assert np.array_equal(nb["idx"], g["idx"].astype(np.int32))
    assert np.array_equal(nb["distance"], np.sqrt(g["d2"].astype(np.float64)))


def check_digits_real(nb, g):
    assert np.array_equal(nb["idx"], g["idx"].astype(np.int32))
    assert np.array_equal(nb["distance"].view(np.uint64), g["dist_bits"])


@pytest.mark.parametrize("block", [None, "700"], ids=["one-block", "three-blocks"])
@pytest.mark.parametrize("name", ["digits", "digits_real"])
def test_equals_search_and_golden(knn, monkeypatch, name, block):
    if block:
        monkeypatch.setenv("KNN_QUERY_BLOCK", block)
    X, y = getattr(datasets, name)()
    with knn.Index(X, labels=y) as ix:
        nb, _ = ix.neighbours(None, 30, keep_zero=False)
    one, _ = knn.search(X, 30, labels=y)
    assert np.array_equal(nb, one)                            # record for record, labels too
    with np.load(os.path.join(GOLD, "%s_k30.npz" % name), allow_pickle=False) as z:
        (check_digits if name == "digits" else check_digits_real)(nb, {k: z[k] for k in z.files})
    with open(os.path.join(GOLD, "reference_runs.json")) as f:
        runs = json.load(f)
    _, matches = knn.classify(nb, y, 10, knn.VOTE_SERIAL)
    assert matches == runs[name]["matches_serial_rule"]


# ------------------------------------------------- 3. against knn_index_query

@pytest.mark.parametrize("env", ENVS[:2], ids=ENV_IDS[:2])
def test_equals_index_query_under_flags_0(knn, int_data, monkeypatch, env):
    X, y, trips, group, ref = int_data
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    lst = the_list(group, trips)
    with knn.Index(X[:M], labels=y[:M]) as ix:
        got, _ = ix.neighbours(lst, K, keep_zero=False)
        q, _ = ix.query(X[lst - 1], K, keep_zero=False)
    assert np.array_equal(got, q) and same(got, q)
    assert (got["label"] == y[got["idx"] - 1]).all()


# -------------------------------------------------------------- 4. lifecycle

def test_lifecycle(knn, int_data, monkeypatch):
    X, y, trips, group, ref = int_data
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    Y = X.copy()                                              # by id, as the index holds it
    live = np.arange(1, M + 1)
    U, _ = datasets.mnist_like(16, seed=99)

    def check(ix, bits8=True, whole=False):
        """the graph against the expectation on a spread of rows (whole: on every row), and a list against the graph"""
        rows = np.arange(len(live)) if whole else np.unique(np.concatenate(
            [[0, 1, 254, 255, 256, 257, 511, 512, len(live) - 1], np.searchsorted(live, group[[0, 2, GROUP - 1]]),
             np.arange(7, len(live), 23)]))
        for kz in (True, False):
            graph, _ = ix.neighbours(None, K, keep_zero=kz)
            assert graph.shape == (len(live), K)
            assert same(graph[rows], expected(Y, live, live[rows], K, kz))
            lst = live[[len(live) - 1, 0, 255, 256, 257, 0]]
            some, _ = ix.neighbours(lst, K, keep_zero=kz)
            assert same(some, graph[np.searchsorted(live, lst)])
        assert (ix.info().last_bits == 8) == bits8

    with knn.Index(X[:M]) as ix:
        gone = [3, 200, 256, 257, 600, int(group[1])]
        assert ix.remove(gone) == len(gone)
        live = live[~np.isin(live, gone)]
        check(ix)                                             # the id map in use: ids reported, not positions
        graph, _ = ix.neighbours(None, K)
        assert not np.isin(graph["idx"], gone).any() and graph["idx"].max() > len(live)
        for dead in gone:                                     # a removed id: refused, nothing changed
            with pytest.raises(knn.KnnError) as e:
                ix.neighbours([1, dead], K)
            assert e.value.status == knn.ERR_INVALID
        again, _ = ix.neighbours(None, K)
        assert np.array_equal(again, graph)
        assert ix.add(X[M:M + 60]) == M + 1
        live = np.concatenate([live, np.arange(M + 1, M + 61)])
        check(ix)
        ids = [M + 60, 2, 258, 512, int(group[0])]
        ix.update(ids, U[:len(ids)])
        Y[np.asarray(ids) - 1] = U[:len(ids)]
        check(ix, whole=True)
        V = U[8:9].copy()
        V[0, 17] = 300.5                                      # neither 8-bit nor an integer: the byte blocks go
        ix.update([5], V)
        Y[4] = V[0]
        check(ix, bits8=False)


# ------------------------------------------------------------ 5. real-valued

@pytest.mark.parametrize("keep_zero", [False, True])
def test_real_f32_k100(knn, monkeypatch, keep_zero):
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    X, _ = datasets.mnist_real(600)
    F, _ = datasets.mnist_real(120, seed=77)
    X, _, trips = make_queries(X, 160, 120, F)
    live = np.arange(1, 601)
    lst = np.asarray([256, 257, 1, 600, 257] + [t + 1 for t in trips[0]] + list(range(300, 340)))
    with knn.Index(X.astype(np.float32), dtype="f32") as ix:
        got, _ = ix.neighbours(lst, 100, keep_zero=keep_zero)
        assert ix.info().last_bits != 8
        graph, _ = ix.neighbours(None, 100, keep_zero=keep_zero)
    assert same(got, expected(X, live, lst, 100, keep_zero, dtype="f32"))
    assert same(graph[lst - 1], got) and graph.shape == (600, 100)


# ------------------------------------------------------------ 6. device records

@pytest.mark.parametrize("keep_zero", [False, True])
def test_device_records(knn, int_data, monkeypatch, keep_zero):
    import torch
    X, y, trips, group, ref = int_data
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    dev = torch.device("cuda", 0)
    lst = the_list(group, trips)
    with knn.Index(X[:M], labels=y[:M]) as ix:
        ix.remove([9, 400])                                   # (the id map: written on the device)
        host, _ = ix.neighbours(None, K, keep_zero=keep_zero)
        buf = torch.zeros((M - 2) * K * 16, dtype=torch.uint8, device=dev)
        out, _ = ix.neighbours(None, K, keep_zero=keep_zero, out=buf)
        torch.cuda.synchronize()
        rec = out.cpu().numpy().view(knn.NB_DTYPE).reshape(M - 2, K)
        with pytest.raises(ValueError):
            ix.neighbours(lst, K, out=buf[:16])
    assert host["label"].any() and (host["label"] == y[host["idx"] - 1]).all()
    zeroed = host.copy()
    zeroed["label"] = 0
    assert np.array_equal(rec, zeroed)


# ------------------------------------------------------------ 7. tiles

@pytest.mark.parametrize("keep_zero", [False, True])
def test_several_tiles_last_one_partial(knn, int_data, monkeypatch, keep_zero):
    X, y, trips, group, ref = int_data
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    monkeypatch.setenv("KNN_QUERY_TILE", "128")               # 700 rows: five tiles of 128 and one of 60
    with knn.Index(X[:M]) as ix:
        graph, _ = ix.neighbours(None, K, keep_zero=keep_zero)
        lst = np.arange(M, 0, -1)[:300]                       # two tiles and one of 44
        some, _ = ix.neighbours(lst, K, keep_zero=keep_zero)
    assert same(graph, ref(keep_zero)) and same(some, ref(keep_zero)[lst - 1])


@pytest.mark.parametrize("env", ENVS[:3], ids=ENV_IDS[:3])
def test_small_batch_behind_a_large_one(knn, int_data, monkeypatch, env):
    """the tile buffers keep the large batch's rows past the small batch's own"""
    X, y, trips, group, ref = int_data
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    small = np.asarray([5, 300, 699, int(group[-1])])
    with knn.Index(X[:M]) as ix:
        first, _ = ix.neighbours(small, K)                    # a fresh tile buffer: never written past its 4 rows
        ix.neighbours(None, K)
        for kz in (True, False):
            got, _ = ix.neighbours(small, K, keep_zero=kz)
            assert same(got, ref(kz)[small - 1])
        one, _ = ix.neighbours([M], K)
        q, _ = ix.query(X[:3], K)                             # and a packed batch behind the gathered ones
    assert same(first, ref(True)[small - 1]) and same(one, ref(True)[[M - 1]])
    assert same(q, query_ref(X[:M], X[:3], K, True))


# ------------------------------------------------------ 8. limits, refusals

def test_k_limits(knn, int_data, monkeypatch):
    X, y, trips, group, ref = int_data
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    live = np.arange(1, M + 1)
    lst = np.concatenate([group[-4:], [1, 256, 257, M]])
    with knn.Index(X[:M]) as ix:
        got32, _ = ix.neighbours(lst, 32, keep_zero=False)    # fp64's limit under flags 0
        got31, _ = ix.neighbours(lst, 31, keep_zero=True)     # k + 1 = 32 under keep-zero
        with pytest.raises(knn.KnnError) as e:
            ix.neighbours(lst, 32, keep_zero=True)
        assert e.value.status == knn.ERR_UNSUPPORTED
        with pytest.raises(knn.KnnError) as e:
            ix.neighbours(lst, 33, keep_zero=False)
        assert e.value.status == knn.ERR_UNSUPPORTED
        after, _ = ix.neighbours(lst, 31, keep_zero=True)
    assert same(got32, expected(X, live, lst, 32, False))
    assert same(got31, expected(X, live, lst, 31, True)) and np.array_equal(after, got31)
    with knn.Index(X[:300].astype(np.float32), dtype="f32") as ix:
        with pytest.raises(knn.KnnError) as e:
            ix.neighbours([1], 128, keep_zero=True)
        assert e.value.status == knn.ERR_UNSUPPORTED
        got, _ = ix.neighbours([1, 300], 128, keep_zero=False)
    assert same(got, expected(X[:300], np.arange(1, 301), [1, 300], 128, False, dtype="f32"))


def test_refused_calls_leave_the_index_alone(knn, int_data, monkeypatch):
    X, y, trips, group, ref = int_data
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    out = np.zeros(M * K, dtype=knn.NB_DTYPE)

    def raw(ix, ids, count=None, k=K, flags=0, o=out):
        a = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32)
        n = (0 if a is None else len(a)) if count is None else count
        return knn.lib.knn_index_neighbours(ix._h, None if a is None else p(a), n, k, flags, None if o is None else p(o))

    for with_map in (False, True):
        with knn.Index(X[:M]) as ix:
            if with_map:
                assert ix.remove([10, 300]) == 2
            want, _ = ix.neighbours([1, 2, 500], K)
            qwant, _ = ix.query(X[:8], K)
            state = ix.info()[:3], ix.last_id, ix.m

            def unchanged():
                got, _ = ix.neighbours([1, 2, 500], K)
                q, _ = ix.query(X[:8], K)
                assert np.array_equal(got, want) and np.array_equal(q, qwant)
                assert (ix.info()[:3], ix.last_id, ix.m) == state

            assert raw(ix, [5], o=None) == knn.ERR_INVALID                # NULL out
            assert raw(ix, None, count=3) == knn.ERR_INVALID              # NULL ids with a count
            assert raw(ix, [5], count=0) == knn.ERR_INVALID               # ids with no count
            assert raw(ix, [5], k=0) == knn.ERR_INVALID
            assert raw(ix, [5], k=-3) == knn.ERR_INVALID
            assert raw(ix, [5], flags=2) == knn.ERR_INVALID               # KNN_INDEX_DEVICE_SRC: there is no source
            assert raw(ix, [5], flags=8) == knn.ERR_INVALID
            assert raw(ix, [0]) == knn.ERR_INVALID
            assert raw(ix, [5, M + 1]) == knn.ERR_INVALID                 # last_id + 1
            assert raw(ix, [-1]) == knn.ERR_INVALID
            assert raw(ix, [5, 5, 6]) == knn.OK                           # a repeat is no error
            if with_map:
                assert raw(ix, [5, 300]) == knn.ERR_INVALID               # no longer live
                assert raw(ix, [10]) == knn.ERR_INVALID
            unchanged()
            for bad in ([0], [M + 1], [2 ** 31], []) + (([300],) if with_map else ()):
                with pytest.raises(knn.KnnError) as e:
                    ix.neighbours(bad, K)
                assert e.value.status == knn.ERR_INVALID
            with pytest.raises(ValueError):
                ix.neighbours([1.5], K)
            unchanged()
    with pytest.raises(ValueError):
        ix.neighbours([1], K)                                             # closed
