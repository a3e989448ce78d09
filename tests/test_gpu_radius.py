"""knn_index_radius* / mpiknn.Index.radius* on the GPU: counts, offsets, ids
and distance bits equal to the numpy restatement (tests/radius_ref.py) on every
path -- the int8 MFMA kernel on byte blocks (long rows n = 784, short rows n =
128, n = 100 with padding inside the last K-step), the exact scan on the same
integer data (KNN_NO_I8=1), on real-valued fp64 data and on an fp32 index --
under both zero rules, at a radius that is some row's distance exactly and at
the double below it; the rows forms (the corpus's epsilon-graph, a shuffled
list with repeats); after a remove / add / update lifecycle; over several
query tiles and for a small batch behind a large one; with every row a hit
(segments past the sort's LDS threshold) and none; the two-call contract
(short, long and shifted offsets, a guard band); device outputs and sources;
and a query behind a radius call.

Shapes: M = 700 rows, KNN_QUERY_BLOCK=256 (three blocks, the last partial), as
the other index tests; tests/test_radius_cpu.py checks on the CPU that the
radii give empty and long segments, a hit at the radius and a zero pair."""
import ctypes

import numpy as np
import pytest

import radius_ref as R
from radius_ref import M, case, same

pytestmark = pytest.mark.gpu

BLOCK = "256"


def both(ix, Q, r, keep_zero):
    """radius_count and radius, and that they agree"""
    counts = ix.radius_count(Q, r, keep_zero=keep_zero)
    indptr, rec = ix.radius(Q, r, keep_zero=keep_zero)
    assert np.array_equal(np.diff(indptr), counts)
    return counts, indptr, rec


def both_rows(ix, ids, r, keep_zero):
    counts = ix.radius_rows_count(ids, r, keep_zero=keep_zero)
    indptr, rec = ix.radius_rows(ids, r, keep_zero=keep_zero)
    assert np.array_equal(np.diff(indptr), counts)
    return counts, indptr, rec


# ------------------------------------------------ 1. count and fill, every path

@pytest.mark.parametrize("keep_zero", [False, True])
@pytest.mark.parametrize("name,env", [("mnist", {}), ("mnist", {"KNN_NO_I8": "1"}), ("sift", {}), ("n100", {}),
                                      ("real", {}), ("f32", {})],
                         ids=["mnist-i8", "mnist-scan", "sift-i8", "n100-i8", "real", "f32"])
def test_paths(knn, monkeypatch, name, env, keep_zero):
    c = case(name)
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    src = c.X.astype(np.uint8) if name in ("mnist", "sift", "n100") else c.X
    q = c.Q.astype(np.uint8) if name in ("mnist", "sift", "n100") else c.Q
    with knn.Index(src, dtype=c.dtype) as ix:
        assert ix.info().nblocks == 3
        for r in (c.r_at, c.r_below):
            got = both(ix, q, r, keep_zero)
            assert same(got, c.ref(r, keep_zero)), (name, r)
            assert (got[2]["distance"] <= r).all()


def test_byte_and_element_paths_agree(knn, monkeypatch):
    c = case("mnist")
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    with knn.Index(c.X) as ix:
        a = both(ix, c.Q, c.r_at, True)
    monkeypatch.setenv("KNN_NO_I8", "1")
    with knn.Index(c.X) as ix:
        b = both(ix, c.Q, c.r_at, True)
    assert same(a, b) and a[0].max() >= 100 and a[0].min() == 0


# ------------------------------------------------------------ 2. rows forms

@pytest.mark.parametrize("keep_zero", [False, True])
@pytest.mark.parametrize("name,env", [("mnist", {}), ("mnist", {"KNN_NO_I8": "1"}), ("sift", {})],
                         ids=["mnist-i8", "mnist-scan", "sift-i8"])
def test_rows(knn, monkeypatch, name, env, keep_zero):
    c = case(name)
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(8)
    lst = [256, 257, 258, 1, M, 257] + (c.group[-3:] + 1).tolist() + [int(c.group[0]) + 1] + \
        (c.trips[0] + 1).tolist() + rng.permutation(np.arange(1, M + 1))[:60].tolist()
    lst = np.asarray(lst + lst[3:9])
    lst = lst[np.random.default_rng(9).permutation(len(lst))]
    with knn.Index(c.X) as ix:
        graph = both_rows(ix, None, c.r_at, keep_zero)
        some = both_rows(ix, lst, c.r_at, keep_zero)
    assert same(graph, c.rows_ref(c.r_at, keep_zero))
    assert same(some, c.rows_ref(c.r_at, keep_zero, pos=lst - 1))
    # the epsilon-graph is symmetric, and no row is its own neighbour
    counts, indptr, rec = graph
    src = np.repeat(np.arange(1, M + 1), counts)
    pairs = set(zip(src.tolist(), rec["idx"].tolist()))
    assert len(pairs) == len(rec) and all((b, a) in pairs for a, b in pairs)
    assert not (src == rec["idx"]).any()
    g = c.group + 1
    seg = rec[indptr[g[3] - 1]:indptr[g[3]]]
    if keep_zero:   # the group's other rows at 0.0, lower id first
        assert seg["idx"][:len(g) - 1].tolist() == [i for i in g if i != g[3]]
        assert (seg["distance"][:len(g) - 1] == 0.0).all()
    else:
        assert (rec["distance"] > 0.0).all() and not np.isin(seg["idx"], g).any()


# ------------------------------------------------------------- 3. mutations

def test_after_remove_add_update(knn, monkeypatch):
    c = case("mnist")
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    X = c.X.copy()
    gone = np.array([3, 256, 257, 300, 640])
    with knn.Index(X[:650], labels=c.labels[:650]) as ix:
        assert ix.remove(gone) == len(gone)
        ix.add(X[650:], labels=c.labels[650:])
        X[9] = X[499]
        ix.update([10], X[9:10])
        live = np.setdiff1d(np.arange(1, M + 1), gone)
        d = R.distances(X[live - 1], c.Q)
        got = both(ix, c.Q, c.r_at, True)
        want = R.radius_from(d, c.r_at, True, ids=live, labels=c.labels)
        assert same(got, want) and np.array_equal(got[2]["label"], want[2]["label"])
        assert not np.isin(got[2]["idx"], gone).any() and (got[2]["idx"] > 650).any()
        lst = np.array([10, 500, 700, 1, 651])
        pos = np.searchsorted(live, lst)
        dd = R.distances(X[live - 1], X[lst - 1])
        assert same(both_rows(ix, lst, c.r_at, True), R.radius_from(dd, c.r_at, True, ids=live, self_pos=pos))
        for f in (ix.radius_rows_count, ix.radius_rows):
            with pytest.raises(knn.KnnError) as e:
                f([10, 256], c.r_at)                      # a dead id is refused
            assert e.value.status == knn.ERR_INVALID
        assert same(both(ix, c.Q, c.r_at, True), want)    # and the index answers as before


# ---------------------------------------------------------------- 4. tiling

def test_tiles_and_stale_rows(knn, monkeypatch):
    c = case("mnist")
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    monkeypatch.setenv("KNN_QUERY_TILE", "128")
    with knn.Index(c.X) as ix:
        assert same(both_rows(ix, None, c.r_at, True), c.rows_ref(c.r_at, True))    # six tiles, the last partial
        Qb = np.vstack([c.Q] * 5)                                                   # two tiles
        want = c.ref(c.r_at, False)
        got = both(ix, Qb, c.r_at, False)
        assert np.array_equal(got[0], np.tile(want[0], 5))
        monkeypatch.delenv("KNN_QUERY_TILE")
        assert same(both_rows(ix, None, c.r_at, False), c.rows_ref(c.r_at, False))  # one large tile
        assert same(both(ix, c.Q[:5], c.r_at, False), R.radius_from(c.d[:5], c.r_at, False))
        assert same(both_rows(ix, [7, 300, 7], c.r_at, True), c.rows_ref(c.r_at, True, pos=[6, 299, 6]))


# --------------------------------------------------- 5. everything hits / 6. nothing

@pytest.fixture(scope="module")
def big():
    import datasets
    X = datasets.sift_like(4500, n=32)
    Q = datasets.sift_like(12, n=32, seed=3)
    return X, Q, R.distances(X, Q)


@pytest.mark.parametrize("env", [{}, {"KNN_NO_I8": "1"}], ids=["i8", "scan"])
def test_everything_hits(knn, monkeypatch, big, env):
    """m = 4500 > KNN_RADIUS_SORT_LDS = 2048: with r above the largest distance
    every segment is the whole corpus and is sorted in global memory; the
    second radius (a query's 1500th distance) keeps every segment sorted in
    LDS.  The first radius is past the byte path's clamp, 32 * 255^2."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    X, Q, d = big
    r_small = float(np.sort(d, axis=1)[:, 1499].min())
    with knn.Index(X) as ix:
        for r in (1e9, float(d.max()), r_small):
            got = both(ix, Q, r, True)
            want = R.radius_from(d, r, True)
            assert same(got, want)
        assert (ix.radius_count(Q, 1e9) == 4500).all()
    assert 1500 <= R.radius_from(d, r_small, True)[0].max() <= 2048


def test_nothing_hits_and_duplicates_only(knn, monkeypatch):
    c = case("mnist")
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    with knn.Index(c.X) as ix:
        counts, indptr, rec = both(ix, c.Q, 0.0, False)
        assert not counts.any() and not indptr.any() and len(rec) == 0
        got = both(ix, c.Q, 0.0, True)
        assert same(got, c.ref(0.0, True)) and got[0].max() == 3 and (got[2]["distance"] == 0.0).all()
        got = both_rows(ix, None, 0.0, True)
        assert same(got, c.rows_ref(0.0, True)) and got[0].max() == R.GROUP - 1


# -------------------------------------------------------------- 7. contract

def test_two_call_contract(knn, monkeypatch):
    c = case("mnist")
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    want = c.ref(c.r_at, True)
    counts, indptr, rec = want
    mq, total, guard = len(c.Q), len(rec), 64
    q = c.q_many
    with knn.Index(c.X) as ix:
        def fill(ip):
            buf = np.zeros(total + 2 * guard + 8, dtype=knn.NB_DTYPE)
            buf["idx"] = -7
            before = buf.copy()
            ip = np.ascontiguousarray(ip, dtype=np.int64)
            rc = knn.lib.knn_index_radius(ix._h, c.Q.ctypes.data_as(ctypes.c_void_p), mq, knn.ROWMAJOR, knn.F64,
                                          c.r_at, knn.QUERY_KEEP_ZERO, ip.ctypes.data_as(ctypes.c_void_p),
                                          ctypes.c_void_p(buf.ctypes.data + guard * knn.NB_DTYPE.itemsize))
            n = int(ip[-1] - ip[0])
            assert np.array_equal(buf[:guard], before[:guard])                 # the guard bands
            assert np.array_equal(buf[guard + n:], before[guard + n:])
            return rc, buf[guard:guard + n]
        rc, got = fill(indptr)
        assert rc == knn.OK and same((counts, indptr, got), want)
        rc, got = fill(indptr + 12345)                                          # any offset indptr[0] >= 0
        assert rc == knn.OK and same((counts, indptr, got), want)
        short = indptr.copy()
        short[q + 1:] -= 1
        assert fill(short)[0] == knn.ERR_INVALID
        long_ = indptr.copy()
        long_[q + 1:] += 1
        assert fill(long_)[0] == knn.ERR_INVALID
        assert fill(indptr)[0] == knn.OK
        with pytest.raises(knn.KnnError):
            ix.radius(c.Q, c.r_below, indptr=indptr)                            # another radius: other counts


# ------------------------------------------- 8. device outputs and sources

def test_device_outputs_and_sources(knn, monkeypatch):
    import torch
    c = case("mnist")
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    with knn.Index(c.X, labels=c.labels) as ix:
        host = both(ix, c.Q, c.r_at, True)
        want = c.ref(c.r_at, True, labels=c.labels)
        assert same(host, want) and np.array_equal(host[2]["label"], want[2]["label"]) and host[2]["label"].any()
        Qd = torch.from_numpy(c.Q.astype(np.uint8)).cuda()
        dc = ix.radius_count(Qd, c.r_at, out=True)
        assert dc.is_cuda and np.array_equal(dc.cpu().numpy(), host[0])
        ip, out = ix.radius(Qd, c.r_at, device=True)
        assert ip.is_cuda and out.is_cuda and np.array_equal(ip.cpu().numpy(), host[1])
        rec = out.cpu().numpy().view(knn.NB_DTYPE)[:len(host[2])]
        assert same((host[0], host[1], rec), host) and not rec["label"].any()
        ip, out = ix.radius_rows([5, 600], c.r_at, device=True)
        rec = out.cpu().numpy().view(knn.NB_DTYPE)[:int(ip[-1])]
        assert same((np.diff(ip.cpu().numpy()).astype(np.int32), ip.cpu().numpy(), rec),
                    c.rows_ref(c.r_at, True, pos=[4, 599]))


# ------------------------------------------------------ 9. query after radius

def test_query_after_radius(knn, monkeypatch):
    from query_ref import query_ref, same as same_nb
    c = case("mnist")
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    with knn.Index(c.X) as ix:
        first, _ = ix.query(c.Q, 30)
        b0 = ix.info().device_bytes
        both(ix, c.Q, c.r_at, True)
        b1 = ix.info().device_bytes
        again, _ = ix.query(c.Q, 30)
        assert ix.info().device_bytes == b1
    # the radius calls' tiles (128 rows: element and byte form), offsets, counters, flag and records
    mq, total = len(c.Q), int(c.ref(c.r_at, True)[1][-1])
    tiles = knn.block_bytes(128, 784) + knn.s8_block_bytes(128, 784)
    assert b1 - b0 >= tiles + (mq + 1) * 8 + mq * 4 + 4
    assert b1 - b0 <= tiles + (mq + 1) * 8 + mq * 4 + 4 + total * 16
    assert same_nb(first, again) and same_nb(again, query_ref(c.X, c.Q, 30, True))
