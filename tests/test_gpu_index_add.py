"""knn_index_add / mpiknn.Index.add on the GPU: an index that grew by adds
answers exactly as knn_query on the concatenated corpus and as the numpy
restatement of tests/query_ref.py -- idx equal and distance equal bit for bit
-- on every path, between adds, from every source type, after the byte blocks
were dropped, after a re-block, with labels, after refused calls.  (Inputs as
tests/test_gpu_index.py.)"""
import functools

import numpy as np
import pytest

import datasets
from query_ref import query_ref, same, vote_ref

pytestmark = pytest.mark.gpu

M0, ADDS = 700, (1, 300, 523)               # 1524 rows: with KNN_QUERY_BLOCK=256 the adds fill a
BLOCK = "256"                               # partial last block and cross into new blocks
ENVS = [{}, {"KNN_NO_I8": "1"}, {"KNN_NO_I8": "1", "KNN_NO_H16": "1"}, {"KNN_FORCE_RESCAN": "1"}]


def make_queries(X, nq, nfresh, fresh, rng_seed=5):
    """tests/test_gpu_index.py's make_queries restated: nq queries -- nfresh
    new rows, then (nq - nfresh) / 2 exact copies of corpus rows, then as many
    copies of corpus rows that each appear three times in the corpus (made so
    by overwriting two other corpus rows).  Returns (corpus, queries)."""
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
    return X, Q


def cuts(m0, adds):
    """[(first row, end row)] of every add"""
    out, m = [], m0
    for a in adds:
        out.append((m, m + a))
        m += a
    return out


def grown(knn, X, m0, adds, labels=None, cast=None, **kw):
    """an index over X[:m0] that grew by the adds"""
    cast = cast or (lambda a: a)
    ix = knn.Index(cast(X[:m0]), labels=None if labels is None else labels[:m0], **kw)
    for lo, hi in cuts(m0, adds):
        first = ix.add(cast(X[lo:hi]), labels=None if labels is None else labels[lo:hi])
        assert first == lo + 1 and ix.m == hi
    return ix


@pytest.fixture(scope="module")
def int_data():
    m = M0 + sum(ADDS)
    X, y = datasets.mnist_like(m)
    F, _ = datasets.mnist_like(160, seed=77)
    X, Q = make_queries(X, 200, 160, F)
    ref = functools.lru_cache(None)(lambda kz, rows=m, nq=len(Q): query_ref(X[:rows], Q[:nq], 30, kz))
    return X, y, Q, ref


@pytest.fixture(scope="module")
def real_data():
    X, y = datasets.mnist_real(1000)
    F, _ = datasets.mnist_real(120, seed=77)
    X, Q = make_queries(X, 160, 120, F)
    ref = functools.lru_cache(None)(lambda kz, dt, k: query_ref(X, Q, k, kz, dtype=dt))
    return X, Q, ref


# --------------------------------------------------- 1. parity on every path

@pytest.mark.parametrize("keep_zero", [False, True])
@pytest.mark.parametrize("env", ENVS, ids=["i8", "h16", "f64int", "rescan"])
def test_add_int(knn, int_data, monkeypatch, env, keep_zero):
    X, y, Q, ref = int_data
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    with grown(knn, X, M0, ADDS) as ix:
        info = ix.info()
        assert (info.m, info.nblocks) == (len(X), 6)
        got, secs = ix.query(Q, 30, keep_zero=keep_zero)
        bits = ix.info().last_bits
    one, _ = knn.query(X, Q, 30, keep_zero=keep_zero)
    assert same(got, ref(keep_zero)) and same(got, one)
    assert secs > 0.0
    if "KNN_NO_I8" not in env:
        assert bits == 8
    else:
        assert bits == (64 if "KNN_NO_H16" in env else 16)


# ------------------------------------------------------ 2. query between adds

def test_query_between_adds(knn, int_data, monkeypatch):
    X, y, Q, ref = int_data
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    Qs = Q[:64]
    with knn.Index(X[:M0]) as ix:
        got, _ = ix.query(Qs, 30)
        assert same(got, ref(True, M0, 64))
        for lo, hi in cuts(M0, ADDS):
            assert ix.add(X[lo:hi]) == lo + 1
            got, _ = ix.query(Qs, 30)
            assert same(got, ref(True, hi, 64))
            assert ix.info().m == hi and ix.info().last_bits == 8
            # a query equal to a just-added row finds it first, at 0.0, under its new id
            # (the last added row that make_queries gave no twin)
            row = next(r for r in range(hi - 1, lo - 1, -1) if (X[:hi] == X[r]).all(axis=1).sum() == 1)
            me, _ = ix.query(X[[row]], 30, keep_zero=True)
            assert me["distance"][0, 0] == 0.0 and me["idx"][0, 0] == row + 1
            assert same(me, query_ref(X[:hi], X[[row]], 30, True))
            gone, _ = ix.query(X[[row]], 30, keep_zero=False)
            assert (gone["distance"] > 0.0).all()


# ------------------------------------------------------- 3. real-valued data

@pytest.mark.parametrize("keep_zero", [False, True])
def test_add_real_f64(knn, real_data, monkeypatch, keep_zero):
    X, Q, ref = real_data
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    with grown(knn, X, 600, (400,)) as ix:
        got, _ = ix.query(Q, 30, keep_zero=keep_zero)
    one, _ = knn.query(X, Q, 30, keep_zero=keep_zero)
    assert same(got, ref(keep_zero, "f64", 30)) and same(got, one)


@pytest.mark.parametrize("keep_zero", [False, True])
@pytest.mark.parametrize("no_split", [False, True])
def test_add_f32_k100(knn, real_data, monkeypatch, no_split, keep_zero):
    X, Q, ref = real_data
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    if no_split:
        monkeypatch.setenv("KNN_NO_SPLIT", "1")
    with grown(knn, X, 600, (400,), dtype="f32") as ix:
        got, _ = ix.query(Q, 100, keep_zero=keep_zero)
    one, _ = knn.query(X, Q, 100, dtype="f32", keep_zero=keep_zero)
    assert same(got, ref(keep_zero, "f32", 100)) and same(got, one)


# ---------------------------------------------------------------- 4. sources

def test_add_sources(knn, int_data, monkeypatch):
    import torch
    X, y, Q, ref = int_data
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    dev = torch.device("cuda", 0)
    casts = {"u8": lambda a: a.astype(np.uint8), "f32": lambda a: a.astype(np.float32),
             "torch-f64": lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev),
             "torch-u8": lambda a: torch.from_numpy(a.astype(np.uint8)).to(dev)}
    with grown(knn, X, M0, ADDS) as ix:
        want, _ = ix.query(Q, 30)
        nbytes = ix.info().device_bytes
    assert same(want, ref(True))
    for name, cast in casts.items():
        with grown(knn, X, M0, ADDS, cast=cast) as ix:
            got, _ = ix.query(Q, 30)
            assert ix.info().last_bits == 8 and ix.info().device_bytes == nbytes, name
        assert np.array_equal(got, want), name
    with grown(knn, X, M0, ADDS, layout="col") as ix:
        got, _ = ix.query(Q, 30)
        assert ix.info().last_bits == 8
    assert np.array_equal(got, want)


# ------------------------------------------------------ 5. byte path dropped

def test_byte_blocks_dropped(knn, int_data, monkeypatch):
    X, y, Q, ref = int_data
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    m1 = M0 + 1
    Xb = X[:M0 + 1 + 300].copy()
    Xb[M0, 11] = 300.0                                   # the one-row add: outside the byte image
    want = query_ref(Xb, Q[:64], 30, True)
    with knn.Index(Xb[:M0]) as ix:
        ix.query(Q[:64], 30)
        assert ix.info().last_bits == 8
        before = ix.info().device_bytes
        ix.add(Xb[M0:m1])
        info = ix.info()
        # 700 and 701 rows are three blocks alike: exactly the byte blocks went
        assert info.nblocks == 3 and before - info.device_bytes == 3 * knn.s8_block_bytes(256, 784)
        mid, _ = ix.query(Q[:64], 30)
        assert same(mid, query_ref(Xb[:m1], Q[:64], 30, True)) and ix.info().last_bits != 8
        bytes_mid = ix.info().device_bytes
        ix.add(Xb[m1:].astype(np.uint8))                 # all 8-bit again: the byte blocks stay away
        info = ix.info()
        assert info.nblocks == 4 and info.device_bytes - bytes_mid == knn.block_bytes(256, 784)
        got, _ = ix.query(Q[:64], 30)
        bits = ix.info().last_bits
    with knn.Index(Xb) as ix:
        fresh, _ = ix.query(Q[:64], 30)
        assert ix.info().last_bits == bits
    assert same(got, want) and same(fresh, want) and bits != 8


# ------------------------------------------------------------- 6. re-block

def test_reblock(knn, int_data, monkeypatch):
    """no KNN_QUERY_BLOCK: the index starts with one 200-row block and ten adds
    of 200 rows would leave eleven; the capacity doubles instead"""
    X, y, Q, ref = int_data
    monkeypatch.delenv("KNN_QUERY_BLOCK", raising=False)
    Xr = np.vstack([X, X[:676] + 1.0])[:2200]
    Xr = np.minimum(Xr, 255.0)
    Qs = Q[:64]
    with knn.Index(Xr[:200]) as ix:
        ix.query(Qs, 30)                                  # a context made for the first capacity
        for a in range(10):
            lo = 200 * (a + 1)
            assert ix.add(Xr[lo:lo + 200].astype(np.uint8) if a % 2 else Xr[lo:lo + 200]) == lo + 1
            info = ix.info()
            assert info.m == lo + 200 and info.nblocks <= 8
            if a in (4, 9):
                got, _ = ix.query(Qs, 30)
                assert ix.info().last_bits == 8
                assert same(got, query_ref(Xr[:lo + 200], Qs, 30, True))
                one, _ = knn.query(Xr[:lo + 200], Qs, 30)
                assert same(got, one)
        assert ix.info().nblocks < 8                      # it did re-block (11 blocks of 200 otherwise)


def test_reblock_real_f32(knn, real_data, monkeypatch):
    """the element blocks of a re-block: rows and fp norms moved, no byte blocks"""
    X, Q, ref = real_data
    monkeypatch.delenv("KNN_QUERY_BLOCK", raising=False)
    with grown(knn, X, 100, (100,) * 9, dtype="f32") as ix:
        assert ix.info().nblocks <= 8
        got, _ = ix.query(Q, 100)
    assert same(got, ref(True, "f32", 100))


# --------------------------------------------------------------- 7. labels

@pytest.mark.parametrize("rule", [0, 1, 2])
def test_add_labels_and_vote(knn, int_data, monkeypatch, rule):
    X, y, Q, ref = int_data
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    with grown(knn, X, M0, ADDS, labels=y) as ix:
        got, _ = ix.query(Q, 30)
    assert same(got, ref(True))
    ok = got["idx"] > 0
    assert (got["idx"] > M0).any()                        # records that point at added rows
    assert (got["label"][ok] == y[got["idx"][ok] - 1]).all() and (got["label"][~ok] == 0).all()
    yq = ((np.arange(len(Q)) % 10) + 1).astype(np.float64)
    pred, matches = knn.classify_query(got, y, yq, 10, rule)
    pred_r, matches_r = vote_ref(got, y, yq, 10, rule)
    assert np.array_equal(pred, pred_r) and matches == matches_r


# --------------------------------------------------------------- 8. errors

def test_add_errors_leave_the_index_alone(knn, int_data, monkeypatch):
    import ctypes
    X, y, Q, ref = int_data
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    Qs = Q[:64]
    want = ref(True, M0, 64)
    A = np.ascontiguousarray(X[M0:M0 + 10])
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)

    def raw(ix, X=A, rows=10, layout=knn.ROWMAJOR, src=knn.F64, labels=None, flags=0):
        return knn.lib.knn_index_add(ix._h, p(X), rows, layout, src, p(labels), flags)

    with knn.Index(X[:M0], labels=y[:M0]) as ix:
        with pytest.raises(knn.KnnError) as e:
            ix.add(A, labels=None)
        assert e.value.status == knn.ERR_INVALID
        got, _ = ix.query(Qs, 30)
        assert same(got, want) and ix.info().m == M0 and ix.m == M0
        lab = np.ascontiguousarray(y[M0:M0 + 10])
        assert raw(ix, X=None, labels=lab) == knn.ERR_INVALID
        assert raw(ix, rows=0, labels=lab) == knn.ERR_INVALID
        assert raw(ix, layout=2, labels=lab) == knn.ERR_INVALID
        assert raw(ix, flags=1, labels=lab) == knn.ERR_INVALID
        assert raw(ix, flags=knn.INDEX_DEVICE_OUT, labels=lab) == knn.ERR_INVALID
        assert raw(ix, rows=2 ** 31 - M0, labels=lab) == knn.ERR_INVALID
        assert raw(ix, src=3, labels=lab) == knn.ERR_UNSUPPORTED
        with pytest.raises(ValueError):
            ix.add(A[:, :100], labels=lab)
        with pytest.raises(ValueError):
            ix.add(A, labels=lab[:5])
        got, _ = ix.query(Qs, 30)
        assert same(got, want) and ix.info().m == M0
        assert raw(ix, labels=lab) == knn.OK and ix.info().m == M0 + 10
    with knn.Index(X[:M0]) as ix:
        with pytest.raises(knn.KnnError) as e:
            ix.add(A, labels=y[M0:M0 + 10])
        assert e.value.status == knn.ERR_INVALID
        got, _ = ix.query(Qs, 30)
        assert same(got, want) and ix.info().m == M0
    with pytest.raises(ValueError):
        ix.add(A)                                         # closed


# ------------------------------------------------------------- 9. ownership

def test_index_owns_added_rows(knn, int_data, monkeypatch):
    X, y, Q, ref = int_data
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    with knn.Index(X[:M0]) as ix:
        for lo, hi in cuts(M0, ADDS):
            A = X[lo:hi].copy()
            ix.add(A)
            A[:] = 0.0
        got, _ = ix.query(Q, 30)
    assert same(got, ref(True))
