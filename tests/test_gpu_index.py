"""The resident corpus index on the GPU (knn_index_*, mpiknn.Index): packed
once, queried many times.  Every path of knn_query -- int8, fp16 / fp64
integer contraction, forced rescan, real-valued fp64, fp32 on the split filter
and without it -- under both zero rules, against the numpy restatement of
tests/query_ref.py and against knn_query itself; state kept between calls,
the path decision per batch, blocks and tiles, ownership of the data, labels,
device pointers in and out, 8-bit sources.  Exact: idx equal and distance
equal bit for bit, every row.  (Inputs as tests/test_gpu_query.py.)"""
import numpy as np
import pytest

import datasets
from query_ref import query_ref, same, vote_ref

pytestmark = pytest.mark.gpu


def make_queries(X, nq, nfresh, fresh, rng_seed=5):
    """nq queries: nfresh new rows, then (nq - nfresh) / 2 exact copies of
    corpus rows, then as many copies of corpus rows that each appear three
    times in the corpus (made so by overwriting two other corpus rows).
    Returns (corpus, queries)."""
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


@pytest.fixture(scope="module")
def int_data():
    X, y = datasets.mnist_like(1000)
    F, yq = datasets.mnist_like(260, seed=77)
    X, Q = make_queries(X, 300, 260, F)
    ref = {kz: query_ref(X, Q, 30, kz) for kz in (False, True)}
    return X, y, Q, ref


@pytest.fixture(scope="module")
def real_data():
    X, y = datasets.mnist_real(1000)
    F, _ = datasets.mnist_real(160, seed=77)
    X, Q = make_queries(X, 200, 160, F)
    ref = {(kz, dt, k): query_ref(X, Q, k, kz, dtype=dt)
           for kz in (False, True) for dt, k in (("f64", 30), ("f32", 100))}
    return X, Q, ref


ENVS = [{}, {"KNN_NO_I8": "1"}, {"KNN_NO_I8": "1", "KNN_NO_H16": "1"}, {"KNN_FORCE_RESCAN": "1"}]


# ------------------------------------------------------------ 1. parity

@pytest.mark.parametrize("keep_zero", [False, True])
@pytest.mark.parametrize("env", ENVS, ids=["i8", "h16", "f64int", "rescan"])
def test_index_int(knn, int_data, monkeypatch, env, keep_zero):
    X, y, Q, ref = int_data
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    with knn.Index(X) as ix:
        assert ix.info().last_bits == 0
        got, secs = ix.query(Q, 30, keep_zero=keep_zero)
        bits = ix.info().last_bits
    one, _ = knn.query(X, Q, 30, keep_zero=keep_zero)
    assert same(got, ref[keep_zero]) and same(got, one)
    assert secs > 0.0
    if "KNN_NO_I8" not in env:
        assert bits == 8
    else:
        assert bits == (64 if "KNN_NO_H16" in env else 16)


@pytest.mark.parametrize("keep_zero", [False, True])
def test_index_real_f64(knn, real_data, keep_zero):
    X, Q, ref = real_data
    with knn.Index(X) as ix:
        got, _ = ix.query(Q, 30, keep_zero=keep_zero)
    one, _ = knn.query(X, Q, 30, keep_zero=keep_zero)
    assert same(got, ref[(keep_zero, "f64", 30)]) and same(got, one)


@pytest.mark.parametrize("keep_zero", [False, True])
@pytest.mark.parametrize("no_split", [False, True])
def test_index_f32_k100(knn, real_data, monkeypatch, no_split, keep_zero):
    X, Q, ref = real_data
    if no_split:
        monkeypatch.setenv("KNN_NO_SPLIT", "1")
    with knn.Index(X, dtype="f32") as ix:
        got, _ = ix.query(Q, 100, keep_zero=keep_zero)
    one, _ = knn.query(X, Q, 100, dtype="f32", keep_zero=keep_zero)
    assert same(got, ref[(keep_zero, "f32", 100)]) and same(got, one)


def test_index_col_layout(knn, int_data):
    X, y, Q, ref = int_data
    with knn.Index(X, layout="col") as ix:
        got, _ = ix.query(Q, 30, keep_zero=True)
        assert ix.info().last_bits == 8
    assert same(got, ref[True])


# ------------------------------------------------- 2. one index, many calls

def test_one_index_many_calls(knn, int_data):
    X, y, Q, ref = int_data
    q1 = Q[[265]]                                  # an exact copy of a corpus row
    with knn.Index(X) as ix:
        a, _ = ix.query(Q, 30, keep_zero=True)
        b, _ = ix.query(q1, 5, keep_zero=False)
        c, _ = ix.query(Q[256:300], 32, keep_zero=True)
        d, _ = ix.query(Q, 30, keep_zero=True)
    assert same(a, ref[True])
    rb = query_ref(X, q1, 5, False)
    assert same(b, rb) and (b["distance"] > 0.0).all()
    assert query_ref(X, q1, 5, True)["distance"][0, 0] == 0.0     # the zero rule shows on this query
    assert same(c, query_ref(X, Q[256:300], 32, True))
    assert same(d, ref[True]) and np.array_equal(a, d)


# ---------------------------------------------- 3. the path follows the batch

def test_path_follows_batch(knn, int_data):
    X, y, Q, ref = int_data
    Q2 = Q[:64].copy()
    Q2[3, 5] = 255.5
    Q2[10, 7] = 256.0
    with knn.Index(X) as ix:
        a, _ = ix.query(Q, 30)
        assert ix.info().last_bits == 8
        b, _ = ix.query(Q2, 30)
        assert ix.info().last_bits != 8
        c, _ = ix.query(Q, 30)
        assert ix.info().last_bits == 8
    assert same(a, ref[True])
    assert same(b, query_ref(X, Q2, 30, True))
    assert np.array_equal(a, c)


# ---------------------------------------------------- 4. blocks and tiles

@pytest.mark.parametrize("keep_zero", [False, True])
def test_blocks_and_tiles(knn, int_data, real_data, monkeypatch, keep_zero):
    """three corpus blocks (the last partial) and three query tiles (the last
    44 rows): the one-block, one-tile result and the restatement"""
    X, y, Q, ref = int_data
    Xr, Qr, refr = real_data
    with knn.Index(X) as ix:
        assert ix.info().nblocks == 1
        one, _ = ix.query(Q, 30, keep_zero=keep_zero)
    with knn.Index(Xr) as ix:
        one_r, _ = ix.query(Qr, 30, keep_zero=keep_zero)
    monkeypatch.setenv("KNN_QUERY_BLOCK", "384")
    ix, ixr = knn.Index(X), knn.Index(Xr)
    try:
        monkeypatch.delenv("KNN_QUERY_BLOCK")
        assert ix.info().nblocks == 3 and ixr.info().nblocks == 3
        monkeypatch.setenv("KNN_QUERY_TILE", "128")
        got, _ = ix.query(Q, 30, keep_zero=keep_zero)
        assert ix.info().last_bits == 8
        assert same(got, one) and same(got, ref[keep_zero])
        got_r, _ = ixr.query(Qr, 30, keep_zero=keep_zero)
        assert same(got_r, one_r) and same(got_r, refr[(keep_zero, "f64", 30)])
        monkeypatch.setenv("KNN_FORCE_RESCAN", "1")
        got, _ = ix.query(Q, 30, keep_zero=keep_zero)
        assert same(got, one) and same(got, ref[keep_zero])
    finally:
        ix.close()
        ixr.close()


# ------------------------------------------------ 5. the index owns its data

def test_index_owns_its_data(knn, int_data):
    X, y, Q, ref = int_data
    Xc = X.copy()
    with knn.Index(Xc) as ix:
        Xc[:] = 0.0
        got, _ = ix.query(Q, 30)
    assert same(got, ref[True])


# ------------------------------------------------------------- 6. labels

@pytest.mark.parametrize("rule", [0, 1, 2])
def test_labels_and_vote(knn, int_data, rule):
    X, y, Q, ref = int_data
    yc = y.copy()
    with knn.Index(X, labels=yc) as ix:
        yc[:] = -1                                    # the index keeps its own copy
        got, _ = ix.query(Q, 30)
    assert same(got, ref[True])
    ok = got["idx"] > 0
    assert ok.any() and (got["label"][ok] == y[got["idx"][ok] - 1]).all()
    assert (got["label"][~ok] == 0).all()
    yq = ((np.arange(len(Q)) % 10) + 1).astype(np.float64)
    pred, matches = knn.classify_query(got, y, yq, 10, rule)
    pred_r, matches_r = vote_ref(got, y, yq, 10, rule)
    assert np.array_equal(pred, pred_r) and matches == matches_r


# ------------------------------------------------ 7. device in, device out

@pytest.mark.parametrize("src", ["f64", "u8"])
def test_device_in_device_out(knn, int_data, src):
    import torch
    X, y, Q, ref = int_data
    dev = torch.device("cuda", 0)
    cast = (lambda a: a) if src == "f64" else (lambda a: a.astype(np.uint8))
    d_X, d_Q = torch.from_numpy(cast(X)).to(dev), torch.from_numpy(cast(Q)).to(dev)
    with knn.Index(X, labels=y) as ix:
        host, _ = ix.query(Q, 30)
    with knn.Index(d_X, labels=y) as ix:
        d_X.zero_()
        d_out = torch.full((len(Q) * 30 * knn.NB_DTYPE.itemsize,), 0xAB, dtype=torch.uint8, device=dev)
        res, secs = ix.query(d_Q, 30, out=d_out)
        assert res is d_out and secs > 0.0 and ix.info().last_bits == 8
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(knn.NB_DTYPE).reshape(len(Q), 30)
    assert same(got, host) and same(got, ref[True])
    assert (got["label"] == 0).all() and (host["label"] != 0).any()


# --------------------------------------------------------- 8. 8-bit sources

@pytest.mark.parametrize("keep_zero", [False, True])
def test_u8_sources(knn, int_data, keep_zero):
    X, y, Q, ref = int_data
    assert np.array_equal(X.astype(np.uint8), X) and np.array_equal(Q.astype(np.uint8), Q)
    with knn.Index(X) as ix:
        f64, _ = ix.query(Q, 30, keep_zero=keep_zero)
        big = ix.info().device_bytes
    with knn.Index(X.astype(np.uint8)) as ix:
        got, _ = ix.query(Q.astype(np.uint8), 30, keep_zero=keep_zero)
        assert ix.info().last_bits == 8
        mixed, _ = ix.query(Q, 30, keep_zero=keep_zero)
        assert ix.info().last_bits == 8
        f32q, _ = ix.query(Q.astype(np.float32), 30, keep_zero=keep_zero)
        assert ix.info().device_bytes == big            # the same resident blocks, whatever the source
    assert np.array_equal(got, f64) and np.array_equal(mixed, f64) and np.array_equal(f32q, f64)
    assert same(got, ref[keep_zero])


def test_index_info_and_errors(knn, int_data):
    X, y, Q, ref = int_data
    with knn.Index(X.astype(np.uint8), dtype="f32") as ix:
        info = ix.info()
        assert (info.m, info.n, info.nblocks, info.last_bits) == (1000, 784, 1, 0)
        # the element block; no byte block (pixels at n = 784 are past fp32's exact-integer range)
        assert knn.block_bytes(1000, 784, "f32") <= info.device_bytes < \
            knn.block_bytes(1000, 784, "f32") + knn.s8_block_bytes(1000, 784)
        with pytest.raises(knn.KnnError) as e:
            ix.query(Q, knn.MAX_K_F32 + 1)
        assert e.value.status == knn.ERR_UNSUPPORTED
        with pytest.raises(ValueError):
            ix.query(Q[:, :100], 30)
        got, _ = ix.query(Q, 30)                        # (8-bit pixels at n = 784 are not fp32-exact: GEMM mode)
        assert same(got, query_ref(X, Q, 30, True, dtype="f32"))
        assert ix.info().device_bytes > info.device_bytes
    with pytest.raises(ValueError):
        ix.query(Q, 30)                                 # closed


# ------------------- a kept context across paths whose list buffers coincide

def test_other_path_then_larger_batch_f64(knn, int_data):
    """Same k throughout, so one context serves every call.  1024 integer rows
    set the tile capacity; 384 real-valued rows take the element path (4 x 16
    lists a query and split: 384 * 64 list entries a split); 1024 integer rows
    take the byte path again (2 x 12 lists: 1024 * 24, the same count), so the
    partial-list buffers are reused as they are and only the per-split bounds
    need 1024 entries a split where 384 were in use."""
    X, y, Q, ref = int_data
    Qi, _ = datasets.mnist_like(1024, seed=78)
    Qr, _ = datasets.mnist_like(384, seed=79)
    Qr = Qr + 0.25
    want_i, _ = knn.query(X, Qi, 30)
    want_r = query_ref(X, Qr, 30, True)
    with knn.Index(X) as ix:
        a, _ = ix.query(Qi, 30)
        assert ix.info().last_bits == 8
        b, _ = ix.query(Qr, 30)
        assert ix.info().last_bits != 8
        c, _ = ix.query(Qi, 30)
        assert ix.info().last_bits == 8
        d, _ = ix.query(Qr, 30)
    assert same(a, want_i) and same(c, want_i) and np.array_equal(a, c)
    assert same(b, want_r) and np.array_equal(b, d)
    assert same(a[:8], query_ref(X, Qi[:8], 30, True))


def test_other_path_then_larger_batch_f32(knn):
    """the same with fp32 blocks at n = 128 (SIFT's width: 8-bit values are
    fp32-exact there), where the ratio is 4 : 1 -- 128 real-valued rows (4 x 24
    lists at k = 30), then 512 integer rows (2 x 12)"""
    rng = np.random.default_rng(11)
    X = rng.integers(0, 256, (1000, 128)).astype(np.float64)
    Qi = rng.integers(0, 256, (512, 128)).astype(np.float64)
    Qi[:16] = X[:16]
    Qr = rng.integers(0, 256, (128, 128)).astype(np.float64) + 0.25
    want_i, _ = knn.query(X, Qi, 30, dtype="f32")
    want_r = query_ref(X, Qr, 30, True, dtype="f32")
    with knn.Index(X.astype(np.uint8), dtype="f32") as ix:
        a, _ = ix.query(Qi.astype(np.uint8), 30)
        assert ix.info().last_bits == 8
        b, _ = ix.query(Qr, 30)
        assert ix.info().last_bits != 8
        c, _ = ix.query(Qi.astype(np.uint8), 30)
        assert ix.info().last_bits == 8
    assert same(a, want_i) and np.array_equal(a, c)
    assert same(b, want_r)
    assert same(a[:24], query_ref(X, Qi[:24], 30, True, dtype="f32"))


# ------------------------------------- knn_index_query's argument checks

def test_index_query_argument_checks(knn, int_data):
    """every KNN_ERR_INVALID / KNN_ERR_UNSUPPORTED case of knn_index_query on a
    live index, through the raw entry point; the index serves a valid call
    afterwards"""
    import ctypes
    X, y, Q, ref = int_data
    Qs = np.ascontiguousarray(Q[:4])
    out = np.zeros((4, 30), dtype=knn.NB_DTYPE)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    with knn.Index(X) as ix:
        ok = dict(h=ix._h, Q=Qs, mq=4, layout=knn.ROWMAJOR, src=knn.F64, k=30, flags=0, out=out)

        def call(**kw):
            a = dict(ok, **kw)
            return knn.lib.knn_index_query(a["h"], p(a["Q"]), a["mq"], a["layout"], a["src"], a["k"], a["flags"],
                                           p(a["out"]))

        assert call(h=None) == knn.ERR_INVALID
        assert call(Q=None) == knn.ERR_INVALID
        assert call(out=None) == knn.ERR_INVALID
        assert call(mq=0) == knn.ERR_INVALID
        assert call(k=0) == knn.ERR_INVALID
        assert call(k=-2) == knn.ERR_INVALID
        assert call(layout=2) == knn.ERR_INVALID
        assert call(layout=-1) == knn.ERR_INVALID
        assert call(flags=8) == knn.ERR_INVALID
        assert call(flags=knn.QUERY_KEEP_ZERO | 16) == knn.ERR_INVALID
        assert call(mq=2 ** 31 - 1000) == knn.ERR_INVALID          # m + mq = INT32_MAX + 1
        assert call(mq=2 ** 31) == knn.ERR_INVALID
        assert call(src=3) == knn.ERR_UNSUPPORTED
        assert call(src=-1) == knn.ERR_UNSUPPORTED
        assert call(k=knn.MAX_K + 1) == knn.ERR_UNSUPPORTED
        assert ix.info().last_bits == 0                             # none of them reached the device
        for flags in (0, knn.QUERY_KEEP_ZERO):
            assert call(flags=flags) == knn.OK
            assert same(out, ref[bool(flags)][:4])
        got, _ = ix.query(Q, 30)
        assert same(got, ref[True])


def test_index_rejects_other_device_and_small_out(knn, int_data):
    import torch
    X, y, Q, ref = int_data
    dev = torch.device("cuda", 0)
    with knn.Index(X) as ix:
        small = torch.zeros(16, dtype=torch.uint8, device=dev)
        with pytest.raises(ValueError):
            ix.query(Q, 30, out=small)
        with pytest.raises(ValueError):
            ix.query(Q, 30, out=np.zeros(len(Q) * 30 * 16, dtype=np.uint8))
        if torch.cuda.device_count() > 1:
            other = torch.device("cuda", 1)
            with pytest.raises(ValueError):
                ix.query(torch.from_numpy(Q).to(other), 30)
            with pytest.raises(ValueError):
                knn.Index(torch.from_numpy(X).to(other))
