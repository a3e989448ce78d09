"""Out-of-sample queries on the GPU (knn_query, knn_ctx_set_keep_zero): every
path -- int8, fp16 / fp64 integer contraction, forced rescan, real-valued
fp64, fp32 on the split filter and without it -- under both zero rules,
against the numpy restatement of tests/query_ref.py.  Exact: idx equal and
distance equal bit for bit, every row."""
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


def test_data_has_zeros_and_ties(int_data):
    X, y, Q, ref = int_data
    keep, drop = ref[True], ref[False]
    assert (keep["distance"][260:280, 0] == 0.0).all() and (keep["distance"][260:280, 1] > 0.0).all()
    assert (keep["distance"][280:, :3] == 0.0).all()                  # id ties at distance 0
    assert (np.diff(keep["idx"][280:, :3], axis=1) > 0).all()
    assert (drop["distance"] > 0.0).all()


ENVS = [{}, {"KNN_NO_I8": "1"}, {"KNN_NO_I8": "1", "KNN_NO_H16": "1"}, {"KNN_FORCE_RESCAN": "1"}]


@pytest.mark.parametrize("keep_zero", [False, True])
@pytest.mark.parametrize("env", ENVS, ids=["i8", "h16", "f64int", "rescan"])
def test_query_int(knn, int_data, monkeypatch, env, keep_zero):
    X, y, Q, ref = int_data
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    got, secs = knn.query(X, Q, 30, labels=y, keep_zero=keep_zero)
    assert same(got, ref[keep_zero])
    ok = got["idx"] > 0
    assert (got["label"][ok] == y[got["idx"][ok] - 1]).all()
    assert secs > 0.0


@pytest.mark.parametrize("keep_zero", [False, True])
def test_query_real_f64(knn, real_data, keep_zero):
    X, Q, ref = real_data
    got, _ = knn.query(X, Q, 30, keep_zero=keep_zero)
    assert same(got, ref[(keep_zero, "f64", 30)])


@pytest.mark.parametrize("keep_zero", [False, True])
@pytest.mark.parametrize("no_split", [False, True])
def test_query_f32_k100(knn, real_data, monkeypatch, no_split, keep_zero):
    X, Q, ref = real_data
    if no_split:
        monkeypatch.setenv("KNN_NO_SPLIT", "1")
    got, _ = knn.query(X, Q, 100, dtype="f32", keep_zero=keep_zero)
    assert same(got, ref[(keep_zero, "f32", 100)])


@pytest.mark.parametrize("keep_zero", [False, True])
def test_query_col_layout(knn, int_data, keep_zero):
    X, y, Q, ref = int_data
    got, _ = knn.query(X, Q, 30, layout="col", keep_zero=keep_zero)
    assert same(got, ref[keep_zero])


@pytest.mark.parametrize("keep_zero", [False, True])
def test_query_block_384(knn, int_data, real_data, monkeypatch, keep_zero):
    """three corpus blocks, the last partial: the one-block result and the
    restatement"""
    X, y, Q, ref = int_data
    one, _ = knn.query(X, Q, 30, keep_zero=keep_zero)
    Xr, Qr, refr = real_data
    one_r, _ = knn.query(Xr, Qr, 30, keep_zero=keep_zero)
    monkeypatch.setenv("KNN_QUERY_BLOCK", "384")
    got, _ = knn.query(X, Q, 30, keep_zero=keep_zero)
    assert same(got, one) and same(got, ref[keep_zero])
    got_r, _ = knn.query(Xr, Qr, 30, keep_zero=keep_zero)
    assert same(got_r, one_r) and same(got_r, refr[(keep_zero, "f64", 30)])
    monkeypatch.setenv("KNN_NO_I8", "1")
    got, _ = knn.query(X, Q, 30, keep_zero=keep_zero)
    assert same(got, ref[keep_zero])


@pytest.mark.parametrize("keep_zero", [False, True])
def test_query_tiles(knn, int_data, real_data, monkeypatch, keep_zero):
    """KNN_QUERY_TILE=128: three query tiles, the last partial (44 rows), over
    three corpus blocks -- int8 path, forced rescan, real-valued fp64; the
    one-tile result and the restatement"""
    X, y, Q, ref = int_data
    one, _ = knn.query(X, Q, 30, keep_zero=keep_zero)
    monkeypatch.setenv("KNN_QUERY_TILE", "128")
    monkeypatch.setenv("KNN_QUERY_BLOCK", "384")
    got, secs = knn.query(X, Q, 30, labels=y, keep_zero=keep_zero)
    assert same(got, one) and same(got, ref[keep_zero]) and secs > 0.0
    ok = got["idx"] > 0
    assert (got["label"][ok] == y[got["idx"][ok] - 1]).all()
    Xr, Qr, refr = real_data
    got_r, _ = knn.query(Xr, Qr, 30, keep_zero=keep_zero)
    assert same(got_r, refr[(keep_zero, "f64", 30)])
    monkeypatch.setenv("KNN_FORCE_RESCAN", "1")
    got, _ = knn.query(X, Q, 30, keep_zero=keep_zero)
    assert same(got, ref[keep_zero])


@pytest.mark.parametrize("keep_zero", [False, True])
def test_query_fewer_rows_than_k(knn, keep_zero):
    X, _ = datasets.mnist_like(20, seed=9)
    F, _ = datasets.mnist_like(110, seed=78)
    Q = np.vstack([F, X])                       # 130 queries, the last 20 copy the corpus
    got, _ = knn.query(X, Q, 30, keep_zero=keep_zero)
    assert same(got, query_ref(X, Q, 30, keep_zero))
    filled = (got["idx"] > 0).sum(axis=1)
    assert (filled[:110] == 20).all()
    assert (filled[110:] == (20 if keep_zero else 19)).all()
    empty = got[got["idx"] == 0]
    assert np.isinf(empty["distance"]).all() and (empty["label"] == 0).all()


def _device_search(knn, ctx, d_q, mq, m, k, d_meta, steps):
    """begin / step(s) / end / rescan on packed element blocks (steps: (block,
    rows, base) each); host records"""
    import torch
    dev = d_q.device
    st = torch.cuda.current_stream(dev).cuda_stream
    d_out = torch.zeros(mq * k * knn.NB_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    ctx.begin(d_q.data_ptr(), mq, m, d_meta.data_ptr(), st)
    for blk, nc, base in steps:
        ctx.step(blk.data_ptr(), nc, base, st)
    if ctx.end(d_out.data_ptr(), st):
        for blk, nc, base in steps:
            ctx.rescan_step(blk.data_ptr(), nc, base, st)
        ctx.rescan_end(d_out.data_ptr(), st)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(knn.NB_DTYPE).reshape(mq, k)


def test_device_api_keep_zero_and_back(knn, int_data):
    """Context.set_keep_zero(True), q_base = m, two steps; then the flag off
    on the same context: a later search gives the excluded result"""
    import torch
    X, y, Q, ref = int_data
    m, n = X.shape
    mq, k, cap = len(Q), 30, 512
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    d_X, d_Q = torch.from_numpy(X).to(dev), torch.from_numpy(Q).to(dev)
    blocks, metas = [], []
    for r0, rows, bc, src in ((0, cap, cap, d_X), (cap, m - cap, cap, d_X), (0, mq, mq, d_Q)):
        b = torch.zeros(knn.block_bytes(bc, n), dtype=torch.uint8, device=dev)
        knn.block_pack(b.data_ptr(), bc, rows, n, src[r0:].data_ptr(), n, knn.ROWMAJOR, st)
        off = knn.block_meta_offset(bc, n)
        metas.append(b[off:off + 64].view(torch.float64))
        blocks.append(b)
    d_meta = torch.stack(metas).max(dim=0).values.contiguous()
    steps = [(blocks[0], cap, 0), (blocks[1], m - cap, cap)]
    ctx = knn.Context(0, mq, n, cap, k)
    try:
        ctx.set_keep_zero(True)
        got = _device_search(knn, ctx, blocks[2], mq, m, k, d_meta, steps)
        assert same(got, ref[True])
        ctx.set_keep_zero(False)
        got = _device_search(knn, ctx, blocks[2], mq, m, k, d_meta, steps)
        assert same(got, ref[False])
    finally:
        ctx.close()


@pytest.mark.parametrize("rule", [0, 1, 2])
def test_classify_device_on_queries(knn, int_data, rule):
    """knn_classify_device with q_base = m and the corpus labels followed by
    the query labels: classify_query's pred and matches"""
    import torch
    X, y, Q, ref = int_data
    m, mq = len(X), len(Q)
    yq = ((np.arange(mq) % 10) + 1).astype(np.float64)
    nb, _ = knn.query(X, Q, 30, keep_zero=True)
    pred_h, match_h = knn.classify_query(nb, y, yq, 10, rule)
    pred_r, match_r = vote_ref(nb, y, yq, 10, rule)
    assert np.array_equal(pred_h, pred_r) and match_h == match_r
    dev = torch.device("cuda", 0)
    d_nb = torch.from_numpy(np.ascontiguousarray(nb).view(np.uint8).reshape(-1).copy()).to(dev)
    d_lab = torch.from_numpy(np.concatenate([y, yq])).to(dev)
    d_pred = torch.full((mq,), -7, dtype=torch.int32, device=dev)
    d_match = torch.zeros(1, dtype=torch.int64, device=dev)
    knn.classify_device(d_nb.data_ptr(), mq, 30, 10, rule, d_lab.data_ptr(), m + mq, m,
                        d_pred.data_ptr(), d_match.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_pred.cpu().numpy(), pred_h) and int(d_match.item()) == match_h
