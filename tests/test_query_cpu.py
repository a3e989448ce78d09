"""Out-of-sample queries without a GPU: the numpy restatement (query_ref.py)
against the oracle's block fold, knn_query's argument checks (all before any
device call), and knn_classify_query against a numpy vote."""
import ctypes

import numpy as np
import pytest

import datasets
from query_ref import query_ref, same, vote_ref


@pytest.fixture(scope="module")
def digits_split():
    X, y = datasets.digits()
    return X[:1500], y[:1500], X[1500:], y[1500:]


@pytest.fixture(scope="module")
def ref_excluded(digits_split):
    X, y, Q, _ = digits_split
    return query_ref(X, Q, 30, keep_zero=False, labels=y)


def test_restatement_equals_oracle_fold(oracle, digits_split, ref_excluded):
    """zeros dropped: oracle.knn_block folded over two corpus blocks"""
    X, y, Q, _ = digits_split
    L = oracle.lists_init(len(Q), 30)
    oracle.knn_block(Q, 1500, X[:800], 0, L)
    oracle.knn_block(Q, 1500, X[800:], 800, L)
    assert same(L, ref_excluded)


def test_restatement_keep_zero():
    """a query equal to corpus rows 2 and 5: both lead its list at distance
    0.0, lower idx first; excluded, neither appears"""
    X = np.arange(40, dtype=np.float64).reshape(8, 5) % 7
    X[5] = X[2]
    Q = X[[2]]
    keep = query_ref(X, Q, 4, keep_zero=True)
    assert list(keep["idx"][0, :2]) == [3, 6] and list(keep["distance"][0, :2]) == [0.0, 0.0]
    drop = query_ref(X, Q, 4, keep_zero=False)
    assert 3 not in drop["idx"][0] and 6 not in drop["idx"][0] and (drop["distance"][0] > 0).all()


def _raw_query(knn, X, m, Q, mq, n, layout, k, dtype, flags, out):
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    return knn.lib.knn_query(p(X), m, p(Q), mq, n, layout, None, k, dtype, flags, p(out))


def test_query_argument_checks(knn):
    """each bad argument returns its status with no device present (the
    checks come before any device call)"""
    X, Q = np.ones((5, 3)), np.ones((2, 3))
    out = np.zeros((2, 2), dtype=knn.NB_DTYPE)
    ok = dict(X=X, m=5, Q=Q, mq=2, n=3, layout=knn.ROWMAJOR, k=2, dtype=knn.F64, flags=0, out=out)

    def call(**kw):
        a = dict(ok, **kw)
        return _raw_query(knn, a["X"], a["m"], a["Q"], a["mq"], a["n"], a["layout"], a["k"], a["dtype"],
                          a["flags"], a["out"])

    assert call(X=None) == knn.ERR_INVALID
    assert call(Q=None) == knn.ERR_INVALID
    assert call(out=None) == knn.ERR_INVALID
    assert call(m=0) == knn.ERR_INVALID
    assert call(mq=0) == knn.ERR_INVALID
    assert call(n=0) == knn.ERR_INVALID
    assert call(k=0) == knn.ERR_INVALID
    assert call(k=-3) == knn.ERR_INVALID
    assert call(k=knn.MAX_K + 1) == knn.ERR_UNSUPPORTED
    assert call(k=knn.MAX_K_F32 + 1, dtype=knn.F32) == knn.ERR_UNSUPPORTED
    assert call(layout=2) == knn.ERR_INVALID
    assert call(dtype=7) == knn.ERR_UNSUPPORTED
    assert call(flags=2) == knn.ERR_INVALID
    assert call(flags=knn.QUERY_KEEP_ZERO | 4) == knn.ERR_INVALID


def test_query_no_device(knn):
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("GPU present")
    except ImportError:
        pass
    with pytest.raises(knn.KnnError) as e:
        knn.query(np.ones((5, 3)), np.ones((2, 3)), 2)
    assert e.value.status == knn.ERR_NODEVICE


@pytest.mark.parametrize("rule", [0, 1, 2])
@pytest.mark.parametrize("with_qlabels", [True, False])
def test_classify_query(knn, digits_split, ref_excluded, rule, with_qlabels):
    _, y, _, yq = digits_split
    ql = yq if with_qlabels else None
    pred, matches = knn.classify_query(ref_excluded, y, ql, 10, rule)
    pred_r, matches_r = vote_ref(ref_excluded, y, ql, 10, rule)
    assert np.array_equal(pred, pred_r) and matches == matches_r
    if not with_qlabels:
        assert matches == 0
    elif rule == 0:
        assert matches > 250   # the vote means something: digits classify well


def test_classify_query_empty_slots(knn):
    # fewer than k neighbours: idx 0 slots are skipped, and so is an idx past
    # the corpus labels (as knn_classify_device counts ids > nlabels)
    nb = np.zeros((3, 4), dtype=knn.NB_DTYPE)
    nb["idx"] = [[2, 0, 0, 0], [1, 0, 0, 0], [9, 2, 0, 0]]
    labels = np.array([3.0, 5.0])
    pred, m = knn.classify_query(nb, labels, np.array([5.0, 1.0, 5.0]), 10, knn.VOTE_SERIAL)
    assert list(pred) == [5, 3, 5] and m == 2
    pred_r, m_r = vote_ref(nb, labels, np.array([5.0, 1.0, 5.0]), 10, knn.VOTE_SERIAL)
    assert list(pred) == list(pred_r) and m == m_r
