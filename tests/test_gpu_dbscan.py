"""knn_index_dbscan / mpiknn.Index.dbscan on the GPU: cluster, neighbours and
nclusters equal to the Python restatement (tests/dbscan_ref.py) and to the host
twin on the index's own epsilon-graph, on every path -- the int8 MFMA kernel
(long rows n = 784, short rows n = 128, n = 100), the exact scan on the same
integer data (KNN_NO_I8=1), on real-valued fp64 data and on an fp32 index -- at
a radius that is the one link between two clusters and at the double below it;
the duplicate groups alone at eps = 0; min_pts = 1; one cluster of everything
(every pair a union); all noise; more blocks than one launch takes; after a
remove / add / update lifecycle; device outputs; a query around a call; and the
memory the call keeps.

Shapes: M = 700 rows, KNN_QUERY_BLOCK=256 (three blocks, the last partial), as
the other index tests; tests/test_dbscan_cpu.py checks on the CPU that the
cases hold clusters, border rows, noise and a border row between two clusters."""
import numpy as np
import pytest

import dbscan_ref as D
import radius_ref as R
from dbscan_ref import M, case, same

pytestmark = pytest.mark.gpu

BLOCK = "256"
PATHS = [("mnist", {}), ("mnist", {"KNN_NO_I8": "1"}), ("sift", {}), ("n100", {}), ("real", {}), ("f32", {})]
PATH_IDS = ["mnist-i8", "mnist-scan", "sift-i8", "n100-i8", "real", "f32"]


@pytest.mark.parametrize("name,env", PATHS, ids=PATH_IDS)
def test_paths(knn, monkeypatch, name, env):
    c = case(name)
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with knn.Index(c.source(), dtype=c.dtype) as ix:
        assert ix.info().nblocks == 3
        for eps in (c.eps_at, c.eps_below):
            got = ix.dbscan(eps, c.min_pts, neighbours=True)
            assert same(got, c.ref(eps)), (name, eps)
            assert got.seconds > 0.0
            twin = knn.dbscan_graph(*ix.radius_rows(None, eps, keep_zero=True), c.min_pts)
            assert same(got, twin)
        assert ix.dbscan(c.eps_at, c.min_pts).neighbours is None


def test_byte_and_element_paths_agree(knn, monkeypatch):
    c = case("mnist")
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    with knn.Index(c.X) as ix:
        a = ix.dbscan(c.eps_at, c.min_pts, neighbours=True)
    monkeypatch.setenv("KNN_NO_I8", "1")
    with knn.Index(c.X) as ix:
        b = ix.dbscan(c.eps_at, c.min_pts, neighbours=True)
    assert same(a, b) and a.nclusters >= 3 and (a.cluster == 0).any()


@pytest.mark.parametrize("name,env", [("mnist", {}), ("mnist", {"KNN_NO_I8": "1"}), ("real", {})],
                         ids=["mnist-i8", "mnist-scan", "real"])
def test_edges_of_eps_and_min_pts(knn, monkeypatch, name, env):
    c = case(name)
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with knn.Index(c.source(), dtype=c.dtype) as ix:
        # eps = 0, min_pts = 2: the duplicate groups, and only they
        got = ix.dbscan(0.0, 2, neighbours=True)
        assert same(got, c.ref(0.0, 2)) and got.nclusters == len(c.trips) + 1
        assert (got.cluster > 0).sum() == 3 * len(c.trips) + R.GROUP
        # min_pts = 1: every row core, no noise
        got = ix.dbscan(c.eps_at, 1, neighbours=True)
        assert same(got, c.ref(c.eps_at, 1)) and (got.cluster > 0).all()
        # past the largest distance: one cluster of everything
        got = ix.dbscan(float(c.dd.max()), c.min_pts, neighbours=True)
        assert got.nclusters == 1 and (got.cluster == 1).all() and (got.neighbours == M).all()
        # min_pts past the largest neighbourhood: all noise
        got = ix.dbscan(c.eps_at, M + 1)
        assert got.nclusters == 0 and not got.cluster.any()


@pytest.mark.parametrize("env", [{}, {"KNN_NO_I8": "1"}], ids=["i8", "scan"])
def test_every_pair_a_union_and_all_noise(knn, monkeypatch, env):
    """4500 x 32 without duplicates (test_gpu_radius.py's corpus): with eps
    past the largest distance every pair of rows is a union, the contended
    case; with a very small eps every row is noise."""
    import datasets
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    X = datasets.sift_like(4500, n=32)
    assert len(np.unique(X, axis=0)) == len(X)
    with knn.Index(X) as ix:
        got = ix.dbscan(1e9, 5, neighbours=True)
        assert got.nclusters == 1 and (got.cluster == 1).all() and (got.neighbours == 4500).all()
        got = ix.dbscan(0.5, 2, neighbours=True)
        assert got.nclusters == 0 and not got.cluster.any() and (got.neighbours == 1).all()


@pytest.mark.parametrize("name,env", [("mnist", {}), ("mnist", {"KNN_NO_I8": "1"}), ("real", {})],
                         ids=["mnist-i8", "mnist-scan", "real"])
def test_more_blocks_than_a_launch(knn, monkeypatch, name, env):
    """KNN_QUERY_BLOCK=64: eleven blocks, two launches a query block and pass"""
    c = case(name)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("KNN_QUERY_BLOCK", "64")
    with knn.Index(c.source(), dtype=c.dtype) as ix:
        assert ix.info().nblocks == 11
        small = [ix.dbscan(eps, c.min_pts, neighbours=True) for eps in (c.eps_at, c.eps_below)]
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    with knn.Index(c.source(), dtype=c.dtype) as ix:
        for got, eps in zip(small, (c.eps_at, c.eps_below)):
            assert same(got, ix.dbscan(eps, c.min_pts, neighbours=True)) and same(got, c.ref(eps))


def test_after_remove_add_update(knn, monkeypatch):
    c = case("mnist")
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    X = c.X.copy()
    gone = np.array([3, 256, 257, 300, 640, int(c.at[D.A[3]]) + 1])
    with knn.Index(X[:650]) as ix:
        assert ix.remove(gone) == len(gone)
        ix.add(X[650:])
        X[9] = X[c.at[D.C[0]]]
        ix.update([10], X[9:10])
        live = np.setdiff1d(np.arange(1, M + 1), gone)
        d = R.distances(X[live - 1], X[live - 1])
        for eps in (c.eps_at, c.eps_below):
            want = D.dbscan_from(d, eps, c.min_pts, ids=live)
            got = ix.dbscan(eps, c.min_pts, neighbours=True)
            assert same(got, want) and want[2] >= 3
            ip, rec = ix.radius_rows(None, eps, keep_zero=True)
            assert same(got, knn.dbscan_graph(ip, rec, c.min_pts, ids=live))


def test_device_outputs(knn, monkeypatch):
    c = case("mnist")
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    with knn.Index(c.X) as ix:
        host = ix.dbscan(c.eps_at, c.min_pts, neighbours=True)
        dev = ix.dbscan(c.eps_at, c.min_pts, neighbours=True, device=True)
        assert dev.cluster.is_cuda and dev.neighbours.is_cuda and dev.nclusters == host.nclusters
        assert same((dev.cluster.cpu().numpy(), dev.neighbours.cpu().numpy(), dev.nclusters), host)
        dev = ix.dbscan(c.eps_at, c.min_pts, device=True)
        assert dev.neighbours is None and np.array_equal(dev.cluster.cpu().numpy(), host.cluster)
        for bad in (dict(eps=-1.0), dict(eps=float("nan")), dict(eps=float("inf")), dict(eps=1.0, min_pts=0)):
            with pytest.raises(knn.KnnError) as e:
                ix.dbscan(**bad)
            assert e.value.status == knn.ERR_INVALID


@pytest.mark.parametrize("env", [{}, {"KNN_NO_I8": "1"}], ids=["i8", "scan"])
def test_query_around_dbscan_and_memory(knn, monkeypatch, env):
    from query_ref import same as same_nb
    c = case("mnist")
    monkeypatch.setenv("KNN_QUERY_BLOCK", BLOCK)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    Q = R.case("mnist").Q
    with knn.Index(c.X) as ix:
        first, _ = ix.query(Q, 30)
        b0 = ix.info().device_bytes
        got = ix.dbscan(c.eps_at, c.min_pts)
        b1 = ix.info().device_bytes
        # less than one byte-form copy of the corpus, which a gather would need nine times over
        assert 0 < b1 - b0 < M * 784
        assert same(ix.dbscan(c.eps_below, c.min_pts), c.ref(c.eps_below))
        assert ix.info().device_bytes == b1
        again, _ = ix.query(Q, 30)
        assert ix.info().device_bytes == b1
    assert same(got, c.ref(c.eps_at)) and same_nb(first, again)
