"""knn_index_classify_weighted / knn_index_regress and their _rows forms
(mpiknn.Index.classify_weighted, classify_weighted_rows, regress,
regress_rows) on the GPU: the distance-weighted vote and the regression over
records that never leave the device.  Every comparison is exact: pred, sums
and the regression's values bit for bit against the host twins
(knn_classify_weighted / knn_regress) applied to the records query /
neighbours return for the same call with the index's labels by id, and
against the plain-Python restatement in tests/predict_ref.py."""
import numpy as np
import pytest

from predict_ref import DISTANCE, UNIFORM, bits, classify_weighted_ref, regress_ref

pytestmark = pytest.mark.gpu

WEIGHTS = [UNIFORM, DISTANCE]


def same_vote(knn, res, rec, table, qlabels, nclasses, weights):
    """res: a WeightedResult with sums, against both yardsticks on records rec"""
    pred, sums, hits = knn.classify_weighted(rec, table, qlabels, nclasses, weights)
    rpred, rsums, rhits = classify_weighted_ref(rec, table, qlabels, nclasses, weights)
    assert np.array_equal(pred, rpred) and np.array_equal(bits(sums), bits(rsums)) and hits == rhits
    assert np.array_equal(res.pred, pred)
    assert res.sums.shape == (len(rec), nclasses) and np.array_equal(bits(res.sums), bits(sums))
    assert res.matches == (hits if qlabels is not None else 0)


def same_mean(knn, res, rec, targets, weights):
    pred = knn.regress(rec, targets, weights)
    assert np.array_equal(bits(pred), bits(regress_ref(rec, targets, weights)))
    assert res.pred.dtype == np.float64 and np.array_equal(bits(res.pred), bits(pred))


def make(rng, m, n, kind, mq=37, copies=5):
    """corpus, queries (the first `copies` exact copies of corpus rows), class labels 1..10, real targets"""
    if kind == "u8":
        X = rng.integers(0, 256, (m, n)).astype(np.uint8)
        Q = rng.integers(0, 256, (mq, n)).astype(np.uint8)
    else:
        X = rng.normal(0.0, 1.0, (m, n)).astype(kind)
        Q = rng.normal(0.0, 1.0, (mq, n)).astype(kind)
    Q[:copies] = X[rng.permutation(m)[:copies]]
    y = rng.integers(1, 11, m).astype(np.float64)
    t = rng.normal(-1.5, 20.0, m)
    return X, Q, y, t


def check_queries(knn, X, Q, y, t, k, dtype, bits_are_8):
    rng = np.random.default_rng(5)
    yq = rng.integers(1, 11, len(Q)).astype(np.float64)
    with knn.Index(X, labels=y, dtype=dtype) as ix, knn.Index(X, labels=t, dtype=dtype) as rx:
        for kz in (True, False):
            rec, _ = ix.query(Q, k, keep_zero=kz)
            zeros = int((rec["distance"][:, 0] == 0.0).sum())
            if bits_are_8:   # integer distances: the copies, and only under the keep-zero rule, are exact matches
                assert zeros == (5 if kz else 0)
            for weights in WEIGHTS:
                res = ix.classify_weighted(Q, k=k, keep_zero=kz, qlabels=yq, nclasses=10, weights=weights, sums=True,
                                           neighbours=True)
                assert (ix.info().last_bits == 8) == bits_are_8
                same_vote(knn, res, rec, y, yq, 10, weights)
                assert res.neighbours.tobytes() == rec.tobytes() and res.seconds > 0
                if weights == UNIFORM:
                    assert (res.sums.sum(axis=1) == k).all()
                bare = ix.classify_weighted(Q, k=k, keep_zero=kz, nclasses=10, weights=weights)
                assert bare.sums is None and bare.neighbours is None and bare.matches == 0
                assert np.array_equal(bare.pred, res.pred)
                out = rx.regress(Q, k=k, keep_zero=kz, weights=weights, neighbours=True)
                same_mean(knn, out, rec, t, weights)
                assert np.array_equal(out.neighbours["idx"], rec["idx"]) and (out.neighbours["label"] == 0).all()
                assert np.array_equal(bits(rx.regress(Q, k=k, keep_zero=kz, weights=weights).pred), bits(out.pred))
                if kz and weights == DISTANCE and zeros:   # an exact match decides
                    hit = rec["distance"][:, 0] == 0.0
                    first = rec["idx"][hit, 0] - 1
                    assert np.array_equal(res.pred[hit], y[first].astype(np.int32))
                    assert (res.sums[hit].sum(axis=1) == (rec["distance"][hit] == 0.0).sum(axis=1)).all()


# --------------------------------------------------------------- 1. byte path

def test_byte_path(knn):
    X, Q, y, t = make(np.random.default_rng(1), 400, 16, "u8")
    check_queries(knn, X, Q, y, t, 7, "f64", True)


# ----------------------------------------------------------- 2. element paths

def test_element_path_f32_k100(knn):
    """k = 100: more than one record a lane"""
    X, Q, y, t = make(np.random.default_rng(2), 300, 24, np.float32)
    check_queries(knn, X, Q, y, t, 100, "f32", False)


def test_element_path_f64_k30(knn):
    X, Q, y, t = make(np.random.default_rng(3), 300, 24, np.float64)
    check_queries(knn, X, Q, y, t, 30, "f64", False)


# ------------------------------------------------------------ 3. rows variants

@pytest.mark.parametrize("kz", [False, True], ids=["drop0", "keep0"])
def test_rows(knn, kz):
    """ids=None and a shuffled list with a repeat; keep0: rows 11 and 200 are
    an exact duplicate pair, so each finds the other at distance 0 through the
    k + 1 search"""
    rng = np.random.default_rng(4)
    X, _, y, t = make(rng, 400, 16, "u8")
    X[199] = X[10]
    y[199] = y[10] % 10 + 1   # the duplicate is of another class
    ids = (rng.permutation(400)[:41] + 1).astype(np.int32)
    ids[-1] = ids[0]
    ids[1], ids[2] = 11, 200
    k = 7
    with knn.Index(X, labels=y) as ix, knn.Index(X, labels=t) as rx:
        for lst in (None, ids):
            rec, _ = ix.neighbours(lst, k, keep_zero=kz)
            own = y if lst is None else y[lst - 1]
            if kz:
                at = {11: 200, 200: 11}
                for row, (r, i) in enumerate(zip(rec, range(1, 401) if lst is None else lst)):
                    if int(i) in at:
                        assert r["distance"][0] == 0.0 and r["idx"][0] == at[int(i)]
                    assert int(i) not in r["idx"]
            for weights in WEIGHTS:
                res = ix.classify_weighted_rows(lst, k=k, keep_zero=kz, nclasses=10, weights=weights, sums=True,
                                                neighbours=True)
                same_vote(knn, res, rec, y, own, 10, weights)
                assert res.neighbours.tobytes() == rec.tobytes()
                out = rx.regress_rows(lst, k=k, keep_zero=kz, weights=weights)
                same_mean(knn, out, rec, t, weights)
                if kz and weights == DISTANCE and lst is not None:
                    assert res.pred[1] == int(y[199]) and res.pred[2] == int(y[10])
                    assert out.pred[1] == t[199] and out.pred[2] == t[10]


# ------------------------------------------------------------------- 4. edges

def test_tiny_index_empty_slots(knn):
    """5 rows at k = 8: three empty slots a query; nclasses 1 and 1024; labels 0 and 1025 are nobody's"""
    rng = np.random.default_rng(6)
    X = rng.integers(0, 50, (5, 4)).astype(np.float64)   # integers: a copy is at distance exactly 0
    y = np.array([0.0, 1025.0, 1.0, 700.0, 700.0])
    Q = rng.integers(0, 50, (9, 4)).astype(np.float64)
    Q[0] = X[3]
    with knn.Index(X, labels=y) as ix:
        rec, _ = ix.query(Q, 8)
        assert (rec["idx"][:, 5:] == 0).all() and (rec["idx"][:, :5] > 0).all() and rec["distance"][0, 0] == 0.0
        for nclasses in (1, 1024):
            for weights in WEIGHTS:
                res = ix.classify_weighted(Q, k=8, qlabels=np.full(9, 700.0), nclasses=nclasses, weights=weights,
                                           sums=True, neighbours=True)
                same_vote(knn, res, rec, y, np.full(9, 700.0), nclasses, weights)
                assert res.neighbours.tobytes() == rec.tobytes()
                # query 0's exact match is of class 700: with one class it is counted by nobody and,
                # weighted by distance, leaves the others no weight either
                assert res.pred[0] == (700 if nclasses == 1024 else 0 if weights == DISTANCE else 1)
                assert set(res.pred[1:].tolist()) <= ({1} if nclasses == 1 else {1, 700})
        for weights in WEIGHTS:
            same_mean(knn, ix.regress(Q, k=8, weights=weights), rec, y, weights)
            own, _ = ix.neighbours(None, 8)
            same_mean(knn, ix.regress_rows(None, k=8, weights=weights), own, y, weights)
            same_vote(knn, ix.classify_weighted_rows(None, k=8, nclasses=1024, weights=weights, sums=True), own, y, y,
                      1024, weights)


def test_three_tiles(knn, monkeypatch):
    """mq = 37 in tiles of 16: one vote over three tiles' records; 37 is no multiple of the four waves"""
    monkeypatch.setenv("KNN_QUERY_TILE", "16")
    X, Q, y, t = make(np.random.default_rng(7), 300, 16, "u8")
    with knn.Index(X, labels=y) as ix, knn.Index(X, labels=t) as rx:
        rec, _ = ix.query(Q, 7)
        for weights in WEIGHTS:
            res = ix.classify_weighted(Q, k=7, qlabels=y[:37], nclasses=10, weights=weights, sums=True)
            same_vote(knn, res, rec, y, y[:37], 10, weights)
            same_mean(knn, rx.regress(Q, k=7, weights=weights), rec, t, weights)


# ------------------------------------------ 5. after mutations (stale labels)

def test_after_add_remove_update(knn):
    rng = np.random.default_rng(8)
    X, Q, y, _ = make(rng, 400, 16, "u8")
    k = 7
    with knn.Index(X, labels=y) as ix:
        rec0, _ = ix.query(Q, k)
        first = ix.classify_weighted(Q, k=k, nclasses=10, sums=True)   # the labels' device copy exists from here on
        same_vote(knn, first, rec0, y, None, 10, DISTANCE)
        Xa = rng.integers(0, 256, (20, 16)).astype(np.uint8)
        ya = rng.integers(1, 11, 20).astype(np.float64)
        assert ix.add(Xa, labels=ya) == 401
        table = np.concatenate([y, ya])
        gone = np.unique(np.concatenate([np.arange(3, 400, 29), rec0["idx"][6, :2]]))
        assert ix.remove(gone) == len(gone)
        live = np.setdiff1d(np.arange(1, 421), gone)
        # rows near query 5 get query 5's own values and a label of their own: exact matches of a new class
        near = [int(i) for i in rec0["idx"][5] if i not in set(gone.tolist())][:3]
        new = float(int(y[near[0] - 1]) % 10 + 1)
        ix.update(near, np.repeat(Q[5:6], 3, axis=0), labels=np.full(3, new))
        table[np.array(near) - 1] = new
        assert ix.last_id == 420 and ix.info().m == len(live)
        rec, _ = ix.query(Q, k)
        assert not np.isin(rec["idx"], gone).any() and (rec["distance"][5, :3] == 0.0).all()
        assert sorted(rec["idx"][5, :3].tolist()) == sorted(near)
        yq = rng.integers(1, 11, len(Q)).astype(np.float64)
        for weights in WEIGHTS:
            res = ix.classify_weighted(Q, k=k, qlabels=yq, nclasses=10, weights=weights, sums=True)
            same_vote(knn, res, rec, table, yq, 10, weights)
            same_mean(knn, ix.regress(Q, k=k, weights=weights), rec, table, weights)
        assert res.pred[5] == int(new) and res.sums[5, int(new) - 1] == 3.0 and res.sums[5].sum() == 3.0
        # the rows calls on the mutated index: own labels through the id map
        graph, _ = ix.neighbours(None, k)
        for weights in WEIGHTS:
            res = ix.classify_weighted_rows(None, k=k, nclasses=10, weights=weights, sums=True)
            same_vote(knn, res, graph, table, table[live - 1], 10, weights)
            same_mean(knn, ix.regress_rows(None, k=k, weights=weights), graph, table, weights)


# ---------------------------------------------------------- 6. device outputs

def test_device_outputs(knn):
    import torch
    X, Q, y, t = make(np.random.default_rng(9), 400, 16, "u8")
    k = 7
    ids = np.array([7, 400, 3, 7], dtype=np.int32)
    with knn.Index(X, labels=y) as ix:
        host = ix.classify_weighted(Q, k=k, qlabels=y[:37], nclasses=10, sums=True, neighbours=True)
        for src in (Q, torch.from_numpy(Q).to("cuda:0")):
            buf = torch.zeros(len(Q) * k * 16, dtype=torch.uint8, device="cuda:0")
            dev = ix.classify_weighted(src, k=k, qlabels=y[:37], nclasses=10, sums=True, out=buf)
            assert dev.neighbours is buf and dev.pred.is_cuda and dev.sums.is_cuda
            assert dev.pred.dtype == torch.int32 and dev.sums.dtype == torch.float64
            assert tuple(dev.sums.shape) == (len(Q), 10) and dev.matches == host.matches
            assert np.array_equal(dev.pred.cpu().numpy(), host.pred)
            assert np.array_equal(bits(dev.sums.cpu().numpy()), bits(host.sums))
            assert buf.cpu().numpy().tobytes() == host.neighbours.tobytes()
        assert (host.neighbours["label"] > 0).all()
        host = ix.classify_weighted_rows(ids, k=k, nclasses=10, sums=True, neighbours=True)
        buf = torch.zeros(len(ids) * k * 16, dtype=torch.uint8, device="cuda:0")
        dev = ix.classify_weighted_rows(ids, k=k, nclasses=10, sums=True, out=buf)
        assert dev.matches == host.matches and np.array_equal(dev.pred.cpu().numpy(), host.pred)
        assert np.array_equal(bits(dev.sums.cpu().numpy()), bits(host.sums))
        assert buf.cpu().numpy().tobytes() == host.neighbours.tobytes()
        assert (host.neighbours["label"] > 0).all()
    with knn.Index(X, labels=t) as rx:
        host = rx.regress(Q, k=k, weights=DISTANCE, neighbours=True)
        buf = torch.zeros(len(Q) * k * 16, dtype=torch.uint8, device="cuda:0")
        dev = rx.regress(Q, k=k, weights=DISTANCE, out=buf)
        assert dev.neighbours is buf and dev.pred.is_cuda and dev.pred.dtype == torch.float64
        assert np.array_equal(bits(dev.pred.cpu().numpy()), bits(host.pred))
        assert buf.cpu().numpy().tobytes() == host.neighbours.tobytes()
        host = rx.regress_rows(ids, k=k, neighbours=True)
        buf = torch.zeros(len(ids) * k * 16, dtype=torch.uint8, device="cuda:0")
        dev = rx.regress_rows(ids, k=k, out=buf)
        assert np.array_equal(bits(dev.pred.cpu().numpy()), bits(host.pred))
        assert buf.cpu().numpy().tobytes() == host.neighbours.tobytes()


# ---------------------------------------------------------------- 7. refusals

def test_refusals_leave_the_index_answering(knn):
    X, Q, y, _ = make(np.random.default_rng(10), 400, 16, "u8")
    k = 7

    def refused(status, call):
        with pytest.raises(knn.KnnError) as e:
            call()
        assert e.value.status == status

    with knn.Index(X) as bare:
        ref, _ = bare.query(Q, k)
        for call in (lambda: bare.classify_weighted(Q, k=k), lambda: bare.classify_weighted_rows(None, k=k),
                     lambda: bare.regress(Q, k=k), lambda: bare.regress_rows(None, k=k)):
            refused(knn.ERR_INVALID, call)
            assert bare.query(Q, k)[0].tobytes() == ref.tobytes()
    with knn.Index(X.astype(np.float64), labels=y) as ix:   # fp64: k <= 32
        ref, _ = ix.query(Q, k)
        vote = ix.classify(Q, k=k, nclasses=10, counts=True)
        for status, call in [
                (knn.ERR_INVALID, lambda: ix.classify_weighted(Q, k=k, weights=2)),
                (knn.ERR_INVALID, lambda: ix.classify_weighted_rows(None, k=k, weights=-1)),
                (knn.ERR_INVALID, lambda: ix.regress(Q, k=k, weights=2)),
                (knn.ERR_INVALID, lambda: ix.regress_rows([3], k=k, weights=7)),
                (knn.ERR_INVALID, lambda: ix.classify_weighted(Q, k=k, nclasses=0)),
                (knn.ERR_INVALID, lambda: ix.classify_weighted_rows(None, k=k, nclasses=0)),
                (knn.ERR_UNSUPPORTED, lambda: ix.classify_weighted(Q, k=k, nclasses=1025, sums=True)),
                (knn.ERR_UNSUPPORTED, lambda: ix.classify_weighted_rows(None, k=k, nclasses=1025)),
                (knn.ERR_UNSUPPORTED, lambda: ix.classify_weighted(Q, k=33)),
                (knn.ERR_UNSUPPORTED, lambda: ix.regress(Q, k=33)),
                (knn.ERR_UNSUPPORTED, lambda: ix.classify_weighted_rows(None, k=32, keep_zero=True)),
                (knn.ERR_UNSUPPORTED, lambda: ix.regress_rows(None, k=32, keep_zero=True)),
                (knn.ERR_INVALID, lambda: ix.classify_weighted_rows([401], k=k)),
                (knn.ERR_INVALID, lambda: ix.regress_rows([0], k=k))]:
            refused(status, call)
            assert ix.query(Q, k)[0].tobytes() == ref.tobytes()
            again = ix.classify(Q, k=k, nclasses=10, counts=True)
            assert np.array_equal(again.pred, vote.pred) and np.array_equal(again.counts, vote.counts)
        assert ix.classify_weighted_rows(None, k=32, keep_zero=False).pred.shape == (400,)
        assert ix.regress_rows(None, k=32, keep_zero=False).pred.shape == (400,)


# --------------------------------------------------------- 8. untouched paths

def test_existing_calls_untouched_and_device_bytes(knn):
    X, Q, y, _ = make(np.random.default_rng(11), 400, 16, "u8")
    k = 7
    ids = np.array([5, 17, 400, 5], dtype=np.int32)

    def existing(ix):
        rec, _ = ix.query(Q, k)
        a = ix.classify(Q, k=k, qlabels=y[:37], nclasses=10, rule=knn.VOTE_MAJORITY, counts=True, neighbours=True)
        b = ix.classify_rows(ids, k=k, keep_zero=False, nclasses=10, counts=True, neighbours=True)
        c = ix.classify_rows(None, k=k, keep_zero=False, nclasses=10)
        return [rec.tobytes(), a.pred.tobytes(), a.counts.tobytes(), a.neighbours.tobytes(), a.matches,
                b.pred.tobytes(), b.counts.tobytes(), b.neighbours.tobytes(), b.matches, c.pred.tobytes(), c.matches]

    with knn.Index(X, labels=y) as ix:
        before = existing(ix)
        held = ix.info().device_bytes
        for weights in WEIGHTS:
            ix.regress(Q, k=k, weights=weights, neighbours=True)
            ix.classify_weighted(Q, k=k, qlabels=y[:37], nclasses=10, weights=weights, sums=True, neighbours=True)
            ix.regress_rows(ids, k=k, keep_zero=False, weights=weights)
            ix.classify_weighted_rows(ids, k=k, keep_zero=False, nclasses=1024, weights=weights, sums=True)
            ix.classify_weighted_rows(None, k=k, keep_zero=False, nclasses=10, weights=weights, sums=True)
            assert ix.info().device_bytes == held   # the new vote's buffers live for the call
        assert existing(ix) == before
        assert ix.info().device_bytes == held
