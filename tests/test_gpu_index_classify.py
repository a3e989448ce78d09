"""knn_index_classify / knn_index_classify_rows (mpiknn.Index.classify,
classify_rows) on the GPU: the vote on the index's own labels, over records
that never leave the device.  Every comparison is exact: pred and matches
against the host vote (knn_classify_query / knn_classify, and the numpy
vote_ref of tests/query_ref.py) of the records query / neighbours return for
the same call, counts against a numpy histogram of those records' labels, the
reference's committed match counts, device outputs byte for byte against the
host ones."""
import json
import os

import numpy as np
import pytest

import datasets
from query_ref import query_ref, vote_ref

pytestmark = pytest.mark.gpu

K = 30
RULES = [0, 1, 2]   # SERIAL, MPI, MAJORITY
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def hist(rec, table, nclasses):
    """the labels of the records' idx (table: by id), counted a query"""
    idx = rec["idx"]
    table = np.asarray(table)
    out = np.zeros((idx.shape[0], nclasses), dtype=np.int32)
    ok = (idx > 0) & (idx <= len(table))
    lab = np.zeros(idx.shape, dtype=np.int64)
    lab[ok] = table[idx[ok] - 1].astype(np.int64)
    ok &= (lab >= 1) & (lab <= nclasses)
    np.add.at(out, (np.nonzero(ok)[0], lab[ok] - 1), 1)
    return out


@pytest.fixture(scope="module")
def split():
    """digits: rows 0..1499 a uint8 corpus with labels, the other 297 queries"""
    X, y = datasets.digits()
    return X[:1500].astype(np.uint8), y[:1500], X[1500:].astype(np.uint8), y[1500:]


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLD, "reference_runs.json")) as fh:
        return json.load(fh)


# ------------------------------------------------------- 1. host twin, int8

@pytest.mark.parametrize("kz", [True, False], ids=["keep0", "drop0"])
def test_host_twin_integer_path(knn, split, kz):
    Xc, yc, Q, yq = split
    with knn.Index(Xc, labels=yc) as ix:
        rec, _ = ix.query(Q, K, keep_zero=kz)
        for rule in RULES:
            want, hits = knn.classify_query(rec, yc, yq, 10, rule)
            res = ix.classify(Q, k=K, keep_zero=kz, qlabels=yq, nclasses=10, rule=rule, counts=True, neighbours=True)
            assert ix.info().last_bits == 8
            assert np.array_equal(res.pred, want) and res.matches == hits and hits > 200
            assert np.array_equal(res.pred, vote_ref(rec, yc, yq, 10, rule)[0])
            assert np.array_equal(res.counts, hist(rec, yc, 10))
            assert res.neighbours.tobytes() == rec.tobytes()   # (a host-out query fills .label too)
            assert res.seconds > 0
        none = ix.classify(Q, k=K, keep_zero=kz, nclasses=10)
        assert none.matches == 0 and none.counts is None and none.neighbours is None
        assert np.array_equal(none.pred, knn.classify_query(rec, yc, None, 10, 0)[0])


# ----------------------------------- 2. the reference's program on the index

def test_reference_program_on_the_index(knn, golden):
    X, y = datasets.digits()
    keys = ["matches_serial_rule", "matches_mpi_rule", "matches_true_majority"]
    ids = np.random.default_rng(3).permutation(len(X))[:301].astype(np.int32) + 1
    ids[-1] = ids[0]   # a repeat
    with knn.Index(X, labels=y) as ix:
        graph, _ = ix.neighbours(None, K, keep_zero=False)
        part, _ = ix.neighbours(ids, K, keep_zero=False)
        for rule, key in zip(RULES, keys):
            res = ix.classify_rows(None, k=K, keep_zero=False, nclasses=10, rule=rule, counts=True)
            want, hits = knn.classify(graph, y, 10, rule)
            assert res.matches == golden["digits"][key] == hits
            assert np.array_equal(res.pred, want)
            assert np.array_equal(res.counts, hist(graph, y, 10))
            res = ix.classify_rows(ids, k=K, keep_zero=False, nclasses=10, rule=rule, neighbours=True)
            want, hits = knn.classify_query(part, y, y[ids - 1], 10, rule)
            assert np.array_equal(res.pred, want) and res.matches == hits
            assert res.neighbours.tobytes() == part.tobytes()


# ------------------------------------------------------ 3. real-valued paths

def test_real_valued_f64_reference_count(knn, golden):
    X, y = datasets.digits_real()
    with knn.Index(X, labels=y) as ix:
        res = ix.classify_rows(None, k=K, keep_zero=False, nclasses=10, rule=knn.VOTE_SERIAL)
        assert res.matches == golden["digits_real"]["matches_serial_rule"] == 1631
        assert ix.info().last_bits > 8


def test_real_valued_f32_k100_majority(knn):
    """k = 100: two records on the first 36 lanes of the wave"""
    X, y = datasets.digits_real()
    Q = X[:300] + np.random.default_rng(11).normal(0.0, 1e-3, (300, X.shape[1]))
    with knn.Index(X, labels=y, dtype="f32") as ix:
        rec, _ = ix.query(Q, 100)
        want, hits = knn.classify_query(rec, y, y[:300], 10, knn.VOTE_MAJORITY)
        res = ix.classify(Q, k=100, qlabels=y[:300], nclasses=10, rule=knn.VOTE_MAJORITY, counts=True)
        assert np.array_equal(res.pred, want) and res.matches == hits
        assert np.array_equal(res.counts, hist(rec, y, 10)) and (res.counts.sum(axis=1) == 100).all()


# ------------------------------------ 4. after mutations (stale label copy)

def test_after_add_remove_update(knn, split, monkeypatch):
    monkeypatch.setenv("KNN_QUERY_BLOCK", "256")
    Xc, yc, Qall, yqall = split
    Q, yq = Qall[64:], yqall[64:]
    with knn.Index(Xc, labels=yc) as ix:
        assert ix.info().nblocks == 6
        rec0, _ = ix.query(Q, K)
        before = {rule: ix.classify(Q, k=K, qlabels=yq, nclasses=10, rule=rule) for rule in RULES}   # the labels' copy exists
        for rule in RULES:
            assert np.array_equal(before[rule].pred, knn.classify_query(rec0, yc, yq, 10, rule)[0])
        # the host state, by id
        rows = {i + 1: Xc[i].copy() for i in range(1500)}
        table = np.concatenate([yc, yqall[:64]])
        assert ix.add(Qall[:64], labels=yqall[:64]) == 1501
        for i in range(64):
            rows[1501 + i] = Qall[i].copy()
        gone = np.arange(5, 1500, 37)   # 41 ids, in every block but the added rows'
        near = [int(i) for i in rec0["idx"][0] if i not in set(gone.tolist())][:16]   # query 0's nearest rows
        assert len(near) == 16 and ix.remove(gone) == len(gone)
        for i in gone:
            del rows[int(i)]
        # 16 rows move next to query 0 and take a label that is not its own
        wrong = float(int(yq[0]) % 10 + 1)
        Xu = np.repeat(Q[:1], 16, axis=0)
        Xu[np.arange(16), np.arange(16)] ^= 1
        old = table.copy()
        ix.update(near, Xu, labels=np.full(16, wrong))
        for j, i in enumerate(near):
            rows[i] = Xu[j]
            table[i - 1] = wrong
        assert ix.last_id == len(table) == 1564 and ix.info().m == len(rows)
        # on the CPU: the records, and that this choice flips query 0's
        # majority -- with the labels as they were it would not
        live = np.array(sorted(rows))
        exp = query_ref(np.array([rows[i] for i in live], dtype=np.float64), Q, K, True)
        exp["idx"] = np.where(exp["idx"] > 0, live[exp["idx"] - 1], 0)
        rec, _ = ix.query(Q, K)
        assert np.array_equal(rec["idx"], exp["idx"])
        assert set(near) <= set(exp["idx"][0].tolist())
        for rule in RULES:
            want, hits = vote_ref(exp, table, yq, 10, rule)
            if rule == knn.VOTE_MAJORITY:   # 16 of 30 votes; the other two rules compare counts with labels (F7)
                assert want[0] == wrong != before[rule].pred[0]
                assert vote_ref(exp[:1], old, None, 10, rule)[0][0] != wrong
            res = ix.classify(Q, k=K, qlabels=yq, nclasses=10, rule=rule, counts=True)
            assert np.array_equal(res.pred, want) and res.matches == hits
            twin, twin_hits = knn.classify_query(rec, table, yq, 10, rule)
            assert np.array_equal(res.pred, twin) and res.matches == twin_hits
            assert np.array_equal(res.counts, hist(exp, table, 10))
        # the rows call on the mutated index: own labels through the id map
        graph, _ = ix.neighbours(None, K)
        res = ix.classify_rows(None, k=K, nclasses=10, rule=knn.VOTE_MAJORITY)
        want, hits = vote_ref(graph, table, table[live - 1], 10, 2)
        assert np.array_equal(res.pred, want) and res.matches == hits


# ------------------------------------------------------------------ 5. edges

def test_tiny_index_empty_slots_and_stray_labels(knn):
    """5 rows at k = 8: empty slots; labels 0 and nclasses + 1 are counted by nobody"""
    rng = np.random.default_rng(2)
    X = rng.normal(size=(5, 4))
    y = np.array([0.0, 11.0, 1.0, 2.0, 2.0])
    for mq in (1, 37):
        Q = rng.normal(size=(mq, 4))
        with knn.Index(X, labels=y) as ix:
            rec, _ = ix.query(Q, 8)
            assert (rec["idx"][:, 5:] == 0).all()
            for nclasses in (1, 10, 1024):
                for rule in RULES:
                    res = ix.classify(Q, k=8, qlabels=np.full(mq, 2.0), nclasses=nclasses, rule=rule, counts=True,
                                      neighbours=True)
                    want, hits = vote_ref(rec, y, np.full(mq, 2.0), nclasses, rule)
                    assert np.array_equal(res.pred, want) and res.matches == hits
                    assert np.array_equal(res.pred, knn.classify_query(rec, y, None, nclasses, rule)[0])
                    assert res.counts.shape == (mq, nclasses) and np.array_equal(res.counts, hist(rec, y, nclasses))
                    assert res.counts.sum(axis=1).max() <= 5
                    assert res.neighbours.tobytes() == rec.tobytes()
            own, _ = ix.neighbours(None, 8)
            res = ix.classify_rows(None, k=8, nclasses=10, counts=True)
            want, hits = vote_ref(own, y, y, 10, 0)
            assert np.array_equal(res.pred, want) and res.matches == hits
            assert np.array_equal(res.counts, hist(own, y, 10)) and res.counts.sum(axis=1).max() <= 4


def test_three_tiles(knn, split, monkeypatch):
    """mq = 37 in tiles of 16: one vote over three tiles' records; 37 is no multiple of the four waves"""
    monkeypatch.setenv("KNN_QUERY_TILE", "16")
    Xc, yc, Q, yq = split
    with knn.Index(Xc[:300], labels=yc[:300]) as ix:
        rec, _ = ix.query(Q[:37], K)
        for rule in RULES:
            res = ix.classify(Q[:37], k=K, qlabels=yq[:37], nclasses=10, rule=rule, counts=True)
            want, hits = knn.classify_query(rec, yc[:300], yq[:37], 10, rule)
            assert np.array_equal(res.pred, want) and res.matches == hits
            assert np.array_equal(res.counts, hist(rec, yc[:300], 10))


def test_built_tie(knn):
    """k = 4, classes 2 and 3 at 2-2, the nearest neighbour in class 3: SERIAL
    gives the tie to the nearest's label, MPI to that label minus one (blk:265)
    which is the other class, MAJORITY to the tied label met first"""
    X = np.array([[1.0, 0.0], [2.0, 0.0], [3.0, 0.0], [4.0, 0.0]])
    y = np.array([3.0, 2.0, 2.0, 3.0])
    Q = np.array([[0.0, 0.0]])
    with knn.Index(X, labels=y) as ix:
        rec, _ = ix.query(Q, 4)
        assert rec["idx"].tolist() == [[1, 2, 3, 4]]
        got = []
        for rule in RULES:
            res = ix.classify(Q, k=4, qlabels=[3.0], nclasses=3, rule=rule, counts=True)
            assert res.counts.tolist() == [[0, 2, 2]]
            assert res.pred[0] == vote_ref(rec, y, None, 3, rule)[0][0] == knn.classify_query(rec, y, None, 3, rule)[0][0]
            assert res.matches == int(res.pred[0] == 3)
            got.append(int(res.pred[0]))
        assert got == [3, 2, 3]


# --------------------------------------------------------- 6. device outputs

def test_device_outputs(knn, split):
    import torch
    Xc, yc, Q, yq = split
    with knn.Index(Xc, labels=yc) as ix:
        host = ix.classify(Q, k=K, qlabels=yq, nclasses=10, counts=True, neighbours=True)
        for src in (Q, torch.from_numpy(Q).to("cuda:0")):
            buf = torch.zeros(len(Q) * K * 16, dtype=torch.uint8, device="cuda:0")
            dev = ix.classify(src, k=K, qlabels=yq, nclasses=10, counts=True, out=buf)
            assert dev.neighbours is buf and dev.pred.is_cuda and dev.counts.is_cuda
            assert dev.pred.dtype == torch.int32 and tuple(dev.counts.shape) == (len(Q), 10)
            assert dev.matches == host.matches
            assert np.array_equal(dev.pred.cpu().numpy(), host.pred)
            assert np.array_equal(dev.counts.cpu().numpy(), host.counts)
            assert buf.cpu().numpy().tobytes() == host.neighbours.tobytes()
        ids = np.array([7, 1500, 3, 7], dtype=np.int32)
        host = ix.classify_rows(ids, k=K, nclasses=10, counts=True, neighbours=True)
        buf = torch.zeros(len(ids) * K * 16, dtype=torch.uint8, device="cuda:0")
        dev = ix.classify_rows(ids, k=K, nclasses=10, counts=True, out=buf)
        assert dev.matches == host.matches and np.array_equal(dev.pred.cpu().numpy(), host.pred)
        assert np.array_equal(dev.counts.cpu().numpy(), host.counts)
        assert buf.cpu().numpy().tobytes() == host.neighbours.tobytes()
        assert (host.neighbours["label"] > 0).all()


# --------------------------------------------------------------- 7. refusals

def test_refusals_leave_the_index_answering(knn, split):
    Xc, yc, Q, yq = split
    Q = Q[:20]

    def refused(status, call):
        with pytest.raises(knn.KnnError) as e:
            call()
        assert e.value.status == status

    with knn.Index(Xc[:400]) as bare:
        ref, _ = bare.query(Q, K)
        refused(knn.ERR_INVALID, lambda: bare.classify(Q, k=K))
        refused(knn.ERR_INVALID, lambda: bare.classify_rows(None, k=K))
        assert bare.query(Q, K)[0].tobytes() == ref.tobytes()
    with knn.Index(Xc[:400].astype(np.float64), labels=yc[:400]) as ix:
        assert ix.remove([9]) == 1
        ref, _ = ix.query(Q, K)
        for status, call in [
                (knn.ERR_INVALID, lambda: ix.classify(Q, k=K, nclasses=0)),
                (knn.ERR_INVALID, lambda: ix.classify(Q, k=K, rule=3)),
                (knn.ERR_INVALID, lambda: ix.classify_rows([9], k=K)),
                (knn.ERR_INVALID, lambda: ix.classify_rows([401], k=K)),
                (knn.ERR_UNSUPPORTED, lambda: ix.classify(Q, k=K, nclasses=1025)),
                (knn.ERR_UNSUPPORTED, lambda: ix.classify(Q, k=33)),
                (knn.ERR_UNSUPPORTED, lambda: ix.classify_rows(None, k=32, keep_zero=True))]:
            refused(status, call)
            assert ix.query(Q, K)[0].tobytes() == ref.tobytes()
        assert ix.classify_rows(None, k=32, keep_zero=False).pred.shape == (399,)


# -------------------------------------------------------- 8. untouched paths

def test_query_and_neighbours_untouched_and_device_bytes(knn, split):
    Xc, yc, Q, yq = split
    with knn.Index(Xc, labels=yc) as ix, knn.Index(Xc, labels=yc) as twin:
        # twin: the same calls with query in classify's place -- what the
        # engine holds depends on the batches it has seen, the same on both
        for each in (ix, twin):
            rec, _ = each.query(Q, K)
            own, _ = each.neighbours([1, 2, 3], K, keep_zero=False)
        assert ix.info().device_bytes == twin.info().device_bytes
        ix.classify(Q, k=K, qlabels=yq, nclasses=10, counts=True, neighbours=True)
        twin.query(Q, K)
        # the labels' copy, and nothing that grows with the batch beyond query's own
        assert ix.info().device_bytes == twin.info().device_bytes + 1500 * 8
        assert ix.query(Q, K)[0].tobytes() == rec.tobytes()
        assert ix.neighbours([1, 2, 3], K, keep_zero=False)[0].tobytes() == own.tobytes()
        twin.query(Q, K)
        twin.neighbours([1, 2, 3], K, keep_zero=False)
        ix.classify(Q[:50], k=K, nclasses=10, counts=True)
        twin.query(Q[:50], K)
        assert ix.info().device_bytes == twin.info().device_bytes + 1500 * 8
        ix.classify_rows(None, k=K, keep_zero=False, nclasses=10, counts=True)
        twin.neighbours(None, K, keep_zero=False)
        assert ix.info().device_bytes == twin.info().device_bytes + 1500 * 8
