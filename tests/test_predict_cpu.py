"""knn_classify_weighted / knn_regress (mpiknn.classify_weighted, regress): the
host twins of the index's weighted vote and regression, on built records,
against the plain-Python restatement in tests/predict_ref.py.  sums and the
regression's pred are compared bit for bit.  No device is touched."""
import ctypes

import numpy as np
import pytest

from predict_ref import DISTANCE, UNIFORM, bits, classify_weighted_ref, regress_ref

WEIGHTS = [UNIFORM, DISTANCE]
INF = np.inf


def records(rows):
    """(mq, k) records from rows of (distance, idx) pairs"""
    nb = np.zeros((len(rows), len(rows[0])), dtype=[("distance", "<f8"), ("idx", "<i4"), ("label", "<i4")])
    for q, row in enumerate(rows):
        for i, (d, idx) in enumerate(row):
            nb[q, i] = (d, idx, 0)
    return nb


def random_records(rng, mq, k, nlabels, zero_every=0):
    """ascending random distances over random ids; every zero_every-th query starts with a zero distance"""
    nb = np.zeros((mq, k), dtype=[("distance", "<f8"), ("idx", "<i4"), ("label", "<i4")])
    nb["distance"] = np.sort(rng.uniform(0.05, 40.0, (mq, k)), axis=1)
    nb["idx"] = rng.integers(1, nlabels + 1, (mq, k))
    if zero_every:
        nb["distance"][::zero_every, 0] = 0.0
    return nb


def check_classify(knn, nb, labels, qlabels, nclasses, weights):
    pred, sums, hits = knn.classify_weighted(nb, labels, qlabels, nclasses, weights)
    rpred, rsums, rhits = classify_weighted_ref(nb, labels, qlabels, nclasses, weights)
    assert np.array_equal(pred, rpred)
    assert np.array_equal(bits(sums), bits(rsums))
    assert hits == rhits
    return pred, sums, hits


def check_regress(knn, nb, targets, weights):
    pred = knn.regress(nb, targets, weights)
    assert np.array_equal(bits(pred), bits(regress_ref(nb, targets, weights)))
    return pred


@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("nclasses", [1, 10, 1024])
@pytest.mark.parametrize("k", [1, 8, 128])
def test_random_lists(knn, k, nclasses, weights):
    rng = np.random.default_rng(1000 * k + nclasses)
    nlabels = 300
    labels = rng.integers(1, nclasses + 1, nlabels).astype(np.float64)
    nb = random_records(rng, 12, k, nlabels, zero_every=5)
    qlabels = rng.integers(1, nclasses + 1, 12).astype(np.float64)
    pred, sums, _ = check_classify(knn, nb, labels, qlabels, nclasses, weights)
    assert (pred >= 1).all()
    if weights == UNIFORM:
        assert (sums.sum(axis=1) == k).all()
    else:   # the exact match decides: the zero-distance queries carry weight 1 a zero record, nothing else
        assert (sums[::5].sum(axis=1) == 1.0).all() and (pred[::5] == labels[nb["idx"][::5, 0] - 1]).all()
    targets = rng.normal(0.0, 3.0, nlabels)
    check_regress(knn, nb, targets, weights)


@pytest.mark.parametrize("weights", WEIGHTS)
def test_empty_slots_and_stray_ids_and_labels(knn, weights):
    labels = np.array([0.0, 11.0, 1.0, 2.0, 2.0])   # nclasses 10: labels 0 and nclasses + 1 are nobody's
    nb = records([
        [(1.0, 3), (2.0, 1), (3.0, 2), (INF, 0), (INF, 0)],      # empty slots at the tail, labels 0 and 11
        [(INF, 0), (INF, 0), (INF, 0), (INF, 0), (INF, 0)],      # only empty slots
        [(1.0, 6), (2.0, 4), (2.5, -3), (3.0, 99), (4.0, 5)],    # ids past nlabels (and a negative one)
        [(1.0, 1), (2.0, 2), (INF, 0), (INF, 0), (INF, 0)],      # neighbours, but none is counted
    ])
    pred, sums, hits = check_classify(knn, nb, labels, np.array([1.0, 0.0, 2.0, 0.0]), 10, weights)
    assert pred.tolist() == [1, 0, 2, 0] and hits == 4
    assert sums[1].sum() == 0 and sums[3].sum() == 0
    assert sums[2, 1] == (2.0 if weights == UNIFORM else 0.5 + 0.25)
    out = check_regress(knn, nb, labels, weights)
    assert np.isnan(out[1]) and not np.isnan(out[[0, 2, 3]]).any()
    assert out[2] == 2.0


def test_zero_distance_decides(knn):
    """two zero-distance records of different classes: the first in record
    order wins, and the farther records weigh nothing"""
    labels = np.array([4.0, 7.0, 7.0, 7.0, 7.0])
    nb = records([[(0.0, 1), (0.0, 2), (0.5, 3), (0.5, 4), (0.75, 5)]])
    pred, sums, _ = check_classify(knn, nb, labels, None, 10, DISTANCE)
    assert pred.tolist() == [4]
    assert sums[0, 3] == 1.0 and sums[0, 6] == 1.0 and sums.sum() == 2.0
    pred, sums, _ = check_classify(knn, nb, labels, None, 10, UNIFORM)
    assert pred.tolist() == [7] and sums[0, 6] == 4.0
    targets = np.array([10.0, 20.0, -1e6, 1e6, 3.25])
    assert check_regress(knn, nb, targets, DISTANCE)[0] == 15.0
    # a zero distance in an empty or stray slot is no match
    nb = records([[(0.0, 0), (0.0, 9), (0.5, 3), (1.0, 1)]])
    pred, sums, _ = check_classify(knn, nb, labels, None, 10, DISTANCE)
    assert pred.tolist() == [7] and sums[0, 6] == 2.0 and sums[0, 3] == 1.0


def test_built_weighted_tie(knn):
    """classes 2 and 3 at 1/0.5 + 1/1 = 1/0.4 + 1/2 = 3 exactly: the class met first wins"""
    labels = np.array([3.0, 2.0, 2.0, 3.0])
    nb = records([[(0.4, 1), (0.5, 2), (1.0, 3), (2.0, 4)]])
    pred, sums, _ = check_classify(knn, nb, labels, None, 3, DISTANCE)
    assert sums[0].tolist() == [0.0, 3.0, 3.0] and pred.tolist() == [3]
    nb["idx"] = [[2, 1, 4, 3]]   # the same weights with class 2 met first
    pred, sums, _ = check_classify(knn, nb, labels, None, 3, DISTANCE)
    assert sums[0].tolist() == [0.0, 3.0, 3.0] and pred.tolist() == [2]
    pred, sums, _ = check_classify(knn, nb, labels, None, 3, UNIFORM)
    assert sums[0].tolist() == [0.0, 2.0, 2.0] and pred.tolist() == [2]


def test_uniform_and_distance_differ(knn):
    """one near neighbour of class 1, two far ones of class 2"""
    labels = np.array([1.0, 2.0, 2.0])
    nb = records([[(0.1, 1), (5.0, 2), (6.0, 3)]])
    pred, _, hits = check_classify(knn, nb, labels, np.array([1.0]), 2, DISTANCE)
    assert pred.tolist() == [1] and hits == 1
    pred, _, hits = check_classify(knn, nb, labels, np.array([1.0]), 2, UNIFORM)
    assert pred.tolist() == [2] and hits == 0
    targets = np.array([-8.0, 1.0, 1.0])
    uni, dist = check_regress(knn, nb, targets, UNIFORM)[0], check_regress(knn, nb, targets, DISTANCE)[0]
    assert uni == -2.0 and dist < -7.0


@pytest.mark.parametrize("weights", WEIGHTS)
def test_regression_targets(knn, weights):
    """negative and non-integer targets; a NaN target propagates"""
    rng = np.random.default_rng(9)
    targets = rng.normal(-2.5, 100.0, 200)
    nb = random_records(rng, 20, 30, 200, zero_every=7)
    pred = check_regress(knn, nb, targets, weights)
    assert np.isfinite(pred).all() and (pred < 0).any() and (pred != np.round(pred)).all()
    targets[nb["idx"][3, 10] - 1] = np.nan
    pred = check_regress(knn, nb, targets, weights)
    assert np.isnan(pred[3]) and np.isfinite(pred).sum() >= 10
    # the products are rounded on their own: a fused multiply-add would show here
    nb = records([[(3.0, 1), (7.0, 2), (11.0, 3)]])
    check_regress(knn, nb, np.array([1.0 / 3.0, 1e16 + 2.0, -1e16]), weights)


def test_refusals(knn):
    lib = knn.lib
    nb = records([[(1.0, 1), (2.0, 2)]])
    labels = np.array([1.0, 2.0])
    pred, dpred = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.float64)
    sums = np.zeros((1, 10))
    hit = ctypes.c_size_t()
    P = knn._ptr

    def classify(nbp=P(nb), k=2, nclasses=10, weights=1, lab=P(labels), nlabels=2):
        return lib.knn_classify_weighted(nbp, 1, k, nclasses, weights, lab, nlabels, None, P(pred), P(sums),
                                         ctypes.byref(hit))

    def regress(nbp=P(nb), k=2, weights=1, tg=P(labels), ntargets=2, out=P(dpred)):
        return lib.knn_regress(nbp, 1, k, weights, tg, ntargets, out)

    assert classify() == knn.OK and regress() == knn.OK
    for bad in (dict(nbp=None), dict(lab=None), dict(k=0), dict(k=-1), dict(nclasses=0), dict(nclasses=-5),
                dict(weights=2), dict(weights=-1), dict(nlabels=0)):
        assert classify(**bad) == knn.ERR_INVALID, bad
    for bad in (dict(nbp=None), dict(tg=None), dict(k=0), dict(weights=2), dict(weights=-1), dict(ntargets=0),
                dict(out=None)):
        assert regress(**bad) == knn.ERR_INVALID, bad
    # pred, sums and matches of the vote are optional
    assert lib.knn_classify_weighted(P(nb), 1, 2, 10, 1, P(labels), 2, None, None, None, None) == knn.OK
    with pytest.raises(knn.KnnError) as e:
        knn.classify_weighted(nb, labels, weights=7)
    assert e.value.status == knn.ERR_INVALID
    with pytest.raises(knn.KnnError):
        knn.regress(nb, labels, weights=7)
    assert (knn.WEIGHT_UNIFORM, knn.WEIGHT_DISTANCE) == (UNIFORM, DISTANCE)
