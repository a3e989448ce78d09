"""The distance-weighted vote and kNN regression, restated in plain Python: the
yardstick for knn_classify_weighted / knn_regress (knn_vote.c) and for the
kernels behind Index.classify_weighted / Index.regress (knn_predict.hip).

Explicit loops over numpy float64 scalars: every quotient, product and sum is
one IEEE operation in record order (np.sum adds pairwise and is not used), so
the results can be compared bit for bit.  include/knn.h has the definition.
"""
import numpy as np

UNIFORM, DISTANCE = 0, 1
QNAN = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]   # the positive quiet NaN


def _valid(rec, nlabels):
    return 1 <= int(rec["idx"]) <= nlabels


def _weights(L, nlabels, weights):
    """w of every record of one query (None: not valid)"""
    valid = [_valid(r, nlabels) for r in L]
    if weights == UNIFORM:
        return [np.float64(1.0) if v else None for v in valid]
    assert weights == DISTANCE
    dist = [np.float64(r["distance"]) for r in L]
    if any(v and d == 0.0 for v, d in zip(valid, dist)):
        return [(np.float64(1.0) if d == 0.0 else np.float64(0.0)) if v else None for v, d in zip(valid, dist)]
    with np.errstate(all="ignore"):
        return [np.float64(1.0) / d if v else None for v, d in zip(valid, dist)]


def classify_weighted_ref(nb, labels, qlabels, nclasses, weights):
    """(pred int32 (mq,), sums float64 (mq, nclasses), matches)"""
    labels = np.asarray(labels, dtype=np.float64)
    mq, k = nb.shape
    pred = np.zeros(mq, dtype=np.int32)
    sums = np.zeros((mq, nclasses), dtype=np.float64)
    hit = 0
    for q in range(mq):
        L = nb[q]
        w = _weights(L, len(labels), weights)
        lab = [0] * k
        for i in range(k):
            if w[i] is None:
                continue
            c = int(labels[int(L[i]["idx"]) - 1])
            if 1 <= c <= nclasses:
                lab[i] = c
                with np.errstate(all="ignore"):
                    sums[q, c - 1] = sums[q, c - 1] + w[i]
        best = np.float64(0.0)
        for j in range(nclasses):
            if sums[q, j] > best:
                best = sums[q, j]
        most = 0
        if best > 0.0:
            for i in range(k):
                if lab[i] and sums[q, lab[i] - 1] == best:
                    most = lab[i]
                    break
        pred[q] = most
        if qlabels is not None and most == qlabels[q]:
            hit += 1
    return pred, sums, hit


def regress_ref(nb, targets, weights):
    """pred float64 (mq,)"""
    targets = np.asarray(targets, dtype=np.float64)
    mq, k = nb.shape
    pred = np.zeros(mq, dtype=np.float64)
    for q in range(mq):
        L = nb[q]
        w = _weights(L, len(targets), weights)
        num, den, seen = np.float64(0.0), np.float64(0.0), False
        with np.errstate(all="ignore"):
            for i in range(k):
                if w[i] is None:
                    continue
                p = w[i] * targets[int(L[i]["idx"]) - 1]
                num = num + p
                den = den + w[i]
                seen = True
            pred[q] = num / den if seen else QNAN
    return pred


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
