"""numpy restatement of the out-of-sample query semantics (knn_query,
include/knn.h): for every query row the k nearest corpus rows by
(sqrt(S), idx), S = sum_j (q_j - x_j)^2 accumulated in j order in fp64 --
elementwise numpy operations only, so no FMA and no pairwise summation --
zero distances optionally dropped (the reference's rule, blk:217-242), empty
slots {inf, 0, 0}.  Shared by test_query_cpu.py (which pins it to the oracle's
block fold) and test_gpu_query.py."""
import numpy as np

NB_DTYPE = np.dtype([("distance", "<f8"), ("idx", "<i4"), ("label", "<i4")])


def query_ref(X, Q, k, keep_zero, labels=None, dtype="f64"):
    X = np.asarray(X, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    if dtype == "f32":
        X = X.astype(np.float32).astype(np.float64)
        Q = Q.astype(np.float32).astype(np.float64)
    m, n = X.shape
    mq = Q.shape[0]
    S = np.zeros((mq, m), dtype=np.float64)
    for j in range(n):
        t = Q[:, j, None] - X[None, :, j]
        S += t * t
    d = np.sqrt(S)
    out = np.zeros((mq, k), dtype=NB_DTYPE)
    out["distance"] = np.inf
    ids = np.arange(m)
    for q in range(mq):
        ok = np.isfinite(d[q]) if keep_zero else (np.isfinite(d[q]) & (d[q] != 0.0))
        cand = ids[ok]
        order = np.lexsort((cand, d[q][cand]))[:k]
        sel = cand[order]
        out["distance"][q, :len(sel)] = d[q][sel]
        out["idx"][q, :len(sel)] = sel + 1
        if labels is not None:
            out["label"][q, :len(sel)] = np.asarray(labels)[sel].astype(np.int32)
    return out


def same(a, b):
    """exact: idx equal and distance equal bit for bit, every row"""
    return (np.array_equal(a["idx"], b["idx"]) and
            np.array_equal(np.ascontiguousarray(a["distance"]).view(np.uint64),
                           np.ascontiguousarray(b["distance"]).view(np.uint64)))


def vote_ref(nb, labels, qlabels, nclasses, rule):
    """ten-line numpy vote: rule 0 SERIAL, 1 MPI, 2 MAJORITY (knn_vote.c)"""
    labels = np.asarray(labels)
    pred = np.zeros(nb.shape[0], dtype=np.int32)
    for q, row in enumerate(nb["idx"]):
        labs = [int(labels[i - 1]) for i in row if 0 < i <= len(labels)]
        labs = [v for v in labs if 1 <= v <= nclasses]
        cnt = np.bincount(labs, minlength=nclasses + 1)[1:] if labs else np.zeros(nclasses, dtype=int)
        if rule == 2:
            pred[q] = next((v for v in labs if cnt[v - 1] == cnt.max()), 0) if labs else 0
            continue
        nn0 = int(labels[row[0] - 1]) if 0 < row[0] <= len(labels) else 0
        tie, most = (nn0 - 1 if rule == 1 else nn0), 0
        for j in range(nclasses):
            if cnt[j] > most or (cnt[j] == most and j + 1 == tie):
                most = j + 1
        pred[q] = most
    matches = 0 if qlabels is None else int((pred == np.asarray(qlabels)).sum())
    return pred, matches
