"""numpy restatement of radius search (knn_index_radius*, include/knn.h), and
the corpora, queries and radii tests/test_radius_cpu.py (which checks that the
radii are worth testing with) and tests/test_gpu_radius.py share.

query_ref.py's arithmetic: S = sum_j (q_j - x_j)^2 accumulated in j order in
fp64 by elementwise numpy operations (no FMA, no pairwise summation), over the
fp32-rounded values for dtype "f32"; a hit is a row with sqrt(S) <= r, finite;
a zero distance is a hit only under keep_zero; a query that is a resident row
(self_pos) never hits itself; each query's hits by (distance, id)."""
import functools

import numpy as np

import datasets
from query_ref import NB_DTYPE

M = 700
GROUP = 34


def distances(X, Q, dtype="f64"):
    X = np.asarray(X, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    if dtype == "f32":
        X = X.astype(np.float32).astype(np.float64)
        Q = Q.astype(np.float32).astype(np.float64)
    S = np.zeros((Q.shape[0], X.shape[0]), dtype=np.float64)
    for j in range(X.shape[1]):
        t = Q[:, j, None] - X[None, :, j]
        S += t * t
    return np.sqrt(S)


def radius_from(d, r, keep_zero, ids=None, self_pos=None, labels=None, start=0):
    """(counts int32, indptr int64, records) of the distance matrix d (query x
    live row position); ids: the live rows' ids, ascending (None: position +
    1); self_pos: query q is the row at position self_pos[q]; labels: by id"""
    mq, m = d.shape
    ids = np.arange(1, m + 1) if ids is None else np.asarray(ids)
    hit = np.isfinite(d) & (d <= r)
    if not keep_zero:
        hit &= d != 0.0
    if self_pos is not None:
        hit[np.arange(mq), np.asarray(self_pos)] = False
    counts = hit.sum(axis=1).astype(np.int32)
    indptr = np.zeros(mq + 1, dtype=np.int64)
    np.cumsum(counts, out=indptr[1:])
    rec = np.zeros(int(indptr[-1]), dtype=NB_DTYPE)
    for q in range(mq):
        cand = np.flatnonzero(hit[q])
        sel = cand[np.lexsort((ids[cand], d[q][cand]))]
        seg = rec[indptr[q]:indptr[q + 1]]
        seg["distance"] = d[q][sel]
        seg["idx"] = ids[sel]
        if labels is not None:
            seg["label"] = np.asarray(labels)[ids[sel] - 1].astype(np.int32)
    return counts, indptr + start, rec


def radius_ref(X, Q, r, keep_zero, dtype="f64", **kw):
    return radius_from(distances(X, Q, dtype), r, keep_zero, **kw)


def same(got, want):
    """counts, indptr, idx and distance bits, all equal"""
    return (np.array_equal(got[0], want[0]) and got[0].dtype == np.int32 and
            np.array_equal(got[1], want[1]) and
            np.array_equal(got[2]["idx"], want[2]["idx"]) and
            np.array_equal(np.ascontiguousarray(got[2]["distance"]).view(np.uint64),
                           np.ascontiguousarray(want[2]["distance"]).view(np.uint64)))


def with_copies(X, nq, fresh, seed=5):
    """test_gpu_index_neighbours.py's make_queries restated: corpus rows that
    occur three times, and queries that are fresh rows, single rows and
    tripled rows; then one group of GROUP identical rows in every block of 256"""
    X = X.copy()
    m = len(X)
    rng = np.random.default_rng(seed)
    ncopy = (nq - len(fresh)) // 2
    rows = rng.permutation(m)
    single, trip = rows[:ncopy], rows[ncopy:2 * ncopy]
    a, b = rows[2 * ncopy:3 * ncopy], rows[3 * ncopy:4 * ncopy]
    X[a] = X[trip]
    X[b] = X[trip]
    trips = np.stack([trip, a, b], axis=1)
    free = np.setdiff1d(np.arange(m), np.concatenate([trips.reshape(-1), single]))
    group = np.sort(np.random.default_rng(21).choice(free, GROUP, replace=False))
    assert group[0] < 256 and group[-1] >= 512
    X[group] = X[group[0]]
    Q = np.vstack([fresh, X[single], X[trip]])
    return X, Q, trips, group


class Case:
    """a corpus X (M rows), queries Q (fresh rows, one of them far from
    everything; single rows; tripled rows), the reference distances, and two
    radii taken from them: r_at, the NTH smallest distance of the query that
    has the smallest one -- that query has >= NTH hits, one of them at r_at
    exactly -- and r_below, the double below r_at: the row at r_at is then at
    the next representable distance above the radius, and no hit."""
    NTH = 100

    def __init__(self, X, fresh, dtype="f64", far=255.0):
        fresh = fresh.copy()
        fresh[0] = far                                   # nothing lies near this query
        self.X, self.Q, self.trips, self.group = with_copies(X, 24 + len(fresh), fresh)
        self.dtype = dtype
        self.d = distances(self.X, self.Q, dtype)
        kth = np.sort(np.where(self.d > 0.0, self.d, np.inf), axis=1)[:, self.NTH - 1]
        self.q_many = int(np.argmin(kth))
        self.r_at = float(kth[self.q_many])
        self.r_below = float(np.nextafter(self.r_at, 0.0))
        self.labels = (np.arange(len(self.X)) % 10 + 1).astype(np.float64)

    def ref(self, r, keep_zero, **kw):
        return radius_from(self.d, r, keep_zero, **kw)

    @functools.cached_property
    def dd(self):
        """the corpus against itself: the rows forms' distances"""
        return distances(self.X, self.X, self.dtype)

    def rows_ref(self, r, keep_zero, pos=None, **kw):
        pos = np.arange(len(self.X)) if pos is None else np.asarray(pos)
        return radius_from(self.dd[pos], r, keep_zero, self_pos=pos, **kw)


@functools.lru_cache(None)
def case(name):
    if name == "mnist":        # n = 784: the long-row norm encoding
        X, _ = datasets.mnist_like(M)
        F, _ = datasets.mnist_like(40, seed=77)
        return Case(X, F)
    if name == "sift":         # n = 128: the short-row encoding
        return Case(datasets.sift_like(M), datasets.sift_like(40, seed=0x77))
    if name == "n100":         # padding past n inside the last 32-byte K-step
        X, _ = datasets.mnist_like(M, n=100)
        F, _ = datasets.mnist_like(40, n=100, seed=77)
        return Case(X, F)
    if name == "real":         # real-valued fp64: the element path
        X, _ = datasets.mnist_real(M)
        F, _ = datasets.mnist_real(40, seed=77)
        return Case(X, F, far=1.0)
    if name == "f32":          # the same values on an fp32 index
        X, _ = datasets.mnist_real(M)
        F, _ = datasets.mnist_real(40, seed=77)
        return Case(X, F, dtype="f32", far=1.0)
    raise KeyError(name)


CASES = ["mnist", "sift", "n100", "real", "f32"]
