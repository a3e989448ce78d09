"""numpy / Python restatement of DBSCAN as include/knn.h defines it
(knn_index_dbscan, knn_dbscan_graph), from radius_ref.distances, and the cases
tests/test_dbscan_cpu.py (which checks that they are worth testing with) and
tests/test_gpu_dbscan.py share.

The definition, literally: N(x) = the number of rows y with d(x, y) <= eps, x
and its duplicates included; core: N(x) >= min_pts; clusters: the connected
components of the core rows under d <= eps, by a plain union-find over the
boolean hit matrix, numbered 1 .. C in ascending order of their lowest
position; a row that is not core takes the cluster of its nearest core
neighbour by (distance, id); everything else is 0.  Nothing here calls the
library.

A case is radius_ref's corpus of the same name (M = 700 rows: rows that occur
three times -- never core at min_pts = 5 -- and one group of 34 identical rows
spread over all three blocks of 256, core at eps = 0) with 36 rows replaced by
a planted figure: copies of one base row that differ in two coordinates only,
by the offsets below times a unit (1 on integer data; 1/64 around 0.5 on real
data, where every offset, difference and squared sum is exact in fp32 and
fp64), so that the distance of two planted rows is the distance of their
offsets, exactly.

      v = 43          P                      (9, 43): sqrt(90) from C's end AND D's end
      v = 40  C C C C C C C C . . . D D D D D D D D        C: u = -7 .. 0, D: u = 18 .. 25
      v = 10              E                  (3, 10): 10 from A's (3, 0) alone
      v =  0          A A A A A A A A . . . B B B B B B B B   A: u = 0 .. 7, B: u = 17 .. 24

At eps_at = 10 units -- read from the reference distances: the distance of
A's end (7, 0) and B's end (17, 0), both core, the only pair that links A and
B -- the clusters are A + B, C, D and the duplicate group; at eps_below, the
double below it, A and B are two clusters.  P is a border row whose two
nearest core neighbours, at equal distances, lie in C and in D: the lower id
decides.  E is a border row at the radius exactly, and noise below it.  The
rest of the corpus is noise at this radius."""
import functools

import numpy as np

import radius_ref as R

M = R.M
MIN_PTS = 5

A = [(u, 0) for u in range(0, 8)]
B = [(u, 0) for u in range(17, 25)]
C = [(u, 40) for u in range(-7, 1)]
D = [(u, 40) for u in range(18, 26)]
P = (9, 43)
E = (3, 10)
FIGURE = A + B + C + D + [P, E]


def dbscan_from(d, eps, min_pts, ids=None):
    """(cluster int32, neighbours int32, nclusters) of the m x m distance
    matrix d (live rows by position); ids: their ids, ascending (None:
    position + 1)"""
    m = len(d)
    ids = np.arange(1, m + 1) if ids is None else np.asarray(ids)
    hit = np.isfinite(d) & (d <= eps)
    nbr = hit.sum(axis=1).astype(np.int32)          # the row itself: d = 0 <= eps
    core = nbr >= min_pts
    parent = list(range(m))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for x, y in np.argwhere(np.triu(hit & core[:, None] & core[None, :], 1)).tolist():
        a, b = find(x), find(y)
        if a != b:
            parent[max(a, b)] = min(a, b)           # a root is its component's lowest position
    cluster = np.zeros(m, dtype=np.int32)
    number = {}
    for x in range(m):
        if core[x]:
            cluster[x] = number.setdefault(find(x), len(number) + 1)
    for x in np.flatnonzero(~core):
        cand = np.flatnonzero(hit[x] & core)
        if len(cand):
            cluster[x] = cluster[cand[np.lexsort((ids[cand], d[x][cand]))[0]]]
    return cluster, nbr, len(number)


def same(got, want):
    """a DbscanResult (or a triple) against dbscan_from's triple"""
    return (np.array_equal(got[0], want[0]) and got[0].dtype == np.int32 and
            (got[1] is None or (np.array_equal(got[1], want[1]) and got[1].dtype == np.int32)) and
            got[2] == want[2])


class Case:
    def __init__(self, name):
        c = R.case(name)
        self.name, self.dtype, self.group, self.trips = name, c.dtype, c.group, c.trips
        self.integer = name in ("mnist", "sift", "n100")
        X = c.X.copy()
        free = np.setdiff1d(np.arange(M), np.concatenate([c.trips.reshape(-1), c.group]))
        self.rows = np.random.default_rng(33).choice(free, len(FIGURE), replace=False)
        base = X[free[0]].copy()
        unit, origin = (1.0, 128.0) if self.integer else (1.0 / 64, 0.5)
        for row, (u, v) in zip(self.rows, FIGURE):
            X[row] = base
            X[row, 0] = origin + u * unit
            X[row, 1] = origin + v * unit
        self.X = X
        self.min_pts = MIN_PTS
        self.at = dict(zip(FIGURE, self.rows.tolist()))          # offset -> position
        self.eps_at = float(self.dd[self.at[A[-1]], self.at[B[0]]])
        self.eps_below = float(np.nextafter(self.eps_at, 0.0))

    @functools.cached_property
    def dd(self):
        return R.distances(self.X, self.X, self.dtype)

    @functools.lru_cache(None)
    def ref(self, eps, min_pts=None):
        out = dbscan_from(self.dd, eps, self.min_pts if min_pts is None else min_pts)
        for a in out[:2]:
            a.setflags(write=False)
        return out

    def rows_ref(self, eps, keep_zero=True):
        """the epsilon-graph in CSR, as knn_index_radius_rows(ids = NULL) gives it"""
        return R.radius_from(self.dd, eps, keep_zero, self_pos=np.arange(M))

    def source(self):
        """what the index is made from: bytes for the integer cases"""
        return self.X.astype(np.uint8) if self.integer else self.X


@functools.lru_cache(None)
def case(name):
    return Case(name)


CASES = list(R.CASES)
