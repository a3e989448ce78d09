"""The int8 kernel's tile epilogue (knn_i8.hip: the first extraction round,
the second-survivor test i8_second32, the rounds after it and the merges
between them), on planted data.

A lane's 32 candidates of a 64-row tile are rows 32 b + 8 j + 4 h + i (b < 2,
j < 4, i < 4) for one h, in slot 16 b + 4 j + i; slots 3 s .. 3 s + 2 are one
first-level triple of the max tree.  Every case takes integer rows in 0..255,
one query (row Q, not in the first tile) and near-copies of it -- the query
with one feature moved by delta, d^2 = delta^2 -- planted in chosen slots of
one lane class of one tile, so that this lane meets 2, 3, 8 or 13 survivors
in that tile: in one triple, in two triples, in two m-blocks, tied, next to
the query's own (masked) slot, in the last partial tile, or with an exact
duplicate among them.  Random rows lie at d^2 of about n 10^4, so the planted
ones are the query's nearest.

Before the GPU runs, each case proves from the oracle's own answer (k = 30,
the query alone) what it exercises: the planted rows are in the answer, each
in the intended tile, lane class and slot, at least the intended number of
them, and no other row is nearer than the farthest planted one.  At k = 3 the
same proof holds for k = 30 and the query's three nearest are planted rows:
the lane still meets every planted row under the open bound its split starts
from, and the merge in the middle of the tile then closes it.  The exact
duplicate (d^2 = 0) is dropped under the default zero rule, so the proof
takes it as absent from the answer.

Then the whole result is compared with the oracle bit for bit, as check() of
test_gpu_i8.py does."""
import functools

import numpy as np
import pytest

from test_gpu_h16 import run_engine

pytestmark = pytest.mark.gpu

M = 1500          # 23 whole tiles and one of 28 rows; 12 query blocks of 128
Q = 700           # tile 10 (rows 640..703), local row 60: b 1, j 3, h 1, i 0 -- slot 28
NS = (40, 200, 400, 784, 896)   # 2, 7, 13, 25, 28 K-steps: the buckets 4, 8, 16, 25, 28


def row_of(tile, h, slot):
    return 64 * tile + 32 * (slot >> 4) + 8 * ((slot >> 2) & 3) + 4 * h + (slot & 3)


def place_of(row):
    """(tile, h, slot) of a corpus row."""
    loc = row & 63
    b, w = loc >> 5, loc & 31
    return row >> 6, (w >> 2) & 1, 16 * b + 4 * (w >> 3) + (w & 3)


# case: (tile, lane class h, [(slot, delta), ...], intended survivors);
# delta 0 is an exact duplicate of the query
CASES = {
    # two and three survivors inside one triple (slots 3..5, 6..8)
    "two_in_triple": (5, 1, [(3, 2), (4, 3)], 2),
    "three_in_triple": (5, 1, [(6, 3), (7, 1), (8, 2)], 3),
    # two survivors in different triples of one m-block (triples 0 and 3)
    "two_triples": (5, 1, [(1, 2), (10, 3)], 2),
    # two survivors in different m-blocks (slot 5: b 0, slot 21: b 1)
    "two_mblocks": (5, 1, [(5, 3), (21, 2)], 2),
    # equal d^2: one pair inside a triple (slots 9, 10), one across triples
    # (slots 14, 20, also across m-blocks); at k = 3 the third neighbour is
    # the lower row of the second pair
    "ties": (5, 1, [(9, 2), (10, 2), (14, 3), (20, 3)], 4),
    # more survivors than a buffer holds (5 entries, 6 at 25 K-steps): the
    # merge lands in the middle of the tile; the ties (delta 5, and 4 of the
    # thirteen) sit on both sides of the 5th and of the 6th survivor
    "eight": (5, 1, [(0, 1), (31, 2), (12, 3), (17, 4), (2, 5), (18, 5), (29, 5), (7, 6)], 8),
    "thirteen": (5, 1, [(30, 1), (4, 2), (13, 3), (14, 4), (22, 4), (3, 4), (9, 4), (25, 5), (10, 5),
                        (19, 6), (0, 6), (27, 7), (16, 8)], 13),
    # the query's own tile and lane: slot 28 is the query (masked); 27 and 29
    # share its triple, 30 and 24 sit in the triples beside it
    "diagonal": (10, 1, [(27, 2), (29, 1), (30, 3), (24, 2)], 4),
    # the last tile, 28 rows: of lane class 0 the slots 0..15 exist
    "partial_tile": (23, 0, [(0, 2), (1, 3), (7, 1), (13, 2)], 4),
    # an exact duplicate of the query among the survivors of one triple
    "duplicate": (5, 1, [(3, 0), (4, 1), (5, 2), (11, 2)], 3),
}


@functools.lru_cache(maxsize=None)
def build(case, n):
    tile, h, plant, want = CASES[case]
    rng = np.random.default_rng(1000 * n + sorted(CASES).index(case))
    X = rng.integers(0, 256, (M, n)).astype(np.float64)
    X[Q] = rng.integers(20, 236, n)
    rows = []
    for c, (slot, delta) in enumerate(plant):
        r = row_of(tile, h, slot)
        assert r != Q and r < M and r >= 64
        X[r] = X[Q]
        X[r, c % n] += delta if c % 2 == 0 else -delta
        rows.append(r)
    X.setflags(write=False)
    return X, rows


@functools.lru_cache(maxsize=None)
def reference(case, n, k):
    import oracle
    return oracle.knn(build(case, n)[0], k)


def prove(oracle, case, n, k):
    """What the case exercises, from the oracle's answer for the query."""
    tile, h, plant, want = CASES[case]
    X, rows = build(case, n)
    ans = oracle.knn(X, 30, rows=(Q, 1))[0]
    near = [int(i) - 1 for i in ans["idx"]]          # the answer's rows, nearest first
    live = [r for r, (slot, delta) in zip(rows, plant) if delta != 0]
    dups = [r for r, (slot, delta) in zip(rows, plant) if delta == 0]
    assert len(live) >= want
    # the planted rows are the query's nearest, in the intended places
    assert sorted(near[:len(live)]) == sorted(live)
    assert not set(dups) & set(near)
    for r, (slot, delta) in zip(rows, plant):
        assert place_of(r) == (tile, h, slot)
    assert place_of(Q)[0] != 0 and (place_of(Q)[:2] == (tile, h)) == (case == "diagonal")
    # at the planted distances (the oracle reports sqrt(d^2) = delta), ties included
    dist = {int(i) - 1: float(d) for i, d in zip(ans["idx"], ans["distance"])}
    for r, (slot, delta) in zip(rows, plant):
        assert delta == 0 or dist[r] == float(delta)
    slots = [slot for slot, delta in plant]
    if case in ("two_in_triple", "three_in_triple"):
        assert len({s // 3 for s in slots}) == 1
    if case == "two_triples":
        assert len({s // 3 for s in slots}) == 2 and len({s >> 4 for s in slots}) == 1
    if case == "two_mblocks":
        assert {s >> 4 for s in slots} == {0, 1}
    if case == "ties":
        assert slots[0] // 3 == slots[1] // 3 and slots[2] // 3 != slots[3] // 3
        assert plant[0][1] == plant[1][1] and plant[2][1] == plant[3][1]
    if case in ("eight", "thirteen"):
        order = sorted(delta for slot, delta in plant)
        # ties across the last entry of a 5-entry and of a 6-entry buffer
        assert order[4] == order[5] == order[6] and want > 6
    if case == "diagonal":
        assert place_of(Q)[2] // 3 in {s // 3 for s in slots}
    if case == "partial_tile":
        assert M % 64 != 0 and tile == (M - 1) // 64
    if case == "duplicate":
        assert len(dups) == 1
    if k < len(live):
        assert set(near[:k]) <= set(live)


def run(oracle, case, n, k):
    prove(oracle, case, n, k)
    X, _ = build(case, n)
    got, bits = run_engine(np.array(X), k, "f64")
    assert bits == 8
    ref = reference(case, n, k)
    assert np.array_equal(got["idx"], ref["idx"])
    assert np.array_equal(got["distance"].view(np.uint64), ref["distance"].view(np.uint64))


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_epilogue_planted(oracle, case, n):
    run(oracle, case, n, 30)


@pytest.mark.parametrize("case", sorted(CASES))
def test_epilogue_planted_k3(oracle, case):
    run(oracle, case, 784, 3)


@pytest.mark.parametrize("case", sorted(CASES))
def test_epilogue_planted_single_split(oracle, monkeypatch, case):
    monkeypatch.setenv("KNN_SPLITS", "1")
    run(oracle, case, 784, 30)
