"""DBSCAN without a GPU: the two entry points exist; the host twin
knn_dbscan_graph, given the reference epsilon-graph, equals the independent
restatement tests/dbscan_ref.py for every case at both radii; a stand-alone
program runs it on hand-made graphs and through its refusals
(tests/dbscan_cpu/dbscan_graph.c with mpi-knn_amd/csrc/knn_cluster.c alone,
built once more with the address and undefined-behaviour sanitizers); every
refusal of knn_index_dbscan comes before any device call, a call leaves the
kept context alone, and a call that fails anywhere leaves the index answering,
its bytes accounted and its host outputs unwritten
(tests/dbscan_cpu/dbscan_checks.c, on tests/index_trace's stubs, likewise
under the sanitizers); and the cases tests/test_gpu_dbscan.py uses are worth
testing with -- from the reference alone, so that a bad choice of radius fails
here and does not pass vacuously on the GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import dbscan_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
HERE = os.path.join(ROOT, "tests", "dbscan_cpu")
CSRC = os.path.join(ROOT, "mpi-knn_amd", "csrc")
SAN = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer")
BASE = ("-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror")


def cc():
    c = shutil.which("gcc") or shutil.which("cc")
    assert c, "no C compiler"
    return c


def sanitizers_link(res):
    return not (res.returncode != 0 and any(w in res.stderr for w in ("sanitize", "asan", "ubsan")))


def test_symbols_exist(knn):
    for name in ("knn_index_dbscan", "knn_dbscan_graph"):
        assert name in knn.API_SYMBOLS and getattr(knn.lib, name).argtypes is not None
    assert callable(knn.Index.dbscan) and callable(knn.dbscan_graph)
    assert knn.DbscanResult._fields == ("cluster", "neighbours", "nclusters", "seconds")


def test_null_index_through_the_library(knn):
    """(the shared library itself: refused with no device)"""
    a = np.zeros(4, dtype=np.int64)
    p = a.ctypes.data
    assert knn.lib.knn_index_dbscan(None, 1.0, 5, 0, p, p, None) == knn.ERR_INVALID
    assert knn.lib.knn_dbscan_graph(None, p, None, 1, 5, p, p, None) == knn.ERR_INVALID


# ------------------------------------------------- the host twin, every case

@pytest.mark.parametrize("name", D.CASES)
def test_host_twin_equals_the_restatement(knn, name):
    c = D.case(name)
    for eps in (c.eps_at, c.eps_below):
        _, indptr, rec = c.rows_ref(eps)
        got = knn.dbscan_graph(indptr, rec, c.min_pts)
        assert D.same(got, c.ref(eps)), (name, eps)
        assert got.neighbours is not None
    # live ids that are not 1 .. m: the same graph under other names
    _, indptr, rec = c.rows_ref(c.eps_at)
    ids = np.arange(1, D.M + 1) * 3 - 1
    rec = rec.copy()
    rec["idx"] = ids[rec["idx"] - 1]
    assert D.same(knn.dbscan_graph(indptr + 11, rec, c.min_pts, ids=ids), c.ref(c.eps_at))
    with pytest.raises(knn.KnnError) as e:
        knn.dbscan_graph(indptr, rec, c.min_pts)             # those are no ids of 1 .. m
    assert e.value.status == knn.ERR_INVALID
    # the duplicate groups alone at eps = 0
    _, indptr, rec = c.rows_ref(0.0)
    assert D.same(knn.dbscan_graph(indptr, rec, 2), c.ref(0.0, 2))


# ------------------------------------------------ the stand-alone host program

def build_graph(exe, extra=()):
    return subprocess.run([cc(), *BASE, *extra, "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(HERE, "dbscan_graph.c"), os.path.join(CSRC, "knn_cluster.c")],
                          capture_output=True, text=True)


def run_graph(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1].split()
    # "ok: G graphs, R refusals"
    assert last[0] == "ok:" and int(last[1]) >= 11 and int(last[3]) >= 11, last


def test_host_twin_on_hand_made_graphs(tmp_path):
    exe = str(tmp_path / "dbscan_graph")
    res = build_graph(exe)
    assert res.returncode == 0, res.stderr
    run_graph(exe)


def test_host_twin_under_sanitizers(tmp_path):
    exe = str(tmp_path / "dbscan_graph_san")
    res = build_graph(exe, SAN)
    if not sanitizers_link(res):
        pytest.skip("-fsanitize=address,undefined does not link here: " + res.stderr.strip().splitlines()[-1])
    assert res.returncode == 0, res.stderr
    run_graph(exe)


# ------------------------------------------- refusals, context, failed calls

def build_checks(exe, extra=()):
    return subprocess.run([
        cc(), *BASE, "-D__HIP_PLATFORM_AMD__", "-ffunction-sections", "-fdata-sections", *extra,
        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + os.path.join(ROCM, "include"), "-o", exe,
        os.path.join(HERE, "dbscan_checks.c"), os.path.join(CSRC, "knn_index.c"), os.path.join(CSRC, "knn_blocks.c"),
        os.path.join(CSRC, "knn_engine.c"), "-Wl,--gc-sections,--allow-multiple-definition", "-lm"],
        capture_output=True, text=True)


def run_checks(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1].split()
    # "ok: R refusals, F faults"
    assert last[0] == "ok:" and int(last[1]) >= 11 and int(last[3]) >= 20, last


def test_refusals_context_and_faults(tmp_path):
    exe = str(tmp_path / "dbscan_checks")
    res = build_checks(exe)
    assert res.returncode == 0, res.stderr
    run_checks(exe)


def test_refusals_context_and_faults_under_sanitizers(tmp_path):
    exe = str(tmp_path / "dbscan_checks_san")
    res = build_checks(exe, SAN)
    if not sanitizers_link(res):
        pytest.skip("-fsanitize=address,undefined does not link here: " + res.stderr.strip().splitlines()[-1])
    assert res.returncode == 0, res.stderr
    run_checks(exe)


# -------------------------------------------------------- fixture properties

@pytest.mark.parametrize("name", D.CASES)
def test_fixture_is_worth_testing_with(name):
    c = D.case(name)
    dd, at = c.dd, c.at
    assert len(c.X) == D.M and np.isfinite(c.eps_at) and c.eps_at > 0.0 and c.min_pts <= D.R.GROUP
    assert np.nextafter(c.eps_below, np.inf) == c.eps_at
    cluster, nbr, nclusters = c.ref(c.eps_at)
    core = nbr >= c.min_pts
    border = ~core & (cluster > 0)
    hit = dd <= c.eps_at
    assert nclusters >= 3 and cluster.max() == nclusters
    assert (cluster == 0).any() and border.any()
    # eps_at is the distance of one actual pair of core rows, the only link of its two clusters:
    a, b = at[D.A[-1]], at[D.B[0]]
    assert dd[a, b] == c.eps_at and core[a] and core[b] and cluster[a] == cluster[b]
    below, _, nbelow = c.ref(c.eps_below)
    assert nbelow == nclusters + 1 and below[a] != below[b]
    ca, cb = np.flatnonzero(below == below[a]), np.flatnonzero(below == below[b])
    assert (hit[np.ix_(ca, cb)].sum(), hit[a, b]) == (1, True)
    # a border row whose core neighbours lie in two clusters, the nearest two at equal distances: the id decides
    p = at[D.P]
    near = np.flatnonzero(hit[p] & core)
    assert border[p] and len(set(cluster[near])) == 2
    first = near[np.lexsort((near, dd[p][near]))]
    assert dd[p][first[0]] == dd[p][first[1]] and cluster[first[0]] != cluster[first[1]]
    assert cluster[p] == cluster[first[0]] and first[0] < first[1]
    # a border row at the radius exactly: noise below it
    e = at[D.E]
    assert border[e] and (dd[e][hit[e] & core] == c.eps_at).all() and below[e] == 0
    # a cluster with rows in all three blocks of 256: the duplicate group, core at eps = 0 as well
    g = c.group
    assert len(set(cluster[g])) == 1 and cluster[g[0]] > 0 and set(g // 256) == {0, 1, 2}
    zero, nzero, czero = c.ref(0.0)
    assert (nzero[g] == D.R.GROUP).all() and czero == 1 and (zero[g] == 1).all() and (np.delete(zero, g) == 0).all()
    # min_pts = 2 at eps = 0: the duplicate groups, and only they
    zero2, _, czero2 = c.ref(0.0, 2)
    assert czero2 == len(c.trips) + 1 and (zero2[c.trips.reshape(-1)] > 0).all()
    assert (zero2 > 0).sum() == 3 * len(c.trips) + D.R.GROUP
    # the planted rows lie in more than one block, as the duplicate group does
    assert len(set(c.rows // 256)) == 3


def test_integer_cases_are_byte_path_data():
    for name, n in (("mnist", 784), ("sift", 128), ("n100", 100)):
        X = D.case(name).X
        assert X.shape[1] == n and (X == np.rint(X)).all() and X.min() >= 0 and X.max() <= 255
    assert not (D.case("real").X == np.rint(D.case("real").X)).all()
