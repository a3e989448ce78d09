#!/usr/bin/env python3
"""Index.dbscan against the only route there was before it: radius_rows_count +
radius_rows for every row, then a union-find on the host.

The corpus and protocol of tools/index_radius_bench.py: the seeded 60000 x 784
uint8 corpus; every device figure is the library's own HIP-event span
(knn_last_search_seconds), median of --runs after --warmup with min and max;
one leg a process, legs alternated by the caller, each under a time limit of
its own and chained with &&.

Two radii, found by bisection on the mean of radius_rows_count over all rows
(keep-zero: a row's other neighbours, N(x) - 1), which is exact on every path,
so every leg arrives at the same radii; a later leg may take them from an
earlier leg's output with --radii and skip the search:

  sparse   a mean count of about --sparse (30)
  dense    a mean count of about --dense (300): where clusters form

Legs:

  dbscan   ix.dbscan(r, min_pts) at both radii: the span, the call's wall
           time, the clusters, core and noise rows it finds, and the device
           bytes the first call adds.  With KNN_NO_I8=1 in the environment the
           same on the element path (leg name dbscan-scan).
  pair     radius_rows_count + radius_rows for all rows with host output --
           the two spans added, and the wall time, which also holds the copy of
           the graph to the host -- then knn_dbscan_graph's time on that graph
           (the host twin, from --twin-root's library: a host-only function, so
           an older checkout's route can be timed with it).  Uses nothing of
           the index this tool's subject added, so it runs on an older
           checkout (--lib-root points at its tree; leg name pair-parent by
           --name).  KNN_NO_I8=1: the element path (pair-scan).

Each leg appends one JSON line to --out; --merge FILES... writes
profiles/index_dbscan.md from such lines.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(t):
    t = sorted(t)
    return {"median_ms": statistics.median(t), "min_ms": t[0], "max_ms": t[-1], "runs": len(t)}


def bisect(ix, target):
    """r with a mean radius_rows_count within 2 % of target"""
    lo, hi = 0.0, 4096.0
    for _ in range(60):
        r = 0.5 * (lo + hi)
        mean = float(ix.radius_rows_count(None, r, keep_zero=True).mean())
        if abs(mean - target) <= 0.02 * target:
            break
        lo, hi = (lo, r) if mean > target else (r, hi)
    return r


def radii_of(ix, a):
    if a.radii:
        return [float(v) for v in a.radii.split(",")]
    return [bisect(ix, a.sparse), bisect(ix, a.dense)]


def leg_dbscan(knn, a, X):
    out = []
    with knn.Index(X) as ix:
        radii = radii_of(ix, a)
        before = ix.info().device_bytes
        for r in radii:
            span, wall = [], []
            for i in range(a.warmup + a.runs):
                t0 = time.perf_counter()
                res = ix.dbscan(r, a.min_pts, neighbours=True)
                t1 = time.perf_counter()
                if i == 0 and r == radii[0]:
                    own = ix.info().device_bytes - before
                if i >= a.warmup:
                    span.append(res.seconds * 1e3)
                    wall.append((t1 - t0) * 1e3)
            out.append({"radius": r, "mean_count": float(res.neighbours.mean()) - 1.0,
                        "max_count": int(res.neighbours.max()) - 1, "nclusters": res.nclusters,
                        "core": int((res.neighbours >= a.min_pts).sum()), "noise": int((res.cluster == 0).sum()),
                        "largest": int((res.cluster == 1).sum() if res.nclusters else 0),
                        "span": stats(span), "wall": stats(wall)})
        return {"bits": ix.info().last_bits, "device_bytes": own, "radii": out}


def leg_pair(knn, a, X):
    import numpy as np
    twin = ctypes.CDLL(os.path.join(a.twin_root, "mpi-knn_amd", "lib", "libknn.so")).knn_dbscan_graph
    twin.restype = ctypes.c_int
    twin.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_size_t, ctypes.c_int] + [ctypes.c_void_p] * 3
    out = []
    with knn.Index(X) as ix:
        for r in radii_of(ix, a):
            span, wall, host = [], [], []
            for i in range(a.warmup + a.runs):
                t0 = time.perf_counter()
                indptr, rec = ix.radius_rows(None, r, keep_zero=True)
                t1 = time.perf_counter()
                if i >= a.warmup:
                    span.append(sum(ix.radius_seconds) * 1e3)
                    wall.append((t1 - t0) * 1e3)
                if i >= a.warmup and len(host) < a.twin_runs:
                    cl = np.zeros(len(X), dtype=np.int32)
                    nc = ctypes.c_int(0)
                    rec = np.ascontiguousarray(rec)
                    t0 = time.perf_counter()
                    rc = twin(indptr.ctypes.data, rec.ctypes.data, None, len(X), a.min_pts, cl.ctypes.data, None,
                              ctypes.byref(nc))
                    host.append((time.perf_counter() - t0) * 1e3)
                    assert rc == 0, rc
            out.append({"radius": r, "records": int(indptr[-1]), "graph_bytes": int(indptr[-1]) * rec.itemsize,
                        "mean_count": float(np.diff(indptr).mean()), "max_count": int(np.diff(indptr).max()),
                        "nclusters": nc.value, "noise": int((cl == 0).sum()),
                        "span": stats(span), "wall": stats(wall), "host_twin": stats(host)})
        return {"radii": out}


def merge(files, out):
    legs = []
    for f in files:
        with open(f) as fh:
            legs += [json.loads(line) for line in fh if line.strip()]

    def med(name, which, key):
        v = [g["results"]["radii"][which][key]["median_ms"] for g in legs if g["leg"] == name]
        return statistics.median(v) if v else None

    def first(name):
        return next((g for g in legs if g["leg"] == name), None)
    d, p = first("dbscan"), first("pair-parent") or first("pair")
    pname = "pair-parent" if first("pair-parent") else "pair"
    with open(out, "w") as fh:
        fh.write("# Index DBSCAN against radius_rows + a host union-find: the 60000 x 784 uint8 corpus\n\n")
        if d:
            fh.write("m = %d, n = %d, min_pts = %d.  Library spans (HIP events) and wall times, median of the runs "
                     "after the warm-up calls (both in each leg's line below), one leg a process, legs alternated.  "
                     "The radii are bisected on the mean of radius_rows_count over all rows.\n\n"
                     % (d["m"], d["n"], d["min_pts"]))
        for which, what in ((0, "sparse"), (1, "dense")):
            if not d:
                break
            g = d["results"]["radii"][which]
            fh.write("## %s: r = %.6f, %.1f other rows within r on average, %d at most\n\n"
                     % (what, g["radius"], g["mean_count"], g["max_count"]))
            fh.write("dbscan finds %d clusters (the first holds %d rows), %d core rows, %d noise rows.\n\n"
                     % (g["nclusters"], g["largest"], g["core"], g["noise"]))
            if p:
                q = p["results"]["radii"][which]
                fh.write("The graph: %d records, %d bytes.\n\n" % (q["records"], q["graph_bytes"]))
            fh.write("| route | device span, ms | wall, ms | host union-find, ms |\n|---|---|---|---|\n")
            for name, label, twin in (("dbscan", "dbscan, byte path", False),
                                      (pname, "radius_rows_count + radius_rows, byte path, parent commit", True),
                                      ("dbscan-scan", "dbscan, element path (KNN_NO_I8=1)", False),
                                      (pname + "-scan", "radius_rows_count + radius_rows, element path, parent commit",
                                       True)):
                s = med(name, which, "span")
                if s is None:
                    continue
                fh.write("| %s | %.3f | %.3f | %s |\n" % (label, s, med(name, which, "wall"),
                                                         "%.3f" % med(name, which, "host_twin") if twin else "-"))
            fh.write("\n")
        if d:
            fh.write("Device bytes the first dbscan adds: %d on the byte path" % d["results"]["device_bytes"])
            s = first("dbscan-scan")
            fh.write(", %d on the element path.\n" % s["results"]["device_bytes"] if s else ".\n")
        fh.write("\nEvery leg's runs:\n\n```\n")
        for g in legs:
            fh.write(json.dumps(g) + "\n")
        fh.write("```\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["dbscan", "pair"])
    ap.add_argument("--name", help="the leg's name in the output (default: the leg, with -scan under KNN_NO_I8=1)")
    ap.add_argument("--lib-root", default=ROOT, help="the checkout whose mpi-knn_amd is measured")
    ap.add_argument("--twin-root", default=ROOT, help="the checkout whose library holds knn_dbscan_graph")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--twin-runs", type=int, default=3)
    ap.add_argument("--m", type=int, default=60000)
    ap.add_argument("--min-pts", type=int, default=5)
    ap.add_argument("--sparse", type=float, default=30.0)
    ap.add_argument("--dense", type=float, default=300.0)
    ap.add_argument("--radii", help="r_sparse,r_dense of an earlier leg: no bisection")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "index_dbscan.jsonl"))
    ap.add_argument("--merge", nargs="+")
    a = ap.parse_args()
    if a.merge:
        merge(a.merge, os.path.join(ROOT, "profiles", "index_dbscan.md"))
        return
    sys.path.insert(0, os.path.join(a.lib_root, "mpi-knn_amd"))
    import numpy as np
    import mpiknn
    from mpiknn import synth

    X = synth.mnist_like(a.m)[0].astype(np.uint8)
    name = a.name or a.leg
    if os.environ.get("KNN_NO_I8") == "1":
        name += "-scan"
    rec = {"leg": name, "warmup": a.warmup, "m": a.m, "n": int(X.shape[1]), "min_pts": a.min_pts,
           "results": (leg_dbscan if a.leg == "dbscan" else leg_pair)(mpiknn, a, X)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
