#!/usr/bin/env python3
"""Device span of knn_query (knn_last_search_seconds) on the seeded 60000 x 784
integer corpus, for query sets of 1, 16, 128, 1024 and 10000 rows, under both
zero rules, on the fast path and with KNN_FORCE_RESCAN=1 (every query through
the exact rescan).  Median of --runs after --warmup.  One process, no
children: the library reads its switches at every call.

    python tools/query_bench.py [--runs 20 --warmup 5 --out profiles/query_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpi-knn_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--m", type=int, default=60000)
    ap.add_argument("--k", type=int, default=30)
    ap.add_argument("--mq", type=int, nargs="*", default=[1, 16, 128, 1024, 10000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_bench.json"))
    a = ap.parse_args()
    import mpiknn
    from mpiknn import synth

    X, _ = synth.mnist_like(a.m)
    Qall, _ = synth.mnist_like(max(a.mq), seed=77)
    rows = []
    for mq in a.mq:
        Q = Qall[:mq]
        for rescan in (0, 1):
            if rescan:
                os.environ["KNN_FORCE_RESCAN"] = "1"
            else:
                os.environ.pop("KNN_FORCE_RESCAN", None)
            for keep in (False, True):
                t = []
                for i in range(a.warmup + a.runs):
                    _, s = mpiknn.query(X, Q, a.k, keep_zero=keep)
                    if i >= a.warmup:
                        t.append(s * 1e3)
                t.sort()
                row = {"mq": mq, "path": "rescan" if rescan else "default", "keep_zero": keep,
                       "median_ms": statistics.median(t), "min_ms": t[0], "max_ms": t[-1], "runs": len(t)}
                rows.append(row)
                print(json.dumps(row), flush=True)
    os.environ.pop("KNN_FORCE_RESCAN", None)
    res = {"corpus": "synth.mnist_like(%d) x 784, k = %d" % (a.m, a.k), "warmup": a.warmup, "results": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
