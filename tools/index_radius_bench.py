#!/usr/bin/env python3
"""Index.radius_count / Index.radius against Index.query(k = 30) of the same batch.

The corpus and protocol of tools/index_bench.py: the seeded 60000 x 784 uint8
corpus, --mq (10000) uint8 queries, the keep-zero rule; every figure is the
library's own HIP-event span (knn_last_search_seconds: pack through the last
kernel, no copy to the host), median of --runs after --warmup with min and max.

Legs (one a process, run in alternation by the caller):

  query   ix.query(Q, 30): the yardstick -- the same contraction plus a
          selection.  Uses nothing this tool's subject added, so it runs on an
          older checkout too (--lib-root points at its tree).
  radius  the radius r first: by bisection on radius_count's mean, so that
          the mean count is about 30 (r and the mean count it gives are stated
          in the output); then radius_count, and radius (count +
          fill + sort: the two calls' spans, added).  With KNN_NO_I8=1 in the
          environment the same on the element path (leg name radius-scan).

Each leg appends one JSON line to --out; --merge FILES... writes
profiles/index_radius.md from such lines: the figures, each radius figure's
ratio to the query span, and the byte-path count's achieved fraction of the
dense int8 rate (2 mq m round_up(n, 32) operations a pass over 5000 TOPS).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I8_DENSE_TOPS = 5000.0


def stats(t):
    t = sorted(t)
    return {"median_ms": statistics.median(t), "min_ms": t[0], "max_ms": t[-1], "runs": len(t)}


def leg_query(knn, a, X, Q):
    with knn.Index(X) as ix:
        span = []
        for i in range(a.warmup + a.runs):
            _, s = ix.query(Q, a.k)
            if i >= a.warmup:
                span.append(s * 1e3)
        return {"bits": ix.info().last_bits, "span": stats(span)}


def leg_radius(knn, a, X, Q):
    import numpy as np
    with knn.Index(X) as ix:
        # r by bisection on the mean count, below the largest 30th distance
        # (counts are exact on every path, so every leg arrives at the same r)
        rec, _ = ix.query(Q, a.k)
        lo, hi = 0.0, float(rec["distance"][:, a.k - 1].max())
        for _ in range(60):
            r = 0.5 * (lo + hi)
            mean = float(ix.radius_count(Q, r).mean())
            if abs(mean - a.k) <= 0.5:
                break
            lo, hi = (lo, r) if mean > a.k else (r, hi)
        count, both = [], []
        for i in range(a.warmup + a.runs):
            counts = ix.radius_count(Q, r)
            s = knn.lib.knn_last_search_seconds()
            ix.radius(Q, r)
            if i >= a.warmup:
                count.append(s * 1e3)
                both.append(sum(ix.radius_seconds) * 1e3)
        return {"radius": r, "mean_count": float(counts.mean()), "max_count": int(counts.max()),
                "empty": int((counts == 0).sum()), "count": stats(count), "count_fill_sort": stats(both)}


def merge(files, out):
    legs = []
    for f in files:
        with open(f) as fh:
            legs += [json.loads(line) for line in fh if line.strip()]

    def med(name, key):
        v = [g["results"][key]["median_ms"] for g in legs if g["leg"] == name]
        return statistics.median(v) if v else None
    q = med("query", "span")
    rows = [("query(k = 30), this commit", q), ("query(k = 30), parent commit", med("query-parent", "span")),
            ("radius_count, byte path", med("radius", "count")),
            ("radius (count + fill + sort), byte path", med("radius", "count_fill_sort")),
            ("radius_count, element path (KNN_NO_I8=1)", med("radius-scan", "count")),
            ("radius, element path (KNN_NO_I8=1)", med("radius-scan", "count_fill_sort"))]
    base = med("query-parent", "span") or q
    g = next((g for g in legs if g["leg"] == "radius"), None)
    with open(out, "w") as fh:
        fh.write("# Index radius search: spans on the 60000 x 784 uint8 corpus\n\n")
        if g:
            fh.write("%d uint8 queries, m = %d, n = %d; r = %.6f (bisected for a mean count of 30), mean count %.2f, "
                     "max %d, %d queries without a hit.  Library spans (HIP events), median of %d runs after %d "
                     "warm-up calls, one leg a process, legs alternated.\n\n"
                     % (g["mq"], g["m"], g["n"], g["results"]["radius"], g["results"]["mean_count"],
                        g["results"]["max_count"], g["results"]["empty"], g["results"]["count"]["runs"], g["warmup"]))
        fh.write("| call | span, ms | ratio to the parent's query span |\n|---|---|---|\n")
        for name, v in rows:
            if v is not None:
                fh.write("| %s | %.3f | %.2f |\n" % (name, v, v / base))
        c = med("radius", "count")
        if g and c:
            ops = 2.0 * g["mq"] * g["m"] * ((g["n"] + 31) // 32 * 32)
            fh.write("\nByte-path count: %.3g int8 operations in %.3f ms = %.0f TOPS, %.1f %% of the dense int8 rate "
                     "(%.0f TOPS); the span also holds the query pack.\n"
                     % (ops, c, ops / (c * 1e-3) / 1e12, 100.0 * ops / (c * 1e-3) / 1e12 / I8_DENSE_TOPS,
                        I8_DENSE_TOPS))
        fh.write("\nEvery leg's runs:\n\n```\n")
        for g in legs:
            fh.write(json.dumps(g) + "\n")
        fh.write("```\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["query", "radius"])
    ap.add_argument("--name", help="the leg's name in the output (default: the leg, radius-scan under KNN_NO_I8=1)")
    ap.add_argument("--lib-root", default=ROOT, help="the checkout whose mpi-knn_amd is measured")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--m", type=int, default=60000)
    ap.add_argument("--k", type=int, default=30)
    ap.add_argument("--mq", type=int, default=10000)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "index_radius.jsonl"))
    ap.add_argument("--merge", nargs="+")
    a = ap.parse_args()
    if a.merge:
        merge(a.merge, os.path.join(ROOT, "profiles", "index_radius.md"))
        return
    sys.path.insert(0, os.path.join(a.lib_root, "mpi-knn_amd"))
    import numpy as np
    import mpiknn
    from mpiknn import synth

    X = synth.mnist_like(a.m)[0].astype(np.uint8)
    Q = synth.mnist_like(a.mq, seed=77)[0].astype(np.uint8)
    name = a.name or (a.leg + ("-scan" if a.leg == "radius" and os.environ.get("KNN_NO_I8") == "1" else ""))
    rec = {"leg": name, "warmup": a.warmup, "m": a.m, "n": int(X.shape[1]), "mq": a.mq,
           "results": (leg_query if a.leg == "query" else leg_radius)(mpiknn, a, X, Q)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
