#!/usr/bin/env python3
"""Index.classify against Index.query followed by classify_query on the host.

Legs (one a process, run in alternation by the caller; the protocol and the
corpus of tools/index_bench.py: seeded 60000 x 784 uint8 corpus with labels,
k = 30, keep-zero rule, median of --runs after --warmup with min and max):

  classify  host wall time of ix.classify(Q, qlabels=...) at every --mq, and
            the search span it reports
  twostep   host wall time of ix.query(Q) followed by classify_query on its
            records (the label table the caller keeps), same batches
  vote      what knn_last_search_seconds leaves out: HIP events around
            ix.classify(Q, out=buf) and around ix.query(Q, out=buf), Q and
            every output on the device, beside the search span -- the
            difference is the vote launch with its counter's memset, the call's
            own buffer (one hipMalloc, one hipFree) and the match count's copy

Each leg appends one JSON line to --out; --merge FILES... folds such lines
into profiles/index_classify.json.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(t):
    t = sorted(t)
    return {"median_ms": statistics.median(t), "min_ms": t[0], "max_ms": t[-1], "runs": len(t)}


def leg_wall(knn, a, X, y, Qall, yq, classify):
    import numpy as np
    rows = []
    with knn.Index(X.astype(np.uint8), labels=y) as ix:
        for mq in a.mq:
            Q, ql = Qall[:mq].astype(np.uint8), yq[:mq]
            wall, span = [], []
            for i in range(a.warmup + a.runs):
                t0 = time.perf_counter()
                if classify:
                    res = ix.classify(Q, k=a.k, qlabels=ql, nclasses=10)
                    s, hits = res.seconds, res.matches
                else:
                    rec, s = ix.query(Q, a.k)
                    _, hits = knn.classify_query(rec, y, ql, 10)
                w = time.perf_counter() - t0
                if i >= a.warmup:
                    wall.append(w * 1e3)
                    span.append(s * 1e3)
            rows.append({"mq": mq, "matches": hits, "bits": ix.info().last_bits, "wall": stats(wall),
                         "span": stats(span)})
    return rows


def leg_vote(knn, a, X, y, Qall, yq):
    import numpy as np
    import torch
    rows = []
    with knn.Index(X.astype(np.uint8), labels=y) as ix:
        for mq in a.mq:
            Q = torch.from_numpy(Qall[:mq].astype(np.uint8)).to("cuda:0")
            buf = torch.empty(mq * a.k * 16, dtype=torch.uint8, device="cuda:0")
            t = {"classify": [], "query": []}
            span = []
            for i in range(a.warmup + a.runs):
                for name in ("classify", "query"):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    if name == "classify":
                        s = ix.classify(Q, k=a.k, qlabels=yq[:mq], nclasses=10, out=buf).seconds
                    else:
                        _, s = ix.query(Q, a.k, out=buf)
                    e1.record()
                    e1.synchronize()
                    if i >= a.warmup:
                        t[name].append(e0.elapsed_time(e1))
                        span.append(s * 1e3)
            rows.append({"mq": mq, "classify_events": stats(t["classify"]), "query_events": stats(t["query"]),
                         "span": stats(span)})
    return rows


def merge(files, out):
    legs = []
    for f in files:
        with open(f) as fh:
            legs += [json.loads(line) for line in fh if line.strip()]
    res = {"corpus": "synth.mnist_like(60000) x 784 as uint8, labels 1..10, k = 30, keep-zero rule", "legs": legs}
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["classify", "twostep", "vote"])
    ap.add_argument("--round", type=int, default=0)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--m", type=int, default=60000)
    ap.add_argument("--k", type=int, default=30)
    ap.add_argument("--mq", type=int, nargs="*", default=[1, 1024, 10000])
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "index_classify.jsonl"))
    ap.add_argument("--merge", nargs="+")
    a = ap.parse_args()
    if a.merge:
        merge(a.merge, os.path.join(ROOT, "profiles", "index_classify.json"))
        return
    sys.path.insert(0, os.path.join(ROOT, "mpi-knn_amd"))
    import mpiknn
    from mpiknn import synth

    X, y = synth.mnist_like(a.m)
    Qall, yq = synth.mnist_like(max(a.mq), seed=77)
    rec = {"leg": a.leg, "round": a.round, "warmup": a.warmup}
    if a.leg == "vote":
        rec["results"] = leg_vote(mpiknn, a, X, y, Qall, yq)
    else:
        rec["results"] = leg_wall(mpiknn, a, X, y, Qall, yq, a.leg == "classify")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
