#!/usr/bin/env python3
"""The resident index against knn_query, and the byte pack from 8-bit sources.

Legs (one a process, so two builds of the library can be run in alternation:
--root names the tree whose mpi-knn_amd/ is imported):

  query   knn_query's device span on the seeded 60000 x 784 integer corpus at
          k = 30 for mq in 1, 16, 128, 1024, 10000 (the protocol of
          tools/query_bench.py, keep-zero rule, default path)
  index   Index.query on the same corpus and queries: device span and host
          wall time of the call, from a float64 and from a uint8 index;
          knn_index_create's time and the index's device bytes once
  pack    knn_block_pack_s8, row-major, 1M x 128 and 60000 x 784, from uint8
          (where the build has it), fp32 and fp64 sources of the same values:
          HIP events, fraction of HBM over the algorithmic bytes (source read
          once + byte rows and two norm words written, as bench.py prices it)

Median of --runs after --warmup, with min and max.  Each leg appends one JSON
line to --out; --merge FILES... folds such lines into profiles/index_bench.json.

    python tools/index_bench.py --leg index --out bench_out/index.jsonl
    python tools/index_bench.py --merge bench_out/*.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK_GBS = 8000.0   # as bench.py


def stats(t):
    t = sorted(t)
    return {"median_ms": statistics.median(t), "min_ms": t[0], "max_ms": t[-1], "runs": len(t)}


def leg_query(knn, a, X, Qall):
    rows = []
    for mq in a.mq:
        Q = Qall[:mq]
        t = []
        for i in range(a.warmup + a.runs):
            _, s = knn.query(X, Q, a.k, keep_zero=True)
            if i >= a.warmup:
                t.append(s * 1e3)
        rows.append(dict(mq=mq, **stats(t)))
    return rows


def leg_index(knn, a, X, Qall):
    import numpy as np
    rows, create = [], {}
    for src in ("f64", "u8"):
        Xs = X if src == "f64" else X.astype(np.uint8)
        t0 = time.perf_counter()
        ix = knn.Index(Xs)
        create[src] = {"create_wall_ms": (time.perf_counter() - t0) * 1e3}
        for mq in a.mq:
            Q = Qall[:mq] if src == "f64" else Qall[:mq].astype(np.uint8)
            span, wall = [], []
            for i in range(a.warmup + a.runs):
                t0 = time.perf_counter()
                _, s = ix.query(Q, a.k, keep_zero=True)
                w = time.perf_counter() - t0
                if i >= a.warmup:
                    span.append(s * 1e3)
                    wall.append(w * 1e3)
            rows.append({"mq": mq, "source": src, "bits": ix.info().last_bits, "span": stats(span),
                         "wall": stats(wall)})
        create[src]["device_bytes"] = ix.info().device_bytes
        create[src]["nblocks"] = ix.info().nblocks
        ix.close()
    return {"results": rows, "create": create}


def leg_pack(knn, a):
    import numpy as np
    import torch
    dev = torch.device("cuda", 0)
    out = []
    for rows, n in ((1000000, 128), (60000, 784)):
        V = torch.randint(0, 256, (rows, n), dtype=torch.uint8, device=dev)
        blk = torch.zeros(knn.s8_block_bytes(rows, n), dtype=torch.uint8, device=dev)
        for src in ("u8", "f32", "f64"):
            if src == "u8" and not hasattr(knn, "U8"):
                continue
            S = V if src == "u8" else V.to(torch.float32 if src == "f32" else torch.float64)
            st = torch.cuda.current_stream(dev).cuda_stream
            t = []
            for i in range(a.warmup + a.runs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                knn.block_pack_s8(blk.data_ptr(), rows, rows, n, S.data_ptr(), n, knn.ROWMAJOR, st, src_dtype=src)
                e1.record()
                e1.synchronize()
                if i >= a.warmup:
                    t.append(e0.elapsed_time(e1))
            es = {"u8": 1, "f32": 4, "f64": 8}[src]
            nbytes = rows * n * es + rows * (-(-n // 32) * 32 + 8)
            r = dict(rows=rows, n=n, source=src, bytes=nbytes, **stats(t))
            r["hbm_frac"] = nbytes / (r["median_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS
            out.append(r)
            del S
        del V, blk
    return out


def merge(files, out):
    legs = []
    for f in files:
        with open(f) as fh:
            legs += [json.loads(line) for line in fh if line.strip()]
    res = {"corpus": "synth.mnist_like(60000) x 784, k = 30, keep-zero rule, default path",
           "protocol": "median of runs after warmup (min, max); builds run in alternation, one process a leg",
           "legs": legs}
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["query", "index", "pack"])
    ap.add_argument("--root", default=ROOT, help="tree whose mpi-knn_amd/ is imported")
    ap.add_argument("--tag", default="this", help="name of the build in the output")
    ap.add_argument("--round", type=int, default=0)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--m", type=int, default=60000)
    ap.add_argument("--k", type=int, default=30)
    ap.add_argument("--mq", type=int, nargs="*", default=[1, 16, 128, 1024, 10000])
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "index_bench.jsonl"))
    ap.add_argument("--merge", nargs="+")
    a = ap.parse_args()
    if a.merge:
        merge(a.merge, os.path.join(ROOT, "profiles", "index_bench.json"))
        return
    sys.path.insert(0, os.path.join(os.path.abspath(a.root), "mpi-knn_amd"))
    import mpiknn
    from mpiknn import synth

    rec = {"leg": a.leg, "build": a.tag, "round": a.round, "warmup": a.warmup}
    if a.leg == "pack":
        rec["results"] = leg_pack(mpiknn, a)
    else:
        X, _ = synth.mnist_like(a.m)
        Qall, _ = synth.mnist_like(max(a.mq), seed=77)
        if a.leg == "query":
            rec["results"] = leg_query(mpiknn, a, X, Qall)
        else:
            rec.update(leg_index(mpiknn, a, X, Qall))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
