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

  add     Index.add of 1, 128 and 10000 rows to the 60000-row index, from uint8
          and from float64 rows: host wall of the call from a host array, host
          wall and device span (events around the call) from a device tensor,
          then the span of the first query (mq = 128) after the add against
          the same query on a fresh index of the grown size
  rebuild what a user without add does: knn_index_create of the 60000 + rows
          concatenated corpus (host wall), same sources and sizes; runs on a
          build without add too
  remove  Index.remove of 1, 128 and 10000 random ids from the 60000-row index
          (uint8 and float64 source) that has served one query: host wall and
          device span (events around the call), the span of the first query
          (mq = 128) after it against the same query on a fresh index of the
          survivors, and what a user without remove does: knn_index_create of
          the surviving rows from a host array (host wall; --tag parent with
          --leg rebuild-survivors runs that on a build without remove)
  gather  knn_block_gather_dt / _s8 alone, 60000 x 784 and 1M x 128, every
          second row dropped: HIP events, fraction of HBM over the algorithmic
          bytes (each moved row read once and written once, plus its norm or
          norm words), beside hipMemcpyAsync device to device of the same
          byte count in the same process
  mapcost Index.query spans at every --mq on one index before and after one
          removal (the id translation at the end of the span)
  update  Index.update of 1 and 1000 rows spread over the whole 60000-row uint8
          index that has served one query: host wall and device span (events
          around the call), and in the same process, on another fresh index,
          what a user without update does for the same rows: Index.remove of
          their ids, then Index.add of the rows (which also changes their ids)
  neighbours  Index.neighbours on the 60000-row uint8 index, flags 0 and
          keep-zero: every live row, one id, 1000 ids; beside knn_search's span
          on the same corpus in the same process

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


ADD_ROWS = (1, 128, 10000)


def leg_add(knn, a, X, Qall):
    """every timed add goes to a fresh 60000-row index (an add's cost must not
    depend on the adds before it); indices are created outside the timings"""
    import numpy as np
    import torch
    dev = torch.device("cuda", 0)
    Q = Qall[:128]
    rows_out = []
    extra, _ = synth_rows(knn, max(ADD_ROWS))
    for src in ("u8", "f64"):
        cast = (lambda A: A.astype(np.uint8)) if src == "u8" else (lambda A: A)
        Xs, Qs = cast(X), cast(Q)
        for rows in ADD_ROWS:
            A = np.ascontiguousarray(cast(extra[:rows]))
            dA = torch.from_numpy(A).to(dev)
            wall_h, wall_d, span_d, q_after, q_fresh = [], [], [], [], []
            for i in range(a.warmup + a.runs):
                for device in (False, True):
                    ix = knn.Index(Xs)
                    ix.query(Qs, a.k)                       # the kept context exists, as in a server
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    e0.record()
                    ix.add(dA if device else A)
                    e1.record()
                    w = (time.perf_counter() - t0) * 1e3
                    e1.synchronize()
                    _, s = ix.query(Qs, a.k)
                    ix.close()
                    if i >= a.warmup:
                        if device:
                            wall_d.append(w)
                            span_d.append(e0.elapsed_time(e1))
                        else:
                            wall_h.append(w)
                            q_after.append(s * 1e3)
            fresh = knn.Index(np.vstack([Xs, A]))
            for i in range(a.warmup + a.runs):
                _, s = fresh.query(Qs, a.k)
                if i >= a.warmup:
                    q_fresh.append(s * 1e3)
            fresh.close()
            rows_out.append({"rows": rows, "source": src, "wall_host_src": stats(wall_h), "wall_device_src": stats(wall_d),
                             "span_device_src": stats(span_d), "first_query_after_add": stats(q_after),
                             "query_fresh_index": stats(q_fresh)})
    return rows_out


def synth_rows(knn, rows):
    from mpiknn import synth
    return synth.mnist_like(rows, seed=99)


def leg_rebuild(knn, a, X):
    import numpy as np
    out = []
    extra, _ = synth_rows(knn, max(ADD_ROWS))
    for src in ("u8", "f64"):
        if src == "u8" and not hasattr(knn, "U8"):
            continue
        for rows in ADD_ROWS:
            C = np.vstack([X, extra[:rows]])
            C = np.ascontiguousarray(C.astype(np.uint8) if src == "u8" else C)
            t = []
            for i in range(a.warmup + a.runs):
                t0 = time.perf_counter()
                ix = knn.Index(C)
                w = (time.perf_counter() - t0) * 1e3
                ix.close()
                if i >= a.warmup:
                    t.append(w)
            out.append(dict(rows=rows, source=src, create_wall=stats(t)))
    return out


def removal_ids(m, rows):
    import numpy as np
    return np.sort(np.random.default_rng(1000 + rows).choice(np.arange(1, m + 1), rows, replace=False)).astype(np.int32)


def leg_rebuild_survivors(knn, a, X):
    """knn_index_create of the rows a removal leaves, from a host array"""
    import numpy as np
    out = []
    for src in ("u8", "f64"):
        for rows in ADD_ROWS:
            keep = np.ones(len(X), dtype=bool)
            keep[removal_ids(len(X), rows) - 1] = False
            C = np.ascontiguousarray(X[keep].astype(np.uint8) if src == "u8" else X[keep])
            t = []
            for i in range(a.warmup + a.runs):
                t0 = time.perf_counter()
                ix = knn.Index(C)
                w = (time.perf_counter() - t0) * 1e3
                ix.close()
                if i >= a.warmup:
                    t.append(w)
            out.append(dict(rows=rows, source=src, create_wall=stats(t)))
    return out


def leg_remove(knn, a, X, Qall):
    """every timed removal meets a fresh 60000-row index that has served one
    query; indices are created outside the timings"""
    import numpy as np
    import torch
    Q = Qall[:128]
    out = []
    for src in ("u8", "f64"):
        cast = (lambda A: A.astype(np.uint8)) if src == "u8" else (lambda A: A)
        Xs, Qs = np.ascontiguousarray(cast(X)), cast(Q)
        for rows in ADD_ROWS:
            ids = removal_ids(len(X), rows)
            wall, span, q_after, q_fresh = [], [], [], []
            for i in range(a.warmup + a.runs):
                ix = knn.Index(Xs)
                ix.query(Qs, a.k)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                ix.remove(ids)
                e1.record()
                w = (time.perf_counter() - t0) * 1e3
                e1.synchronize()
                _, s = ix.query(Qs, a.k)
                ix.close()
                if i >= a.warmup:
                    wall.append(w)
                    span.append(e0.elapsed_time(e1))
                    q_after.append(s * 1e3)
            keep = np.ones(len(X), dtype=bool)
            keep[ids - 1] = False
            fresh = knn.Index(np.ascontiguousarray(Xs[keep]))
            for i in range(a.warmup + a.runs):
                _, s = fresh.query(Qs, a.k)
                if i >= a.warmup:
                    q_fresh.append(s * 1e3)
            fresh.close()
            out.append({"rows": rows, "source": src, "wall": stats(wall), "span": stats(span),
                        "first_query_after_remove": stats(q_after), "query_fresh_index": stats(q_fresh)})
    return out


def leg_gather(knn, a):
    import torch
    dev = torch.device("cuda", 0)
    out = []
    for rows, n in ((60000, 784), (1000000, 128)):
        V = torch.randint(0, 256, (rows, n), dtype=torch.uint8, device=dev)
        lst = torch.arange(0, rows, 2, dtype=torch.int32, device=dev)
        cnt = lst.numel()
        st = torch.cuda.current_stream(dev).cuda_stream
        for form in ("f64", "f32", "s8"):
            nbytes = knn.s8_block_bytes(rows, n) if form == "s8" else knn.block_bytes(rows, n, form)
            src = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
            dst = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
            if form == "s8":
                knn.block_pack_s8(src.data_ptr(), rows, rows, n, V.data_ptr(), n, knn.ROWMAJOR, st, src_dtype="u8")
                moved = cnt * (-(-n // 32) * 32 + 8)
            else:
                knn.block_pack(src.data_ptr(), rows, rows, n, V.data_ptr(), n, knn.ROWMAJOR, st, dtype=form,
                               src_dtype="u8")
                es = 8 if form == "f64" else 4
                moved = cnt * (-(-n * es // 128) * 128 + es)
            tg, tc = [], []
            for i in range(a.warmup + a.runs):
                e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                e0.record()
                if form == "s8":
                    knn.block_gather_s8(dst.data_ptr(), rows, 0, src.data_ptr(), rows, lst.data_ptr(), cnt, n, st)
                else:
                    knn.block_gather(dst.data_ptr(), rows, 0, src.data_ptr(), rows, lst.data_ptr(), cnt, n, st,
                                     dtype=form)
                e1.record()
                dst[:moved].copy_(src[:moved])        # hipMemcpyAsync, device to device
                e2.record()
                e2.synchronize()
                if i >= a.warmup:
                    tg.append(e0.elapsed_time(e1))
                    tc.append(e1.elapsed_time(e2))
            r = dict(rows=rows, n=n, form=form, moved_rows=cnt, bytes=2 * moved, gather=stats(tg), memcpy=stats(tc))
            r["gather_hbm_frac"] = 2 * moved / (r["gather"]["median_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS
            r["memcpy_hbm_frac"] = 2 * moved / (r["memcpy"]["median_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS
            out.append(r)
            del src, dst
        del V, lst
    return out


UPDATE_ROWS = (1, 1000)


def leg_update(knn, a, X, Qall):
    """every timed call meets a fresh index that has served one query; the
    update and the remove + add pair alternate, indices made outside the timings"""
    import numpy as np
    import torch
    Xs, Qs = np.ascontiguousarray(X.astype(np.uint8)), Qall[:128].astype(np.uint8)
    extra, _ = synth_rows(knn, max(UPDATE_ROWS))
    out = []

    def timed(ix, f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        f(ix)
        e1.record()
        w = (time.perf_counter() - t0) * 1e3
        e1.synchronize()
        return w, e0.elapsed_time(e1)

    for rows in UPDATE_ROWS:
        ids = np.linspace(1, len(X), rows + 2).astype(np.int32)[1:-1] if rows > 1 else np.array([len(X) // 8], np.int32)
        A = np.ascontiguousarray(extra[:rows].astype(np.uint8))
        t = {name: [] for name in ("update_wall", "update_span", "pair_wall", "pair_span", "q_update", "q_pair")}
        for i in range(a.warmup + a.runs):
            for pair in (False, True):
                ix = knn.Index(Xs)
                ix.query(Qs, a.k)
                w, sp = timed(ix, (lambda x: (x.remove(ids), x.add(A))) if pair else (lambda x: x.update(ids, A)))
                _, s = ix.query(Qs, a.k)
                ix.close()
                if i >= a.warmup:
                    t["pair_wall" if pair else "update_wall"].append(w)
                    t["pair_span" if pair else "update_span"].append(sp)
                    t["q_pair" if pair else "q_update"].append(s * 1e3)
        out.append({"rows": rows, "source": "u8", "first_id": int(ids[0]), "last_id": int(ids[-1]),
                    "update_wall": stats(t["update_wall"]), "update_span": stats(t["update_span"]),
                    "remove_add_wall": stats(t["pair_wall"]), "remove_add_span": stats(t["pair_span"]),
                    "first_query_after_update": stats(t["q_update"]),
                    "first_query_after_remove_add": stats(t["q_pair"])})
    return out


def leg_mapcost(knn, a, X, Qall):
    import numpy as np
    rows = []
    ix = knn.Index(X.astype(np.uint8))
    # the kept context and tiles at the capacity of the largest batch first, so
    # that both states run every mq on the same buffers
    ix.query(Qall[:max(a.mq)].astype(np.uint8), a.k, keep_zero=True)
    for state in ("before", "after"):
        if state == "after":
            ix.remove([len(X) // 2])
        for mq in a.mq:
            Q = Qall[:mq].astype(np.uint8)
            t = []
            for i in range(a.warmup + a.runs):
                _, s = ix.query(Q, a.k, keep_zero=True)
                if i >= a.warmup:
                    t.append(s * 1e3)
            rows.append({"mq": mq, "state": state, "span": stats(t)})
    ix.close()
    return rows


def leg_neighbours(knn, a, X):
    """Index.neighbours on the uint8 index under both zero rules: every live row
    (the corpus's graph), one id, and 1000 ids spread over the corpus; and the
    yardstick in the same process, knn_search's span on the same corpus"""
    import numpy as np

    def spans(f):
        t = []
        for i in range(a.warmup + a.runs):
            _, s = f()
            if i >= a.warmup:
                t.append(s * 1e3)
        return stats(t)

    out = {"search": spans(lambda: knn.search(X, a.k)), "results": []}
    ix = knn.Index(X.astype(np.uint8))
    lists = {"all": None, "1": [len(X) // 2], "1000": np.random.default_rng(3).permutation(len(X))[:1000] + 1}
    for keep_zero in (False, True):
        for name, ids in lists.items():
            r = spans(lambda: ix.neighbours(ids, a.k, keep_zero=keep_zero))
            out["results"].append({"ids": name, "keep_zero": keep_zero, "bits": ix.info().last_bits, "span": r})
    info = ix.info()
    out["nblocks"], out["device_bytes"] = info.nblocks, info.device_bytes
    ix.close()
    return out


def merge(files, out, keep=False):
    legs = []
    if keep and os.path.exists(out):
        with open(out) as fh:
            legs = json.load(fh).get("legs", [])
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
    ap.add_argument("--leg", choices=["query", "index", "pack", "add", "rebuild", "remove", "rebuild-survivors", "gather",
                                     "mapcost", "update", "neighbours"])
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
    ap.add_argument("--keep", action="store_true", help="--merge: keep the legs profiles/index_bench.json holds")
    a = ap.parse_args()
    if a.merge:
        merge(a.merge, os.path.join(ROOT, "profiles", "index_bench.json"), a.keep)
        return
    sys.path.insert(0, os.path.join(os.path.abspath(a.root), "mpi-knn_amd"))
    import mpiknn
    from mpiknn import synth

    rec = {"leg": a.leg, "build": a.tag, "round": a.round, "warmup": a.warmup}
    if a.leg == "pack":
        rec["results"] = leg_pack(mpiknn, a)
    elif a.leg == "gather":
        rec["results"] = leg_gather(mpiknn, a)
    else:
        X, _ = synth.mnist_like(a.m)
        Qall, _ = synth.mnist_like(max(a.mq), seed=77)
        if a.leg == "query":
            rec["results"] = leg_query(mpiknn, a, X, Qall)
        elif a.leg == "add":
            rec["results"] = leg_add(mpiknn, a, X, Qall)
        elif a.leg == "rebuild":
            rec["results"] = leg_rebuild(mpiknn, a, X)
        elif a.leg == "rebuild-survivors":
            rec["results"] = leg_rebuild_survivors(mpiknn, a, X)
        elif a.leg == "remove":
            rec["results"] = leg_remove(mpiknn, a, X, Qall)
        elif a.leg == "mapcost":
            rec["results"] = leg_mapcost(mpiknn, a, X, Qall)
        elif a.leg == "update":
            rec["results"] = leg_update(mpiknn, a, X, Qall)
        elif a.leg == "neighbours":
            rec.update(leg_neighbours(mpiknn, a, X))
        else:
            rec.update(leg_index(mpiknn, a, X, Qall))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
