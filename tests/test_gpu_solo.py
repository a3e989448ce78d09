"""Solo searches (knn_ctx_set_solo): a P = 1 search's distance kernel and
merge on the caller's stream, and the meta check through knn_ctx_search_meta.

ring_search() turns solo on at P = 1 (bench.py's path, knn-serial.c:72-93
over the whole corpus in one step).  Every result must equal the oracle's,
with solo on and off, across the speculative byte-block begin (hint from the
last search, checked after end() against the meta the kernels read), a data
change that invalidates the hint, and a solo context that is handed two
steps after all (the step schedule takes over after the first) -- single-block
steps, or a fused split-filter step -- and an end() on another stream than the
solo step's.
"""
import numpy as np
import pytest

import datasets
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu


def _engine(X, k=30):
    import torch
    import mpiknn.ring as ring
    m, n = X.shape
    e = ring.GpuEngine(torch, 0, n, m, m, k)
    src = torch.from_numpy(np.ascontiguousarray(X)).to("cuda:0")
    return e, src


def test_solo_ring_search_p1_hint_cycle(oracle):
    """P = 1 through ring_search (solo): first search (meta read back), then
    from the hint (checked with knn_ctx_search_meta), then on rescaled data
    (the hint no longer matches: searched again from the element block),
    then real-valued data (no byte block at all) -- every result exact."""
    import torch
    import mpiknn.ring as ring
    X = datasets.mnist_like(3000, 784, seed=61)[0]
    e, _ = _engine(X)
    cases = [X, X, np.clip(X * 0.5, 0, 255).round(), X / 255.0 + 1e-3]
    for i, Xs in enumerate(cases):
        src = torch.from_numpy(np.ascontiguousarray(Xs)).to("cuda:0")
        e.pack(src, layout_col=False)
        ring.ring_search(None, torch, e, 0, 1, Xs.shape[0], 0)
        assert_same(e.result(), oracle.knn(Xs, 30), "solo P=1 search %d" % i)
        meta = e.ctx.search_meta()
        assert meta[0] == float(np.abs(Xs).max()), (i, meta)


@pytest.mark.parametrize("solo", [False, True])
def test_solo_context_two_steps_falls_back(knn, oracle, solo):
    """A solo context given two steps: the first runs on the caller's
    stream, the second goes back to the step schedule -- results exact and
    byte-identical either way."""
    import torch
    X = datasets.mnist_like(2000, 784, seed=62)[0]
    m, n = X.shape
    half = m // 2
    dev = "cuda:0"
    stream = torch.cuda.current_stream().cuda_stream
    src = torch.from_numpy(np.ascontiguousarray(X)).to(dev)
    qb = torch.zeros(knn.block_bytes(m, n), dtype=torch.uint8, device=dev)
    knn.block_pack(qb.data_ptr(), m, m, n, src.data_ptr(), n, knn.ROWMAJOR, stream)
    blocks = []
    for b in range(2):
        bb = torch.zeros(knn.block_bytes(m, n), dtype=torch.uint8, device=dev)
        part = src[b * half:(b + 1) * half].contiguous()
        knn.block_pack(bb.data_ptr(), m, half, n, part.data_ptr(), n, knn.ROWMAJOR, stream)
        blocks.append((bb, part))
    ctx = knn.Context(0, m, n, m, 30, "f64")
    ctx.set_solo(solo)
    out = torch.zeros(m * 30 * 16, dtype=torch.uint8, device=dev)
    meta_ptr = qb.data_ptr() + knn.block_meta_offset(m, n)
    ctx.begin(qb.data_ptr(), m, 0, meta_ptr, stream)
    for b, (bb, _) in enumerate(blocks):
        ctx.step(bb.data_ptr(), half, b * half, stream)
    unresolved = ctx.end(out.data_ptr(), stream)
    if unresolved:
        for b, (bb, _) in enumerate(blocks):
            ctx.rescan_step(bb.data_ptr(), half, b * half, stream)
        ctx.rescan_end(out.data_ptr(), stream)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(knn.NB_DTYPE).reshape(m, 30)
    assert_same(got, oracle.knn(X, 30), "solo=%s two steps" % solo)
    # and the same context again, one step over the whole query block
    ctx.begin(qb.data_ptr(), m, 0, meta_ptr, stream)
    ctx.step(qb.data_ptr(), m, 0, stream)
    ctx.end(out.data_ptr(), stream)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(knn.NB_DTYPE).reshape(m, 30)
    assert_same(got, oracle.knn(X, 30), "solo=%s one step after two" % solo)
    ctx.close()


# ---- split filter (real-valued fp32): 1024 queries x 64 dims, k = 10 -------

SPLIT_K = 10


@pytest.fixture(scope="module")
def split_case(oracle):
    """2048 real-valued rows: the first 1024 are the queries (the own block),
    the rest two foreign 512-row blocks; the oracle's answers for the queries
    over all of them, and over the own block alone."""
    X = datasets.gist_like(2048, 64, clusters=16, seed=63)
    Xr = X.astype(np.float32).astype(np.float64)
    return X, oracle.knn(Xr, SPLIT_K)[:1024], oracle.knn(Xr[:1024], SPLIT_K)


def _split_search(knn, X, solo, foreign, end_stream=None):
    """The own block by step(), then the foreign blocks (row ranges) by one
    step_n(); end() on end_stream (default: the steps' stream)."""
    import torch
    dev, m, n, k = "cuda:0", 1024, X.shape[1], SPLIT_K
    stream = torch.cuda.current_stream().cuda_stream
    src = torch.from_numpy(np.ascontiguousarray(X)).to(dev)
    blocks = []
    for lo, hi in [(0, m)] + foreign:
        bb = torch.zeros(knn.block_bytes(m, n, "f32"), dtype=torch.uint8, device=dev)
        part = src[lo:hi].contiguous()
        knn.block_pack(bb.data_ptr(), m, hi - lo, n, part.data_ptr(), n, knn.ROWMAJOR, stream, dtype="f32")
        blocks.append((bb, part, lo, hi - lo))
    # the meta of every block, MAX-reduced (as a ring's all-reduce)
    moff = knn.block_meta_offset(m, n, "f32")
    meta = torch.stack([b[0][moff:moff + 64].view(torch.float64) for b in blocks]).max(dim=0).values.contiguous()
    ctx = knn.Context(0, m, n, m, k, "f32")
    ctx.set_solo(solo)
    out = torch.zeros(m * k * 16, dtype=torch.uint8, device=dev)
    qb = blocks[0][0]
    ctx.begin(qb.data_ptr(), m, 0, meta.data_ptr(), stream)
    assert ctx.split() == 1, "expected the split fp16 filter"
    ctx.step(qb.data_ptr(), m, 0, stream)
    if foreign:
        ctx.step_n([b[0].data_ptr() for b in blocks[1:]], [b[3] for b in blocks[1:]], [b[2] for b in blocks[1:]],
                   stream)
    es = stream if end_stream is None else end_stream.cuda_stream
    if ctx.end(out.data_ptr(), es):
        for bb, _, lo, rows in blocks:
            ctx.rescan_step(bb.data_ptr(), rows, lo, es)
        ctx.rescan_end(out.data_ptr(), es)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(knn.NB_DTYPE).reshape(m, k)
    ctx.close()
    return got


def test_solo_then_fused_split_step(knn, split_case):
    """A solo context whose second step is a fused split-filter step
    (knn_ctx_step_n of two 512-row blocks behind the own block): the step
    schedule takes over in front of it -- exact, and byte-identical to the
    same search with solo off."""
    X, ref, _ = split_case
    foreign = [(1024, 1536), (1536, 2048)]
    got = _split_search(knn, X, True, foreign)
    assert_same(got, ref, "solo, then a fused split step")
    plain = _split_search(knn, X, False, foreign)
    assert got.tobytes() == plain.tobytes()


def test_solo_end_on_second_stream(knn, split_case):
    """A solo one-step search whose end() runs on another stream than its
    step: that stream is ordered behind the step's and carries the merge."""
    import torch
    X, _, ref_own = split_case
    got = _split_search(knn, X, True, [], end_stream=torch.cuda.Stream())
    assert_same(got, ref_own, "solo, end() on a second stream")
