"""knn_block_gather_pos_dt / knn_block_gather_pos_s8 against the single-block
gathers, byte for byte.  The source is a corpus of 700 rows held as three
blocks of capacity 256 (the last one partial); `pos` lists 300 global
positions, shuffled, with repeats, from every block and across both block
boundaries, and four entries that are no position at all.  The destination
(capacity 384) is prefilled with a byte pattern and filled from row0 = 37 on by
ONE multi-block gather; it must equal, on every byte, the same prefilled buffer
after one knn_block_gather_dt / _s8 a source block (that block's entries as
local rows, every other entry masked to -1, which writes nothing).  Rows
outside [row0, row0 + 300), the rows of the entries that are no position, the
padding and the meta must still hold the pattern.  Element blocks: fp64 and
fp32, n = 5, 64, 784, 960; byte blocks: n = 64 (short rows, init words) and
784 (long rows)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAP = 256                       # of a source block
NBLK = 3
M = 700                         # rows of the corpus: the last block holds 188
DCAP = 384
ROW0 = 37
ROWS = 300
PATTERN = 0xA5
NOT_A_POSITION = {11: -1, 12: NBLK * CAP, 200: 2 ** 31 - 1, 299: -(2 ** 31)}


def values(n):
    rng = np.random.default_rng(7000 + n)
    V = rng.integers(0, 256, (M, n)).astype(np.float64)
    V[M // 2] = 255.0
    V[0, 0] = 0.0
    return V


def positions():
    rng = np.random.default_rng(31)
    pos = rng.integers(0, M, ROWS).astype(np.int64)
    pos[0:6] = [255, 256, 257, 0, M - 1, 256]               # both sides of a boundary, the ends, a repeat
    pos[60:64] = [511, 512, 513, 511]
    pos[100:103] = pos[100]                                 # one row three times running
    pos[150] = NBLK * CAP - 1                               # the last block's last padded row: a position, if no live row
    for i, v in NOT_A_POSITION.items():
        pos[i] = v
    assert all(((pos >= b * CAP) & (pos < (b + 1) * CAP)).sum() > 50 for b in range(NBLK))
    return pos.astype(np.int32)


def norm_pos(r):
    """i8_norm_pos (knn_device.h): where row r's norm words sit in their arrays"""
    rr = r & 127
    b, w = rr >> 5, rr & 31
    j, h, i = w >> 3, (w >> 2) & 1, w & 3
    return (r & ~127) + (((b * 2 + h) * 4 + j) * 4 + i)


def owner_rows(s8, n, dtype, moff):
    """for every byte of a DCAP block below its meta offset: the block row it belongs to"""
    rp = (DCAP + 127) // 128 * 128
    r = np.arange(rp)
    if s8:
        rs = (n + 31) // 32 * 32
        inv = np.empty(rp, dtype=np.int64)
        inv[norm_pos(r)] = r
        own = np.concatenate([np.repeat(r, rs), np.repeat(inv, 4), np.repeat(inv, 4)])
    else:
        es = 8 if dtype == "f64" else 4
        rb = (n * es + 127) // 128 * 128
        own = np.concatenate([np.repeat(r, rb), np.repeat(r, es)])
    assert len(own) == moff
    return own


CASES = [("elem", n, dt) for dt in ("f64", "f32") for n in (5, 64, 784, 960)] + [("s8", 64, "f64"), ("s8", 784, "f64")]


@pytest.mark.parametrize("form,n,dtype", CASES)
def test_gather_pos_equals_per_block_gathers(knn, form, n, dtype):
    import torch
    dev = torch.device("cuda", 0)
    s8 = form == "s8"
    X, pos = values(n), positions()
    sbytes = knn.s8_block_bytes(CAP, n) if s8 else knn.block_bytes(CAP, n, dtype)
    dbytes = knn.s8_block_bytes(DCAP, n) if s8 else knn.block_bytes(DCAP, n, dtype)
    moff = knn.s8_block_meta_offset(DCAP, n) if s8 else knn.block_meta_offset(DCAP, n, dtype)

    srcs = []
    for b in range(NBLK):
        V = np.ascontiguousarray(X[b * CAP:(b + 1) * CAP])
        t = torch.from_numpy(V).to(dev)
        blk = torch.zeros(sbytes, dtype=torch.uint8, device=dev)
        (knn.block_pack_s8 if s8 else knn.block_pack)(blk.data_ptr(), CAP, len(V), n, t.data_ptr(), n, knn.ROWMAJOR,
                                                      dtype=dtype)
        srcs.append(blk)
    torch.cuda.synchronize()
    before = [s.cpu().numpy() for s in srcs]
    tab = torch.tensor([s.data_ptr() for s in srcs], dtype=torch.int64, device=dev)
    d_pos = torch.from_numpy(pos).to(dev)

    got = torch.full((dbytes,), PATTERN, dtype=torch.uint8, device=dev)
    if s8:
        knn.block_gather_pos_s8(got.data_ptr(), DCAP, ROW0, tab.data_ptr(), CAP, NBLK, d_pos.data_ptr(), ROWS, n)
    else:
        knn.block_gather_pos(got.data_ptr(), DCAP, ROW0, tab.data_ptr(), CAP, NBLK, d_pos.data_ptr(), ROWS, n,
                             dtype=dtype)
    want = torch.full((dbytes,), PATTERN, dtype=torch.uint8, device=dev)
    p64 = pos.astype(np.int64)
    for b in range(NBLK):
        local = np.where((p64 >= b * CAP) & (p64 < (b + 1) * CAP), p64 - b * CAP, -1).astype(np.int32)
        lst = torch.from_numpy(local).to(dev)
        if s8:
            knn.block_gather_s8(want.data_ptr(), DCAP, ROW0, srcs[b].data_ptr(), CAP, lst.data_ptr(), ROWS, n)
        else:
            knn.block_gather(want.data_ptr(), DCAP, ROW0, srcs[b].data_ptr(), CAP, lst.data_ptr(), ROWS, n,
                             dtype=dtype)
    torch.cuda.synchronize()
    got, want = got.cpu().numpy(), want.cpu().numpy()
    assert np.array_equal(got, want)
    # untouched rows, the rows of the entries that are no position, padding and meta: the pattern
    own = owner_rows(s8, n, dtype, moff)
    skipped = np.array([ROW0 + i for i in NOT_A_POSITION])
    kept = (own < ROW0) | (own >= ROW0 + ROWS) | np.isin(own, skipped)
    assert (got[:moff][kept] == PATTERN).all() and (got[moff:] == PATTERN).all()
    # the comparison saw real rows: a written row is not the pattern, and repeats are equal rows
    assert (got[:moff][own == ROW0 + 3] != PATTERN).any()
    if not s8:
        assert np.array_equal(got[:moff][own == ROW0 + 100], got[:moff][own == ROW0 + 101])
        assert not np.array_equal(got[:moff][own == ROW0 + 0], got[:moff][own == ROW0 + 1])
    # the sources are only read
    assert all(np.array_equal(s.cpu().numpy(), b4) for s, b4 in zip(srcs, before))


def test_gather_pos_refusals(knn):
    import torch
    dev = torch.device("cuda", 0)
    n = 64
    blk = torch.zeros(knn.block_bytes(CAP, n), dtype=torch.uint8, device=dev)
    dst = torch.full((knn.block_bytes(DCAP, n),), PATTERN, dtype=torch.uint8, device=dev)
    tab = torch.tensor([blk.data_ptr()], dtype=torch.int64, device=dev)
    d_pos = torch.zeros(8, dtype=torch.int32, device=dev)
    ok = dict(d_dst=dst.data_ptr(), dst_cap=DCAP, row0=0, d_tab=tab.data_ptr(), src_cap=CAP, nblk=1,
              d_pos=d_pos.data_ptr(), rows=8, n=n)
    for f in (knn.block_gather_pos, knn.block_gather_pos_s8):
        for bad in (dict(d_tab=None), dict(nblk=0), dict(d_dst=None), dict(d_pos=None), dict(rows=0),
                    dict(row0=DCAP - 7), dict(src_cap=0), dict(n=0), dict(n=2 ** 31)):
            with pytest.raises(knn.KnnError) as e:
                f(**dict(ok, **bad))
            assert e.value.status == knn.ERR_INVALID
    with pytest.raises(knn.KnnError):
        knn.block_gather_pos_s8(**dict(ok, n=897))
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == PATTERN).all()
