"""knn_block_gather_dt / knn_block_gather_s8 against one-shot packs, byte for
byte.  A source block holds the 300 rows of X; `sel` picks 300 of them with
repeats and a descending stretch (a gather, not only a compaction).  A
destination packed from X[sel][:row0] and filled from row0 on by gathers of
sel[row0:], in pieces, must be the block that one knn_block_pack_dt /
knn_block_pack_s8 of X[sel] writes on every byte below the meta offset: rows,
padding, the norms, and both norm-word arrays of a byte block over all 384
padded rows.  row0 and the piece ends sit at 0, 70, 127, 128 and 129, across
the 64- and 128-row boundaries (as tests/test_gpu_append.py).  After every
piece the whole destination is compared: the rows outside the piece and the
meta words are the ones it had before.  cap = 384; n = 20, 31, 128 (short byte
rows with init words), 784 (long rows)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAP = 384
ROWS = 300
CUTS = [0, 70, 127, 128, 129]


def values(n):
    rng = np.random.default_rng(1000 * ROWS + n)
    V = rng.integers(0, 256, (ROWS, n)).astype(np.float64)
    V[ROWS // 2] = 255.0
    V[0, 0] = 0.0
    V[ROWS - 1, n - 1] = 255.0
    return V


def selection():
    rng = np.random.default_rng(9)
    sel = rng.integers(0, ROWS, ROWS)
    sel[100:140] = np.arange(250, 210, -1)          # a descending stretch
    sel[5:9] = sel[5]                               # repeats
    sel[69:72] = [ROWS - 1, 0, ROWS - 1]
    sel[126:131] = [0, ROWS - 1, 17, 17, 1]
    return sel.astype(np.int32)


def norm_pos(r):
    """i8_norm_pos (knn_device.h): where row r's norm words sit in their arrays"""
    rr = r & 127
    b, w = rr >> 5, rr & 31
    j, h, i = w >> 3, (w >> 2) & 1, w & 3
    return (r & ~127) + (((b * 2 + h) * 4 + j) * 4 + i)


def owner_rows(form, n, dtype, moff):
    """for every byte of a block below its meta offset: the block row it belongs to"""
    rp = 384
    r = np.arange(rp)
    if form == "s8":
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


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", [20, 31, 128, 784])
@pytest.mark.parametrize("form", ["elem", "s8"])
def test_gather_equals_pack(knn, form, n, dtype):
    import torch
    dev = torch.device("cuda", 0)
    X, sel = values(n), selection()
    s8 = form == "s8"
    nbytes = knn.s8_block_bytes(CAP, n) if s8 else knn.block_bytes(CAP, n, dtype)
    moff = knn.s8_block_meta_offset(CAP, n) if s8 else knn.block_meta_offset(CAP, n, dtype)
    own = owner_rows(form, n, dtype, moff)

    def pack(V):
        t = torch.from_numpy(np.ascontiguousarray(V)).to(dev)
        b = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        (knn.block_pack_s8 if s8 else knn.block_pack)(b.data_ptr(), CAP, len(V), n, t.data_ptr(), n, knn.ROWMAJOR,
                                                      dtype=dtype)
        torch.cuda.synchronize()
        return b

    def gather(dst, row0, lst):
        if s8:
            knn.block_gather_s8(dst.data_ptr(), CAP, row0, src.data_ptr(), CAP, lst.data_ptr(), len(lst), n)
        else:
            knn.block_gather(dst.data_ptr(), CAP, row0, src.data_ptr(), CAP, lst.data_ptr(), len(lst), n, dtype=dtype)
        torch.cuda.synchronize()

    src = pack(X)
    src_before = src.cpu().numpy()
    want = pack(X[sel]).cpu().numpy()
    d_sel = torch.from_numpy(sel).to(dev)
    for row0 in CUTS:
        dst = pack(X[sel][:max(row0, 1)])             # (a pack takes at least one row; row 0 is then overwritten)
        before = dst.cpu().numpy()
        ends = [c for c in CUTS if c > row0] + [ROWS]
        a = row0
        for b in ends:
            gather(dst, a, d_sel[a:b])
            got = dst.cpu().numpy()
            # the piece's rows as the one-shot pack has them, every other byte as before the piece
            exp = before.copy()
            mine = (own >= a) & (own < b)
            exp[:moff][mine] = want[:moff][mine]
            assert np.array_equal(got, exp), (form, n, dtype, row0, a, b)
            before, a = got, b
        assert np.array_equal(before[:moff], want[:moff]), (form, n, dtype, row0)
    assert np.array_equal(src.cpu().numpy(), src_before)
    # the comparison saw real rows and real norms
    assert want[:moff].any() and len(np.unique(want[:moff][own == 3])) > 2


def test_gather_one_row_everywhere(knn):
    """one row gathered to each of the 384 rows of a byte block with init words
    (n = 128) and of one without (n = 784): the norm words of every position"""
    import torch
    dev = torch.device("cuda", 0)
    for n in (128, 784):
        X = values(n)
        nbytes, moff = knn.s8_block_bytes(CAP, n), knn.s8_block_meta_offset(CAP, n)
        t = torch.from_numpy(np.ascontiguousarray(np.repeat(X[[7]], CAP, axis=0))).to(dev)
        want = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        knn.block_pack_s8(want.data_ptr(), CAP, CAP, n, t.data_ptr(), n, knn.ROWMAJOR)
        ts = torch.from_numpy(np.ascontiguousarray(X)).to(dev)
        src = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        knn.block_pack_s8(src.data_ptr(), CAP, ROWS, n, ts.data_ptr(), n, knn.ROWMAJOR)
        dst = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        lst = torch.full((CAP,), 7, dtype=torch.int32, device=dev)
        knn.block_gather_s8(dst.data_ptr(), CAP, 0, src.data_ptr(), CAP, lst.data_ptr(), CAP, n)
        torch.cuda.synchronize()
        assert np.array_equal(dst.cpu().numpy()[:moff], want.cpu().numpy()[:moff]), n
