"""knn_block_append_dt / knn_block_append_s8 against their own one-shot packs:
a block packed over its first 70 rows and appended to at (70, 59), (129, 1) and
(130, 170) -- pieces that cross the 64- and 128-row boundaries at unaligned
offsets, one of a single row -- is byte for byte (rows, norms or norm words,
meta, padding) the block one pack of all 300 rows writes.  cap = 300 (384
padded rows); n = 20 (a padded short row; the row-major u8 pieces start
unaligned), 31 (no row-major source has 16-byte-aligned rows: the scalar-load
forms of every row kernel, fp32 and fp64 sources included), 128 (SIFT's short
rows with init words), 784 (MNIST's long rows).
Both buffers start zero-filled and are compared whole."""
import numpy as np
import pytest

import datasets

pytestmark = pytest.mark.gpu

CAP = ROWS = 300
R1 = 70
PIECES = [(70, 59), (129, 1), (130, 170)]
NP_SRC = {"f64": np.float64, "f32": np.float32, "u8": np.uint8}


def values(n, seed=0):
    """integers in [0, 255] as tests/test_gpu_u8.py makes them"""
    rng = np.random.default_rng(seed + 1000 * ROWS + n)
    V = rng.integers(0, 256, (ROWS, n)).astype(np.uint8)
    V[ROWS // 2] = 255
    for r in (0, ROWS - 1):
        V[r, 0] = 0
        V[r, n - 1] = 255
    return V.astype(np.float64)


def dev_src(torch, V, layout, src):
    """rows of V as a device source: (tensor, ld, layout code)"""
    A = np.ascontiguousarray(V.astype(NP_SRC[src]) if layout == "row" else V.astype(NP_SRC[src]).T)
    return torch.from_numpy(A).to(torch.device("cuda", 0)), (V.shape[1] if layout == "row" else V.shape[0])


def one_shot_and_pieces(torch, knn, V, form, layout, dtype, src, pieces=PIECES, r1=R1):
    """(one pack of every row, pack of r1 rows + appends) as host bytes"""
    rows, n = V.shape
    lay = knn.ROWMAJOR if layout == "row" else knn.COLMAJOR
    nbytes = knn.s8_block_bytes(CAP, n) if form == "s8" else knn.block_bytes(CAP, n, dtype)
    pack = knn.block_pack_s8 if form == "s8" else knn.block_pack
    append = knn.block_append_s8 if form == "s8" else knn.block_append
    dev = torch.device("cuda", 0)
    a = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    b = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    t, ld = dev_src(torch, V, layout, src)
    pack(a.data_ptr(), CAP, rows, n, t.data_ptr(), ld, lay, dtype=dtype, src_dtype=src)
    t1, ld1 = dev_src(torch, V[:r1], layout, src)
    pack(b.data_ptr(), CAP, r1, n, t1.data_ptr(), ld1, lay, dtype=dtype, src_dtype=src)
    keep = [t, t1]
    for row0, cnt in pieces:
        tp, ldp = dev_src(torch, V[row0:row0 + cnt], layout, src)
        keep.append(tp)
        append(b.data_ptr(), CAP, row0, cnt, n, tp.data_ptr(), ldp, lay, dtype=dtype, src_dtype=src)
    torch.cuda.synchronize()
    return a.cpu().numpy(), b.cpu().numpy()


def check_byte_block(knn, V, a, what):
    """a byte block against numpy alone: the image x ^ 0x80 in rows [:ROWS, :n]
    and zero elsewhere, and the meta words of V"""
    n = V.shape[1]
    rs = (n + 31) // 32 * 32
    img = a[:384 * rs].reshape(-1, rs)
    assert np.array_equal(img[:ROWS, :n], V.astype(np.uint8) ^ 0x80), what
    assert not img[:, n:].any() and not img[ROWS:].any(), what
    moff = knn.s8_block_meta_offset(CAP, n)
    meta = a[moff:moff + 64].view(np.float64)
    assert meta[0] == np.abs(V).max() and meta[2] == 0.0 and meta[3] == 0.0, what
    assert meta[4] == V.max() and meta[5] == 0.0, what
    assert meta[1] == (V * V).sum(1).max(), what


@pytest.mark.parametrize("n", [20, 31, 128, 784])
@pytest.mark.parametrize("form", ["elem", "s8"])
def test_append_equals_pack(knn, form, n):
    import torch
    V = values(n)
    first = None
    for layout in ("row", "col"):
        for dtype in ("f64", "f32"):
            for src in ("f64", "f32", "u8"):
                a, b = one_shot_and_pieces(torch, knn, V, form, layout, dtype, src)
                assert np.array_equal(a, b), (form, layout, dtype, src)
                if form == "s8" and n == 31:
                    # the unaligned width: every combination against numpy, and
                    # one byte block whatever the layout, block type and source
                    check_byte_block(knn, V, a, (layout, dtype, src))
                    first = a if first is None else first
                    assert np.array_equal(a, first), (layout, dtype, src)
    # the comparison sees the appended rows: they are in the one-shot block
    if form == "s8":
        rs = (n + 31) // 32 * 32
        img = a[:384 * rs].reshape(-1, rs)
        assert np.array_equal(img[:ROWS, :n], V.astype(np.uint8) ^ 0x80) and not img[ROWS:].any()


def test_append_u8_row_source_inside_a_larger_array(knn):
    """a row-major KNN_U8 piece that starts at row0 * n of one array (n = 20:
    no 16-byte alignment), and the same with 16-byte-aligned rows (n = 128)"""
    import torch
    dev = torch.device("cuda", 0)
    for n in (20, 128):
        V = values(n)
        t = torch.from_numpy(V.astype(np.uint8)).to(dev)
        nbytes = knn.s8_block_bytes(CAP, n)
        a = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        b = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        knn.block_pack_s8(a.data_ptr(), CAP, ROWS, n, t.data_ptr(), n, knn.ROWMAJOR, src_dtype="u8")
        knn.block_pack_s8(b.data_ptr(), CAP, R1, n, t.data_ptr(), n, knn.ROWMAJOR, src_dtype="u8")
        for row0, cnt in PIECES:
            knn.block_append_s8(b.data_ptr(), CAP, row0, cnt, n, t.data_ptr() + row0 * n, n, knn.ROWMAJOR,
                                src_dtype="u8")
        torch.cuda.synchronize()
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()), n


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_append_real_valued(knn, dtype):
    """real-valued rows: the fp norms bit for bit (a row is summed in the same
    order wherever it lands)"""
    import torch
    X, _ = datasets.mnist_real(ROWS)
    for layout in ("row", "col"):
        for src in ("f64", "f32"):
            a, b = one_shot_and_pieces(torch, knn, X, "elem", layout, dtype, src)
            assert np.array_equal(a, b), (layout, src)
    es = 8 if dtype == "f64" else 4
    npad = (784 * es + 127) // 128 * 128 // es
    norms = a[384 * npad * es:384 * npad * es + ROWS * es].view(np.float64 if dtype == "f64" else np.float32)
    assert (norms > 0).all() and len(np.unique(norms)) > ROWS // 2


@pytest.mark.parametrize("form", ["elem", "s8"])
def test_append_meta(knn, form):
    """the meta is max(old, new rows): the block's only 255 in an appended
    piece; then a 255.5 there (max|x|, max norm, the non-integer word)"""
    import torch
    n = 128
    rng = np.random.default_rng(3)
    V = rng.integers(0, 200, (ROWS, n)).astype(np.float64)
    V[150, 7] = 255.0
    W = V.copy()
    W[200, 9] = 255.5
    moff = knn.s8_block_meta_offset(CAP, n) if form == "s8" else knn.block_meta_offset(CAP, n, "f64")
    for M, top, nonint in ((V, 255.0, 0.0), (W, 255.5, 1.0)):
        for layout in ("row", "col"):
            a, b = one_shot_and_pieces(torch, knn, M, form, layout, "f64", "f64")
            ma, mb = a[moff:moff + 64].view(np.float64), b[moff:moff + 64].view(np.float64)
            assert np.array_equal(ma, mb)
            assert mb[0] == top and mb[2] == nonint and mb[4] == top and mb[5] == 0.0
            assert mb[1] == (M * M).sum(axis=1).max()
            assert mb[7] == (1.0 if form == "s8" else 0.0)
            assert np.array_equal(a, b)
