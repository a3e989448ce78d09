"""KNN_U8 pack sources: for the same values, the block packed from unsigned
bytes is byte for byte the block packed from the fp64 array -- rows, norms
(norm words) and meta -- for knn_block_pack_s8 (n <= 896) and for
knn_block_pack_dt into fp64 and fp32 blocks (every n).  Both are packed into
zeroed buffers and the whole buffers compared.  Shapes: the smallest at which
the byte kernel can go wrong -- one row, more rows than a wave carries, more
than one workgroup; rows that break 16-byte alignment (n = 31, 100), the MNIST
and SIFT widths; ld > n; a source one byte into its allocation."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(1, 128), (130, 256), (1000, 1024)]      # (rows, cap): cap = rows rounded up to 128


def values(rows, n, seed=0):
    """uniform over 0..255, a forced 0 and 255 in the first and the last row,
    one all-255 row (the largest norm; sum (x - 128)^2 at its extremes)"""
    rng = np.random.default_rng(seed + 1000 * rows + n)
    V = rng.integers(0, 256, (rows, n)).astype(np.uint8)
    if rows >= 3:
        V[rows // 2] = 255
    for r in (0, rows - 1):
        V[r, 0] = 0
        V[r, n - 1] = 255
    return V


def sources(torch, V, layout, pad, offset):
    """the values laid out as a pack source with leading dimension ld = its
    minimum + pad: (u8 device tensor, its pointer `offset` bytes into the
    allocation, fp64 device tensor, ld)"""
    rows, n = V.shape
    if layout == "row":
        ld = n + pad
        H = np.zeros((rows, ld), dtype=np.uint8)
        H[:, :n] = V
    else:
        ld = rows + pad
        H = np.zeros((n, ld), dtype=np.uint8)
        H[:, :rows] = V.T
    flat = H.reshape(-1)
    dev = torch.device("cuda", 0)
    d8 = torch.zeros(flat.size + offset, dtype=torch.uint8, device=dev)
    d8[offset:].copy_(torch.from_numpy(flat))
    d64 = torch.from_numpy(flat.astype(np.float64)).to(dev)
    return d8, d8.data_ptr() + offset, d64, ld


def pack_pair(torch, knn, V, cap, layout, pad, offset, kind):
    """(block from the u8 source, block from the fp64 source) as host bytes;
    kind "s8", "f64" or "f32\""""
    rows, n = V.shape
    d8, p8, d64, ld = sources(torch, V, layout, pad, offset)
    lay = knn.ROWMAJOR if layout == "row" else knn.COLMAJOR
    nbytes = knn.s8_block_bytes(cap, n) if kind == "s8" else knn.block_bytes(cap, n, kind)
    out = []
    for ptr, sd in ((p8, "u8"), (d64.data_ptr(), "f64")):
        blk = torch.zeros(nbytes, dtype=torch.uint8, device=d8.device)
        if kind == "s8":
            knn.block_pack_s8(blk.data_ptr(), cap, rows, n, ptr, ld, lay, src_dtype=sd)
        else:
            knn.block_pack(blk.data_ptr(), cap, rows, n, ptr, ld, lay, dtype=kind, src_dtype=sd)
        torch.cuda.synchronize()
        out.append(blk.cpu().numpy())
    return out


VARIANTS = [("row", 0, 0), ("row", 3, 0), ("row", 0, 1), ("row", 3, 1), ("col", 0, 0), ("col", 5, 0), ("col", 0, 1)]


@pytest.mark.parametrize("n", [1, 31, 100, 128, 784])
@pytest.mark.parametrize("rows,cap", SHAPES)
def test_u8_pack_equals_f64_pack(knn, rows, cap, n):
    import torch
    V = values(rows, n)
    for layout, pad, offset in VARIANTS:
        for kind in ("s8", "f64", "f32"):
            a, b = pack_pair(torch, knn, V, cap, layout, pad, offset, kind)
            assert np.array_equal(a, b), (kind, layout, pad, offset)
        # the meta the u8 byte pack wrote: integer words, and the search may start from it
        moff = knn.s8_block_meta_offset(cap, n)
        a, _ = pack_pair(torch, knn, V, cap, layout, pad, offset, "s8")
        meta = a[moff:moff + 64].view(np.float64)
        sq = (V.astype(np.int64) ** 2).sum(axis=1).max()
        assert list(meta[:6]) == [float(V.max()), float(sq), 0.0, 0.0, float(V.max()), 0.0] and meta[7] == 1.0
        assert knn.s8_spec_ok(meta, n, "f64")
        # the byte image: x ^ 0x80, zero past n and on padding rows
        rs = (n + 31) // 32 * 32
        img = a[:(cap + 127) // 128 * 128 * rs].reshape(-1, rs)
        assert np.array_equal(img[:rows, :n], V ^ 0x80)
        assert not img[:rows, n:].any() and not img[rows:].any()


def test_u8_pack_dt_n1000(knn):
    """above the int8 limit: the element pack only -- block, norms and meta
    (max norm = 1000 * 255^2 for the all-255 row)"""
    import torch
    rows, cap, n = 130, 256, 1000
    V = values(rows, n)
    for layout, pad, offset in VARIANTS:
        for kind in ("f64", "f32"):
            a, b = pack_pair(torch, knn, V, cap, layout, pad, offset, kind)
            assert np.array_equal(a, b), (kind, layout, pad, offset)
            moff = knn.block_meta_offset(cap, n, kind)
            meta = a[moff:moff + 64].view(np.float64)
            assert meta[0] == 255.0 and meta[1] == 1000 * 255.0 ** 2 and not meta[2:4].any()
    # and the byte pack refuses n > 896 for this source as for the others
    d8, p8, d64, ld = sources(torch, V, "row", 0, 0)
    blk = torch.zeros(knn.s8_block_bytes(cap, n), dtype=torch.uint8, device=d8.device)
    with pytest.raises(knn.KnnError) as e:
        knn.block_pack_s8(blk.data_ptr(), cap, rows, n, p8, ld, knn.ROWMAJOR, src_dtype="u8")
    assert e.value.status == knn.ERR_INVALID
