"""knn_block_scatter_dt / knn_block_scatter_s8 against one-shot packs.  A block
of cap = 300 (384 padded rows) is packed from the 300 rows of X; a scatter
then gives `rows` of its rows new values.  Outside its 8 meta doubles the block
must be byte for byte the block one knn_block_pack_dt / knn_block_pack_s8 of
the updated array writes -- rows, padding, norms, both norm-word arrays of a
byte block -- and its meta must be, word by word and exactly, max(the meta
before, the meta of a pack of the listed source rows alone), word 7 as it was.

n = 20, 70 (crosses the 64-column tile of the column kernels), 130 (rs = 160:
16 lanes a row in the u8 kernel); rows = 1, 5, 67 (straddles a 64-row
workgroup); positions unsorted, with 0, 299 and both neighbours of multiples
of 64; srow NULL, and a reversed list with gaps over a larger source; both
layouts with ld above the minimum, the row-major source once 16-byte aligned
(the vector loads) and once offset by one element (the scalar loads); sources
f64, f32, u8; blocks f64, f32.  Also: a block scattered into twice and then
appended to, real-valued rows (the fp norms bit for bit), and list entries
outside the block or the source, which write nothing."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAP = ROWS = 300
NP_SRC = {"f64": np.float64, "f32": np.float32, "u8": np.uint8}
POS = {1: [299], 5: [299, 0, 64, 63, 127]}


def positions(rows):
    """`rows` distinct block rows, unsorted: 0, 299, and both sides of 64, 128, 192, 256"""
    if rows in POS:
        return np.array(POS[rows], dtype=np.int32)
    must = [299, 0, 64, 63, 127, 128, 65, 192, 191, 129, 256, 255, 257]
    rng = np.random.default_rng(rows)
    rest = [p for p in rng.permutation(ROWS).tolist() if p not in must][:rows - len(must)]
    out = np.array(must[:4] + rest + must[4:], dtype=np.int32)
    assert len(out) == rows and len(set(out.tolist())) == rows and (np.diff(out) < 0).any()
    return out


def base_values(n):
    rng = np.random.default_rng(1000 * ROWS + n)
    V = rng.integers(0, 201, (ROWS, n)).astype(np.float64)
    V[0, 0] = 0.0
    V[ROWS - 1, n - 1] = 200.0
    return V


def new_values(rows, n, src_rows):
    """the source: integers in [0, 255]; one row alone stays below the block's maximum (the meta stays)"""
    rng = np.random.default_rng(7 * rows + n)
    top = 101 if rows == 1 else 256
    W = rng.integers(0, top, (src_rows, n)).astype(np.float64)
    if rows > 1:
        W[src_rows // 2] = 255.0
    return W


class Dev:
    """device buffers of one test, kept alive until it ends"""

    def __init__(self, knn):
        import torch
        self.torch, self.knn, self.keep = torch, knn, []
        self.dev = torch.device("cuda", 0)

    def put(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.keep.append(t)
        return t

    def source(self, W, form, src):
        """W as a device source: (pointer, ld, layout code).  form: 'row' --
        16-byte-aligned rows, ld = round_up(n, 16) + 16; 'rowoff' -- ld = n + 3
        and the array one element into its buffer; 'col' -- ld = rows + 5"""
        knn = self.knn
        A = W.astype(NP_SRC[src])
        r, n = A.shape
        es = A.itemsize
        if form == "col":
            ld = r + 5
            buf = np.full((n, ld), 77, dtype=A.dtype)
            buf[:, :r] = A.T
            return self.put(buf).data_ptr(), ld, knn.COLMAJOR
        ld = (n + 15) // 16 * 16 + 16 if form == "row" else n + 3
        off = 0 if form == "row" else 1
        buf = np.full(off + r * ld, 77, dtype=A.dtype)
        buf[off:].reshape(r, ld)[:, :n] = A
        t = self.put(buf)
        assert t.data_ptr() % 16 == 0
        return t.data_ptr() + off * es, ld, knn.ROWMAJOR

    def pack(self, V, s8, n, dtype, rows=None, col=False):
        """a zero-filled buffer with the block of V's first `rows` rows (from
        an fp64 source, row-major or column-major)"""
        knn = self.knn
        nbytes = knn.s8_block_bytes(CAP, n) if s8 else knn.block_bytes(CAP, n, dtype)
        b = self.torch.zeros(nbytes, dtype=self.torch.uint8, device=self.dev)
        t = self.put(V.T if col else V)
        (knn.block_pack_s8 if s8 else knn.block_pack)(b.data_ptr(), CAP, len(V) if rows is None else rows, n,
                                                      t.data_ptr(), len(V) if col else n,
                                                      knn.COLMAJOR if col else knn.ROWMAJOR, dtype=dtype)
        return b

    def scatter(self, b, s8, n, dtype, pos, srow, W, form, src):
        knn = self.knn
        ptr, ld, lay = self.source(W, form, src)
        d_pos = self.put(np.asarray(pos, dtype=np.int32))
        d_srow = 0 if srow is None else self.put(np.asarray(srow, dtype=np.int32)).data_ptr()
        (knn.block_scatter_s8 if s8 else knn.block_scatter)(b.data_ptr(), CAP, d_pos.data_ptr(), d_srow, len(pos), n,
                                                            ptr, len(W), ld, lay, dtype=dtype, src_dtype=src)

    def host(self, b):
        self.torch.cuda.synchronize()
        return b.cpu().numpy()


def moff_of(knn, s8, n, dtype):
    return knn.s8_block_meta_offset(CAP, n) if s8 else knn.block_meta_offset(CAP, n, dtype)


def split(a, moff):
    """(everything outside the meta, the 8 meta doubles)"""
    return np.concatenate([a[:moff], a[moff + 64:]]), a[moff:moff + 64].view(np.float64)


@pytest.mark.parametrize("n", [20, 70, 130])
@pytest.mark.parametrize("form", ["elem", "s8"])
def test_scatter_equals_pack(knn, form, n):
    s8 = form == "s8"
    d = Dev(knn)
    X = base_values(n)
    for dtype in ("f64", "f32"):
        moff = moff_of(knn, s8, n, dtype)
        before_meta = split(d.host(d.pack(X, s8, n, dtype)), moff)[1].copy()
        assert before_meta[0] == 200.0 and before_meta[7] == (1.0 if s8 else 0.0)
        for rows in (1, 5, 67):
            pos = positions(rows)
            for srow_mode in ("none", "rev"):
                src_rows = rows if srow_mode == "none" else 2 * rows + 3
                srow = None if srow_mode == "none" else (src_rows - 1 - 2 * np.arange(rows)).astype(np.int32)
                W = new_values(rows, n, src_rows)
                listed = W if srow is None else W[srow]
                Y = X.copy()
                Y[pos] = listed
                want, _ = split(d.host(d.pack(Y, s8, n, dtype)), moff)
                alone = split(d.host(d.pack(listed, s8, n, dtype)), moff)[1]
                want_meta = np.maximum(before_meta, alone)
                want_meta[7] = before_meta[7]
                assert (want_meta[0] == 255.0) == (rows > 1)
                for src_form in ("row", "rowoff", "col"):
                    for src in ("f64", "f32", "u8"):
                        what = (form, n, dtype, rows, srow_mode, src_form, src)
                        b = d.pack(X, s8, n, dtype)
                        d.scatter(b, s8, n, dtype, pos, srow, W, src_form, src)
                        got, meta = split(d.host(b), moff)
                        assert np.array_equal(got, want), what
                        assert np.array_equal(meta, want_meta), (what, meta, want_meta)
                d.keep.clear()
    # the comparison saw the new rows
    assert not np.array_equal(want, split(d.host(d.pack(X, s8, n, dtype)), moff)[0])


@pytest.mark.parametrize("form", ["elem", "s8"])
def test_scatter_twice_then_append(knn, form):
    """a block packed over its first 200 rows, scattered into twice (the second
    time partly over the first's rows), then appended to"""
    s8 = form == "s8"
    n = 70
    d = Dev(knn)
    X = base_values(n)
    rng = np.random.default_rng(4)
    p1 = rng.permutation(200)[:67].astype(np.int32)
    p2 = np.concatenate([p1[:20][::-1], np.setdiff1d(np.arange(200), p1)[:30][::-1]]).astype(np.int32)
    W1, W2 = new_values(67, n, 67), new_values(50, n, 50) / 1.0
    W2[3, 5] = 254.0
    Y = X.copy()
    Y[p1] = W1
    Y[p2] = W2
    for dtype in ("f64", "f32"):
        moff = moff_of(knn, s8, n, dtype)
        for src_form in ("row", "col"):
            b = d.pack(X, s8, n, dtype, rows=200)
            d.scatter(b, s8, n, dtype, p1, None, W1, src_form, "f64")
            d.scatter(b, s8, n, dtype, p2, None, W2, src_form, "u8")
            ptr, ld, lay = d.source(X[200:], src_form, "f32")
            (knn.block_append_s8 if s8 else knn.block_append)(b.data_ptr(), CAP, 200, 100, n, ptr, ld, lay,
                                                              dtype=dtype, src_dtype="f32")
            got, meta = split(d.host(b), moff)
            want, _ = split(d.host(d.pack(Y, s8, n, dtype)), moff)
            assert np.array_equal(got, want), (form, dtype, src_form)
            # max over the first pack, both scatters' rows (overwritten ones included) and the append
            parts = [X, W1, W2]
            assert meta[0] == max(np.abs(v).max() for v in parts) == 255.0
            assert meta[1] == max((v * v).sum(1).max() for v in parts)
            assert meta[2] == 0.0 and meta[3] == 0.0 and meta[5] == 0.0 and meta[7] == (1.0 if s8 else 0.0)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_scatter_real_valued(knn, dtype):
    """real-valued rows: a row's fp norm is summed by the same lanes in the same
    order whichever source row it is and wherever it lands (the pack it is
    compared with reads the layout the scatter reads: the row and the column
    kernels sum in different orders)"""
    n, rows = 70, 67
    d = Dev(knn)
    rng = np.random.default_rng(8)
    X = rng.normal(0, 1, (ROWS, n))
    pos = positions(rows)
    src_rows = 2 * rows + 3
    srow = (src_rows - 1 - 2 * np.arange(rows)).astype(np.int32)
    W = rng.normal(0, 3, (src_rows, n))
    moff = moff_of(knn, False, n, dtype)
    for src in ("f64", "f32"):
        Ws = W.astype(NP_SRC[src]).astype(np.float64)
        Y = X.copy()
        Y[pos] = Ws[srow]
        for src_form in ("row", "rowoff", "col"):
            col = src_form == "col"
            before = split(d.host(d.pack(X, False, n, dtype, col=col)), moff)[1].copy()
            want, _ = split(d.host(d.pack(Y, False, n, dtype, col=col)), moff)
            alone = split(d.host(d.pack(Ws[srow], False, n, dtype, col=col)), moff)[1]
            b = d.pack(X, False, n, dtype, col=col)
            d.scatter(b, False, n, dtype, pos, srow, W, src_form, src)
            got, meta = split(d.host(b), moff)
            assert np.array_equal(got, want), (dtype, src, src_form)
            assert np.array_equal(meta, np.maximum(before, alone)) and meta[2] == 1.0, (dtype, src, src_form)
    es = 8 if dtype == "f64" else 4
    npad = (n * es + 127) // 128 * 128 // es
    norms = want[384 * npad * es:384 * npad * es + ROWS * es].view(np.float64 if dtype == "f64" else np.float32)
    assert (norms > 0).all() and len(np.unique(norms)) > ROWS // 2


@pytest.mark.parametrize("form", ["elem", "s8"])
def test_entries_outside_write_nothing(knn, form):
    """pos outside [0, cap) (cap = 300: the padded rows 300 .. 383 included) and
    srow outside [0, src_rows) leave the block's rows as they were"""
    s8 = form == "s8"
    n = 70
    d = Dev(knn)
    X = base_values(n)
    pos = np.array([5, -1, 300, 64, 383, 2 ** 30, 7, 63, -2 ** 31, 299], dtype=np.int32)
    srow = np.array([0, 1, 2, 3, 4, 5, -1, 12, 8, 11], dtype=np.int32)
    W = new_values(12, n, 12)
    Y = X.copy()
    for p, s in zip(pos.tolist(), srow.tolist()):
        if 0 <= p < CAP and 0 <= s < 12:
            Y[p] = W[s]
    for dtype in ("f64", "f32"):
        moff = moff_of(knn, s8, n, dtype)
        want, _ = split(d.host(d.pack(Y, s8, n, dtype)), moff)
        for src_form in ("row", "rowoff", "col"):
            for src in ("f64", "u8"):
                b = d.pack(X, s8, n, dtype)
                d.scatter(b, s8, n, dtype, pos, srow, W, src_form, src)
                got, meta = split(d.host(b), moff)
                assert np.array_equal(got, want), (form, dtype, src_form, src)
                assert meta[7] == (1.0 if s8 else 0.0) and 200.0 <= meta[0] <= 255.0
