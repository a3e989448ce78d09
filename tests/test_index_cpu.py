"""The resident index and the KNN_U8 source type without a GPU: every
argument check of knn_index_* returns its status before any device call, a
valid create reports the missing device, the pack entry points take KNN_U8 as
a source and nothing takes it as a block or search dtype."""
import ctypes

import numpy as np
import pytest


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except ImportError:
        return True


def _create(knn, X, m, n, layout, src, dtype, flags, handle=True):
    h = ctypes.c_void_p()
    rc = knn.lib.knn_index_create(ctypes.byref(h) if handle else None, _p(X), m, n, layout, src, None, dtype, flags)
    if rc == knn.OK:
        knn.lib.knn_index_destroy(h)
    return rc


def test_index_create_argument_checks(knn):
    X = np.ones((5, 3))
    ok = dict(X=X, m=5, n=3, layout=knn.ROWMAJOR, src=knn.F64, dtype=knn.F64, flags=0)

    def call(**kw):
        a = dict(ok, **kw)
        return _create(knn, a["X"], a["m"], a["n"], a["layout"], a["src"], a["dtype"], a["flags"],
                       a.get("handle", True))

    assert call(handle=False) == knn.ERR_INVALID
    assert call(X=None) == knn.ERR_INVALID
    assert call(m=0) == knn.ERR_INVALID
    assert call(n=0) == knn.ERR_INVALID
    assert call(layout=2) == knn.ERR_INVALID
    assert call(layout=-1) == knn.ERR_INVALID
    assert call(flags=1) == knn.ERR_INVALID                 # KNN_QUERY_KEEP_ZERO is a query flag
    assert call(flags=knn.INDEX_DEVICE_OUT) == knn.ERR_INVALID
    assert call(flags=8) == knn.ERR_INVALID
    assert call(m=2 ** 31) == knn.ERR_INVALID               # m + mq > INT32_MAX for every mq
    assert call(src=3) == knn.ERR_UNSUPPORTED
    assert call(src=-1) == knn.ERR_UNSUPPORTED
    assert call(dtype=knn.U8) == knn.ERR_UNSUPPORTED        # a source type only
    assert call(dtype=7) == knn.ERR_UNSUPPORTED


def test_index_query_info_destroy_null(knn):
    Q = np.ones((2, 3))
    out = np.zeros((2, 2), dtype=knn.NB_DTYPE)
    assert knn.lib.knn_index_query(None, _p(Q), 2, knn.ROWMAJOR, knn.F64, 2, 0, _p(out)) == knn.ERR_INVALID
    assert knn.lib.knn_index_destroy(None) == knn.ERR_INVALID
    m = ctypes.c_size_t()
    assert knn.lib.knn_index_info(None, ctypes.byref(m), None, None, None, None) == knn.ERR_INVALID


@pytest.mark.skipif(not _no_gpu(), reason="GPU present")
@pytest.mark.parametrize("src", ["f64", "f32", "u8"])
def test_index_create_no_device(knn, src):
    X = np.ones((5, 3), dtype={"f64": np.float64, "f32": np.float32, "u8": np.uint8}[src])
    assert _create(knn, X, 5, 3, knn.ROWMAJOR, knn.SRC_DTYPES[src], knn.F64, 0) == knn.ERR_NODEVICE
    with pytest.raises(knn.KnnError) as e:
        knn.Index(X)
    assert e.value.status == knn.ERR_NODEVICE


@pytest.mark.skipif(not _no_gpu(), reason="GPU present")
def test_pack_accepts_u8_source(knn):
    """KNN_U8 passes the argument checks of both pack entry points (what
    follows is the launch, which has no device here); an unknown source type
    and KNN_U8 as the block's type still fail them"""
    buf = np.zeros(1 << 16, dtype=np.uint8)
    src = np.zeros(128 * 16, dtype=np.uint8)
    L = knn.lib
    for layout, ld in ((knn.ROWMAJOR, 16), (knn.COLMAJOR, 128)):
        assert L.knn_block_pack_dt(_p(buf), knn.F64, 128, 128, 16, _p(src), knn.U8, ld, layout, None) != knn.ERR_INVALID
        assert L.knn_block_pack_s8(_p(buf), knn.F64, 128, 128, 16, _p(src), knn.U8, ld, layout, None) != knn.ERR_INVALID
    assert L.knn_block_pack_dt(_p(buf), knn.F64, 128, 128, 16, _p(src), 3, 16, knn.ROWMAJOR, None) == knn.ERR_INVALID
    assert L.knn_block_pack_s8(_p(buf), knn.F64, 128, 128, 16, _p(src), 3, 16, knn.ROWMAJOR, None) == knn.ERR_INVALID
    assert L.knn_block_pack_dt(_p(buf), knn.U8, 128, 128, 16, _p(src), knn.U8, 16, knn.ROWMAJOR, None) == knn.ERR_INVALID
    assert L.knn_block_pack_s8(_p(buf), knn.U8, 128, 128, 16, _p(src), knn.U8, 16, knn.ROWMAJOR, None) == knn.ERR_INVALID


def test_u8_is_no_block_or_search_dtype(knn):
    h = ctypes.c_void_p()
    assert knn.lib.knn_ctx_create_dt(ctypes.byref(h), 0, 16, 8, 16, 4, knn.U8) == knn.ERR_INVALID
    assert knn.block_bytes(128, 16, knn.F64) > 0
    assert knn.lib.knn_block_bytes_dt(128, 16, knn.U8) == 0
    assert knn.lib.knn_wire_bytes(128, 16, knn.U8) == 0
    X, out = np.ones((5, 3)), np.zeros((5, 2), dtype=knn.NB_DTYPE)
    assert knn.lib.knn_search(_p(X), 5, 3, knn.ROWMAJOR, None, 2, 1, knn.U8, _p(out)) == knn.ERR_UNSUPPORTED
    assert knn.lib.knn_query(_p(X), 5, _p(X), 5, 3, knn.ROWMAJOR, None, 2, knn.U8, 0, _p(out)) == knn.ERR_UNSUPPORTED
    assert knn.SRC_DTYPES["u8"] == knn.U8 == 2 and "u8" not in knn.DTYPES
