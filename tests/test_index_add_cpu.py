"""Adding rows to a resident index, without a GPU: the three entry points
exist, and every argument check of knn_block_append_dt / knn_block_append_s8
and knn_index_add's NULL index return their status before any device call."""
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


def test_symbols_exist(knn):
    for name in ("knn_index_add", "knn_block_append_dt", "knn_block_append_s8"):
        assert name in knn.API_SYMBOLS
        assert getattr(knn.lib, name).argtypes is not None
    assert callable(knn.Index.add) and callable(knn.block_append) and callable(knn.block_append_s8)


def test_index_add_null(knn):
    X = np.ones((2, 3))
    assert knn.lib.knn_index_add(None, _p(X), 2, knn.ROWMAJOR, knn.F64, None, 0) == knn.ERR_INVALID


@pytest.mark.parametrize("entry", ["knn_block_append_dt", "knn_block_append_s8"])
def test_block_append_argument_checks(knn, entry):
    f = getattr(knn.lib, entry)
    buf = np.zeros(1 << 16, dtype=np.uint8)
    src = np.zeros(128 * 16, dtype=np.uint8)
    ok = dict(blk=buf, dtype=knn.F64, cap=128, row0=64, rows=64, n=16, src=src, sd=knn.U8, ld=16, layout=knn.ROWMAJOR)

    def call(**kw):
        a = dict(ok, **kw)
        return f(_p(a["blk"]), a["dtype"], a["cap"], a["row0"], a["rows"], a["n"], _p(a["src"]), a["sd"], a["ld"],
                 a["layout"], None)

    assert call(row0=65) == knn.ERR_INVALID                  # row0 + rows = cap + 1
    assert call(row0=128, rows=1) == knn.ERR_INVALID
    assert call(row0=2 ** 64 - 8, rows=16) == knn.ERR_INVALID   # the sum wraps
    assert call(rows=0) == knn.ERR_INVALID
    assert call(blk=None) == knn.ERR_INVALID
    assert call(src=None) == knn.ERR_INVALID
    assert call(dtype=knn.U8) == knn.ERR_INVALID
    assert call(sd=3) == knn.ERR_INVALID
    assert call(layout=2) == knn.ERR_INVALID
    assert call(ld=15) == knn.ERR_INVALID
    assert call(layout=knn.COLMAJOR, ld=63) == knn.ERR_INVALID


@pytest.mark.skipif(not _no_gpu(), reason="GPU present")
def test_block_append_accepts_valid_arguments(knn):
    """valid arguments pass the checks of both entry points (what follows is
    the launch, which has no device here), from every source type"""
    buf = np.zeros(1 << 16, dtype=np.uint8)
    src = np.zeros(64 * 16 * 8, dtype=np.uint8)
    L = knn.lib
    for sd in (knn.F64, knn.F32, knn.U8):
        for layout, ld in ((knn.ROWMAJOR, 16), (knn.COLMAJOR, 64)):
            for row0, rows in ((64, 64), (127, 1), (0, 128 // 2), (3, 5)):
                assert L.knn_block_append_dt(_p(buf), knn.F64, 128, row0, min(rows, 64), 16, _p(src), sd, ld, layout,
                                             None) != knn.ERR_INVALID
                assert L.knn_block_append_s8(_p(buf), knn.F32, 128, row0, min(rows, 64), 16, _p(src), sd, ld, layout,
                                             None) != knn.ERR_INVALID
