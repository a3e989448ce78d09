"""knn_index_classify / knn_index_classify_rows without a GPU: both are
declared in include/knn.h and exported, refuse a NULL index before any device
call, and the Python wrappers refuse a closed index and a Q of the wrong
width."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

import test_abi

NAMES = ("knn_index_classify", "knn_index_classify_rows")


def test_declared_and_exported(knn):
    out = subprocess.check_output(["nm", "-D", "--defined-only", knn.LIB_PATH]).decode()
    exported = set(re.findall(r" T (knn_\w+)", out))
    for name in NAMES:
        assert name in test_abi.header_functions() and name in exported and name in knn.API_SYMBOLS
        assert getattr(knn.lib, name).argtypes
    # the header / nm comparison of test_abi.py still holds
    assert exported == set(test_abi.header_functions()) == set(knn.API_SYMBOLS)


def test_null_index_is_invalid_without_a_device(knn):
    q = ctypes.c_void_p(8)   # never dereferenced: argument checks come first
    hit = ctypes.c_size_t(7)
    assert knn.lib.knn_index_classify(None, q, 4, 1, 0, 3, 10, 0, 0, None, q, None, ctypes.byref(hit), None) == \
        knn.ERR_INVALID
    assert knn.lib.knn_index_classify_rows(None, None, 0, 3, 10, 0, 0, q, None, ctypes.byref(hit), None) == \
        knn.ERR_INVALID
    assert hit.value == 7


def closed_index(knn, n):
    ix = knn.Index.__new__(knn.Index)   # no device: what close() leaves behind
    ix._h, ix.m, ix.n, ix.layout, ix.dtype = ctypes.c_void_p(), 5, n, "row", "f64"
    return ix


def test_wrappers_refuse_a_closed_index(knn):
    ix = closed_index(knn, 4)
    with pytest.raises(ValueError, match="closed"):
        ix.classify(np.zeros((2, 4)))
    with pytest.raises(ValueError, match="closed"):
        ix.classify_rows(None)


def test_wrapper_refuses_a_wrong_width(knn):
    ix = closed_index(knn, 4)
    ix._h = ctypes.c_void_p(8)   # never reaches the library: the width is checked first
    try:
        with pytest.raises(ValueError, match=r"\(mq, 4\)"):
            ix.classify(np.zeros((2, 5)))
        with pytest.raises(ValueError, match="qlabels"):
            ix.classify(np.zeros((2, 4)), qlabels=[1.0, 2.0, 3.0])
    finally:
        ix._h = ctypes.c_void_p()
