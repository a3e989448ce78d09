"""Updating rows of a resident index in place, without a GPU: the three entry
points exist; knn_index_update refuses a NULL index and every argument check
of knn_block_scatter_dt / knn_block_scatter_s8 returns its status before any
device call; and the host planning of an update
(mpi-knn_amd/csrc/knn_update_plan.h) agrees with a brute-force restatement
(tests/update_plan/update_plan.c, a stand-alone program built here -- with the
address and undefined-behaviour sanitizers where the toolchain links them)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("knn_index_update", "knn_block_scatter_dt", "knn_block_scatter_s8")


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def test_symbols_exist(knn):
    for name in NEW:
        assert name in knn.API_SYMBOLS
        assert getattr(knn.lib, name).argtypes is not None
    assert callable(knn.Index.update)
    assert callable(knn.block_scatter) and callable(knn.block_scatter_s8)


def test_null_index(knn):
    ids = np.array([1, 2], dtype=np.int32)
    X = np.zeros((2, 4))
    lab = np.zeros(2)
    f = knn.lib.knn_index_update
    assert f(None, _p(ids), 2, _p(X), knn.ROWMAJOR, knn.F64, None, 0) == knn.ERR_INVALID
    assert f(None, _p(ids), 2, _p(X), knn.ROWMAJOR, knn.F64, _p(lab), 0) == knn.ERR_INVALID
    assert f(None, None, 0, None, 7, 9, None, -1) == knn.ERR_INVALID


@pytest.mark.parametrize("entry", ["knn_block_scatter_dt", "knn_block_scatter_s8"])
def test_block_scatter_argument_checks(knn, entry):
    """(host buffers stand in for device pointers: no check reads them)"""
    f = getattr(knn.lib, entry)
    blk = np.zeros(1 << 12, dtype=np.uint8)
    src = np.zeros(1 << 12, dtype=np.uint8)
    pos = np.zeros(64, dtype=np.int32)
    srow = np.zeros(64, dtype=np.int32)
    ok = dict(blk=blk, dtype=knn.F64, cap=128, pos=pos, srow=srow, rows=64, n=16, src=src, src_rows=80,
              src_dtype=knn.F64, ld=16, layout=knn.ROWMAJOR)

    def call(**kw):
        a = dict(ok, **kw)
        return f(_p(a["blk"]), a["dtype"], a["cap"], _p(a["pos"]), _p(a["srow"]), a["rows"], a["n"], _p(a["src"]),
                 a["src_rows"], a["src_dtype"], a["ld"], a["layout"], None)

    assert call(blk=None) == knn.ERR_INVALID
    assert call(pos=None) == knn.ERR_INVALID
    assert call(src=None) == knn.ERR_INVALID
    assert call(blk=None, srow=None) == knn.ERR_INVALID       # (a NULL srow alone is no error: see the GPU tests)
    assert call(rows=0) == knn.ERR_INVALID
    assert call(n=0) == knn.ERR_INVALID
    assert call(src_rows=0) == knn.ERR_INVALID
    assert call(cap=2 ** 31) == knn.ERR_INVALID
    assert call(src_rows=2 ** 31, layout=knn.ROWMAJOR) == knn.ERR_INVALID
    assert call(src_rows=2 ** 31, layout=knn.COLMAJOR, ld=2 ** 31) == knn.ERR_INVALID
    assert call(layout=2) == knn.ERR_INVALID
    assert call(layout=-1) == knn.ERR_INVALID
    assert call(layout=knn.ROWMAJOR, ld=15) == knn.ERR_INVALID            # ld < n
    assert call(layout=knn.COLMAJOR, ld=79) == knn.ERR_INVALID            # ld < src_rows
    assert call(layout=knn.COLMAJOR, ld=64) == knn.ERR_INVALID            # (>= rows is not enough)
    assert call(dtype=knn.U8) == knn.ERR_INVALID
    assert call(dtype=7) == knn.ERR_INVALID
    assert call(src_dtype=3) == knn.ERR_INVALID
    assert call(src_dtype=-1) == knn.ERR_INVALID
    if entry == "knn_block_scatter_s8":
        assert call(n=897, ld=897) == knn.ERR_INVALID                     # KNN_I8_MAX_N = 896


def _links(cc, flags, tmp):
    """whether `cc flags` compiles, links and runs a trivial program"""
    src = os.path.join(tmp, "probe.c")
    with open(src, "w") as f:
        f.write("int main(void) { return 0; }\n")
    exe = os.path.join(tmp, "probe")
    try:
        subprocess.check_call([cc] + flags + ["-o", exe, src], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return subprocess.run([exe], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode == 0
    except (subprocess.CalledProcessError, OSError):
        return False


def test_update_plan_against_brute_force(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    flags = san if _links(cc, san, str(tmp_path)) else []
    exe = str(tmp_path / "update_plan")
    # (knn_remove_plan.h, included for its id lookup, defines static functions this program does not call)
    subprocess.check_call([cc, "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function"] + flags + [
        "-I" + os.path.join(ROOT, "mpi-knn_amd", "csrc"), "-o", exe,
        os.path.join(ROOT, "tests", "update_plan", "update_plan.c")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print("sanitizers:", "address,undefined" if flags else "none (the toolchain does not link them)")
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("ok:") and int(last.split()[1]) >= 1000
