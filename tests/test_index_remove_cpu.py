"""Removing rows from a resident index, without a GPU: the four entry points
exist; knn_index_remove / knn_index_last_id refuse a NULL index and every
argument check of knn_block_gather_dt / knn_block_gather_s8 returns its status
before any device call; and the host planning of a removal
(mpi-knn_amd/csrc/knn_remove_plan.h) agrees with a brute-force restatement
(tests/remove_plan/remove_plan.c, a stand-alone program built here -- with the
address and undefined-behaviour sanitizers where the toolchain links them)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("knn_index_remove", "knn_index_last_id", "knn_block_gather_dt", "knn_block_gather_s8")


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def test_symbols_exist(knn):
    for name in NEW:
        assert name in knn.API_SYMBOLS
        assert getattr(knn.lib, name).argtypes is not None
    assert callable(knn.Index.remove) and isinstance(knn.Index.last_id, property)
    assert callable(knn.block_gather) and callable(knn.block_gather_s8)
    assert knn.IndexInfo._fields == ("m", "n", "nblocks", "device_bytes", "last_bits")


def test_null_index(knn):
    ids = np.array([1, 2], dtype=np.int32)
    got = ctypes.c_size_t(7)
    assert knn.lib.knn_index_remove(None, _p(ids), 2, 0, ctypes.byref(got)) == knn.ERR_INVALID
    assert got.value == 7
    assert knn.lib.knn_index_last_id(None, ctypes.byref(got)) == knn.ERR_INVALID
    assert got.value == 7


@pytest.mark.parametrize("entry", ["knn_block_gather_dt", "knn_block_gather_s8"])
def test_block_gather_argument_checks(knn, entry):
    """(host buffers stand in for device pointers: no check reads them)"""
    f = getattr(knn.lib, entry)
    dst = np.zeros(1 << 12, dtype=np.uint8)
    src = np.zeros(1 << 12, dtype=np.uint8)
    lst = np.zeros(64, dtype=np.int32)
    ok = dict(dst=dst, dst_cap=128, row0=64, src=src, src_cap=128, list=lst, rows=64, n=16, dtype=knn.F64)

    def call(**kw):
        a = dict(ok, **kw)
        args = [_p(a["dst"]), a["dst_cap"], a["row0"], _p(a["src"]), a["src_cap"], _p(a["list"]), a["rows"], a["n"]]
        if entry == "knn_block_gather_dt":
            args.append(a["dtype"])
        return f(*args, None)

    assert call(dst=None) == knn.ERR_INVALID
    assert call(src=None) == knn.ERR_INVALID
    assert call(list=None) == knn.ERR_INVALID
    assert call(rows=0) == knn.ERR_INVALID
    assert call(row0=65) == knn.ERR_INVALID                     # row0 + rows = dst_cap + 1
    assert call(row0=128, rows=1) == knn.ERR_INVALID
    assert call(row0=2 ** 64 - 8, rows=16) == knn.ERR_INVALID   # the sum wraps
    assert call(src=dst) == knn.ERR_INVALID                     # dst == src
    assert call(dst_cap=2 ** 31, row0=0) == knn.ERR_INVALID
    assert call(src_cap=2 ** 31) == knn.ERR_INVALID
    if entry == "knn_block_gather_dt":
        assert call(dtype=knn.U8) == knn.ERR_INVALID
        assert call(dtype=7) == knn.ERR_INVALID
    else:
        assert call(n=897) == knn.ERR_INVALID                   # KNN_I8_MAX_N = 896


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


def test_remove_plan_against_brute_force(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    flags = san if _links(cc, san, str(tmp_path)) else []
    exe = str(tmp_path / "remove_plan")
    subprocess.check_call([cc, "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror"] + flags + [
        "-I" + os.path.join(ROOT, "mpi-knn_amd", "csrc"), "-o", exe,
        os.path.join(ROOT, "tests", "remove_plan", "remove_plan.c")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print("sanitizers:", "address,undefined" if flags else "none (the toolchain does not link them)")
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("ok:") and int(last.split()[1]) >= 100
