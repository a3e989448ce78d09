"""Neighbours of resident rows by id, without a GPU: the three entry points
exist; knn_index_neighbours refuses a NULL index and every argument check of
knn_block_gather_pos_dt / knn_block_gather_pos_s8 returns its status before any
device call; and the id -> position mapping of the call
(mpi-knn_amd/csrc/knn_neighbours_plan.h) agrees with a brute-force restatement
(tests/neighbours_plan/neighbours_plan.c, a stand-alone program built here --
with the address and undefined-behaviour sanitizers where the toolchain links
them)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("knn_index_neighbours", "knn_block_gather_pos_dt", "knn_block_gather_pos_s8")


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def test_symbols_exist(knn):
    for name in NEW:
        assert name in knn.API_SYMBOLS
        assert getattr(knn.lib, name).argtypes is not None
    assert callable(knn.Index.neighbours)
    assert callable(knn.block_gather_pos) and callable(knn.block_gather_pos_s8)


def test_null_index(knn):
    ids = np.array([1, 2], dtype=np.int32)
    out = np.zeros(2 * 30, dtype=knn.NB_DTYPE)
    f = knn.lib.knn_index_neighbours
    assert f(None, _p(ids), 2, 30, 0, _p(out)) == knn.ERR_INVALID
    assert f(None, None, 0, 30, knn.QUERY_KEEP_ZERO, _p(out)) == knn.ERR_INVALID
    assert f(None, None, 0, 30, knn.INDEX_DEVICE_OUT, _p(out)) == knn.ERR_INVALID
    assert f(None, None, 5, -1, 64, None) == knn.ERR_INVALID


@pytest.mark.parametrize("entry", ["knn_block_gather_pos_dt", "knn_block_gather_pos_s8"])
def test_block_gather_pos_argument_checks(knn, entry):
    """(host buffers stand in for device pointers: no check reads them)"""
    f = getattr(knn.lib, entry)
    dst = np.zeros(1 << 12, dtype=np.uint8)
    tab = np.zeros(3, dtype=np.uint64)
    pos = np.zeros(64, dtype=np.int32)
    ok = dict(dst=dst, dst_cap=128, row0=10, tab=tab, src_cap=256, nblk=3, pos=pos, rows=64, n=16, dtype=knn.F64)

    def call(**kw):
        a = dict(ok, **kw)
        args = [_p(a["dst"]), a["dst_cap"], a["row0"], _p(a["tab"]), a["src_cap"], a["nblk"], _p(a["pos"]), a["rows"],
                a["n"]]
        if entry == "knn_block_gather_pos_dt":
            args.append(a["dtype"])
        return f(*args, None)

    assert call(dst=None) == knn.ERR_INVALID
    assert call(tab=None) == knn.ERR_INVALID                  # a NULL table
    assert call(pos=None) == knn.ERR_INVALID
    assert call(nblk=0) == knn.ERR_INVALID
    assert call(rows=0) == knn.ERR_INVALID
    assert call(n=0) == knn.ERR_INVALID
    assert call(src_cap=0) == knn.ERR_INVALID
    assert call(dst_cap=2 ** 31) == knn.ERR_INVALID
    assert call(src_cap=2 ** 31) == knn.ERR_INVALID
    assert call(row0=129) == knn.ERR_INVALID                  # row0 > dst_cap
    assert call(row0=65) == knn.ERR_INVALID                   # row0 + rows > dst_cap
    assert call(row0=0, rows=129) == knn.ERR_INVALID
    assert call(tab=dst) == knn.ERR_INVALID                   # d_dst == the table: knn_block_gather_dt's d_dst == d_src
    if entry == "knn_block_gather_pos_dt":
        assert call(dtype=knn.U8) == knn.ERR_INVALID
        assert call(dtype=7) == knn.ERR_INVALID
        assert call(n=2 ** 31) == knn.ERR_INVALID
    else:
        assert call(n=897) == knn.ERR_INVALID                 # KNN_I8_MAX_N = 896


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


def test_neighbours_plan_against_brute_force(tmp_path):
    """no map, a map with gaps, dead and out-of-range ids, repeats that keep
    their order, count = 1, and the NULL list"""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    flags = san if _links(cc, san, str(tmp_path)) else []
    exe = str(tmp_path / "neighbours_plan")
    # (knn_remove_plan.h, included for its id lookup, defines static functions this program does not call)
    subprocess.check_call([cc, "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function"] + flags + [
        "-I" + os.path.join(ROOT, "mpi-knn_amd", "csrc"), "-o", exe,
        os.path.join(ROOT, "tests", "neighbours_plan", "neighbours_plan.c")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print("sanitizers:", "address,undefined" if flags else "none (the toolchain does not link them)")
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("ok:") and int(last.split()[1]) >= 500
