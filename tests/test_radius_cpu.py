"""Radius search without a GPU: the four entry points exist; the byte path's
integer threshold (mpi-knn_amd/csrc/knn_radius_plan.h) keeps its defining
inequality over a sweep of radii (tests/radius_cpu/radius_threshold.c, a
stand-alone program, built once more with the address and undefined-behaviour
sanitizers); every argument refusal of the four entry points comes before any
device call, a count / fill pair leaves the kept context alone and a failed
call leaves the index answering (tests/radius_cpu/radius_checks.c, on
tests/index_trace's stubs); and the corpora and radii tests/test_gpu_radius.py
uses are worth testing with -- from the numpy reference alone, so that a bad
choice of radius fails here and does not pass vacuously on the GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import radius_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
HERE = os.path.join(ROOT, "tests", "radius_cpu")
CSRC = os.path.join(ROOT, "mpi-knn_amd", "csrc")
SAN = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer")
NEW = ("knn_index_radius_count", "knn_index_radius", "knn_index_radius_rows_count", "knn_index_radius_rows")


def cc():
    c = shutil.which("gcc") or shutil.which("cc")
    assert c, "no C compiler"
    return c


def sanitizers_link(res):
    return not (res.returncode != 0 and any(w in res.stderr for w in ("sanitize", "asan", "ubsan")))


def test_symbols_exist(knn):
    for name in NEW:
        assert name in knn.API_SYMBOLS and getattr(knn.lib, name).argtypes is not None
    for name in ("radius_count", "radius", "radius_rows_count", "radius_rows"):
        assert callable(getattr(knn.Index, name))


# ---------------------------------------------------------- threshold header

def build_threshold(exe, extra=()):
    return subprocess.run([cc(), "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", *extra, "-I" + CSRC,
                           "-o", exe, os.path.join(HERE, "radius_threshold.c"), "-lm"], capture_output=True, text=True)


def run_threshold(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("ok:") and int(last.split()[1]) >= 1000000, last


def test_threshold_inequality(tmp_path):
    exe = str(tmp_path / "radius_threshold")
    res = build_threshold(exe)
    assert res.returncode == 0, res.stderr
    run_threshold(exe)


def test_threshold_under_sanitizers(tmp_path):
    exe = str(tmp_path / "radius_threshold_san")
    res = build_threshold(exe, SAN)
    if not sanitizers_link(res):
        pytest.skip("-fsanitize=address,undefined does not link here: " + res.stderr.strip().splitlines()[-1])
    assert res.returncode == 0, res.stderr
    run_threshold(exe)


# ------------------------------------------- refusals, context, failed calls

def build_checks(exe, extra=()):
    return subprocess.run([
        cc(), "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__",
        "-ffunction-sections", "-fdata-sections", *extra,
        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + os.path.join(ROCM, "include"), "-o", exe,
        os.path.join(HERE, "radius_checks.c"), os.path.join(CSRC, "knn_index.c"), os.path.join(CSRC, "knn_blocks.c"),
        os.path.join(CSRC, "knn_engine.c"), "-Wl,--gc-sections,--allow-multiple-definition", "-lm"],
        capture_output=True, text=True)


def run_checks(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1].split()
    # "ok: R refusals, F faults"
    assert last[0] == "ok:" and int(last[1]) >= 46 and int(last[3]) >= 40, last


def test_refusals_context_and_faults(tmp_path):
    exe = str(tmp_path / "radius_checks")
    res = build_checks(exe)
    assert res.returncode == 0, res.stderr
    run_checks(exe)


def test_refusals_context_and_faults_under_sanitizers(tmp_path):
    exe = str(tmp_path / "radius_checks_san")
    res = build_checks(exe, SAN)
    if not sanitizers_link(res):
        pytest.skip("-fsanitize=address,undefined does not link here: " + res.stderr.strip().splitlines()[-1])
    assert res.returncode == 0, res.stderr
    run_checks(exe)


def test_null_index_through_the_library(knn):
    """(the shared library itself: a NULL index is refused with no device)"""
    lib = knn.lib
    a = np.zeros(4, dtype=np.int64)
    p = a.ctypes.data
    assert lib.knn_index_radius_count(None, p, 1, knn.ROWMAJOR, knn.F64, 1.0, 0, p) == knn.ERR_INVALID
    assert lib.knn_index_radius(None, p, 1, knn.ROWMAJOR, knn.F64, 1.0, 0, p, p) == knn.ERR_INVALID
    assert lib.knn_index_radius_rows_count(None, None, 0, 1.0, 0, p) == knn.ERR_INVALID
    assert lib.knn_index_radius_rows(None, None, 0, 1.0, 0, p, p) == knn.ERR_INVALID


# -------------------------------------------------------- fixture properties

@pytest.mark.parametrize("name", R.CASES)
def test_fixture_is_worth_testing_with(name):
    c = R.case(name)
    assert len(c.X) == R.M and np.isfinite(c.r_at) and c.r_at > 0.0
    assert c.r_at in c.d                                     # taken from an actual reference distance
    for keep_zero in (False, True):
        counts, indptr, rec = c.ref(c.r_at, keep_zero)
        assert counts.min() == 0 and counts[0] == 0          # the far query: an empty segment
        assert counts.max() >= 100 and counts[c.q_many] >= 100
        assert (rec["distance"] == c.r_at).any()             # a hit at distance exactly r
        assert (rec["distance"] <= c.r_at).all()
        assert indptr[-1] == len(rec) == counts.sum()
        # at the double below, that row lies at the next representable distance above the radius: no hit
        below = c.ref(c.r_below, keep_zero)
        assert np.nextafter(c.r_below, np.inf) == c.r_at
        assert below[0].sum() == counts.sum() - (c.d == c.r_at).sum() and not (below[2]["distance"] == c.r_at).any()
    # zero-distance pairs: the two zero rules differ, for queries and for rows
    assert (c.d == 0.0).sum() >= 3 * len(c.trips)
    assert c.ref(c.r_at, True)[0].sum() > c.ref(c.r_at, False)[0].sum()
    assert c.rows_ref(c.r_at, True)[0].sum() > c.rows_ref(c.r_at, False)[0].sum()
    assert c.rows_ref(0.0, True)[0].max() == R.GROUP - 1 and not c.rows_ref(0.0, False)[0].any()
    # ties: equal distances inside a segment, resolved by id
    _, ip, rec = c.rows_ref(c.r_at, True)
    g = c.group[5]
    seg = rec[ip[g]:ip[g + 1]]
    assert (np.diff(seg["distance"]) >= 0).all() and (np.diff(seg["idx"][seg["distance"] == 0.0]) > 0).all()


def test_integer_cases_are_byte_path_data():
    for name, n in (("mnist", 784), ("sift", 128), ("n100", 100)):
        c = R.case(name)
        for a in (c.X, c.Q):
            assert a.shape[1] == n and (a == np.rint(a)).all() and a.min() >= 0 and a.max() <= 255
    assert not (R.case("real").X == np.rint(R.case("real").X)).all()
