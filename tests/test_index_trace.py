"""The index's device calls, traced on a CPU, and its failure paths swept.

tests/index_trace/index_trace.c links knn_index.c and knn_blocks.c against
stubs of the HIP runtime, of the engine boundary (knn_ctx_*, knn_block_pack_*)
and of the kernel launchers; every stub logs its call, so a scenario's trace is
the sequence of allocations, copies, launches and waits the index makes for it.
The size and predicate helpers are knn_engine.c's own: it is linked behind the
harness, whose definitions win (--allow-multiple-definition), and the engine
code nothing then references is dropped with its imports (--gc-sections).

tests/index_trace/expected/NAME.txt holds each scenario's trace as recorded
from the knn_index.c before its entry points were folded onto shared helpers
(add_reblock and add_reblock_real once more behind the one change the fold
made: a rebuilt block's meta words go out as async copies from a staging
array).  The classify_* traces (knn_index_classify, knn_index_classify_rows:
the labels' device copy, its stale range, the vote's buffer, the vote) were
recorded from the knn_index.c before its device memory got one owner.  It is
the definition of "the index does what it did" on success paths; to record a
scenario again: index_trace NAME > expected/NAME.txt.

The sweep (index_trace --sweep, described in index_trace.c) fails every
fallible call of every step in turn and checks what the failed call left.
"""
import glob
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
HERE = os.path.join(ROOT, "tests", "index_trace")
CSRC = os.path.join(ROOT, "mpi-knn_amd", "csrc")

EXPECTED = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(HERE, "expected", "*.txt")))


def build(exe, extra=()):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    return subprocess.run([
        cc, "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__",
        "-ffunction-sections", "-fdata-sections", *extra,
        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + os.path.join(ROCM, "include"), "-o", exe,
        os.path.join(HERE, "index_trace.c"), os.path.join(CSRC, "knn_index.c"), os.path.join(CSRC, "knn_blocks.c"),
        os.path.join(CSRC, "knn_engine.c"), "-Wl,--gc-sections,--allow-multiple-definition", "-lm"],
        capture_output=True, text=True)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("index_trace") / "index_trace")
    res = build(path)
    assert res.returncode == 0, res.stderr
    return path


@pytest.fixture(scope="module")
def traces(exe):
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    res, cur = {}, None
    for line in out.splitlines():
        if line.startswith("## "):
            cur = res.setdefault(line[3:], [])
        else:
            cur.append(line)
    return res


def test_every_scenario_is_recorded(traces):
    assert sorted(traces) == EXPECTED and len(EXPECTED) >= 30


@pytest.mark.parametrize("name", EXPECTED)
def test_trace_is_the_recorded_one(traces, name):
    with open(os.path.join(HERE, "expected", name + ".txt")) as fh:
        want = fh.read().splitlines()
    assert want[0] == "## " + name
    assert traces[name] == want[1:]


def check_sweep(res):
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-4000:]
    last = res.stdout.splitlines()[-1].split()
    # "sweep: S steps, F faults, V violations"
    assert last[0] == "sweep:" and int(last[1]) >= 123 and int(last[3]) >= 2164 and int(last[5]) == 0, res.stdout


def test_fault_sweep(exe):
    check_sweep(subprocess.run([exe, "--sweep"], capture_output=True, text=True))


def test_traces_and_sweep_under_sanitizers(tmp_path, traces):
    """The same program built with the address and undefined-behaviour
    sanitizers (a program of its own: nothing is preloaded)."""
    path = str(tmp_path / "index_trace_san")
    res = build(path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"))
    if res.returncode != 0 and any(w in res.stderr for w in ("sanitize", "asan", "ubsan")):
        pytest.skip("-fsanitize=address,undefined does not link here: " + res.stderr.strip().splitlines()[-1])
    assert res.returncode == 0, res.stderr
    out = subprocess.run([path], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
    assert out.stdout.splitlines() == [x for n in traces for x in ["## " + n] + traces[n]]
    check_sweep(subprocess.run([path, "--sweep"], capture_output=True, text=True))
