"""The engine's step schedule, traced on a CPU.

tests/engine_trace/engine_trace.c links knn_engine.c against stubs of the HIP
runtime and of the kernel launchers; every stub logs its call, so a scenario's
trace is the sequence of launches, event records and stream waits the engine
enqueues for it.  The scenarios: a solo one-step int8 search (and one whose
end() gets another stream), a solo context given two steps, six single-block
steps (paired int8 merges; plain fp64), the direct exchange (own block, then 7
blocks in one fused step) on byte blocks and on the split filter, a fused
split-filter step of 9 blocks, and a solo context whose second step is a
fused split-filter step -- each once more with knn_ctx_profile on.

Further scenarios reach every allocation site of knn_engine.c (DESIGN.md has
the table).  tests/engine_trace/expected/NAME.txt holds each scenario's trace
as recorded from the knn_engine.c before its device memory was folded behind
one owner, except that knn_ctx_destroy's lines are in the order the fold gave
them (profiles/engine_fold_ab.md); to record a scenario again:
engine_trace NAME > expected/NAME.txt.  The sweep (engine_trace --sweep,
described in engine_trace.c) fails every fallible call of every call into the
engine in turn and checks what the failed call left.

Names in a trace: S1 and S2 are the caller's streams, S3 and S4 the distance
streams, S5 the merge stream; events are numbered as knn_ctx_create makes
them: ev_m[p] = E(2p+1), ev_ds[p] = E(2p+2).

Checked here: the launches of every scenario, that every merge is ordered
behind the distance launches whose lists it reads (through that step's ev_ds
event, or by running on their stream), and that leaving solo mode in front of
a fused split-filter step gives the schedule of a context that never was solo.
"""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")

DIST = ("knn_launch_dist_i8", "knn_launch_dist_topk", "knn_launch_dist_split_n")
MERGE = ("knn_launch_merge_rank", "knn_launch_merge_n")


HERE = os.path.join(ROOT, "tests", "engine_trace")
EXPECTED = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(HERE, "expected", "*.txt")))
CALLER, CALLER2, MERGE_STREAM = "S1", "S2", "S5"


def ev_ds(p):
    return "E%d" % (2 * p + 2)


def build(exe, extra=()):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    return subprocess.run([
        cc, "-O1", "-g", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", *extra,
        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mpi-knn_amd", "csrc"),
        "-I" + os.path.join(ROCM, "include"), "-o", exe,
        os.path.join(HERE, "engine_trace.c"),
        os.path.join(ROOT, "mpi-knn_amd", "csrc", "knn_engine.c"), "-lm"], capture_output=True, text=True)


def sanitizers_link(flags, tmp):
    """Whether the toolchain links and runs a trivial program with `flags`."""
    cc = shutil.which("gcc") or shutil.which("cc")
    src, probe = str(tmp / "probe.c"), str(tmp / "probe")
    with open(src, "w") as fh:
        fh.write("int main(void) { return 0; }\n")
    try:
        subprocess.check_call([cc, *flags, "-o", probe, src], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return subprocess.run([probe], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode == 0
    except (subprocess.CalledProcessError, OSError):
        return False


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("engine_trace") / "engine_trace")
    res = build(path)
    assert res.returncode == 0, res.stderr
    return path


@pytest.fixture(scope="module")
def traces(exe):
    # (exit status 1: knn_ctx_device_bytes was not the live bytes behind some call)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    res, cur = {}, None
    for line in out.splitlines():
        if line.startswith("## "):
            cur = res.setdefault(line[3:], [])
        else:
            cur.append(line)
    return res


def test_every_scenario_is_recorded(traces):
    assert sorted(traces) == EXPECTED and len(EXPECTED) == 28


@pytest.mark.parametrize("name", EXPECTED)
def test_trace_is_the_recorded_one(traces, name):
    with open(os.path.join(HERE, "expected", name + ".txt")) as fh:
        want = fh.read().splitlines()
    assert want[0] == "## " + name
    assert traces[name] == want[1:]


def check_sweep(res):
    lines = res.stdout.splitlines()
    assert lines, res.stderr[-4000:]
    last = lines[-1].split()
    # "sweep: C calls, F faults, A absorbed, W warm, V violations"
    assert last[0] == "sweep:" and int(last[1]) >= 270 and int(last[3]) >= 5000, res.stdout[-4000:] + res.stderr[-4000:]
    assert res.returncode == 0 and int(last[9]) == 0, res.stdout[-4000:]


def test_fault_sweep(exe):
    check_sweep(subprocess.run([exe, "--sweep"], capture_output=True, text=True))


def test_traces_and_sweep_under_sanitizers(tmp_path, traces):
    """The same program built with the address and undefined-behaviour
    sanitizers (a program of its own: nothing is preloaded)."""
    san = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer")
    if not sanitizers_link(san, tmp_path):
        pytest.skip("-fsanitize=address,undefined does not link here")
    path = str(tmp_path / "engine_trace_san")
    res = build(path, san)
    assert res.returncode == 0, res.stderr
    out = subprocess.run([path], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
    assert out.stdout.splitlines() == [x for n in traces for x in ["## " + n] + traces[n]]
    check_sweep(subprocess.run([path, "--sweep"], capture_output=True, text=True))


def searches(lines):
    """The scenario's searches: each the lines from its begin to its end."""
    out = []
    for line in lines:
        if line == "# begin":
            out.append([])
        elif line == "# destroy":
            break
        if out:
            out[-1].append(line)
    return out


def count(lines, name):
    return sum(1 for x in lines if x.split()[0] == name)


def finalizing(lines):
    """Rank merges that finalize (their record pointer is set)."""
    return sum(1 for x in lines if x.startswith("knn_launch_merge_rank") and " fin 0 " not in x)


# per scenario and search: distance launches, merges, finalizing rank merges,
# k_finalize launches
EXPECT = {
    "solo1_i8": [dict(dist=1, merge=1, fin=1, finalize=0)],
    "solo1_end_other_stream": [dict(dist=1, merge=1, fin=1, finalize=0)],
    # two steps of one size share a merge; no later step: k_finalize
    "solo2_i8": [dict(dist=2, merge=1, fin=0, finalize=1)],
    "six_i8": [dict(dist=6, merge=3, fin=0, finalize=1)],
    "six_f64": [dict(dist=6, merge=6, fin=0, finalize=1)],
    # first search: the pair's lists grow, the own block is merged alone;
    # second: one merge of both steps at end(), finalizing
    "shadow_own_then_7": [dict(dist=2, merge=2, fin=0, finalize=1), dict(dist=2, merge=1, fin=1, finalize=0)],
    "split_own_then_7": [dict(dist=2, merge=2, fin=0, finalize=1), dict(dist=2, merge=1, fin=0, finalize=1)],
    "split_9": [dict(dist=2, merge=2, fin=0, finalize=1)],
    "split_own_then_2": [dict(dist=2, merge=1, fin=0, finalize=1)] * 2,
    "solo_split_own_then_2": [dict(dist=2, merge=1, fin=0, finalize=1)] * 2,
}


@pytest.mark.parametrize("prof", ["", "+prof"])
@pytest.mark.parametrize("name", sorted(EXPECT))
def test_launch_counts(traces, name, prof):
    lines = traces[name + prof]
    ss = searches(lines)
    assert len(ss) == len(EXPECT[name])
    for s, want in zip(ss, EXPECT[name]):
        got = dict(dist=sum(count(s, d) for d in DIST), merge=sum(count(s, m) for m in MERGE),
                   fin=finalizing(s), finalize=count(s, "knn_launch_finalize"))
        assert got == want, (name + prof, s)
    if prof:
        # every step and every merge was bracketed and counted
        last = [x for x in lines if x.startswith("# profiled")][-1]
        steps, merges = map(int, re.match(r"# profiled steps (\d+) merges (\d+)", last).groups())
        assert steps == sum(w["dist"] for w in EXPECT[name])
        assert merges == sum(w["merge"] for w in EXPECT[name])


def test_solo_one_step_has_no_event_traffic(traces):
    """The solo P = 1 search: kernel and merge on the caller's stream, no
    record or wait between begin and the read-back."""
    s = searches(traces["solo1_i8"])[0]
    assert count(s, "hipEventRecord") == 0 and count(s, "hipStreamWaitEvent") == 0
    streams = {stream_of(x) for x in s if x.startswith(DIST + ("knn_launch_merge_rank", "knn_launch_count_out"))}
    assert streams == {CALLER}, s


def test_solo_end_on_second_stream_orders_it(traces):
    """end() on another stream than the solo step's: that stream waits for the
    step's, then carries the merge."""
    s = searches(traces["solo1_end_other_stream"])[0]
    body = s[s.index("# end"):]
    ops = [x for x in body if x.startswith(("hipEventRecord", "hipStreamWaitEvent", "knn_launch_merge_rank"))]
    assert ops[0].split()[2] == CALLER and ops[1].split()[:3] == ["hipStreamWaitEvent", CALLER2, ops[0].split()[1]]
    assert ops[2].split()[-1] == CALLER2


def stream_of(line):
    """The stream a launch line ran on: the last S<id> before a block table."""
    head = line.split(" blocks ")[0]
    return head.split()[-1]


def nsplit_of(line):
    f = line.split()
    return int(f[{"knn_launch_dist_i8": 11, "knn_launch_dist_topk": 14, "knn_launch_dist_split_n": 11,
                  "knn_launch_merge_rank": 8, "knn_launch_merge_n": 7}[f[0]]])


@pytest.mark.parametrize("prof", ["", "+prof"])
@pytest.mark.parametrize("name", sorted(EXPECT))
def test_every_merge_follows_its_distance_launches(traces, name, prof):
    """A merge reads the lists of the oldest unmerged steps.  For each of
    them it runs on the step's distance stream, or its stream (or, in end(),
    the host) has waited for an event recorded on that stream behind the
    launch -- on the merge stream that event is ev_ds of the step's
    partial set."""
    for s in searches(traces[name + prof]):
        pending = []   # [step, stream, splits, events recorded behind the launch]
        waited = {}    # stream -> events it waited for, each with the records it then covered
        step = 0
        for line in s:
            f = line.split()
            if f[0] in DIST:
                pending.append([step, stream_of(line), nsplit_of(line), []])
                step += 1
            elif f[0] == "hipEventRecord":
                for p in pending:
                    if p[1] == f[2]:
                        p[3].append(f[1])
            elif f[0] in ("hipStreamWaitEvent", "hipEventSynchronize"):
                who, ev = (f[1], f[2]) if f[0] == "hipStreamWaitEvent" else ("host", f[1])
                waited.setdefault(who, []).append((ev, [(p[0], ev in p[3]) for p in pending]))
            elif f[0] in MERGE:
                ms, left = stream_of(line), nsplit_of(line)
                while left > 0:
                    assert pending, (name, line)
                    st, ds, ns, _ = pending.pop(0)
                    left -= ns
                    if ds == ms:
                        continue
                    evs = [e for e, cov in waited.get(ms, []) + waited.get("host", []) if (st, True) in cov]
                    assert evs, (name, st, line)
                    if ms == MERGE_STREAM:
                        assert ev_ds(st % 4) in evs, (name, st, line)
                assert left == 0, (name, line)
        assert not pending, (name, pending)


@pytest.mark.parametrize("prof", ["", "+prof"])
def test_solo_then_fused_split_step_is_the_step_schedule(traces, prof):
    """A solo context whose second step is a fused split-filter step leaves
    solo mode in front of it: ev_ds[0] is recorded behind step 0 on the
    caller's stream and the merge stream waits for it; from there on the trace
    is the one of a context that never was solo."""
    for solo, plain in zip(searches(traces["solo_split_own_then_2" + prof]),
                           searches(traces["split_own_then_2" + prof])):
        second = [i for i, x in enumerate(solo) if x == "# step"][1]
        tail = solo[second:]
        leave = ["hipEventRecord %s %s" % (ev_ds(0), CALLER), "hipStreamWaitEvent %s %s 0" % (MERGE_STREAM, ev_ds(0))]
        at = tail.index(leave[0])
        assert tail[at:at + 2] == leave
        # (in front of the step's own first record, that of ev_in)
        assert not any(x.startswith(("hipEventRecord", "knn_launch")) for x in tail[:at])
        del tail[at:at + 2]
        assert tail == plain[[i for i, x in enumerate(plain) if x == "# step"][1]:]
