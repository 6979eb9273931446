"""bin/redecodeStatistics and bin/replayGDBF on the GPU against the reference's recorded runs
(tests/golden/reference_runs_redecode.json). Under LDPC_RNG=glibc with the recorded seeds both
programs reproduce stdout and log byte for byte; the replay program, started from the state
file the statistics program wrote for a frame, reproduces that frame's row and the recorded
traces' sha-256. Under LDPC_RNG=philox a replay of frame k reproduces row k of the statistics
run that wrote its state file."""
import glob
import hashlib
import os
import shutil
import subprocess

import pytest

import rstat_oracle as SO
from conftest import ROOT, code_path

pytestmark = pytest.mark.gpu

STAT = os.path.join(ROOT, "bin", "redecodeStatistics")
REPLAY = os.path.join(ROOT, "bin", "replayGDBF")
RUNS, REPLAYS = SO.golden()


def env_of(**kw):
    env = {k: v for k, v in os.environ.items() if not k.startswith("LDPC_")}
    env.update({k: str(v) for k, v in kw.items()})
    return env


def run_cli(exe, run, cwd, **env):
    alist = code_path(run["code"])
    args = ["log.txt" if x == "@LOG@" else "frame.state" if x == "@STATE@" else x for x in run["args"]]
    cw = [code_path(run["cwfile"])] if run.get("cwfile") else []
    p = subprocess.run([exe, alist] + args + cw, cwd=cwd, env=env_of(**env), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    out = p.stdout.replace(alist, "@ALIST@")
    return out.replace(cw[0], "@CWFILE@") if cw else out


def state_files(cwd):
    return sorted(glob.glob(os.path.join(cwd, "tmp", "*_RanState_*.state")),
                  key=lambda p: int(p.rsplit("_", 1)[1].split(".")[0]))


def workdir(tmp_path, name):
    wd = tmp_path / name
    (wd / "tmp").mkdir(parents=True)
    return str(wd)


@pytest.mark.parametrize("run", RUNS, ids=[r["name"] for r in RUNS])
def test_statistics_cli_reproduces_the_reference(tmp_path, run):
    wd = workdir(tmp_path, "stat")
    out = run_cli(STAT, run, wd, LDPC_SEED=run["seed"])
    assert out == run["stdout"]
    assert open(os.path.join(wd, "log.txt")).read() == run["log"]
    states = state_files(wd)
    assert [os.path.basename(p).split("_", 1)[1] for p in states] == [f.split("_", 1)[1] for f in run["state_files"]]
    for f, (p, rec) in enumerate(zip(states, run["states"])):   # the reference's state: "seed draws"
        text = open(p).read().split("\n")
        assert text[:6] == ["ldpc-rstat-state 1", "rng glibc", "seed %s" % rec.split()[0], "stream 0", "frame %d" % f,
                            "position %s" % rec.split()[1]]


@pytest.mark.parametrize("rep", REPLAYS, ids=[r["name"] for r in REPLAYS])
def test_replay_cli_reproduces_the_reference(tmp_path, rep):
    """From the state file our statistics program wrote for the frame."""
    run = [r for r in RUNS if r["name"] == rep["of"]][0]
    wd = workdir(tmp_path, "stat")
    run_cli(STAT, run, wd, LDPC_SEED=run["seed"])
    rwd = workdir(tmp_path, "replay")
    shutil.copy(state_files(wd)[rep["frame"]], os.path.join(rwd, "frame.state"))
    out = run_cli(REPLAY, rep, rwd, LDPC_SEED=1)          # the state file's seed counts, not this one
    assert out == rep["stdout"]
    assert open(os.path.join(rwd, "log.txt")).read() == rep["log_line"]
    assert rep["log_line"].split("\t", 1)[1] == run["log"].splitlines()[rep["frame"]].split("\t", 1)[1] + "\n"
    for k, tr in enumerate(rep["traces"]):
        (path,) = glob.glob(os.path.join(rwd, "tmp", "*_log.txt_%d.trace" % k))
        raw = open(path, "rb").read()
        assert raw.count(b"\n") == tr["rows"]
        assert hashlib.sha256(raw).hexdigest() == tr["sha256"], k


def test_philox_replay_reproduces_the_statistics_row(tmp_path):
    """LDPC_RNG=philox: frames x attempts batched on the device; the state file holds the global
    frame index, and a replay of frame k gives row k again, with one trace row per iteration."""
    run = RUNS[0]
    wd = workdir(tmp_path, "stat")
    out = run_cli(STAT, run, wd, LDPC_SEED=17, LDPC_RNG="philox", LDPC_BATCH=3)
    table = open(os.path.join(wd, "log.txt")).read().splitlines()
    assert len(table) == 8 and "Final result:" in out
    outcomes = [[int(x) for x in l.split()[1:]] for l in table]
    assert any(0 in r for r in outcomes) and any(max(r) > 0 for r in outcomes)
    rep = REPLAYS[0]
    for k in (0, 5):
        rwd = workdir(tmp_path, "replay%d" % k)
        st = state_files(wd)[k]
        assert open(st).read().split("\n")[:6] == ["ldpc-rstat-state 1", "rng philox", "seed 17", "stream 0", "frame %d" % k,
                                                   "position %d" % k]
        shutil.copy(st, os.path.join(rwd, "frame.state"))
        rout = run_cli(REPLAY, rep, rwd)                    # no LDPC_RNG: the state file says philox
        line = open(os.path.join(rwd, "log.txt")).read()
        assert [int(x) for x in line.split()[1:]] == outcomes[k]
        done = [l for l in rout.splitlines() if l.startswith("Completed phase with ")]
        assert done == ["Completed phase with %d errors." % w for w in outcomes[k]]
        assert len(glob.glob(os.path.join(rwd, "tmp", "*.trace"))) == 6
