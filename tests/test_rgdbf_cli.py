"""bin/decodeRSMNGDBF (cli_gdbf.cpp -D redecode ...) against the reference's own stdout.

With LDPC_RNG=glibc (default) and LDPC_SEED equal to the reference's seed, the GPU front-end
must print exactly what the reference's decodeRSMNGDBF printed (golden stdout of
tests/golden/reference_runs_rsmngdbf.json: the maxphase line, the "Phase histogram:" block
after every incremental result, the final block with its empty line) and append the same log
line (per-phase smoothingUsed, trailing maxphase; RNGDBF.cpp:457-483)."""
import os
import subprocess

import pytest

import rgdbf_oracle as RO
from conftest import ROOT, code_path

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "bin", "decodeRSMNGDBF")
RUNS, _ = RO.golden_runs()


@pytest.mark.parametrize("run", RUNS, ids=[r["name"] for r in RUNS])
def test_cli_stdout_identical_to_reference(tmp_path, run):
    alist = code_path(run["code"])
    log = tmp_path / "log.txt"
    cmd = [EXE, alist] + [str(log) if x == "@LOG@" else x for x in run["args"]]
    if run["cwfile"]:
        cmd.append(code_path(run["cwfile"]))
    env = dict(os.environ, LDPC_SEED=str(run["seed"]), LDPC_RNG="glibc")
    env.pop("LDPC_PRECISION", None)
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    out = p.stdout.replace(alist, "@ALIST@").replace(str(log), "@LOGFILE@")
    if run["cwfile"]:
        out = out.replace(code_path(run["cwfile"]), "@CWFILE@")
    assert "Phase histogram:\n\n" in out
    assert out == run["stdout"]
    assert log.read_text().replace(alist, "@ALIST@") == run["log_line"]


def test_cli_philox_batches(tmp_path):
    """LDPC_RNG=philox: frames generated on the GPU in batches; the phase histogram printed
    at the end sums to the words counted, and re-decoding lowers the word errors' share."""
    log = tmp_path / "log.txt"
    run = RUNS[1]
    cmd = [EXE, code_path(run["code"])] + [str(log) if x == "@LOG@" else x for x in run["args"]]
    env = dict(os.environ, LDPC_SEED="7", LDPC_RNG="philox", LDPC_BATCH="2048")
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    tail = p.stdout[p.stdout.rindex("Phase histogram:\n\n") + len("Phase histogram:\n\n"):]
    hist = [int(l.split(":\t")[1]) for l in tail.splitlines()]
    f = log.read_text().rstrip("\n").split("\t")
    assert sum(hist) == int(f[5]) and len(hist) == 3
    assert 0.005 < float(f[3]) < 0.06          # reference: 200 / 10057 = 0.020
    assert f[15] == "3" and f[16].endswith(run["code"])
