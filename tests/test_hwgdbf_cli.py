"""bin/NGDBFhw (cli_hwgdbf.cpp) against the reference's own output.

With LDPC_RNG=glibc (default) the GPU front-end must print exactly what the reference's
NGDBFhw printed (golden stdout of tests/golden/reference_runs_ngdbfhw.json), append the same
log line and write the same <log>_<SNR>_itdist.dat, for all five recorded runs."""
import os
import subprocess

import pytest

import hwgdbf_oracle as HO
from conftest import ROOT, code_path

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "bin", "NGDBFhw")
RUNS, _ = HO.golden_runs()


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if not k.startswith("LDPC_")}
    env.update(kw)
    return env


@pytest.mark.parametrize("run", RUNS, ids=[r["name"] for r in RUNS])
def test_cli_output_identical_to_reference(tmp_path, run):
    alist = code_path(run["code"])
    log = tmp_path / "log.txt"
    p = subprocess.run([EXE, alist, run["snr"], str(run["frames"]), str(run["seed"]), str(log)], env=_env(),
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    assert p.stdout.replace(alist, "@ALIST@").replace(str(log), "@LOGFILE@") == run["stdout"]
    assert log.read_text() == run["log_line"]
    assert (tmp_path / ("log.txt" + run["itdist_suffix"])).read_text() == run["itdist"]


def test_cli_philox_batches(tmp_path):
    """LDPC_RNG=philox: frames generated on the GPU in batches (the last one partial); the
    log line's counts are consistent and the frame error rate is the operating point's."""
    log = tmp_path / "log.txt"
    p = subprocess.run([EXE, code_path("802_3_H.alist"), "4.0", "5000", "7", str(log)],
                       env=_env(LDPC_RNG="philox", LDPC_BATCH="2048"), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    f = log.read_text().rstrip("\n").split("\t")
    assert len(f) == 16 and f[7] == "5000" and f[6] == str(5000 * 2048) and f[15] == "7"
    assert int(f[2]) == p.stdout.count("Ferr with ") and p.stdout.count("Incremental result:") == 50
    assert 0.02 < float(f[5]) < 0.08          # reference: 459 / 10000
