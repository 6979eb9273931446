"""The sweep driver's --fx-kernel wg on the GPU (tests/test_fxlms_wg_host.py has the argument rules
and the checkpoint settings): the totals of a sweep do not depend on the kernel, the JSON line
names it, and DVB-S2 N=64800 sweeps with it and is refused without it."""
import json
import subprocess
import sys

import pytest

from conftest import ROOT, code_path
from ldpcsimulation_amd import sim

PEG, DVBS2 = "PEGReg504x1008.alist", "dvbs2_1_2.alist"
SETTINGS = ["--variant", "nms", "--scale", "3", "2", "--quantize", "1.9375", "5", "--precision", "f32", "--early-stop", "--seed", "3",
            "--json", "--fxlms"]


def _sweep(code, *extra):
    cmd = [sys.executable, "-m", "ldpcsimulation_amd.sweep", code_path(code), "--rate", "0.5"] + SETTINGS + list(extra)
    return subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)


def _lines(p):
    assert p.returncode == 0, p.stderr[-3000:]
    return [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]


@pytest.mark.gpu
def test_sweep_totals_do_not_depend_on_the_kernel():
    point = ["--snr", "2.0", "-T", "12", "--msg-bits", "8", "--app-bits", "9", "--batch", "256", "--first-round", "64",
             "--max-frames", "600"]
    a, b = _lines(_sweep(PEG, *point)), _lines(_sweep(PEG, *point, "--fx-kernel", "wg"))
    assert len(a) == len(b) == 1 and (a[0]["kernel"], b[0]["kernel"]) == ("fxlms_i16", "fxlms_wg_i16")
    for key in sim.COUNT_KEYS + ("ber", "fer", "avg_iters"):
        assert a[0][key] == b[0][key], key
    assert 0 < b[0]["frame_err"] < b[0]["frames"] and b[0]["decoder"] == "fxlms" and b[0]["schedule"] == "layered"


@pytest.mark.gpu
def test_sweep_dvbs2_needs_the_workgroup_kernel():
    point = ["--snr", "3.0", "-T", "6", "--msg-bits", "8", "--app-bits", "8", "--batch", "16", "--max-frames", "16"]
    p = _sweep(DVBS2, *point)
    assert p.returncode != 0 and "65536" in p.stderr and "LDPC_OPT_KERNEL = 3" in p.stderr
    js = _lines(_sweep(DVBS2, *point, "--fx-kernel", "wg"))
    assert len(js) == 1 and js[0]["kernel"] == "fxlms_wg_i8" and js[0]["frames"] == 16
    assert 0 < js[0]["bit_err"] < js[0]["uncoded_bit_err"] and 0 < js[0]["avg_iters"] <= 6
