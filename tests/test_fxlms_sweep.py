"""The sweep driver's --fxlms switch on the GPU: its totals against direct ldpc_fxlms_sim_batch
calls and its log line (tests/test_fxlms_host.py has the argument rules and the checkpoint key)."""
import json
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, code_path
from ldpcsimulation_amd import native, sim

PEG = "PEGReg504x1008.alist"
T = 12


def _run(*extra):
    cmd = [sys.executable, "-m", "ldpcsimulation_amd.sweep", code_path(PEG), "--rate", "0.5", "--snr", "1.5", "2.5",
           "-T", str(T), "--fxlms", "--batch", "256", "--first-round", "64", "--max-frames", "600", "--seed", "3",
           "--json"] + list(extra)
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]


@pytest.mark.gpu
@pytest.mark.parametrize("early_stop", [True, False])
def test_sweep_driver_fxlms(tmp_path, early_stop):
    """sweep --fxlms over two points at one rank: the totals are those of direct fxlms_sim_batch
    calls (point k on stream k) under the min-sum stop rule, avgIt is the true mean with
    --early-stop and T without, and the log line has the documented fields."""
    log = tmp_path / "fx.txt"
    settings = ["--variant", "nms", "--scale", "13", "4", "--msg-bits", "8", "--app-bits", "10", "--quantize", "1.9375", "5",
                "--precision", "f32"]
    js = _run("--log", str(log), *settings, *(["--early-stop"] if early_stop else []))
    lines = log.read_text().splitlines()
    assert len(js) == len(lines) == 2
    ctx = native.Context(native.Graph.from_alist(code_path(PEG)), 0, 1024)
    cfg = native.FxlmsConfig(variant=native.NMS, T=T, qbits=5, msg_bits=8, app_bits=10, nms_num=13, nms_shift=4, ymax=1.9375,
                             early_stop=early_stop, precision=native.F32)
    for k, snr in enumerate((1.5, 2.5)):
        fr, _ = ctx.fxlms_sim_batch(snr, 0.5, cfg, seed=3, stream_id=k, first_cw=0, batch=600)
        raw = np.ascontiguousarray(fr).view(np.int32).reshape(-1, 4)
        acc, used = sim.exact_cut(np.zeros(6, dtype=np.int64), raw, T, 200, 40, early_stop)
        assert 0 < used <= 600
        assert [js[k][key] for key in sim.COUNT_KEYS] == [int(x) for x in acc], (k, js[k])
        assert js[k]["kernel"] == "fxlms_i16" and js[k]["decoder"] == "fxlms" and ("avg_iters" in js[k]) == early_stop
        assert (js[k]["variant"], js[k]["schedule"], js[k]["precision"]) == ("nms", "layered", "f32")
        f = lines[k].split("\t")
        # SNR BER avgIt FER T Ymax Q msgBits appBits num shift alist
        assert len(f) == 12 and f[0] == "%g" % snr
        assert f[4:11] == [str(T), "1.9375", "5", "8", "10", "13", "4"] and f[11].endswith(PEG)
        assert f[1] == "%g" % (acc[0] / (acc[3] * 1008)) and f[3] == "%g" % (acc[1] / acc[3])
        assert f[2] == ("%g" % (acc[4] / acc[3]) if early_stop else str(T))
        if early_stop:   # avgIt is the true mean of the iterations the frames ran
            assert acc[4] == int(raw[:used, 3].sum()) and 0 < acc[4] < T * used
