"""The sweep driver's --hwgdbf switch: its argument rules and checkpoint settings (CPU), and
on the GPU its counts against direct ldpc_hwgdbf_sim_batch calls and an exact checkpoint resume."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, code_path
from ldpcsimulation_amd import native, sim, sweep

PEG = "PEGReg504x1008.alist"
BASE = [code_path(PEG), "--rate", "0.8413", "--snr", "5.5", "-T", "100"]


def test_hwgdbf_arguments():
    a = sweep.parse(BASE + ["--hwgdbf"])
    assert a.hwgdbf and sweep._hwgdbf_settings(a) == {"w": 0.185, "ymax": 1.625, "noise_scale": 0.95, "theta0": -0.525,
                                                      "nq": 5, "maxphase": 1, "qlen": 2648}
    a = sweep.parse(BASE + ["--hwgdbf", "--w", "0.2", "--ymax", "1.5", "--noise-scale", "0.9", "--theta0", "-0.5",
                            "--nq", "6", "--maxphase", "2", "--qlen", "3000"])
    assert sweep._hwgdbf_settings(a) == {"w": 0.2, "ymax": 1.5, "noise_scale": 0.9, "theta0": -0.5, "nq": 6,
                                         "maxphase": 2, "qlen": 3000}
    for bad in (["--hwgdbf", "--gdbf", "SMNGDBF"], ["--hwgdbf", "--ems"], ["--hwgdbf", "--variant", "nms"],
                ["--hwgdbf", "--schedule", "layered"], ["--hwgdbf", "--theta", "-0.6"], ["--hwgdbf", "--lam", "0.9"],
                ["--hwgdbf", "--window", "8"], ["--hwgdbf", "--saturate", "2.0"], ["--hwgdbf", "--qbits", "3"],
                ["--w", "0.2"], ["--theta0", "-0.5"], ["--qlen", "3000"]):
        p = subprocess.run([sys.executable, "-m", "ldpcsimulation_amd.sweep"] + BASE + bad, cwd=ROOT,
                           capture_output=True, text=True, timeout=120)
        assert p.returncode == 2 and "hwgdbf" in p.stderr, (bad, p.stderr[-300:])


def test_gdbf_rules_and_checkpoints_unchanged():
    """--gdbf keeps its rules and messages, and a sweep without --hwgdbf keeps the checkpoint
    settings it had before the switch existed."""
    base = [code_path(PEG), "--rate", "0.5", "--snr", "3.5", "-T", "100"]
    a = sweep.parse(base + ["--gdbf", "RSMNGDBF", "--maxphase", "4", "--nq", "8"])
    assert not a.hwgdbf and sweep._gdbf_settings(a)["maxphase"] == 4
    for bad in (["--theta", "-0.6"], ["--maxphase", "3"], ["--nq", "5"], ["--noise-scale", "0.9"]):
        p = subprocess.run([sys.executable, "-m", "ldpcsimulation_amd.sweep"] + base + bad, cwd=ROOT,
                           capture_output=True, text=True, timeout=120)
        assert p.returncode == 2 and "belongs to --gdbf" in p.stderr, (bad, p.stderr[-300:])
    keys = {"alist", "alist_md5", "rate", "snr", "T", "variant", "alpha", "delta", "quantize", "saturate",
            "precision", "schedule", "min_bit_errors", "min_frame_errors", "max_frames", "codewords_md5", "ems",
            "nm", "offset", "early_stop"}
    assert set(sweep._checkpoint_config(sweep.parse(base + ["--variant", "nms", "--alpha", "1.25"]))) == keys
    g = sweep._checkpoint_config(sweep.parse(base + ["--gdbf", "RSMNGDBF", "--maxphase", "2"]))
    assert set(g) == keys | {"gdbf", "theta", "lam", "noise_scale", "window", "nq", "maxphase", "ymax"}
    h = sweep._checkpoint_config(sweep.parse(BASE + ["--hwgdbf"]))
    assert set(h) == keys | {"hwgdbf", "w", "ymax", "noise_scale", "theta0", "nq", "maxphase", "qlen"}
    assert h != sweep._checkpoint_config(sweep.parse(BASE + ["--hwgdbf", "--qlen", "3000"]))


def _run(tmp_path, *extra):
    cmd = [sys.executable, "-m", "ldpcsimulation_amd.sweep", code_path(PEG), "--rate", "0.8413", "--snr", "5.5", "6.5",
           "-T", "100", "--hwgdbf", "--batch", "256", "--first-round", "64", "--max-frames", "700", "--seed", "3",
           "--json"] + list(extra)
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]


@pytest.mark.gpu
def test_sweep_driver_hwgdbf(tmp_path):
    """sweep --hwgdbf over two points at one rank: the totals are those of direct
    hwgdbf_sim_batch calls (point k on stream k) under the family's stop rule, the log line
    has the documented fields, and a checkpoint cut back to mid-point resumes exactly."""
    log = tmp_path / "hw.txt"
    js = _run(tmp_path, "--log", str(log))
    lines = log.read_text().splitlines()
    assert len(js) == len(lines) == 2
    ctx = native.Context(native.Graph.from_alist(code_path(PEG)), 0, 1024)
    cfg = native.HwGdbfConfig(T=100)
    for k, snr in enumerate((5.5, 6.5)):
        fr, _ = ctx.hwgdbf_sim_batch(snr, 0.8413, cfg, seed=3, stream_id=k, first_cw=0, batch=700)
        raw = np.ascontiguousarray(fr).view(np.int32).reshape(-1, 4)
        acc, used = sim.exact_cut(np.zeros(6, dtype=np.int64), raw, 100, 200, 20, True)
        assert 0 < used <= 700
        assert [js[k][key] for key in sim.COUNT_KEYS] == [int(x) for x in acc], (k, js[k])
        assert js[k]["kernel"] == "hwgdbf_wg" and js[k]["gdbf"] == "NGDBFhw"
        f = lines[k].split("\t")
        assert len(f) == 13 and f[0] == "%g" % snr
        assert f[4:12] == ["100", "-0.525", "0.95", "0.185", "1.625", "5", "1", "2648"] and f[12].endswith(PEG)
        assert f[1] == "%g" % (acc[0] / (acc[3] * 1008)) and f[2] == "%g" % (acc[4] / acc[3])
    ck = tmp_path / "ck.partial"
    _run(tmp_path, "--log", str(tmp_path / "a.txt"), "--checkpoint", str(ck), "--checkpoint-interval", "0")
    assert (tmp_path / "a.txt").read_text().splitlines() == lines
    recs = [json.loads(l) for l in ck.read_text().splitlines()]
    r1 = [r for r in recs if r["kind"] == "round" and r["k"] == 1]
    assert len(r1) >= 2, len(r1)
    kept = [r for r in recs if r["kind"] == "header" or (r["kind"] == "round" and r["k"] == 0)] + r1[:1]
    ck.write_text("".join(json.dumps(r) + "\n" for r in kept))
    js2 = _run(tmp_path, "--log", str(tmp_path / "b.txt"), "--checkpoint", str(ck))
    assert (tmp_path / "b.txt").read_text().splitlines() == lines
    assert js2[1]["resumed_from_frame"] == r1[0]["next_frame"] > 0
