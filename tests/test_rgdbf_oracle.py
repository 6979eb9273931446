"""The numpy restatement of the re-decoding NGDBF decoder (tests/rgdbf_oracle.py) against the
reference's recorded runs and against the pinned GDBF oracle. CPU only."""
import re

import numpy as np
import pytest

import rgdbf_oracle as RO
from conftest import code_path
from ldpcsimulation_amd import native

RUNS, POOLED = RO.golden_runs()


def _final(run):
    m = re.match(r"Final result: (\d+) bit errs in (\d+) words.*Average iterations = ([0-9.e+-]+)\. "
                 r"Uncoded errors = (\d+)", run["final"])
    return int(m.group(1)), int(m.group(2)), float(m.group(3)), int(m.group(4))


@pytest.mark.parametrize("run", RUNS, ids=[r["name"] for r in RUNS])
def test_restatement_replays_the_golden_run(run):
    """Totals, the sequence of frame error weights, average iterations, the phase histogram
    and the log line's smoothingUsed of the unmodified reference, exactly."""
    out = RO.replay(run)
    errors, words, avg_it, uncoded = _final(run)
    assert (out["errors"], out["words"], out["uncoded"]) == (errors, words, uncoded)
    assert out["ferr_weights"] == run["ferr_weights"]
    assert float("%g" % (out["iters"] / out["words"])) == avg_it
    assert out["phase_hist"] == run["phase_hist"]
    # log line: SNR BER avgIt FER bits words T theta noiseScale lambda alpha smoothingUsed ratio window Ymax maxphase alist
    log = run["log_line"].rstrip("\n").split("\t")
    assert int(log[11]) == out["smoothing_used"]
    assert int(log[15]) == int(run["args"][10])
    # "All checks satisfied." marks the frame errors whose last phase was satisfied
    marks = [l.endswith("All checks satisfied.") for l in run["stdout"].splitlines() if l.startswith("Ferr with ")]
    assert marks == out["satisfied"]


def test_golden_runs_fill_every_phase_bin():
    for run in RUNS[:2] + RUNS[3:5]:
        assert all(n > 0 for n in run["phase_hist"]), run["name"]
    assert POOLED["frames"] > 8000 and POOLED["frame_errors"] >= 200


def test_phase_formulas_match_the_restatement():
    """native.rgdbf_phases / rgdbf_smoothing_used (from the total iterations alone) against the
    per-phase counts of the restatement, on a run that fills every bin."""
    run = RUNS[0]
    R, snr, kw, ns = RO.run_config(run)
    code = RO.Rgdbf(code_path(run["code"]))
    y, pert = RO.glibc_frames(code, R, snr, ns, kw["maxphase"] * kw["T"], 77, 12)
    _, fr = code.decode(y, pert, **kw)
    assert len(set(fr["phases"])) > 1
    assert np.array_equal(native.rgdbf_phases(fr["iters"], kw["T"], kw["maxphase"]), fr["phases"])
    assert np.array_equal(native.rgdbf_smoothing_used(fr["iters"], kw["T"], kw["maxphase"], kw["windowsize"]),
                          fr["smoothing_used"])
    assert np.array_equal(native.rgdbf_smoothing_used(fr["iters"], kw["T"], kw["maxphase"], 0), 0 * fr["iters"])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_regular_code_single_phase_equals_the_gdbf_oracle(dtype):
    """On PEG (dv = 3 for every bit) with maxphase 1 the per-bit weight is the scalar
    alpha*Ymax/3: the restatement must equal the pinned oracle's SMNGDBF with that alpha."""
    from oracle import oracle as O
    path = code_path("PEGReg504x1008.alist")
    code, al = RO.Rgdbf(path), O.Alist(path)
    assert set(code.deg) == {3}
    T, alpha, ymax = 40, 0.96, 2.5
    y, pert = RO.glibc_frames(code, 0.5, 3.5, 0.75, T, 11, 8)
    a3 = float(dtype(np.float64(alpha) * np.float64(ymax) / 3.0))   # the weight the restatement rounds to dtype
    cfg = O.GdbfCfg(flags=RO.ALL, T=T, theta=-0.6, lambda_=0.99, alpha=a3, noise_scale=0.75, ymax=ymax,
                    windowsize=16)
    its = []
    for f in range(y.shape[0]):
        d, it, sat = al.gdbf_decode(y[f].astype(dtype), pert[f].astype(dtype), cfg)
        fr = code.decode_frame(y[f], pert[f], T=T, maxphase=1, alpha=alpha, ymax=ymax, dtype=dtype)
        assert np.array_equal(d, fr["d"]) and it == fr["iters"] and sat == fr["satisfied"]
        its.append(it)
    assert min(its) < T <= max(its)   # both a satisfied and a failed frame
