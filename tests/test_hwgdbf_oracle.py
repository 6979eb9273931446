"""The numpy restatement of the fixed-point NGDBF hardware model (tests/hwgdbf_oracle.py)
against the reference's recorded runs (tests/golden/reference_runs_ngdbfhw.json), fed glibc
random() / rann() in the reference's order. CPU only."""
import re

import numpy as np
import pytest

import hwgdbf_oracle as HO
from conftest import code_path

RUNS, POOLED = HO.golden_runs()
BY_NAME = {r["name"]: r for r in RUNS}
# three of the five recorded runs: the 802.3 code at 4.0 dB, the run whose failed phases advance
# the pointer by exactly qlen - N = 600, and the column-degree-11 code
REPLAYED = ["ngdbfhw_802_3_4.0_200_s1234", "ngdbfhw_802_3_3.5_30_s11", "ngdbfhw_1944_8.0_60_s3"]


def _final(run):
    m = re.match(r"Final result: (\d+) bit errs in (\d+) words, BER=([0-9.e+-]+)\. Average iterations = ([0-9.e+-]+)\. "
                 r"Uncoded errors = (\d+), uncBER=([0-9.e+-]+)$", run["final"])
    return int(m.group(1)), int(m.group(2)), m.group(3), m.group(4), int(m.group(5))


@pytest.mark.parametrize("name", REPLAYED)
def test_restatement_replays_the_golden_run(name):
    """Per-frame error weights, the satisfied marks, the final line's numbers, the log line's
    fields and the completion-time distribution of the unmodified reference, exactly."""
    run = BY_NAME[name]
    out = HO.replay(run)
    errors, words, ber, avg_it, uncoded = _final(run)
    assert (out["errors"], out["words"]) == (errors, words) and uncoded == 0
    assert out["ferr_weights"] == run["ferr_weights"]
    N = HO.HwGdbf(code_path(run["code"])).N
    assert "%g" % (out["errors"] / (words * N)) == ber and "%g" % (out["iters"] / words) == avg_it
    marks = [l.endswith("All checks satisfied.") for l in run["stdout"].splitlines() if l.startswith("Ferr with ")]
    assert marks == out["satisfied"]
    # SNR errors wordErrors BER avgIt FER bits words T theta0 noiseScale w Ymax NQ maxPhases seed (:451-459)
    log = run["log_line"].rstrip("\n").split("\t")
    assert len(log) == 16
    assert log == ["%g" % float(run["snr"]), str(errors), str(out["word_errors"]), ber, avg_it,
                   "%g" % (out["word_errors"] / words), str(words * N), str(words), "600", "-0.525", "0.95", "0.185",
                   "1.625", "5", "1", str(run["seed"])]
    want = "".join("%d\t%g\n" % (i, v) for i, v in enumerate(out["itdist"]))
    assert want == run["itdist"]


def test_failed_phases_advance_the_pointer_by_a_full_turn():
    """Run 2: a failed phase runs T = 600 = qlen - N iterations on the 802.3 code, so the
    pointer comes back to where it started."""
    run = BY_NAME["ngdbfhw_802_3_3.5_30_s11"]
    code = HO.HwGdbf(code_path(run["code"]))
    y, q = HO.glibc_frames(code, run["snr"], run["seed"], 2)
    fr = code.decode_frame(y[0], q[0], 123)
    assert fr["iters_run"] == 600 and fr["qptr"] == 123 and not fr["satisfied"]


def test_golden_runs_recorded_counts():
    got = {r["name"]: _final(r)[:2] + (len(r["ferr_weights"]),) for r in RUNS}
    assert got == {"ngdbfhw_802_3_4.0_200_s1234": (909, 200, 9), "ngdbfhw_802_3_3.5_30_s11": (3645, 30, 28),
                   "ngdbfhw_802_3_4.5_400_s5": (0, 400, 0), "ngdbfhw_peg_6.0_200_s7": (296, 200, 45),
                   "ngdbfhw_1944_8.0_60_s3": (35, 60, 5)}
    assert BY_NAME["ngdbfhw_802_3_4.5_400_s5"]["stdout"].count("Incremental result:") == 4
    assert (POOLED["frames"], POOLED["frame_errors"]) == (10000, 459)


def test_known_answers_of_the_defaults():
    lmax, NL, smult, theta = HO.constants()
    assert (NL, smult, theta) == (31.0, 7, 15) and abs(lmax - 4.391891891891892) < 1e-15
    code = HO.HwGdbf(code_path("802_3_H.alist"))
    assert (code.N, code.M, code.maxdv) == (2048, 384, 6) and set(np.diff(code.row_ptr)) == {32}
    y, q = HO.glibc_frames(code, 4.0, 1, 3)
    for dtype in (np.float64, np.float32):
        Y, r = code.front(y, dtype=dtype)
        Q = code.noise(q, dtype=dtype)
        for v in (Y, Q):
            assert (v % 2 != 0).all() and np.abs(v).max() == 31 and np.abs(v).min() >= 1
        assert np.array_equal(Y < 0, r.reshape(Y.shape) == 1)   # w > 0: the sign is the decision
    # samples beyond Ymax saturate to the top level, a zero is negative (sgn is > 0 ? 1 : -1)
    Y, r = code.front(np.array([5.0, -5.0, 0.0, 1e-9] + [1.0] * (code.N - 4)))
    assert list(Y[:4]) == [31, -31, -1, 1] and list(r[:4]) == [0, 1, 1, 0]


@pytest.mark.parametrize("nq", [2, 5, 7])
def test_pack_unpack_round_trip(nq):
    top = (1 << (nq - 1)) - 1
    for m in range(top + 1):
        for neg in (False, True):
            code = HO.pack(m, neg, nq)
            assert 0 <= code < (1 << nq)
            assert HO.unpack(code, nq) == (-(2 * m + 1) if neg else 2 * m + 1)
    assert HO.unpack(HO.pack(top + 1, False, nq), nq) == -1   # bit NQ - 1 of the magnitude is the sign bit
    vals = HO.quant(np.linspace(-5, 5, 1001), 4.0, nq, np.float64)
    assert (vals % 2 != 0).all() and np.abs(vals).max() <= (1 << nq) - 1
