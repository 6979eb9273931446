"""The numpy restatement of DD-BMP (tests/ddbmp_oracle.py) against the reference itself:
it replays every golden run of tests/golden/reference_runs_ddbmp.json (recorded from the
unmodified decodeDDBMP.cpp by tests/golden/make_golden_ddbmp.py) frame by frame -- glibc
noise, the quantiser, the stop rule -- and must give the same totals, the same sequence of
frame error weights and the same average iterations. No GPU."""
import re

import numpy as np
import pytest

import ddbmp_oracle as D
from conftest import code_path
from oracle import oracle as O

RUNS, POOLED = D.golden_runs()


def final_numbers(line):
    m = re.match(r"Final result: (\d+) bit errs in (\d+) words.*Average iterations = ([0-9.e+-]+)\. "
                 r"Uncoded errors = (\d+)", line)
    return int(m.group(1)), int(m.group(2)), m.group(3), int(m.group(4))


def test_golden_file_holds_the_runs_the_decoder_is_pinned_by():
    assert [r["binary"] for r in RUNS] == ["decodeDDBMP"] * 6
    assert {r["code"] for r in RUNS} == {"PEGReg504x1008.alist", "80211n_1944_r12.alist", "4000.2000.4.244.alist"}
    assert final_numbers(RUNS[0]["final"]) == (2270, 71, "75.3662", 5719)
    assert final_numbers(RUNS[2]["final"])[2] == "0.97561"   # a frame that stops in iteration `it` counts `it`
    assert POOLED["frames"] > 10000 and POOLED["frame_errors"] >= 400


def test_quantize_equals_the_oracle_quantiser():
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.normal(1.0, 0.7, 4000), [0.0, -0.0, 1.0, -1.0, 1.2, -1.2, 0.1, -0.1, 1e-9, 5.0]])
    for ymax, q in ((1.0, 3), (1.0, 4), (1.2, 2), (1.4, 3)):
        got = D.quantize(x, ymax, q)
        assert got.tolist() == [O.quantize(float(v), ymax, q) for v in x]
        got32 = D.quantize(x.astype(np.float32), ymax, q)
        assert got32.dtype == np.float32
        assert got32.tolist() == [O.quantize_f32(float(v), ymax, q) for v in x.astype(np.float32)]


@pytest.mark.parametrize("run", RUNS, ids=[r["name"] for r in RUNS])
def test_restatement_replays_the_reference(run):
    R, snr, T, front = D.run_config(run)
    dec = D.Ddbmp(code_path(run["code"]))
    got = D.replay(run, lambda y, c: dec.decode(y, T, c=c, **front)[1])
    errors, words, avg_it, uncoded = final_numbers(run["final"])
    assert (got["errors"], got["words"], got["uncoded"]) == (errors, words, uncoded)
    assert got["ferr_weights"] == run["ferr_weights"]
    assert "%g" % (got["iters"] / got["words"]) == avg_it


def test_float32_is_an_arithmetic_of_its_own():
    """The same replay in float32 decodes differently (2293 bit errors in 70 words against the
    reference's 2270 in 71): fp32 is pinned by this restatement, not by the reference."""
    run = RUNS[0]
    R, snr, T, front = D.run_config(run)
    dec = D.Ddbmp(code_path(run["code"]))
    got = D.replay(run, lambda y, c: dec.decode(y.astype(np.float32), T, c=c, dtype=np.float32, **front)[1])
    assert (got["errors"], got["words"]) == (2293, 70)


def test_iteration_accounting_and_T0():
    dec = D.Ddbmp(code_path("PEGReg504x1008.alist"))
    y = np.ones((2, dec.N))
    y[1, :40] = -0.3
    d, fr = dec.decode(y, 0)
    assert fr["iters"].tolist() == [0, 0] and fr["bit_err"].tolist() == [0, 40] and fr["syndrome_fail"].tolist() == [0, 1]
    assert (d[1, :40] == -1).all()
    d, fr = dec.decode(y, 5)
    assert fr["iters"][0] == 0          # a codeword stops inside iteration index 0
    assert fr["uncoded_bit_err"].tolist() == [0, 40]
