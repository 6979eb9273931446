"""The numpy restatement of the every-attempt decoders (tests/rstat_oracle.py) against the
reference's recorded redecodeStatistics and replayGDBF runs
(tests/golden/reference_runs_redecode.json, made by tests/golden/make_golden_redecode.py from
the unmodified sources), and against the single-phase decode of tests/rgdbf_oracle.py that an
attempt is. Everything is compared for equality."""
import hashlib

import numpy as np
import pytest

import rstat_oracle as SO

RUNS, REPLAYS = SO.golden()


def test_recorded_runs_show_both_outcomes():
    """Every recorded statistics run has attempts that succeed and attempts that fail."""
    assert len(RUNS) == 4 and len(REPLAYS) == 3
    for run in RUNS:
        t = np.array([[int(x) for x in l.split()[1:]] for l in run["log"].splitlines()])
        assert (t == 0).any() and (t > 0).any(), run["name"]
        assert t.shape[1] <= 7                      # the reference's phase_hist has 7 bins


@pytest.mark.parametrize("run", RUNS, ids=[r["name"] for r in RUNS])
def test_statistics_runs_replay_exactly(run):
    """The log table, the final line, the Ferr weights and the state files' draw counts."""
    out = SO.replay_run(run)
    N = SO.code_of(run["code"]).N
    assert SO.log_text(0, out["attempts_out"][:, :, 0]) == run["log"]
    assert SO.final_line(N, out) == run["final"]
    last = out["frames"]["bit_err"]
    assert [int(x) for x in last[last > 0]] == run["ferr_weights"]
    assert ["%d %d" % (run["seed"], n) for n in out["draws"]] == run["states"]
    sat = [bool(fr[-1]["satisfied"]) for fr in out["att"]]
    want = [l.endswith("All checks satisfied.") for l in run["stdout"].splitlines() if l.startswith("Ferr with ")]
    assert [s for s, w in zip(sat, last) if w > 0] == want


@pytest.mark.parametrize("run", REPLAYS, ids=[r["name"] for r in REPLAYS])
def test_replay_runs_replay_exactly(run):
    """The log line (the statistics run's row of that frame), the trace files' row counts,
    the -1 counts of every row, and the trace text's sha-256."""
    out = SO.replay_run(run)
    of = [r for r in RUNS if r["name"] == run["of"]][0]
    assert SO.log_text(0, out["attempts_out"][:, :, 0]) == run["log_line"]
    # the replay numbers its one frame 0; the outcomes are the statistics run's row of that frame
    assert run["log_line"].rstrip("\n").split("\t", 1)[1] == of["log"].splitlines()[run["frame"]].split("\t", 1)[1]
    for k, tr in enumerate(run["traces"]):
        x = out["att"][0][k]
        assert len(x["rows"]) == tr["rows"] == x["iters"]
        assert [int((d < 0).sum()) for d, _ in x["rows"]] == tr["d_neg"]
        assert [int((s < 0).sum()) for _, s in x["rows"]] == tr["s_neg"]
        assert hashlib.sha256(SO.trace_text(x["rows"]).encode()).hexdigest() == tr["sha256"], k
    done = [l for l in run["stdout"].splitlines() if l.startswith("Completed phase with ")]
    assert done == ["Completed phase with %d errors." % w for w in out["attempts_out"][0, :, 0]]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_an_attempt_is_a_single_phase_decode(dtype):
    """Rstat.attempt equals Rgdbf.decode_frame(maxphase=1) on the first recorded frames, also
    with windowsize > T and with a flag subset."""
    run = RUNS[0]
    R, snr, ns, attempts, frames, kw = SO.run_config(run)
    code = SO.code_of(run["code"])
    out = SO.replay_run(run)
    for extra in ({}, {"windowsize": kw["T"] + 5}, {"flags": SO.ADAPT | SO.NOISE}):
        k2 = dict(kw, **extra)
        for f in range(3):
            for a in range(attempts):
                x = code.attempt(out["y"][f], out["pert"][f, a], dtype=dtype, **k2)
                w = code.decode_frame(out["y"][f], out["pert"][f, a], maxphase=1, dtype=dtype, **k2)
                for key in ("iters", "satisfied", "smoothing_used", "bit_err", "uncoded_bit_err", "syndrome_fail"):
                    assert x[key] == w[key], (extra, f, a, key)
                assert np.array_equal(x["d"], w["d"])
                assert len(x["rows"]) == x["iters"]
