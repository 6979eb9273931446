"""The numpy restatement of fixed-point min-sum (tests/fxms_oracle.py) against the C oracle.
With Ymax = 31/16 and Q = 5 the reference's quantiser puts every sample on the grid u = 1/16,
where fp64 MS and OMS are exact integer arithmetic in disguise: a fixed-point decoder whose
messages never saturate must give the oracle's fp64 decisions bit for bit. Each case asserts
that premise (peak <= V, no clamped message) before the claim. CPU only."""
import numpy as np
import pytest

import fxms_oracle as FO
from conftest import code_path
from oracle import oracle as O

G = FO.GRID


@pytest.fixture(scope="module", params=list(FO.GRID_CASES))
def case(request):
    code, snr, T = FO.GRID_CASES[request.param]
    path = code_path(code)
    fx = FO.Fxms(path)
    return request.param, fx, O.Alist(path), FO.grid_samples(fx.N, snr), T


def test_front_end_codes_are_the_reference_quantiser(case):
    _, fx, _, y, _ = case
    for dtype, q in ((np.float64, O.quantize), (np.float32, O.quantize_f32)):
        yt = y.astype(dtype)
        Y = FO.front(yt, G["ymax"], G["qbits"], dtype)
        want = np.array([q(float(v), G["ymax"], G["qbits"]) for v in yt.ravel()], dtype=dtype).reshape(y.shape)
        assert np.array_equal((Y * G["u"]).astype(dtype), want)
        assert np.abs(Y).min() >= 2 and np.abs(Y).max() == 31 and ((Y % 2 == 0) | (np.abs(Y) == 31)).all()


@pytest.mark.parametrize("variant", [FO.MS, FO.OMS])
def test_unsaturated_decisions_equal_fp64_min_sum(case, variant):
    name, fx, A, y, T = case
    Y = FO.front(y, G["ymax"], G["qbits"])
    out = fx.decode(Y, variant, T, G["msg_bits"], beta=G["beta"])
    V = (1 << (G["msg_bits"] - 1)) - 1
    print(name, variant, "peak", out["peak"], "clamped", out["clamped"], "failing", int((out["frames"]["bit_err"] > 0).sum()))
    assert out["peak"] <= V and out["clamped"] == 0   # the premise: no message saturates
    want = A.decode(Y * G["u"], T, O.Cfg(variant=variant, delta=G["delta"]))
    assert np.array_equal(out["d"], want)
    failing = int((out["frames"]["bit_err"] > 0).sum())
    assert 0 < failing < G["frames"]   # frames that decode and frames that do not


def test_identities_and_clamping(case):
    _, fx, _, y, T = case
    Y = FO.front(y, G["ymax"], G["qbits"])
    for bits in (16, 6):
        ms = fx.decode(Y, FO.MS, T, bits)
        for other in (fx.decode(Y, FO.NMS, T, bits, num=8, shift=3), fx.decode(Y, FO.OMS, T, bits, beta=0)):
            assert np.array_equal(other["d"], ms["d"]) and (other["peak"], other["clamped"]) == (ms["peak"], ms["clamped"])
    narrow = fx.decode(Y, FO.MS, T, 4)
    assert narrow["clamped"] > 0 and narrow["peak"] > 7
    # early stop: D(s) is what T = s returns, frame by frame
    es = fx.decode(Y, FO.NMS, T, 6, num=3, shift=2, early_stop=True)
    assert np.array_equal(es["frames"]["iters"], es["s"]) and es["s"].min() < T
    assert es["frames"]["syndrome_fail"].any() and (es["s"][es["frames"]["syndrome_fail"] == 1] == T).all()
    for t in range(T + 1):
        fixed = fx.decode(Y, FO.NMS, t, 6, num=3, shift=2)
        at = es["s"] == t
        assert np.array_equal(fixed["d"][at], es["d"][at])
        assert np.array_equal(fixed["frames"]["syndrome_fail"][at], es["frames"]["syndrome_fail"][at])
        assert fixed["frames"]["syndrome_fail"][es["s"] > t].all() and not fixed["frames"]["iters"].any()
