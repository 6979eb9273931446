"""The numpy restatement of layered fixed-point min-sum (tests/fxlms_oracle.py) against the C
oracle's fp64 layered decoder. With Ymax = 31/16 and Q = 5 every quantised sample sits on the
grid u = 1/16, where fp64 layered MS and OMS are exact integer arithmetic in disguise: a
fixed-point decoder whose clamps never act must give the oracle's decisions bit for bit, in the
same row order. Each case asserts that premise (no clamped value) before the claim. CPU only:
the library gives its layer order (Graph.layers(), host code), no device is touched."""
import numpy as np
import pytest

import fxlms_oracle as FL
from conftest import code_path
from ldpcsimulation_amd import native
from oracle import oracle as O

G = FL.GRID
PEG, W1944 = "PEGReg504x1008.alist", "80211n_1944_r12.alist"


def library_layers(code):
    """(row_order, layer_ptr) of the library's Graph.layers()."""
    return native.Graph.from_alist(code_path(code)).layers()


@pytest.fixture(scope="module", params=list(FL.GRID_CASES))
def case(request):
    code, snr, T = FL.GRID_CASES[request.param]
    path = code_path(code)
    fx = FL.Fxlms(path)
    return request.param, code, fx, O.Alist(path), FL.front(FL.grid_samples(fx.N, snr), G["ymax"], G["qbits"]), T


# peak_x, peak_app, failing frames in natural row order
NATURAL = {("w1944", FL.MS): (1168, 1317, 12), ("w1944", FL.OMS): (1090, 1219, 3),
           ("peg", FL.MS): (1277, 1913, 8), ("peg", FL.OMS): (814, 1231, 5)}


@pytest.mark.parametrize("which", ["natural", "library"])
@pytest.mark.parametrize("variant", [FL.MS, FL.OMS])
def test_unclamped_decisions_equal_fp64_layered_min_sum(case, variant, which):
    name, code, fx, A, Y, T = case
    order = None
    if which == "library":
        order = library_layers(code)[0]
    out = fx.decode(Y, variant, T, G["msg_bits"], 16, beta=G["beta"], order=order)
    failing = int((out["frames"]["bit_err"] > 0).sum())
    print(name, variant, which, "T", T, "peak_x", out["peak_x"], "peak_app", out["peak_app"], "clamped", out["clamped"],
          "failing", failing)
    assert out["clamped"] == 0 and max(out["peak_x"], out["peak_app"]) <= 32767   # the premise: no clamp acts
    want = A.decode_layered(Y * G["u"], T, O.Cfg(variant=variant, delta=G["delta"]), order)
    assert np.array_equal(out["d"], want)
    assert 0 < failing < G["frames"]   # frames that decode and frames that do not
    if which == "natural":
        assert (out["peak_x"], out["peak_app"], failing) == NATURAL[name, variant]


def test_rows_of_a_layer_commute(case):
    """Shuffling the rows inside each layer of Graph.layers() changes nothing, at 6-bit messages
    and 7-bit APPs, where the message clamp is frequent."""
    name, code, fx, _, Y, T = case
    order, ptr = library_layers(code)
    rng = np.random.default_rng(5)
    shuffled = np.concatenate([rng.permutation(order[ptr[l]:ptr[l + 1]]) for l in range(len(ptr) - 1)])
    assert not np.array_equal(shuffled, order) and sorted(shuffled.tolist()) == list(range(fx.M))
    for variant, kw in ((FL.NMS, dict(num=3, shift=2)), (FL.MS, {})):
        a = fx.trajectory(Y, variant, T, 6, 7, order=order, **kw)
        b = fx.trajectory(Y, variant, T, 6, 7, order=shuffled, **kw)
        assert a["clamped"].sum() > 0
        assert all(np.array_equal(a[k], b[k]) for k in a)


def test_rows_of_a_layer_commute_at_row_degree_32():
    """The same on 802.3an, whose rows of degree 32 the library's layer order has to cover (six
    layers of 64 rows), at 6/7 and at 12/13 bits."""
    code = "802_3_H.alist"
    fx = FL.Fxlms(code_path(code))
    order, ptr = library_layers(code)
    assert fx.maxdc == 32 and np.diff(ptr).tolist() == [64] * 6 and sorted(order.tolist()) == list(range(fx.M))
    y = 1.0 + np.linspace(0.38, 0.60, 8)[:, None] * np.random.default_rng(7).standard_normal((8, fx.N))
    Y = FL.front(y, G["ymax"], G["qbits"])
    rng = np.random.default_rng(6)
    shuffled = np.concatenate([rng.permutation(order[ptr[l]:ptr[l + 1]]) for l in range(len(ptr) - 1)])
    assert not np.array_equal(shuffled, order)
    for mb, ab in ((6, 7), (12, 13)):
        a = fx.trajectory(Y, FL.NMS, 4, mb, ab, num=3, shift=2, order=order)
        b = fx.trajectory(Y, FL.NMS, 4, mb, ab, num=3, shift=2, order=shuffled)
        assert all(np.array_equal(a[k], b[k]) for k in a)
    es = fx.result(a, 4, early_stop=True)
    assert (es["s"] < 4).any() and (es["s"] == 4).any()   # frames that decode and frames that do not


def test_identities_and_clamping(case):
    name, _, fx, _, Y, T = case
    for bits, abits in ((16, 16), (6, 7)):
        ms = fx.decode(Y, FL.MS, T, bits, abits)
        for other in (fx.decode(Y, FL.NMS, T, bits, abits, num=8, shift=3), fx.decode(Y, FL.OMS, T, bits, abits, beta=0)):
            assert np.array_equal(other["d"], ms["d"])
            assert all(other[k] == ms[k] for k in ("peak_x", "peak_app", "clamped"))
    # app_bits = msg_bits + 1 is app_bits = 16 when |Y| <= 2 V + 1 (msg_bits >= qbits): A = 2 V + 1, and
    # |x + c| <= 2 V never reaches it
    for bits in (5, 6, 8):
        assert bits >= G["qbits"]
        a = fx.trajectory(Y, FL.NMS, T, bits, bits + 1, num=3, shift=2)
        b = fx.trajectory(Y, FL.NMS, T, bits, 16, num=3, shift=2)
        assert all(np.array_equal(a[k], b[k]) for k in a)
        assert a["peak_app"].max() <= 2 * ((1 << (bits - 1)) - 1) + 1
    # app_bits = msg_bits does clamp
    wide, tight = fx.decode(Y, FL.MS, T, 6, 7), fx.decode(Y, FL.MS, T, 6, 6)
    assert tight["clamped"] > wide["clamped"]
    if name == "w1944":
        assert (tight["d"] != wide["d"]).any(axis=1).sum() >= 1


def test_early_stop_is_the_fixed_t_result(case):
    """D(s) is what T = s returns, frame by frame. At 8-bit messages: with 6 bits against 5-bit
    samples no frame of the 1944-bit code decodes, so nothing would stop early."""
    _, _, fx, _, Y, T = case
    kw = dict(num=3, shift=2)
    es = fx.decode(Y, FL.NMS, T, 8, 9, early_stop=True, **kw)
    assert np.array_equal(es["frames"]["iters"], es["s"]) and es["s"].min() < T
    assert es["frames"]["syndrome_fail"].any() and (es["s"][es["frames"]["syndrome_fail"] == 1] == T).all()
    for t in range(T + 1):
        fixed = fx.decode(Y, FL.NMS, t, 8, 9, **kw)   # a pass of its own, not a cut of the longer one
        at = es["s"] == t
        assert np.array_equal(fixed["d"][at], es["d"][at])
        assert np.array_equal(fixed["frames"]["syndrome_fail"][at], es["frames"]["syndrome_fail"][at])
        assert fixed["frames"]["syndrome_fail"][es["s"] > t].all() and not fixed["frames"]["iters"].any()
