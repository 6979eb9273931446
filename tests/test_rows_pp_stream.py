"""The check waves' instruction stream of the ping-pong kernel (rows_pp.hip: one premise
test per barrier interval, row 1's front issued inside row 0's store chain) leaves every
value as it was: on the 802.11n N=1944 code -- the bundled code with row pairs and both
check-wave shapes (7/7 and 7/8 edges) -- per-frame results, counters and the re-decode list
equal the one-codeword-per-block kernel's (rows64=fast) and the fp64 oracle's on all frames,
for batches of 5 (slot 1 of the last step empty) and 6, T = 0..3, MS, NMS with the one-FMA
division (alpha 1.25) and the IEEE one (alpha 1.3), OMS, given samples and Philox noise, and
the three pp_slots shapes (k_rows_ppi, k_rows_pp on the plain and on the degree-aware slots).
"""
import math

import numpy as np
import pytest

from conftest import code_path
from oracle import oracle as O

CODE = "80211n_1944_r12.alist"
VARIANTS = {
    "ms": dict(variant=0),
    "nms_fma": dict(variant=1, alpha=1.25),
    "nms_ieee": dict(variant=1, alpha=1.3),
    "oms": dict(variant=2, delta=0.15),
}
BATCHES = (5, 6)
TS = (0, 1, 2, 3)
SIM = dict(seed=4711, stream_id=3, first_cw=77)
_REF = {}      # (variant, source, batch, T) -> the rows64=fast run and the oracle's decisions
_ALIST = []


def _alist():
    if not _ALIST:
        _ALIST.append(O.Alist(code_path(CODE)))
    return _ALIST[0]


def _given(batch):
    g = O.GlibcRandom(991 + batch)
    sigma = math.sqrt(10 ** (-1.5 / 10) / 0.5 / 2)
    c = np.ones(1944, dtype=np.int32)
    return np.stack([g.channel(c, sigma) for _ in range(batch)])


def _run(ctx, cfg, source, batch, y=None):
    """(y, decisions, frames, counters, re-decode list) of one launch."""
    if source == "given":
        y = _given(batch) if y is None else y
        d, fr, cnt = ctx.decode(y, cfg)
    else:
        y, d, fr, cnt = ctx.sim_trace(1.5, 0.5, cfg, batch=batch, **SIM)
    return y, d, fr, cnt, ctx.redo_list()


def _reference(ctx, native, vname, source, batch, T):
    key = (vname, source, batch, T)
    if key not in _REF:
        cfg = native.DecoderConfig(T=T, precision=native.F64, **VARIANTS[vname])
        ctx.set_option("rows64", "fast")
        assert ctx.kernel_info(cfg)["kernel"] == "rows_fast"
        run = _run(ctx, cfg, source, batch)
        want = _alist().decode(run[0], T, O.Cfg(**VARIANTS[vname]), workers=8)
        _REF[key] = (run, want)
    return _REF[key]


@pytest.mark.gpu
@pytest.mark.parametrize("slots", ["split", "plain", "split_lds"])
@pytest.mark.parametrize("vname", list(VARIANTS))
def test_pp_stream_equals_rows_fast_and_oracle(gpu_ctx_factory, vname, slots):
    from ldpcsimulation_amd import native
    ctx = gpu_ctx_factory(CODE)
    try:
        for source in ("given", "philox"):
            for batch in BATCHES:
                for T in TS:
                    (y0, d0, f0, c0, r0), want = _reference(ctx, native, vname, source, batch, T)
                    cfg = native.DecoderConfig(T=T, precision=native.F64, **VARIANTS[vname])
                    ctx.set_option("rows64", "pp")
                    ctx.set_option("pp_slots", slots)
                    assert ctx.kernel_info(cfg)["kernel"] == "rows_pp"
                    assert (ctx.pp_inreg_info(cfg)["inreg_bits"] > 0) == (slots == "split")
                    y1, d1, f1, c1, r1 = _run(ctx, cfg, source, batch)
                    at = f"{source} batch={batch} T={T}"
                    assert np.array_equal(y0, y1), at
                    assert np.array_equal(d1, d0) and np.array_equal(f1, f0), at
                    assert c1.as_dict() == c0.as_dict(), at
                    assert np.array_equal(r1, r0), at
                    # and the fp64 oracle (decodeMinSum.cpp:247-263) on every frame
                    assert int((d1 != want).sum()) == 0, at
                    w = (want != 1).sum(axis=1)
                    assert np.array_equal(f1["bit_err"], w), at
                    assert c1.frames == batch and c1.bit_err == int(w.sum()) and c1.iters == T * batch, at
                    assert c1.frame_err == int((w > 0).sum()), at
    finally:
        ctx.reset_options()


BOUND = 2.0 ** 1000   # the fast check nodes' premise: |yq| and every row's normalised second minimum below it


def _premise_model(H, y, T, v):
    """Flooding min-sum of one frame in numpy (decodeMinSum.cpp:410-476; MS, NMS, OMS), returning
    the (iteration, row) pairs whose normalised second minimum M2 is not below 2^1000 -- what the
    rows' premise test (fast64.h: hi32(M2) against kFast64MaxHi) sees. The one-row inputs below
    keep every M2 at least 25 % away from the bound and the growth input passes it in several rows
    and iterations, so the model's rounding (its sums are not in nlist order) does not matter."""
    def norm(m):
        if v.get("variant") == 1:
            return m / v["alpha"]
        if v.get("variant") == 2:
            return max(m - v["delta"], 0.0)
        return m
    c2v = [np.zeros(len(r)) for r in H.rows]
    hits = []
    for it in range(T):
        app = y.astype(np.float64).copy()
        for j, r in enumerate(H.rows):
            np.add.at(app, r, c2v[j])
        new = []
        for j, r in enumerate(H.rows):
            x = app[r] - c2v[j]
            a = np.abs(x)
            o = np.argsort(a, kind="stable")
            m1, m2 = norm(a[o[0]]), norm(a[o[1]])
            if not m2 < BOUND:
                hits.append((it, j))
            sg = np.where(x < 0, -1.0, 1.0)
            out = np.where(a == a[o[0]], m2, m1) * sg * np.prod(sg)
            new.append(out)
        c2v = new
    return hits


def _thread_rows(ctx, cfg, H, t):
    """The check rows of H that thread t of the device's ping-pong schedule holds as its row 0 and
    row 1 (ldpc_ctx_pp_row_slots: slot t and slot threads + t), found by their bit sets."""
    cols, deg = ctx.pp_row_slots(cfg)
    threads = len(deg) // 2
    assert threads == 512
    by_bits = {frozenset(r): j for j, r in enumerate(H.rows)}
    rows = []
    for slot in (t, threads + t):
        assert deg[slot] > 0
        rows.append(by_bits[frozenset(int(c) for c in cols[slot] if c < H.N)])
    return rows


def _one_row_break(H, y, row, other):
    """y with a premise break in `row` alone, at iteration 1, from inputs below 2^1000: the bits of
    `row` that `other` (the thread's second row) does not hold, and every bit of one further row per
    such bit, are set to +0.9 * 2^1000. At iteration 0 those rows have M2 = 0.9 * 2^1000 (/ alpha);
    at iteration 1 each of these bits brings its further row's message along, so all but at most
    one edge of `row` carry about 1.6 * 2^1000 and its M2 passes the bound, while every other row
    still has at most one such edge."""
    y = y.copy()
    big = 0.9 * BOUND
    mine = [b for b in H.rows[row] if b not in H.rows[other]]
    assert len(mine) >= len(H.rows[row]) - 1
    taken = {row, other}
    for b in mine:
        further = [j for j in H.cols[b] if j not in taken]
        assert further, (row, b)
        # a further row that shares no bit with the thread's second row, where there is one
        further.sort(key=lambda j: len(set(H.rows[j]) & set(H.rows[other])))
        taken.add(further[0])
        y[H.rows[further[0]]] = big
    y[mine] = big
    return y


@pytest.mark.gpu
@pytest.mark.parametrize("frame", [2, 3], ids=["slot0", "slot1"])
@pytest.mark.parametrize("r", [0, 1], ids=["row0", "row1"])
@pytest.mark.parametrize("vname", ["nms_fma", "oms"])
def test_pp_stream_premise_break_in_one_row_of_a_thread(gpu_ctx_factory, vname, r, frame):
    """A premise break that only the rows' test can see (every input below 2^1000, so the
    channel's own bound check passes), in row r alone of one check thread, at iteration 1, in a
    codeword of slot 0 (frame 2 of 6) or slot 1 (frame 3). The row is taken from the device's
    schedule of each pp_slots shape (an older-wave thread and a younger-wave one), the break is
    predicted by a numpy model of the decoder (exactly that row, exactly iteration 1), and the
    re-decode list must be that frame alone -- as k_rows_fast lists it -- and every frame equal the
    oracle's. With the interval's single premise test, a row-0 break is seen only through the
    maximum carried into row 1's, a row-1 break through row 1's own."""
    from ldpcsimulation_amd import codes, native
    ctx = gpu_ctx_factory(CODE)
    H = codes.read_alist(code_path(CODE))
    v = VARIANTS[vname]
    cfg = native.DecoderConfig(T=2, precision=native.F64, **v)
    try:
        for slots in ("split", "plain", "split_lds"):
            for t in (5, 300):
                ctx.set_option("rows64", "pp")
                ctx.set_option("pp_slots", slots)
                assert ctx.kernel_info(cfg)["kernel"] == "rows_pp"
                rows = _thread_rows(ctx, cfg, H, t)
                y = _given(6)
                y[frame] = _one_row_break(H, y[frame], rows[r], rows[1 - r])
                assert np.abs(y).max() < BOUND
                assert _premise_model(H, y[frame], 2, v) == [(1, rows[r])], (slots, t)
                _, d1, f1, c1, r1 = _run(ctx, cfg, "given", 6, y)
                assert r1.tolist() == [frame], (slots, t)
                ctx.set_option("rows64", "fast")
                _, d0, f0, c0, r0 = _run(ctx, cfg, "given", 6, y)
                assert r0.tolist() == [frame], (slots, t)
                assert np.array_equal(d1, d0) and np.array_equal(f1, f0) and c1.as_dict() == c0.as_dict(), (slots, t)
                want = _alist().decode(y, 2, O.Cfg(**v), workers=8)
                assert int((d1 != want).sum()) == 0, (slots, t)
    finally:
        ctx.reset_options()


@pytest.mark.gpu
@pytest.mark.parametrize("frame", [2, 3], ids=["slot0", "slot1"])
def test_pp_stream_growth_past_the_premise_is_flagged_as_by_rows_fast(gpu_ctx_factory, frame):
    """A noisy frame scaled by 2^999 and clipped to |y| <= 1.9 * 2^999 passes the channel's own
    test; its messages grow past 2^1000 after the first iterations (the numpy model: no row at
    iteration 0, some row before iteration 8), which only the rows' premise test sees. The
    re-decode list is that frame alone in k_rows_fast and in every ping-pong shape, and every
    frame equals the oracle."""
    from ldpcsimulation_amd import codes, native
    ctx = gpu_ctx_factory(CODE)
    H = codes.read_alist(code_path(CODE))
    v = VARIANTS["nms_fma"]
    y = _given(6)
    y[frame] = np.clip(y[frame], -1.9, 1.9) * 2.0 ** 999
    assert np.abs(y).max() < BOUND
    hits = _premise_model(H, y[frame], 8, v)
    assert hits and min(it for it, _ in hits) >= 1
    cfg = native.DecoderConfig(T=8, precision=native.F64, **v)
    want = _alist().decode(y, 8, O.Cfg(**v), workers=8)
    try:
        ctx.set_option("rows64", "fast")
        _, d0, f0, c0, r0 = _run(ctx, cfg, "given", 6, y)
        assert r0.tolist() == [frame]
        for slots in ("split", "plain", "split_lds"):
            ctx.set_option("rows64", "pp")
            ctx.set_option("pp_slots", slots)
            _, d1, f1, c1, r1 = _run(ctx, cfg, "given", 6, y)
            assert r1.tolist() == [frame], slots
            assert np.array_equal(d1, d0) and np.array_equal(f1, f0) and c1.as_dict() == c0.as_dict(), slots
            assert int((d1 != want).sum()) == 0, slots
    finally:
        ctx.reset_options()
