"""Layered fixed-point min-sum (ldpc_fxlms_*; fxlms.hip) on the GPU against its numpy restatement
(tests/fxlms_oracle.py, itself pinned to the C oracle's fp64 layered decoder by
tests/test_fxlms_oracle.py), in the row order of Graph.layers(). Everything after the front end
is integer, so every comparison is exact, with the fp64 and the fp32 front end, each against
the restatement in the same arithmetic."""
import functools

import numpy as np
import pytest

import fxlms_oracle as FL
from conftest import code_path
from ldpcsimulation_amd import codes, native

pytestmark = pytest.mark.gpu

PEG, W1944, C802, C4000 = "PEGReg504x1008.alist", "80211n_1944_r12.alist", "802_3_H.alist", "4000.2000.4.244.alist"
DVBS2 = "dvbs2_1_2.alist"
PREC = {"f64": (native.F64, np.float64), "f32": (native.F32, np.float32)}
# sigma of the given samples rises over the 16 frames from the first value to the second: around
# the waterfall of the wider decoders, so their first frames decode within 8 iterations and their last do not
SIGMA = {PEG: (0.55, 0.95), W1944: (0.55, 0.95), C802: (0.38, 0.60), C4000: (0.55, 0.95)}
FRAMES = 16
RATE = {PEG: 0.5, W1944: 0.5, C802: 0.8413, C4000: 0.5}
FIELDS = ("bit_err", "uncoded_bit_err", "syndrome_fail", "iters")
TMAX = 8

# name -> cfg fields (msg_bits / app_bits)
CASES = {
    "ms_6_7": dict(variant=FL.MS, msg_bits=6, app_bits=7),
    "nms34_6_7": dict(variant=FL.NMS, msg_bits=6, app_bits=7, nms_num=3, nms_shift=2),
    "oms1_6_7": dict(variant=FL.OMS, msg_bits=6, app_bits=7, beta=1),
    "nms34_8_8": dict(variant=FL.NMS, msg_bits=8, app_bits=8, nms_num=3, nms_shift=2),
    "ms_12_13": dict(variant=FL.MS, msg_bits=12, app_bits=13),
    "ms_16_16": dict(variant=FL.MS, msg_bits=16, app_bits=16),
    "nms1316_4_5_q3": dict(variant=FL.NMS, msg_bits=4, app_bits=5, nms_num=13, nms_shift=4, qbits=3, ymax=7 / 4),
}
CODES = (PEG, W1944, C802, C4000)
MATRIX = [(c, k) for c in CODES for k in CASES]


@functools.lru_cache(maxsize=None)
def oracle(path):
    """(the restatement, the library's row order) of a code file."""
    p = path if "/" in path else code_path(path)
    return FL.Fxlms(p), native.Graph.from_alist(p).layers()[0]


def noisy(N, frames, lo, hi, seed):
    """Frames of rising noise, sigma from lo to hi: the first decode early, the last do not."""
    sigma = np.linspace(lo, hi, frames)[:, None]
    return 1.0 + sigma * np.random.default_rng(seed).standard_normal((frames, N))


@functools.lru_cache(maxsize=None)
def given(code, frames=FRAMES, seed=11):
    y = noisy(oracle(code)[0].N, frames, *SIGMA[code], seed)
    y.setflags(write=False)
    return y


def case_kw(case):
    kw = dict(variant=FL.MS, msg_bits=6, app_bits=7, qbits=5, ymax=31 / 16, nms_num=1, nms_shift=0, beta=0)
    kw.update(CASES[case] if isinstance(case, str) else case)
    return kw


def cfg_of(kw, prec, T, early_stop=False):
    return native.FxlmsConfig(precision=PREC[prec][0], T=T, early_stop=early_stop, **kw)


_TRAJ = {}


def trajectory(code, kw, prec, T, y):
    """One pass of the restatement per (code, cfg, integer codes, T), shared by the tests: the fp32 and
    the fp64 front end give the same codes for most sample sets."""
    fx, order = oracle(code)
    Y = FL.front(np.asarray(y).astype(PREC[prec][1]), kw["ymax"], kw["qbits"], PREC[prec][1])
    key = (code, tuple(sorted(kw.items())), T, Y.tobytes())
    if key not in _TRAJ:
        _TRAJ[key] = fx.trajectory(Y, kw["variant"], T, kw["msg_bits"], kw["app_bits"], kw["nms_num"], kw["nms_shift"],
                                   kw["beta"], order=order)
    return _TRAJ[key]


def restate(code, kw, prec, T, y, early_stop=False, c=None, tmax=None):
    return oracle(code)[0].result(trajectory(code, kw, prec, tmax or T, y), T, early_stop, c)


def assert_equal(got, want, T, early_stop, where=""):
    d, fr, cnt = got
    for k in FIELDS:
        assert np.array_equal(fr[k], want["frames"][k]), (where, k, fr[k], want["frames"][k])
    assert np.array_equal(d, want["d"]), where
    c, wf = cnt.as_dict(), want["frames"]
    assert c["frames"] == len(d) and c["iters"] == (int(want["s"].sum()) if early_stop else T * len(d)), where
    assert c["bit_err"] == int(wf["bit_err"].sum()) and c["frame_err"] == int((wf["bit_err"] > 0).sum()), where
    assert c["uncoded_bit_err"] == int(wf["uncoded_bit_err"].sum()), where
    assert c["syndrome_fail"] == int(wf["syndrome_fail"].sum()), where


def info_of(ctx, cfg):
    info = ctx.fxlms_kernel_info(cfg)
    assert info["kernel"] == ("fxlms_i8" if cfg.app_bits <= 8 else "fxlms_i16")
    assert 0 < info["lds_bytes"] <= FL.WG_LDS_BOUND
    return info


def staged(ctx, info, app_bits):
    """Whether the workgroup's LDS holds the schedule beside its codewords: lds_bytes is a whole
    number of codeword states, with or without the schedule's bytes in front."""
    g = ctx.graph
    cw, sched = FL.cw_bytes(g.N, g.M, g.maxdc, app_bits), FL.sched_bytes(g.M, g.maxdc)
    assert cw <= FL.CW_LDS_BOUND
    plain, with_sched = info["lds_bytes"] % cw == 0, info["lds_bytes"] > sched and (info["lds_bytes"] - sched) % cw == 0
    assert plain != with_sched, (info, cw, sched)
    return with_sched


# The cases in which no frame reaches a codeword within 8 iterations (from the restatement; DESIGN §13g:
# at messages one bit wider than the samples a saturated APP holds no more than one message and the sample,
# which the 1944-bit code's bits of degree up to 11 do not survive).
UNDECODED = {(W1944, "ms_6_7"), (W1944, "oms1_6_7"), (W1944, "nms1316_4_5_q3")}


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("code,case", MATRIX, ids=["%s-%s" % (c.split(".")[0][:8], k) for c, k in MATRIX])
def test_exact_against_the_restatement(gpu_ctx_factory, code, case, prec):
    """T = 0, 1, 2 and 8 without early stop, and T = 8 and 0 with it: decisions, frame records, counters."""
    ctx = gpu_ctx_factory(code)
    kw = case_kw(case)
    y = given(code).astype(PREC[prec][1])
    info_of(ctx, cfg_of(kw, prec, TMAX))
    for T, es in ((0, False), (1, False), (2, False), (TMAX, False), (TMAX, True), (0, True)):
        want = restate(code, kw, prec, T, y, es, tmax=TMAX)
        assert_equal(ctx.fxlms_decode(y, cfg_of(kw, prec, T, es)), want, T, es, (code, case, prec, T, es))
    full, es = restate(code, kw, prec, TMAX, y), restate(code, kw, prec, TMAX, y, True)
    assert full["frames"]["bit_err"].any()   # the noisiest frames fail everywhere
    if case in ("nms34_8_8", "nms1316_4_5_q3"):
        assert full["clamped"] > 0   # the clamps are at work
    if case == "ms_16_16":
        assert full["peak_app"] > 127   # two-byte APPs are needed
    if (code, case) in UNDECODED:
        assert (es["s"] == TMAX).all()
    else:   # frames that stop at a codeword, unevenly, and frames that do not
        assert ((es["s"] > 0) & (es["s"] < TMAX)).any() and (es["s"] == TMAX).any()
        assert 0 < (es["frames"]["bit_err"] > 0).sum() < len(y), (code, case)


@pytest.mark.parametrize("code,case,prec", [(PEG, "nms34_6_7", "f32"), (W1944, "nms34_8_8", "f64"), (C802, "ms_12_13", "f64")])
def test_early_stop_equals_the_fixed_T_launches(gpu_ctx_factory, code, case, prec):
    """D(s) is what the launch at T = s returns, frame by frame, for T = 0..8."""
    ctx = gpu_ctx_factory(code)
    kw = case_kw(case)
    y = given(code).astype(PREC[prec][1])
    fixed = [ctx.fxlms_decode(y, cfg_of(kw, prec, t)) for t in range(TMAX + 1)]
    d, fr, cnt = ctx.fxlms_decode(y, cfg_of(kw, prec, TMAX, True))
    s = fr["iters"]
    assert len(set(s[s < TMAX].tolist())) >= 2 and fr["syndrome_fail"].any() and cnt.iters == int(s.sum())
    for f in range(len(y)):
        df, ff, _ = fixed[s[f]]
        assert np.array_equal(d[f], df[f]) and all(fr[k][f] == ff[k][f] for k in FIELDS[:3])
        assert all(fixed[t][1]["syndrome_fail"][f] for t in range(s[f])) and not ff["iters"].any()
        assert fr["syndrome_fail"][f] == 0 or s[f] == TMAX


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_batch_sizes(gpu_ctx_factory, prec):
    """A frame's result does not depend on the batch it is decoded in: batches of 1, of 7 and of
    one more than the codewords of a workgroup."""
    ctx = gpu_ctx_factory(PEG)
    kw = case_kw("nms34_8_8")
    y = given(PEG, 26, 14).astype(PREC[prec][1])
    want = restate(PEG, kw, prec, TMAX, y, True)
    cfg = cfg_of(kw, prec, TMAX, True)
    per_wg = 16   # at most 16 wavefronts, so 16 codewords, per workgroup
    for lo, n in ((0, 1), (5, 1), (1, 7), (8, per_wg + 1)):
        d, fr, cnt = ctx.fxlms_decode(y[lo:lo + n], cfg)
        assert np.array_equal(d, want["d"][lo:lo + n]) and cnt.frames == n
        assert all(np.array_equal(fr[k], want["frames"][k][lo:lo + n]) for k in FIELDS)


def test_tickets_and_first_cw_splits(gpu_ctx_factory):
    """16,384 frames in one launch -- more than the waves of the first grid take, so the rest go
    out by ticket -- against the same frames in launches of 2,048: identical frame records, totals
    and histogram."""
    ctx = gpu_ctx_factory(PEG, 16384)
    cfg = cfg_of(case_kw("nms34_8_8"), "f32", 3, True)
    ctx.read_histogram(reset=True)
    fr, cnt = ctx.fxlms_sim_batch(2.6, 0.5, cfg, seed=5, stream_id=3, first_cw=1000, batch=16384)
    hist = ctx.read_histogram(reset=True)
    parts, tot = [], np.zeros(6, dtype=np.int64)
    for lo in range(0, 16384, 2048):
        f, c = ctx.fxlms_sim_batch(2.6, 0.5, cfg, seed=5, stream_id=3, first_cw=1000 + lo, batch=2048)
        parts.append(f)
        tot += c.as_array()
    parts = np.concatenate(parts)
    assert all(np.array_equal(fr[k], parts[k]) for k in FIELDS) and np.array_equal(cnt.as_array(), tot)
    assert np.array_equal(hist, ctx.read_histogram(reset=True))
    assert np.array_equal(hist, np.bincount(fr["bit_err"], minlength=ctx.graph.N + 1)[1:])
    assert cnt.frames == 16384 and 0 < cnt.frame_err < 16384 and cnt.iters == int(fr["iters"].sum())
    assert len(set(fr["iters"].tolist())) >= 2   # codewords finish unevenly (within T = 3: after 2 or 3 iterations)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_nonzero_codewords(gpu_ctx_factory, prec):
    """Codewords of the reference's PEGReg504x1008_data20.enc, through `c` and through the table."""
    ctx = gpu_ctx_factory(PEG)
    N = ctx.graph.N
    bits = codes.read_codeword_file(code_path("PEGReg504x1008_data20.enc"), N)
    assert bits.any() and len(bits) == 20
    kw = case_kw("nms34_8_8")
    frames = 27
    c = (1 - 2 * bits[np.arange(frames) % len(bits)].astype(np.int8)).astype(np.int8)
    y = (c * given(PEG, frames, 13)).astype(PREC[prec][1])
    for es in (False, True):
        want = restate(PEG, kw, prec, TMAX, y, es, c)
        assert want["frames"]["uncoded_bit_err"].min() > 0
        assert_equal(ctx.fxlms_decode(y, cfg_of(kw, prec, TMAX, es), c=c), want, TMAX, es)
    ctx.set_codewords(bits)
    try:
        cfg = cfg_of(kw, prec, TMAX, True)
        y2, code, d, fr, cnt = ctx.fxlms_sim_trace(1.8, 0.5, cfg, seed=7, stream_id=2, first_cw=33, batch=frames)
        c2 = (1 - 2 * bits[(33 + np.arange(frames)) % len(bits)].astype(np.int8)).astype(np.int8)
        assert (np.sign(y2) != c2).any() and (np.sign(y2) == c2).mean() > 0.8
        assert_equal((d, fr, cnt), restate(PEG, kw, prec, TMAX, y2, True, c2), TMAX, True)
    finally:
        ctx.set_codewords(None)


@pytest.mark.parametrize("code,case,prec", [(PEG, "nms34_6_7", "f32"), (PEG, "ms_16_16", "f64"), (W1944, "nms34_8_8", "f64"),
                                            (C802, "ms_12_13", "f32")])
def test_sim_path(gpu_ctx_factory, code, case, prec):
    """sim_batch = sim_trace = decode_batch on the traced samples = the restatement; the traced
    samples and codes are fixed-point min-sum's, bit for bit."""
    ctx = gpu_ctx_factory(code)
    kw = case_kw(case)
    snr, R, frames = {PEG: 1.8, W1944: 1.6, C802: 3.6}[code], RATE[code], 29
    cfg = cfg_of(kw, prec, TMAX, True)
    args = dict(seed=21, stream_id=4, first_cw=7, batch=frames)
    ctx.read_histogram(reset=True)
    y, ycode, d, fr, cnt = ctx.fxlms_sim_trace(snr, R, cfg, **args)
    hist = ctx.read_histogram(reset=True)
    assert y.dtype == PREC[prec][1]
    flood = native.FxmsConfig(variant=kw["variant"], T=0, qbits=kw["qbits"], msg_bits=kw["msg_bits"], ymax=kw["ymax"],
                              precision=PREC[prec][0])
    yf, ycodef = ctx.fxms_sim_trace(snr, R, flood, **args)[:2]
    assert np.array_equal(y, yf) and np.array_equal(ycode, ycodef)
    assert np.array_equal(ycode, FL.front(y, kw["ymax"], kw["qbits"], PREC[prec][1]))
    want = restate(code, kw, prec, TMAX, y, True)
    assert_equal((d, fr, cnt), want, TMAX, True)
    assert np.array_equal(hist, np.bincount(fr["bit_err"], minlength=ctx.graph.N + 1)[1:])
    fr2, cnt2 = ctx.fxlms_sim_batch(snr, R, cfg, **args)
    assert all(np.array_equal(fr[k], fr2[k]) for k in FIELDS) and np.array_equal(cnt.as_array(), cnt2.as_array())
    assert_equal(ctx.fxlms_decode(y, cfg), want, TMAX, True)
    # the asynchronous launch: the same frame records in device memory, counts in the context
    import torch
    dev = torch.zeros((frames, 4), dtype=torch.int32, device="cuda:0")
    before = ctx.read_counts().as_array()
    ctx.fxlms_sim_launch(snr, R, cfg, frames_dev=dev, **args)
    ctx.synchronize()
    after = ctx.read_counts().as_array()
    assert np.array_equal(after - before, cnt.as_array())
    assert np.array_equal(dev.cpu().numpy(), np.asarray(fr).view(np.int32).reshape(frames, 4))


@pytest.mark.parametrize("name", list(FL.GRID_CASES))
@pytest.mark.parametrize("variant", [FL.MS, FL.OMS])
def test_unclamped_decoder_equals_the_shipped_fp64_layered_decoder(gpu_ctx_factory, name, variant):
    """The inputs of tests/test_fxlms_oracle.py: on grid samples 16-bit messages and APPs never
    clamp and the decisions are those of the fp64 layered decoder with the same quantiser."""
    G = FL.GRID
    code, snr, T = FL.GRID_CASES[name]
    ctx = gpu_ctx_factory(code)
    y = FL.grid_samples(ctx.graph.N, snr)
    fx = native.FxlmsConfig(variant=variant, T=T, qbits=G["qbits"], msg_bits=16, app_bits=16, beta=G["beta"], ymax=G["ymax"])
    d, fr, _ = ctx.fxlms_decode(y, fx)
    ms = native.DecoderConfig(variant=variant, T=T, precision=native.F64, delta=G["delta"], quantize=True, ymax=G["ymax"],
                              qbits=G["qbits"], schedule=native.LAYERED)
    dm, frm, _ = ctx.decode(y, ms)
    assert np.array_equal(d, dm) and all(np.array_equal(fr[k], frm[k]) for k in FIELDS)
    assert 0 < (fr["bit_err"] > 0).sum() < len(y)


def write_uneven_code(path):
    """A code whose layers are 40, 200 and 40 rows: 40 disjoint rows, 200 rows that each hold a bit
    of one of them, and 40 rows that each hold a bit of both kinds."""
    rows = [list(range(6 * i, 6 * i + 6)) for i in range(40)]
    nxt = 240
    for i in range(200):
        rows.append([i] + list(range(nxt, nxt + 5)))
        nxt += 5
    for i in range(40):
        rows.append([200 + i, 240 + 5 * i + 1] + list(range(nxt, nxt + 4)))
        nxt += 4
    codes.write_alist(codes.ParityCheck.from_rows(nxt, rows), path)
    return path


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    """Generated codes: (4, 8)-regular ones where a copy of the schedule in LDS would cost more than
    a quarter of the resident waves, so the kernel reads it from global memory; PEG with checks of
    degree 0, 1 and 2 and a bit of degree 0; and a code with a short layer before a long one."""
    root = tmp_path_factory.mktemp("fxlms_codes")
    return {"r8000": FL.write_regular_code(str(root / "r8000.alist"), 8000),
            "r6400": FL.write_regular_code(str(root / "r6400.alist"), 6400),
            "edge": FL.write_edge_code(str(root / "peg_edge.alist"), code_path(PEG)),
            "uneven": write_uneven_code(str(root / "uneven.alist"))}


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("name,bits", [("r8000", (6, 7)), ("r8000", (8, 8)), ("r6400", (12, 13)), ("r6400", (16, 16))])
def test_schedule_not_staged(gpu_ctx_factory, generated, name, bits, prec):
    """The kernel instances that read the schedule from global memory, exact against the
    restatement, with given samples and with the on-device channel."""
    ctx = gpu_ctx_factory(generated[name], 64)
    kw = dict(case_kw("nms34_6_7"), msg_bits=bits[0], app_bits=bits[1])
    info = info_of(ctx, cfg_of(kw, prec, TMAX))
    assert not staged(ctx, info, bits[1])
    y = noisy(ctx.graph.N, 11, 0.5, 0.9, 31).astype(PREC[prec][1])
    for T, es in ((0, False), (2, False), (TMAX, False), (TMAX, True)):
        want = restate(generated[name], kw, prec, T, y, es, tmax=TMAX)
        assert_equal(ctx.fxlms_decode(y, cfg_of(kw, prec, T, es)), want, T, es, (name, bits, prec, T, es))
    assert want["frames"]["syndrome_fail"].any()
    cfg = cfg_of(kw, prec, TMAX, True)
    ys, ycode, d, fr, cnt = ctx.fxlms_sim_trace(2.5, 0.5, cfg, seed=3, stream_id=1, first_cw=5, batch=7)
    assert_equal((d, fr, cnt), restate(generated[name], kw, prec, TMAX, ys, True), TMAX, True)


def test_staged_and_not_on_the_shipped_codes(gpu_ctx_factory):
    """The four codes take the staged instances, but 802.3an at one-byte APPs, where the copy of
    its 32 slots a row would cost nine of twenty-seven resident waves."""
    for code in CODES:
        ctx = gpu_ctx_factory(code)
        for ab in (7, 13):
            info = info_of(ctx, native.FxlmsConfig(msg_bits=6, app_bits=ab))
            assert staged(ctx, info, ab) == ((code, ab) != (C802, 7)), (code, ab, info)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("case", ["ms_6_7", "nms34_8_8", "oms1_6_7", "ms_16_16"])
def test_checks_of_degree_0_1_2_and_a_bit_of_degree_0(gpu_ctx_factory, generated, case, prec):
    """A check of degree 1 sends f(V) (m2 = V where the row has one edge), a check of degree 0
    nothing, and a bit without checks keeps its channel decision."""
    ctx = gpu_ctx_factory(generated["edge"], 64)
    fx = oracle(generated["edge"])[0]
    assert (ctx.graph.N, ctx.graph.M) == (1009, 507) and fx.E == ctx.graph.E == 3027
    kw = case_kw(case)
    y = noisy(ctx.graph.N, 13, 0.6, 0.9, 32).astype(PREC[prec][1])
    for T, es in ((0, False), (1, False), (TMAX, False), (TMAX, True)):
        want = restate(generated["edge"], kw, prec, T, y, es, tmax=TMAX)
        assert_equal(ctx.fxlms_decode(y, cfg_of(kw, prec, T, es)), want, T, es, (case, prec, T, es))
    assert np.array_equal(want["d"][:, 1008], np.where(y[:, 1008] >= 0, 1, -1))   # the bit without checks
    assert (want["d"][:, 1008] == -1).any() and want["frames"]["syndrome_fail"].any()


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_short_layer_before_a_long_one(gpu_ctx_factory, generated, prec):
    """Layers of 40, 200 and 40 rows: a wave's only pass over a layer with idle lanes, then four
    passes, the last of them partial."""
    ctx = gpu_ctx_factory(generated["uneven"], 64)
    _, ptr = ctx.graph.layers()
    sizes = np.diff(ptr).tolist()
    assert any(a < 64 and b > 128 for a, b in zip(sizes, sizes[1:])), sizes
    y = noisy(ctx.graph.N, 9, 0.7, 1.1, 33).astype(PREC[prec][1])
    for case in ("nms34_6_7", "ms_12_13"):
        kw = case_kw(case)
        for T, es in ((1, False), (TMAX, False), (TMAX, True)):
            want = restate(generated["uneven"], kw, prec, T, y, es, tmax=TMAX)
            assert_equal(ctx.fxlms_decode(y, cfg_of(kw, prec, T, es)), want, T, es, (case, prec, T, es))


def test_dvbs2_is_unsupported(gpu_ctx_factory):
    ctx = gpu_ctx_factory(DVBS2, 8)
    for bits in (6, 12):
        with pytest.raises(native.LdpcError) as e:
            ctx.fxlms_kernel_info(native.FxlmsConfig(msg_bits=bits))
        assert e.value.code == -4 and "65536" in str(e.value)
    with pytest.raises(native.LdpcError) as e:
        ctx.fxlms_sim_batch(1.0, 0.5, native.FxlmsConfig(), seed=1, stream_id=0, first_cw=0, batch=2)
    assert e.value.code == -4


def test_kernel_info(gpu_ctx_factory):
    for code in CODES:
        ctx = gpu_ctx_factory(code)
        lds = [info_of(ctx, native.FxlmsConfig(msg_bits=m, app_bits=a))["lds_bytes"] for m, a in ((2, 2), (8, 8), (9, 9), (16, 16))]
        assert lds[0] == lds[1] and lds[2] == lds[3]
    ctx = gpu_ctx_factory(PEG)
    assert ctx.fxlms_kernel_info(native.FxlmsConfig(msg_bits=8, app_bits=8))["kernel"] == "fxlms_i8"
    assert ctx.fxlms_kernel_info(native.FxlmsConfig(msg_bits=9, app_bits=9))["kernel"] == "fxlms_i16"
    assert ctx.fxlms_kernel_info(native.FxlmsConfig(msg_bits=4, app_bits=9))["kernel"] == "fxlms_i16"
    with pytest.raises(native.LdpcError) as e:
        ctx.fxlms_kernel_info(native.FxlmsConfig(variant=native.BP))
    assert e.value.code == -4
