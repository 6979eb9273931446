"""Fixed-point min-sum (ldpc_fxms_*; fxms.hip) on the GPU against its numpy restatement
(tests/fxms_oracle.py, itself pinned to the C oracle by tests/test_fxms_oracle.py). Everything
after the front end is integer, so every comparison is exact, with the fp64 and the fp32 front
end, each against the restatement in the same arithmetic."""
import functools

import numpy as np
import pytest

import fxms_oracle as FO
from conftest import code_path
from ldpcsimulation_amd import codes, native

pytestmark = pytest.mark.gpu

PEG, W1944, C802, C4000 = "PEGReg504x1008.alist", "80211n_1944_r12.alist", "802_3_H.alist", "4000.2000.4.244.alist"
DVBS2 = "dvbs2_1_2.alist"
PREC = {"f64": (native.F64, np.float64), "f32": (native.F32, np.float32)}
# sigma of the given samples: some of the frames decode within 20 iterations and some do not
SIGMA = {PEG: 0.80, W1944: 0.84, C802: 0.50, C4000: 0.80}
FRAMES = {PEG: 37, W1944: 23, C802: 23, C4000: 19}   # no multiples of the codewords of a workgroup
RATE = {PEG: 0.5, W1944: 0.5, C802: 0.8413, C4000: 0.5}
FIELDS = ("bit_err", "uncoded_bit_err", "syndrome_fail", "iters")

# name -> cfg fields
CASES = {
    "ms16": dict(variant=FO.MS, msg_bits=16),
    "ms8": dict(variant=FO.MS, msg_bits=8),
    "ms6": dict(variant=FO.MS, msg_bits=6),
    "ms3": dict(variant=FO.MS, msg_bits=3),
    "nms34_6": dict(variant=FO.NMS, msg_bits=6, nms_num=3, nms_shift=2),
    "nms1316_8": dict(variant=FO.NMS, msg_bits=8, nms_num=13, nms_shift=4),
    "nms34_12": dict(variant=FO.NMS, msg_bits=12, nms_num=3, nms_shift=2),
    "oms1_6": dict(variant=FO.OMS, msg_bits=6, beta=1),
    "q3": dict(variant=FO.MS, msg_bits=6, qbits=3, ymax=7 / 4),
    "q7": dict(variant=FO.NMS, msg_bits=8, nms_num=3, nms_shift=2, qbits=7, ymax=2.5),
    "startclamp": dict(variant=FO.OMS, msg_bits=4, beta=1),   # msg_bits < qbits + 1: V = 7 < |Y|
}
# every case on the small code; on the others the two storage types, the three rules and the wide rows
MATRIX = [(PEG, c) for c in CASES] + [(W1944, c) for c in ("ms16", "ms8", "nms34_6", "oms1_6")] + \
         [(C802, c) for c in ("ms6", "nms1316_8", "nms34_12")] + [(C4000, c) for c in ("nms34_6", "ms16", "startclamp")]
# the cases whose frames both decode and fail within 20 iterations at SIGMA (the very narrow decoders
# decode nothing there, plain MS nothing on the (4, 8)-regular code, NMS everything on 802.3)
BOTH_OUTCOMES = [(c, k) for c, k in MATRIX if k not in ("ms3", "startclamp", "q3") and (c, k) != (C4000, "ms16")
                 and (c != C802 or k == "ms6")]


@functools.lru_cache(maxsize=None)
def oracle(code):
    return FO.Fxms(code_path(code))


@functools.lru_cache(maxsize=None)
def given(code, frames=None, seed=11, sigma=None):
    y = 1.0 + (sigma or SIGMA[code]) * np.random.default_rng(seed).standard_normal((frames or FRAMES[code], oracle(code).N))
    y.setflags(write=False)
    return y


def case_kw(case):
    kw = dict(variant=FO.MS, msg_bits=6, qbits=5, ymax=31 / 16, nms_num=1, nms_shift=0, beta=0)
    kw.update(CASES[case])
    return kw


def cfg_of(kw, prec, T, early_stop=False):
    return native.FxmsConfig(precision=PREC[prec][0], T=T, early_stop=early_stop, **kw)


def restate(code, kw, prec, T, y, early_stop=False, c=None):
    Y = FO.front(y.astype(PREC[prec][1]), kw["ymax"], kw["qbits"], PREC[prec][1])
    return oracle(code).decode(Y, kw["variant"], T, kw["msg_bits"], kw["nms_num"], kw["nms_shift"], kw["beta"],
                               early_stop=early_stop, c=c)


@functools.lru_cache(maxsize=None)
def reference(code, case, prec, T, early_stop=False):
    return restate(code, case_kw(case), prec, T, given(code), early_stop)


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
    info = ctx.fxms_kernel_info(cfg)
    assert info["kernel"] == ("fxms_i8" if cfg.msg_bits <= 8 else "fxms_i16")
    assert 0 < info["lds_bytes"] <= FO.WG_LDS_BOUND
    return info


def staged(ctx, info, msg_bits):
    """Whether the workgroup's LDS holds the graph beside its codewords: without it lds_bytes is a
    whole number of codeword states (the graph copy is never a multiple of one here)."""
    g = ctx.graph
    cw = FO.cw_bytes(g.N, g.M, g.maxdc, msg_bits)
    assert cw <= FO.CW_LDS_BOUND
    return info["lds_bytes"] % cw != 0


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("code,case", MATRIX, ids=["%s-%s" % (c.split(".")[0][:8], k) for c, k in MATRIX])
def test_exact_against_the_restatement(gpu_ctx_factory, code, case, prec):
    """T = 0, 1, 2 and 20 without early stop, and T = 20 with it: decisions, frame records, counters."""
    ctx = gpu_ctx_factory(code)
    kw = case_kw(case)
    y = given(code).astype(PREC[prec][1])
    info_of(ctx, cfg_of(kw, prec, 20))
    for T, es in ((0, False), (1, False), (2, False), (20, False), (20, True), (0, True)):
        want = reference(code, case, prec, T, es)
        assert_equal(ctx.fxms_decode(y, cfg_of(kw, prec, T, es)), want, T, es, (code, case, prec, T, es))
    full, es = reference(code, case, prec, 20), reference(code, case, prec, 20, True)
    if case in ("ms3", "startclamp"):
        assert full["clamped"] > 0   # the clamp is at work
    if case == "ms16" and code != C4000:   # (plain MS decodes nothing on that code at this noise, its messages stay small)
        assert full["peak"] > 127   # two-byte messages are needed
    if (code, case) in BOTH_OUTCOMES:
        assert 0 < (full["frames"]["bit_err"] > 0).sum() < len(y)
        assert ((es["s"] > 0) & (es["s"] < 20)).any() and (es["s"] == 20).any()
    elif code == C802:
        assert len(set(es["s"].tolist())) >= 3   # codewords finish unevenly


@pytest.mark.parametrize("code,case,prec,sigma", [(PEG, "nms34_6", "f32", 0.74), (W1944, "oms1_6", "f64", 0.74),
                                                  (C802, "nms34_12", "f64", 0.50)])
def test_early_stop_equals_the_fixed_T_launches(gpu_ctx_factory, code, case, prec, sigma):
    """D(s) is what the launch at T = s returns, frame by frame, for T = 0..8, at a noise level
    where the frames stop at more than one s below 8 and some not by 8."""
    ctx = gpu_ctx_factory(code)
    kw = case_kw(case)
    y = given(code, sigma=sigma).astype(PREC[prec][1])
    fixed = [ctx.fxms_decode(y, cfg_of(kw, prec, t)) for t in range(9)]
    d, fr, cnt = ctx.fxms_decode(y, cfg_of(kw, prec, 8, True))
    s = fr["iters"]
    assert len(set(s[s < 8].tolist())) >= 2 and fr["syndrome_fail"].any() and cnt.iters == int(s.sum())
    for f in range(len(y)):
        df, ff, _ = fixed[s[f]]
        assert np.array_equal(d[f], df[f]) and all(fr[k][f] == ff[k][f] for k in FIELDS[:3])
        assert all(fixed[t][1]["syndrome_fail"][f] for t in range(s[f])) and not ff["iters"].any()
        assert fr["syndrome_fail"][f] == 0 or s[f] == 8


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_batch_sizes(gpu_ctx_factory, prec):
    """A frame's result does not depend on the batch it is decoded in: batches of 1, of 7 and of
    one more than the codewords of a workgroup."""
    ctx = gpu_ctx_factory(PEG)
    kw = case_kw("nms34_6")
    y = given(PEG).astype(PREC[prec][1])
    want = reference(PEG, "nms34_6", prec, 20, True)
    cfg = cfg_of(kw, prec, 20, True)
    per_wg = 16   # at most 16 wavefronts, so 16 codewords, per workgroup
    for lo, n in ((0, 1), (5, 1), (1, 7), (8, per_wg + 1)):
        d, fr, cnt = ctx.fxms_decode(y[lo:lo + n], cfg)
        assert np.array_equal(d, want["d"][lo:lo + n]) and cnt.frames == n
        assert all(np.array_equal(fr[k], want["frames"][k][lo:lo + n]) for k in FIELDS)


@pytest.mark.parametrize("es", [False, True])
def test_1500_frames(gpu_ctx_factory, es):
    ctx = gpu_ctx_factory(PEG)
    kw = case_kw("nms34_6")
    y = given(PEG, 1500, seed=12, sigma=0.62).astype(np.float32)
    want = restate(PEG, kw, "f32", 4, y, es)
    assert_equal(ctx.fxms_decode(y, cfg_of(kw, "f32", 4, es)), want, 4, es)
    if es:
        assert len(set(want["s"].tolist())) >= 3   # codewords finish unevenly


def test_tickets_and_first_cw_splits(gpu_ctx_factory):
    """16,384 frames in one launch -- more than the 6,656 codewords the waves of the first grid
    take, so the rest go out by ticket -- against the same frames in launches of 2,048, which
    never draw a ticket: identical frame records, totals and histogram."""
    ctx = gpu_ctx_factory(PEG, 16384)
    cfg = cfg_of(case_kw("nms34_6"), "f32", 6, True)
    ctx.read_histogram(reset=True)
    fr, cnt = ctx.fxms_sim_batch(3.6, 0.5, cfg, seed=5, stream_id=3, first_cw=1000, batch=16384)
    hist = ctx.read_histogram(reset=True)
    parts, tot = [], np.zeros(6, dtype=np.int64)
    for lo in range(0, 16384, 2048):
        f, c = ctx.fxms_sim_batch(3.6, 0.5, cfg, seed=5, stream_id=3, first_cw=1000 + lo, batch=2048)
        parts.append(f)
        tot += c.as_array()
    parts = np.concatenate(parts)
    assert all(np.array_equal(fr[k], parts[k]) for k in FIELDS) and np.array_equal(cnt.as_array(), tot)
    assert np.array_equal(hist, ctx.read_histogram(reset=True))
    assert np.array_equal(hist, np.bincount(fr["bit_err"], minlength=ctx.graph.N + 1)[1:])
    assert cnt.frames == 16384 and 0 < cnt.frame_err < 16384 and cnt.iters == int(fr["iters"].sum())
    assert len(set(fr["iters"].tolist())) >= 4   # codewords finish unevenly


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_nonzero_codewords(gpu_ctx_factory, prec):
    """Codewords of the reference's PEGReg504x1008_data20.enc, through `c` and through the table."""
    ctx = gpu_ctx_factory(PEG)
    N = ctx.graph.N
    bits = codes.read_codeword_file(code_path("PEGReg504x1008_data20.enc"), N)
    assert bits.any() and len(bits) == 20
    kw = case_kw("nms34_6")
    frames = 27
    c = (1 - 2 * bits[np.arange(frames) % len(bits)].astype(np.int8)).astype(np.int8)
    y = (c * given(PEG, frames, seed=13)).astype(PREC[prec][1])
    for es in (False, True):
        want = restate(PEG, kw, prec, 10, y, es, c)
        assert want["frames"]["uncoded_bit_err"].min() > 0
        assert_equal(ctx.fxms_decode(y, cfg_of(kw, prec, 10, es), c=c), want, 10, es)
    ctx.set_codewords(bits)
    try:
        cfg = cfg_of(kw, prec, 10, True)
        y2, code, d, fr, cnt = ctx.fxms_sim_trace(1.8, 0.5, cfg, seed=7, stream_id=2, first_cw=33, batch=frames)
        c2 = (1 - 2 * bits[(33 + np.arange(frames)) % len(bits)].astype(np.int8)).astype(np.int8)
        assert (np.sign(y2) != c2).any() and (np.sign(y2) == c2).mean() > 0.8
        assert_equal((d, fr, cnt), restate(PEG, kw, prec, 10, y2, True, c2), 10, True)
    finally:
        ctx.set_codewords(None)


@pytest.mark.parametrize("code,case,prec", [(PEG, "nms34_6", "f32"), (PEG, "ms16", "f64"), (W1944, "oms1_6", "f64"),
                                            (C802, "nms1316_8", "f32")])
def test_sim_path(gpu_ctx_factory, code, case, prec):
    """sim_batch = sim_trace = decode_batch on the traced samples = the restatement; the traced
    samples are the min-sum path's and the codes the restatement's front end."""
    ctx = gpu_ctx_factory(code)
    kw = case_kw(case)
    snr, R, frames = {PEG: 1.8, W1944: 1.9, C802: 3.5}[code], RATE[code], 29
    cfg = cfg_of(kw, prec, 12, True)
    args = dict(seed=21, stream_id=4, first_cw=7, batch=frames)
    ctx.read_histogram(reset=True)
    y, ycode, d, fr, cnt = ctx.fxms_sim_trace(snr, R, cfg, **args)
    hist = ctx.read_histogram(reset=True)
    assert y.dtype == PREC[prec][1]
    ms = native.DecoderConfig(variant=native.MS, T=0, precision=PREC[prec][0])
    assert np.array_equal(y, ctx.sim_trace(snr, R, ms, **args)[0])
    assert np.array_equal(ycode, FO.front(y, kw["ymax"], kw["qbits"], PREC[prec][1]))
    want = restate(code, kw, prec, 12, y, True)
    assert_equal((d, fr, cnt), want, 12, True)
    assert np.array_equal(hist, np.bincount(fr["bit_err"], minlength=ctx.graph.N + 1)[1:])
    fr2, cnt2 = ctx.fxms_sim_batch(snr, R, cfg, **args)
    assert all(np.array_equal(fr[k], fr2[k]) for k in FIELDS) and np.array_equal(cnt.as_array(), cnt2.as_array())
    assert_equal(ctx.fxms_decode(y, cfg), want, 12, True)
    assert 0 < cnt.frame_err < frames
    # the asynchronous launch: the same frame records in device memory, counts in the context
    import torch
    dev = torch.zeros((frames, 4), dtype=torch.int32, device="cuda:0")
    before = ctx.read_counts().as_array()
    ctx.fxms_sim_launch(snr, R, cfg, frames_dev=dev, **args)
    ctx.synchronize()
    after = ctx.read_counts().as_array()
    assert np.array_equal(after - before, cnt.as_array())
    assert np.array_equal(dev.cpu().numpy(), np.asarray(fr).view(np.int32).reshape(frames, 4))


@pytest.mark.parametrize("name", list(FO.GRID_CASES))
@pytest.mark.parametrize("variant", [FO.MS, FO.OMS])
def test_unsaturated_decoder_equals_the_shipped_fp64_min_sum(gpu_ctx_factory, name, variant):
    """The inputs of tests/test_fxms_oracle.py: on grid samples, 16-bit messages never saturate
    and the decisions are those of the fp64 decoder with the same quantiser."""
    G = FO.GRID
    code, snr, T = FO.GRID_CASES[name]
    ctx = gpu_ctx_factory(code)
    y = FO.grid_samples(ctx.graph.N, snr)
    fx = native.FxmsConfig(variant=variant, T=T, qbits=G["qbits"], msg_bits=G["msg_bits"], beta=G["beta"], ymax=G["ymax"])
    d, fr, _ = ctx.fxms_decode(y, fx)
    ms = native.DecoderConfig(variant=variant, T=T, precision=native.F64, delta=G["delta"], quantize=True, ymax=G["ymax"],
                              qbits=G["qbits"])
    dm, frm, _ = ctx.decode(y, ms)
    assert np.array_equal(d, dm) and all(np.array_equal(fr[k], frm[k]) for k in FIELDS)
    assert 0 < (fr["bit_err"] > 0).sum() < len(y)


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    """Generated codes: (4, 8)-regular ones whose codeword fits the 64 KiB bound while the 16-bit
    graph copy does not fit beside it (N = 8000 with one-byte messages: 48 000 + 128 000 bytes;
    N = 6400 with two-byte ones: 64 000 + 102 400), and PEG with checks of degree 0, 1 and 2 and a
    bit of degree 0."""
    root = tmp_path_factory.mktemp("fxms_codes")
    return {"r8000": FO.write_regular_code(str(root / "r8000.alist"), 8000),
            "r6400": FO.write_regular_code(str(root / "r6400.alist"), 6400),
            "edge": FO.write_edge_code(str(root / "peg_edge.alist"), code_path(PEG))}


def noisy(N, frames, lo, hi, seed):
    """Frames of rising noise, sigma from lo to hi: the first decode early, the last do not."""
    sigma = np.linspace(lo, hi, frames)[:, None]
    return 1.0 + sigma * np.random.default_rng(seed).standard_normal((frames, N))


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("name,msg_bits", [("r8000", 6), ("r8000", 8), ("r6400", 12), ("r6400", 16)])
def test_graph_not_staged(gpu_ctx_factory, generated, name, msg_bits, prec):
    """The kernel instances that read the graph from global memory, exact against the
    restatement; the same codes take the staged instances at the other message width."""
    ctx = gpu_ctx_factory(generated[name], 64)
    kw = dict(case_kw("nms34_6"), msg_bits=msg_bits)
    info = info_of(ctx, cfg_of(kw, prec, 12))
    assert not staged(ctx, info, msg_bits)
    if name == "r6400":
        assert staged(ctx, info_of(ctx, cfg_of(dict(kw, msg_bits=8), prec, 12)), 8)
    else:
        with pytest.raises(native.LdpcError) as e:   # two-byte messages exceed the codeword bound there
            ctx.fxms_kernel_info(cfg_of(dict(kw, msg_bits=12), prec, 12))
        assert e.value.code == -4
    y = noisy(ctx.graph.N, 11, 0.6, 1.0, 31).astype(PREC[prec][1])
    for T, es in ((0, False), (2, False), (12, False), (12, True)):
        want = restate(generated[name], kw, prec, T, y, es)
        assert_equal(ctx.fxms_decode(y, cfg_of(kw, prec, T, es)), want, T, es, (name, msg_bits, prec, T, es))
    assert len(set(want["s"].tolist())) >= 3 and want["frames"]["syndrome_fail"].any()
    # the on-device channel through the same instance
    cfg = cfg_of(kw, prec, 12, True)
    ys, ycode, d, fr, cnt = ctx.fxms_sim_trace(2.5, 0.5, cfg, seed=3, stream_id=1, first_cw=5, batch=7)
    assert_equal((d, fr, cnt), restate(generated[name], kw, prec, 12, ys, True), 12, True)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("case", ["ms6", "nms34_6", "oms1_6", "ms16"])
def test_checks_of_degree_0_1_2_and_a_bit_of_degree_0(gpu_ctx_factory, generated, case, prec):
    """A check of degree 1 sends f(V) (both minima are V where the row has fewer edges), a check
    of degree 0 nothing, and a bit without checks keeps its channel decision."""
    ctx = gpu_ctx_factory(generated["edge"], 64)
    fx = oracle(generated["edge"])
    assert (ctx.graph.N, ctx.graph.M) == (1009, 507) and fx.E == ctx.graph.E == 3027
    kw = case_kw(case)
    y = noisy(ctx.graph.N, 13, 0.7, 0.9, 32).astype(PREC[prec][1])
    for T, es in ((0, False), (1, False), (20, False), (20, True)):
        want = restate(generated["edge"], kw, prec, T, y, es)
        assert_equal(ctx.fxms_decode(y, cfg_of(kw, prec, T, es)), want, T, es, (case, prec, T, es))
    assert np.array_equal(want["d"][:, 1008], np.where(y[:, 1008] >= 0, 1, -1))   # the bit without checks
    assert (want["d"][:, 1008] == -1).any() and want["frames"]["syndrome_fail"].any() and (want["s"] < 20).any()


def test_dvbs2_is_unsupported(gpu_ctx_factory):
    ctx = gpu_ctx_factory(DVBS2, 8)
    for bits in (6, 12):
        with pytest.raises(native.LdpcError) as e:
            ctx.fxms_kernel_info(native.FxmsConfig(msg_bits=bits))
        assert e.value.code == -4 and "65536" in str(e.value)
    with pytest.raises(native.LdpcError) as e:
        ctx.fxms_sim_batch(1.0, 0.5, native.FxmsConfig(), seed=1, stream_id=0, first_cw=0, batch=2)
    assert e.value.code == -4


def test_kernel_info(gpu_ctx_factory):
    lds = {}
    for code in (PEG, W1944, C802, C4000):
        ctx = gpu_ctx_factory(code)
        lds[code] = [info_of(ctx, native.FxmsConfig(msg_bits=b))["lds_bytes"] for b in (2, 8, 9, 16)]
        assert lds[code][0] == lds[code][1] and lds[code][2] == lds[code][3]
    with pytest.raises(native.LdpcError) as e:
        gpu_ctx_factory(PEG).fxms_kernel_info(native.FxmsConfig(variant=native.BP))
    assert e.value.code == -4
