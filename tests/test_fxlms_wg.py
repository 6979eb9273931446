"""The workgroup-per-codeword kernel of layered fixed-point min-sum (fxlms_wg.hip),
which option kernel = global selects for the five ldpc_fxlms_* calls: exact against the numpy
restatement taken a layer at a time (tests/fxlms_layer_oracle.py, pinned to the row-serial one by
tests/test_fxlms_wg_host.py) in the row order of Graph.layers(), byte-equal to the default kernel
wherever that one runs, and on DVB-S2 N=64800, which the default kernel refuses. Every case runs
with ctx.set_option("kernel", "global") and asserts the kernel's name; every comparison is exact.
The cfgs, sample sets and helpers are those of tests/test_fxlms.py.

The planner gives a code of a few thousand bits a wavefront per workgroup, so on those codes a
grid holds thousands of codewords; only DVB-S2 runs workgroups of 512 (one-byte APPs) and 1,024
threads (two-byte), whose layers of 275 to 3,044 rows leave waves idle in one layer and take
several passes in the next."""
import functools

import numpy as np
import pytest

import fxlms_layer_oracle as LO
import fxlms_oracle as FL
import test_fxlms as TF
from conftest import code_path
from ldpcsimulation_amd import codes, native

pytestmark = pytest.mark.gpu

PEG, W1944, C802, C4000, DVBS2 = TF.PEG, TF.W1944, TF.C802, TF.C4000, TF.DVBS2
PREC, FIELDS, TMAX = TF.PREC, TF.FIELDS, TF.TMAX
CASES = ("ms_6_7", "nms34_8_8", "oms1_6_7", "ms_12_13", "ms_16_16")
MATRIX = [(c, k) for c in TF.CODES for k in CASES]
NMS_8_9 = dict(variant=FL.NMS, msg_bits=8, app_bits=9, nms_num=3, nms_shift=2)


@functools.lru_cache(maxsize=None)
def oracle(path):
    """(the layer-at-a-time restatement, the library's row order, its layer bounds) of a code file."""
    p = path if "/" in path else code_path(path)
    order, ptr = native.Graph.from_alist(p).layers()
    return LO.LayerFxlms(p), order, ptr


_TRAJ = {}


def restate(code, kw, prec, T, y, early_stop=False, c=None, tmax=None):
    """The restatement's result at T from one pass of tmax iterations per (code, cfg, integer codes)."""
    fx, order, ptr = oracle(code)
    Y = FL.front(np.asarray(y).astype(PREC[prec][1]), kw["ymax"], kw["qbits"], PREC[prec][1])
    key = (code, tuple(sorted(kw.items())), tmax or T, Y.tobytes())
    if key not in _TRAJ:
        _TRAJ[key] = fx.trajectory(Y, kw["variant"], tmax or T, kw["msg_bits"], kw["app_bits"], kw["nms_num"], kw["nms_shift"],
                                   kw["beta"], order=order, ptr=ptr)
    return fx.result(_TRAJ[key], T, early_stop, c)


def wg_ctx(factory, code, max_batch=4096):
    ctx = factory(code, max_batch)
    ctx.set_option("kernel", "global")
    return ctx


def info_of(ctx, cfg):
    info = ctx.fxlms_kernel_info(cfg)
    assert info["kernel"] == ("fxlms_wg_i8" if cfg.app_bits <= 8 else "fxlms_wg_i16"), info
    assert 0 < info["lds_bytes"] <= FL.WG_LDS_BOUND
    return info


def test_kernel_name(gpu_ctx_factory):
    """The option selects the kernel on every code, DVB-S2 included; LDS holds 256 bytes and the APPs."""
    for code in TF.CODES + (DVBS2,):
        ctx = wg_ctx(gpu_ctx_factory, code, 8)
        N = ctx.graph.N
        for mb, ab, size in ((2, 2, 1), (8, 8, 1), (4, 9, 2), (16, 16, 2)):
            info = info_of(ctx, native.FxlmsConfig(msg_bits=mb, app_bits=ab))
            assert info["lds_bytes"] == (256 + N * size + 15) // 16 * 16
        for v in ("auto", "lds", "flood"):   # every other value leaves the choice as it was
            ctx.set_option("kernel", v)
            if code == DVBS2:
                with pytest.raises(native.LdpcError) as e:
                    ctx.fxlms_kernel_info(native.FxlmsConfig())
                assert e.value.code == -4 and "65536" in str(e.value) and "LDPC_OPT_KERNEL = 3" in str(e.value)
            else:
                assert ctx.fxlms_kernel_info(native.FxlmsConfig(msg_bits=8, app_bits=8))["kernel"] == "fxlms_i8"
        ctx.set_option("kernel", "global")
    with pytest.raises(native.LdpcError) as e:   # the cfg is still checked first
        ctx.fxlms_kernel_info(native.FxlmsConfig(variant=native.BP))
    assert e.value.code == -4


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("code,case", MATRIX, ids=["%s-%s" % (c.split(".")[0][:8], k) for c, k in MATRIX])
def test_exact_against_the_restatement(gpu_ctx_factory, code, case, prec):
    """T = 0, 1, 2 and 8 without early stop, and T = 8 and 0 with it: decisions, frame records, counters,
    on sixteen frames of rising noise."""
    ctx = wg_ctx(gpu_ctx_factory, code)
    kw = TF.case_kw(case)
    y = TF.given(code).astype(PREC[prec][1])
    info_of(ctx, TF.cfg_of(kw, prec, TMAX))
    for T, es in ((0, False), (1, False), (2, False), (TMAX, False), (TMAX, True), (0, True)):
        want = restate(code, kw, prec, T, y, es, tmax=TMAX)
        TF.assert_equal(ctx.fxlms_decode(y, TF.cfg_of(kw, prec, T, es)), want, T, es, (code, case, prec, T, es))
    full, es = restate(code, kw, prec, TMAX, y), restate(code, kw, prec, TMAX, y, True)
    assert full["frames"]["bit_err"].any()   # the noisiest frames fail everywhere
    if (code, case) in TF.UNDECODED:
        assert (es["s"] == TMAX).all()
    else:   # frames that stop at a codeword, unevenly, and frames that do not
        assert ((es["s"] > 0) & (es["s"] < TMAX)).any() and (es["s"] == TMAX).any()
    if code == C802:
        assert ctx.graph.maxdc == 32   # two sign words a row


def both_kernels(ctx, run):
    """run() with the option at 0 and at 3, on the same context."""
    ctx.set_option("kernel", "auto")
    a = run()
    ctx.set_option("kernel", "global")
    return a, run()


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_byte_equal_to_the_default_kernel(gpu_ctx_factory, prec):
    """Non-zero codewords in batches of 1 and 7 through fxlms_decode, and fxlms_sim_trace with the
    codeword table: samples, codes, decisions, frame records and counters of the two kernels."""
    ctx = wg_ctx(gpu_ctx_factory, PEG)
    bits = codes.read_codeword_file(code_path("PEGReg504x1008_data20.enc"), ctx.graph.N)
    assert bits.any()
    kw = TF.case_kw("nms34_8_8")
    cfg = TF.cfg_of(kw, prec, TMAX, True)
    info_of(ctx, cfg)
    c = (1 - 2 * bits[np.arange(8) % len(bits)].astype(np.int8)).astype(np.int8)
    y = (c * TF.given(PEG, 8, 13)).astype(PREC[prec][1])
    for lo, n in ((0, 1), (1, 7)):
        (d0, f0, c0), (d1, f1, c1) = both_kernels(ctx, lambda: ctx.fxlms_decode(y[lo:lo + n], cfg, c=c[lo:lo + n]))
        assert np.array_equal(d0, d1) and np.array_equal(f0, f1) and np.array_equal(c0.as_array(), c1.as_array())
        assert c1.frames == n and f1["uncoded_bit_err"].min() > 0
        TF.assert_equal((d1, f1, c1), restate(PEG, kw, prec, TMAX, y[lo:lo + n], True, c[lo:lo + n]), TMAX, True)
    ctx.set_codewords(bits)
    try:
        a, b = both_kernels(ctx, lambda: ctx.fxlms_sim_trace(1.8, 0.5, cfg, seed=7, stream_id=2, first_cw=33, batch=7))
    finally:
        ctx.set_codewords(None)
    assert all(np.array_equal(p, q) for p, q in zip(a[:4], b[:4])) and np.array_equal(a[4].as_array(), b[4].as_array())
    assert b[4].frames == 7 and (np.sign(b[0]) != 1).mean() > 0.3   # non-zero codewords were sent


def test_large_batches_equal_the_default_kernel(gpu_ctx_factory):
    """1,300 PEG frames at T = 2 in one launch, and 16,384, which is more than a grid of one-wave
    workgroups holds (at most 32 a CU), so that codewords go out by ticket: samples, codes, decisions
    (the 1,300), frame records, counters and histogram of the two kernels."""
    ctx = wg_ctx(gpu_ctx_factory, PEG, 16384)
    cfg = TF.cfg_of(TF.case_kw("nms34_8_8"), "f32", 2, True)
    info_of(ctx, cfg)
    a, b = both_kernels(ctx, lambda: ctx.fxlms_sim_trace(2.4, 0.5, cfg, seed=5, stream_id=3, first_cw=1000, batch=1300))
    assert all(np.array_equal(p, q) for p, q in zip(a[:4], b[:4])) and np.array_equal(a[4].as_array(), b[4].as_array())
    assert b[4].frames == 1300 and (b[3]["bit_err"] < b[3]["uncoded_bit_err"]).any() and b[3]["syndrome_fail"].any()

    def big():
        ctx.read_histogram(reset=True)
        fr, cnt = ctx.fxlms_sim_batch(2.4, 0.5, cfg, seed=5, stream_id=3, first_cw=1000, batch=16384)
        return fr, cnt, ctx.read_histogram(reset=True)
    (f0, c0, h0), (f1, c1, h1) = both_kernels(ctx, big)
    assert np.array_equal(f0, f1) and np.array_equal(c0.as_array(), c1.as_array()) and np.array_equal(h0, h1)
    assert np.array_equal(f1[:1300], b[3]) and c1.frames == 16384 and c1.iters == int(f1["iters"].sum())
    assert np.array_equal(h1, np.bincount(f1["bit_err"], minlength=ctx.graph.N + 1)[1:])


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    """PEG with checks of degree 0, 1 and 2 and a bit of degree 0; a code with layers of 40, 200 and 40 rows."""
    root = tmp_path_factory.mktemp("fxlms_wg_codes")
    return {"edge": FL.write_edge_code(str(root / "peg_edge.alist"), code_path(PEG)),
            "uneven": TF.write_uneven_code(str(root / "uneven.alist"))}


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("case", ["ms_6_7", "nms34_8_8", "ms_16_16"])
def test_checks_of_degree_0_1_2_and_a_bit_of_degree_0(gpu_ctx_factory, generated, case, prec):
    ctx = wg_ctx(gpu_ctx_factory, generated["edge"], 64)
    assert (ctx.graph.N, ctx.graph.M, ctx.graph.E) == (1009, 507, 3027)
    kw = TF.case_kw(case)
    info_of(ctx, TF.cfg_of(kw, prec, TMAX))
    y = TF.noisy(ctx.graph.N, 13, 0.6, 0.9, 32).astype(PREC[prec][1])
    for T, es in ((0, False), (1, False), (TMAX, False), (TMAX, True)):
        want = restate(generated["edge"], kw, prec, T, y, es, tmax=TMAX)
        TF.assert_equal(ctx.fxlms_decode(y, TF.cfg_of(kw, prec, T, es)), want, T, es, (case, prec, T, es))
    assert np.array_equal(want["d"][:, 1008], np.where(y[:, 1008] >= 0, 1, -1))   # the bit without checks
    assert (want["d"][:, 1008] == -1).any() and want["frames"]["syndrome_fail"].any()


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_short_layer_before_a_long_one(gpu_ctx_factory, generated, prec):
    """Layers of 40, 200 and 40 rows under a workgroup of 64 threads: idle threads in a layer, then
    four passes, the last of them partial."""
    ctx = wg_ctx(gpu_ctx_factory, generated["uneven"], 64)
    sizes = np.diff(ctx.graph.layers()[1]).tolist()
    assert any(a < 64 and b > 128 for a, b in zip(sizes, sizes[1:])), sizes
    y = TF.noisy(ctx.graph.N, 9, 0.7, 1.1, 33).astype(PREC[prec][1])
    for case in ("nms34_6_7", "ms_12_13"):
        kw = TF.case_kw(case)
        info_of(ctx, TF.cfg_of(kw, prec, TMAX))
        for T, es in ((1, False), (TMAX, False), (TMAX, True)):
            want = restate(generated["uneven"], kw, prec, T, y, es, tmax=TMAX)
            TF.assert_equal(ctx.fxlms_decode(y, TF.cfg_of(kw, prec, T, es)), want, T, es, (case, prec, T, es))


# ---- DVB-S2 N=64800: refused without the option, decoded with it ----
@functools.lru_cache(maxsize=None)
def dvbs2_samples():
    y = TF.noisy(64800, 4, 0.55, 1.0, 41)
    y.setflags(write=False)
    return y


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("case", ["nms34_8_8", "nms34_8_9"])
def test_dvbs2(gpu_ctx_factory, case, prec):
    """Four frames, sigma 0.55 to 1.0, at one-byte and at two-byte APPs: T = 0, 1, 3 and T <= 8 with early
    stop. The premise comes from the restatement in the library's order: some frame stops before T and
    some frame fails. Workgroups of 512 and 1,024 threads over layers of 275 to 3,044 rows."""
    ctx = wg_ctx(gpu_ctx_factory, DVBS2, 8)
    sizes = np.diff(ctx.graph.layers()[1])
    assert (ctx.graph.N, ctx.graph.M, len(sizes), sizes.min(), sizes.max()) == (64800, 32400, 17, 275, 3044)
    kw = TF.case_kw(NMS_8_9 if case == "nms34_8_9" else case)
    info = info_of(ctx, TF.cfg_of(kw, prec, TMAX))
    assert info["lds_bytes"] == 256 + 64800 * (2 if kw["app_bits"] > 8 else 1)
    y = dvbs2_samples().astype(PREC[prec][1])
    es = restate(DVBS2, kw, prec, TMAX, y, True)
    print(case, prec, "stop iterations", es["s"].tolist(), "failing", es["frames"]["syndrome_fail"].tolist())
    assert ((es["s"] > 0) & (es["s"] < TMAX)).any() and es["frames"]["syndrome_fail"].any()   # the premise
    for T, stop in ((0, False), (1, False), (3, False), (TMAX, True)):
        want = restate(DVBS2, kw, prec, T, y, stop, tmax=TMAX)
        TF.assert_equal(ctx.fxlms_decode(y, TF.cfg_of(kw, prec, T, stop)), want, T, stop, (case, prec, T, stop))


def test_dvbs2_sim_trace_and_tickets(gpu_ctx_factory):
    """fxlms_sim_trace with batch 2 through the on-device channel against the restatement on the traced
    samples; and 1,100 frames at T = 1 in one launch -- more than the 512 workgroups a grid has at most,
    so the rest go out by ticket -- against the same frames in launches of 275."""
    ctx = wg_ctx(gpu_ctx_factory, DVBS2, 2048)
    kw = TF.case_kw("nms34_8_8")
    cfg = TF.cfg_of(kw, "f32", TMAX, True)
    info_of(ctx, cfg)
    y, ycode, d, fr, cnt = ctx.fxlms_sim_trace(1.3, 0.5, cfg, seed=21, stream_id=4, first_cw=7, batch=2)
    assert np.array_equal(ycode, FL.front(y, kw["ymax"], kw["qbits"], np.float32))
    TF.assert_equal((d, fr, cnt), restate(DVBS2, kw, "f32", TMAX, y, True), TMAX, True)
    for ab in (8, 9):
        one = TF.cfg_of(dict(kw, app_bits=ab), "f32", 1, True)
        info_of(ctx, one)
        fr, cnt = ctx.fxlms_sim_batch(1.3, 0.5, one, seed=5, stream_id=3, first_cw=100, batch=1100)
        parts, tot = [], np.zeros(6, dtype=np.int64)
        for lo in range(0, 1100, 275):
            f, c = ctx.fxlms_sim_batch(1.3, 0.5, one, seed=5, stream_id=3, first_cw=100 + lo, batch=275)
            parts.append(f)
            tot += c.as_array()
        parts = np.concatenate(parts)
        assert all(np.array_equal(fr[k], parts[k]) for k in FIELDS) and np.array_equal(cnt.as_array(), tot)
        assert cnt.frames == 1100 and fr["uncoded_bit_err"].min() > 0 and len(set(fr["bit_err"].tolist())) > 100
