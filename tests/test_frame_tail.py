"""The partial last Philox group: codes whose N is not a multiple of 4.

Every binary code fixture has N divisible by 4, so nothing else reaches the last group of
four channel samples when it is cut short: the v < N guards, the filler sample, the bound of
the y_out write and of the codeword row (frame.h channel_group; the row kernels' own
channel steps). Three tiny codes, N = 125, 126, 127 (one, two, three bits in the last
group), M = 63, column degree 3 and row degree <= 8, so the BP, GDBF and DD-BMP rows
kernels take them as well as the generic ones. Everything is exact: bytes of y, decisions,
per-frame results, counters."""
import functools

import numpy as np
import pytest

from ldpcsimulation_amd import codes, native

pytestmark = pytest.mark.gpu

M, BATCH, T = 63, 5, 5
SEED, STREAM, FIRST_CW = 0x5EEDF00D5, 0x5A5A5, 3   # stream_id < 2^20 (GDBF keeps the iteration above it)
EBN0, RATE = 0.0, 0.8                               # N0 = 1 / 0.8 on both sides of the ABI, sigma = 0.79
PREC = {"f64": (native.F64, np.float64), "f32": (native.F32, np.float32)}
DDBMP_FRONT = dict(quantize=True, ymax=1.0, qbits=3)

# name -> (config fields, options, the kernel(s) kernel_info must name)
CHOICES = {
    "ms_auto": (dict(), dict(), None),   # whichever kernel the plan prefers
    "ms_lds": (dict(), dict(kernel=1), ("lds",)),
    "ms_flood": (dict(), dict(kernel=2), ("flood",)),
    "ms_flood_persistent": (dict(), dict(kernel=2, flood_mode="persistent"), ("flood",)),
    "ms_global": (dict(), dict(kernel=3), ("global",)),
    "layered": (dict(schedule=native.LAYERED), dict(), ("layered_lds",)),
    "layered_global": (dict(schedule=native.LAYERED), dict(kernel=3), ("layered_global",)),
    "bp_rows": (dict(variant=native.BP, n0=1.0 / RATE), dict(bp_kernel=0), ("bp_rows",)),
    "bp_generic": (dict(variant=native.BP, n0=1.0 / RATE), dict(bp_kernel=1), ("bp_lds",)),
    "ddbmp_rows": (dict(variant=native.DDBMP, **DDBMP_FRONT), dict(ddbmp_kernel=0), ("ddbmp_rows",)),
    "ddbmp_generic": (dict(variant=native.DDBMP, **DDBMP_FRONT), dict(ddbmp_kernel=1), ("ddbmp_lds",)),
}
CASES = [(N, prec) for N in (125, 126, 127) for prec in ("f64", "f32")]


def _code(path, N, seed):
    """Column degree 3; each bit takes the three least loaded rows (ties at random), so the
    row degrees are 5..7 and no row repeats within a bit."""
    rng = np.random.default_rng(seed)
    load = np.zeros(M, dtype=np.int64)
    rows = [[] for _ in range(M)]
    for i in range(N):
        for j in np.lexsort((rng.random(M), load))[:3]:
            rows[j].append(i)
            load[j] += 1
    assert load.max() <= 8
    codes.write_alist(codes.ParityCheck.from_rows(N, rows), path)
    return path


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """(N, prec) -> the table's bipolar rows per frame, and per kernel choice the sim_trace
    result and the decode_batch result of its y: computed once, read by every test."""
    assert native.device_count() > 0, "no HIP device visible"
    root = tmp_path_factory.mktemp("tail")

    @functools.lru_cache(maxsize=None)
    def ctx_of(N):
        ctx = native.Context(native.Graph.from_alist(_code(str(root / f"n{N}.alist"), N, seed=N)), 0, 64)
        bits = np.random.default_rng(N + 1).integers(0, 2, size=(2, N), dtype=np.uint8)
        ctx.set_codewords(bits)
        return ctx, bits

    @functools.lru_cache(maxsize=None)
    def run(N, prec):
        ctx, bits = ctx_of(N)
        c = (1 - 2 * bits[(FIRST_CW + np.arange(BATCH)) % 2].astype(np.int8)).astype(np.int8)
        out = {"c": c, "ctx": ctx}
        for name, (fields, opts, kernels) in CHOICES.items():
            ctx.reset_options()
            ctx.set_options(opts)
            cfg = native.DecoderConfig(T=T, precision=PREC[prec][0], **fields)
            assert kernels is None or ctx.kernel_info(cfg)["kernel"] in kernels, (name, ctx.kernel_info(cfg))
            y, d, fr, cnt = ctx.sim_trace(EBN0, RATE, cfg, SEED, STREAM, FIRST_CW, BATCH)
            gd, gfr, gcnt = ctx.decode(y, cfg, c=c)
            out[name] = dict(y=y, d=d, fr=fr, cnt=cnt.as_array(), gd=gd, gfr=gfr, gcnt=gcnt.as_array())
        ctx.reset_options()
        return out

    return run


@pytest.mark.parametrize("N,prec", CASES)
def test_one_channel(runs, N, prec):
    r = runs(N, prec)
    ref = r["ms_lds"]["y"]
    assert ref.shape == (BATCH, N) and ref.dtype == PREC[prec][1] and np.isfinite(ref).all()
    for name in CHOICES:
        assert r[name]["y"].tobytes() == ref.tobytes(), name


@pytest.mark.parametrize("N,prec", CASES)
def test_given_equals_generated(runs, N, prec):
    r = runs(N, prec)
    for name in CHOICES:
        o = r[name]
        assert np.array_equal(o["gd"], o["d"]), name
        assert np.array_equal(o["gfr"], o["fr"]), name
        assert np.array_equal(o["gcnt"], o["cnt"]), name
        assert o["cnt"][3] == BATCH and o["cnt"][0] == int(o["fr"]["bit_err"].sum()), name
        assert np.array_equal(o["fr"]["bit_err"], (o["d"] != r["c"]).sum(axis=1)), name


@pytest.mark.parametrize("N,prec", CASES)
def test_uncoded_errors(runs, N, prec):
    r = runs(N, prec)
    want = (np.where(r["ms_lds"]["y"] > 0, 1, -1) != r["c"]).sum(axis=1)   # over exactly N bits
    assert want.sum() > 0
    for name in CHOICES:
        assert np.array_equal(r[name]["fr"]["uncoded_bit_err"], want), name
        assert r[name]["cnt"][2] == int(want.sum()), name


@pytest.mark.parametrize("N,prec", CASES)
def test_gdbf(runs, N, prec):
    """GdbfArgs has no y_out: plain GDBF frames are equal between the two kernels, and their
    uncoded column is the min-sum trace's for the same (seed, stream_id, first_cw)."""
    r = runs(N, prec)
    ctx = r["ctx"]
    cfg = native.GdbfConfig(flags=0, T=T, precision=PREC[prec][0])
    frames = {}
    for opt, kernel in ((0, "gdbf_rows"), (1, "gdbf_lds")):
        ctx.reset_options()
        ctx.set_option("gdbf_kernel", opt)
        assert ctx.gdbf_kernel_info(cfg)["kernel"] == kernel
        frames[kernel], cnt = ctx.gdbf_sim_batch(EBN0, RATE, cfg, SEED, STREAM, FIRST_CW, BATCH)
        assert cnt.frames == BATCH and cnt.uncoded_bit_err == int(frames[kernel]["uncoded_bit_err"].sum())
    ctx.reset_options()
    assert np.array_equal(frames["gdbf_rows"], frames["gdbf_lds"])
    assert np.array_equal(frames["gdbf_rows"]["uncoded_bit_err"], r["ms_lds"]["fr"]["uncoded_bit_err"])


# The re-decoding family on these codes. What the N % 4 == 0 fixtures never reach in its
# register-schedule kernels: a cut last Philox group, M = 63 < 512 (most lanes own no row and all
# of row slot 1 is padding), NT = 512 with DVM = 4, and the stop flag's parity across a restart
# with odd T. theta = -0.6, alpha = 0.96 (the golden runs' PEG settings), lambda 0.99, noise scale
# 0.75, Ymax 2.5; window 3 so that smoothing starts inside the T = 5 iterations. At 0 dB hardly a
# frame of these codes decodes in 5 iterations, so frames restart and attempts differ by their
# noise alone; both are asserted.
NGDBF = dict(T=T, theta=-0.6, lambda_=0.99, alpha=0.96, noise_scale=0.75, ymax=2.5, windowsize=3)
MAXPHASE, ATTEMPTS = 3, 3


@pytest.mark.parametrize("N,prec", CASES)
def test_rgdbf(runs, N, prec):
    """rgdbf_rows against rgdbf_lds: frame records and counters equal, with frames that run
    more than one phase; the uncoded column is the min-sum trace's."""
    r = runs(N, prec)
    ctx = r["ctx"]
    cfg = native.RgdbfConfig(maxphase=MAXPHASE, precision=PREC[prec][0], **NGDBF)
    frames, counts = {}, {}
    for opt, kernel in ((0, "rgdbf_rows"), (1, "rgdbf_lds")):
        ctx.reset_options()
        ctx.set_option("gdbf_kernel", opt)
        assert ctx.rgdbf_kernel_info(cfg)["kernel"] == kernel
        frames[kernel], cnt = ctx.rgdbf_sim_batch(EBN0, RATE, cfg, SEED, STREAM, FIRST_CW, BATCH)
        counts[kernel] = cnt.as_array()
        assert cnt.frames == BATCH and cnt.uncoded_bit_err == int(frames[kernel]["uncoded_bit_err"].sum())
    ctx.reset_options()
    assert (native.rgdbf_phases(frames["rgdbf_lds"]["iters"], T, MAXPHASE) > 1).any()
    assert np.array_equal(frames["rgdbf_rows"], frames["rgdbf_lds"])
    assert np.array_equal(counts["rgdbf_rows"], counts["rgdbf_lds"])
    assert np.array_equal(frames["rgdbf_rows"]["uncoded_bit_err"], r["ms_lds"]["fr"]["uncoded_bit_err"])


@pytest.mark.parametrize("N,prec", CASES)
def test_rstat(runs, N, prec):
    """rstat_rows against rstat_wg: attempt records, frame records and counters equal, with
    attempts of one frame that end differently; the uncoded column is the min-sum trace's."""
    r = runs(N, prec)
    ctx = r["ctx"]
    cfg = native.RstatConfig(attempts=ATTEMPTS, precision=PREC[prec][0], **NGDBF)
    att, frames, counts = {}, {}, {}
    for opt, kernel in ((0, "rstat_rows"), (1, "rstat_wg")):
        ctx.reset_options()
        ctx.set_option("gdbf_kernel", opt)
        assert ctx.rstat_kernel_info(cfg)["kernel"] == kernel
        att[kernel], frames[kernel], cnt, _ = ctx.rstat_sim(EBN0, RATE, cfg, SEED, STREAM, FIRST_CW, BATCH)
        counts[kernel] = cnt.as_array()
        assert att[kernel].shape == (BATCH, ATTEMPTS)
        assert cnt.frames == BATCH and cnt.uncoded_bit_err == int(frames[kernel]["uncoded_bit_err"].sum())
    ctx.reset_options()
    a = att["rstat_wg"]
    assert any(len({tuple(x) for x in a[b].tolist()}) > 1 for b in range(BATCH))
    assert np.array_equal(att["rstat_rows"], att["rstat_wg"])
    assert np.array_equal(frames["rstat_rows"], frames["rstat_wg"])
    assert np.array_equal(counts["rstat_rows"], counts["rstat_wg"])
    assert np.array_equal(frames["rstat_rows"]["uncoded_bit_err"], r["ms_lds"]["fr"]["uncoded_bit_err"])
