"""The DD-BMP decoder (variant DDBMP; ddbmp.hip) on the GPU against its numpy restatement
(tests/ddbmp_oracle.py, itself pinned to the reference by tests/test_ddbmp_oracle.py) and,
through the golden runs of tests/golden/reference_runs_ddbmp.json, against the reference.

Every test runs with the option ddbmp_kernel at its default (ddbmp_rows where the code
fits) and at 1 (the generic kernels) and asserts that kernel_info names the kernel meant.
Equality is exact everywhere: decisions, per-frame bit errors, uncoded errors, syndrome
flags and iteration counts, in fp64 and in fp32 (each against the restatement in the same
arithmetic)."""
import functools
import math
import os

import numpy as np
import pytest

import ddbmp_oracle as D
from conftest import code_path
from ldpcsimulation_amd import codes, native

pytestmark = pytest.mark.gpu

PEG, W1944, R4000, DVBS2 = "PEGReg504x1008.alist", "80211n_1944_r12.alist", "4000.2000.4.244.alist", "dvbs2_1_2.alist"
FRONT = dict(quantize=True, ymax=1.0, qbits=3)
PREC = {"f64": (native.F64, np.float64), "f32": (native.F32, np.float32)}
KERNELS = ("rows", "generic")
# the pool of frames per code (larger than the persistent grid of ddbmp_rows, so the tail
# of it is handed out by ticket) and an Eb/N0 at which some frames stop early and some never
POOL = {PEG: (1100, 4.0), W1944: (300, 5.0), R4000: (300, 4.0)}
# generic kernel per (code, precision): 4000.2000 in fp64 is past 160 KB of LDS
GENERIC = {(PEG, "f64"): "ddbmp_lds", (PEG, "f32"): "ddbmp_lds", (W1944, "f64"): "ddbmp_lds",
           (W1944, "f32"): "ddbmp_lds", (R4000, "f64"): "ddbmp_global", (R4000, "f32"): "ddbmp_lds",
           (DVBS2, "f64"): "ddbmp_global", (DVBS2, "f32"): "ddbmp_global"}
RUNS, POOLED = D.golden_runs()


@functools.lru_cache(maxsize=None)
def oracle(code):
    return D.Ddbmp(code_path(code))


@functools.lru_cache(maxsize=None)
def pool(code):
    n, snr = POOL[code]
    sigma = math.sqrt(10.0 ** (-snr / 10.0) / 0.5 / 2.0)
    y = 1.0 + sigma * np.random.default_rng(len(code)).standard_normal((n, oracle(code).N))
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def pool_reference(code, prec, T):
    d, fr = oracle(code).decode(pool(code), T, dtype=PREC[prec][1], **FRONT)
    return d, fr


def cfg_of(prec, T, **kw):
    front = dict(FRONT)
    front.update(kw)
    return native.DecoderConfig(variant=native.DDBMP, T=T, precision=PREC[prec][0], **front)


def pick(ctx, kernel, code, prec, cfg):
    """Set the kernel option and check that the plan names the kernel meant."""
    ctx.set_option("ddbmp_kernel", kernel)
    want = "ddbmp_rows" if kernel == "rows" and code != DVBS2 else GENERIC[(code, prec)]
    info = ctx.kernel_info(cfg)
    assert info["kernel"] == want, info
    return info


def same(fr, ref, n=None):
    for k in ("bit_err", "uncoded_bit_err", "syndrome_fail", "iters"):
        assert np.array_equal(np.asarray(fr[k], dtype=np.int64), ref[k][:n]), k


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("code", [PEG, W1944, R4000])
def test_decode_batch_equals_restatement(gpu_ctx_factory, code, prec, kernel):
    """Batches 1, 3 and one past the persistent grid, T in {0, 1, 2, 30}, c = NULL."""
    import torch
    ctx = gpu_ctx_factory(code)
    y = pool(code).astype(PREC[prec][1])
    for T in (0, 1, 2, 30):
        cfg = cfg_of(prec, T)
        info = pick(ctx, kernel, code, prec, cfg)
        rd, rfr = pool_reference(code, prec, T)
        if T == 30:   # the pool mixes early stops with frames that never stop
            assert rfr["iters"].min() < 15 and (rfr["iters"] == T).any() and (rfr["iters"] < T).sum() > len(y) // 4
        if kernel == "rows":   # the tail of the pool goes through the ticket
            assert len(y) > info["blocks_per_cu"] * torch.cuda.get_device_properties(0).multi_processor_count
        for n in (1, 3, len(y)):
            d, fr, cnt = ctx.decode(np.ascontiguousarray(y[:n]), cfg)
            assert np.array_equal(d, rd[:n]), (T, n)
            same(fr, rfr, n)
            c = cnt.as_dict()
            assert c["frames"] == n and c["iters"] == int(rfr["iters"][:n].sum())
            assert c["bit_err"] == int(rfr["bit_err"][:n].sum()) and c["frame_err"] == int((rfr["bit_err"][:n] > 0).sum())
            assert c["syndrome_fail"] == int(rfr["syndrome_fail"][:n].sum())


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("code", [PEG, W1944, R4000])
def test_decode_batch_with_codewords_given(gpu_ctx_factory, code, prec, kernel):
    """c given: transmitted codewords of the code's file where it has one, else random signs
    (the accounting compares d with whatever c is)."""
    ctx = gpu_ctx_factory(code)
    N = oracle(code).N
    rng = np.random.default_rng(7)
    enc = {PEG: "PEGReg504x1008_data20.enc", R4000: "4000.2000.4.244_data10.enc"}.get(code)
    if enc:
        c = (1 - 2 * codes.read_codeword_file(code_path(enc), N)[:5].astype(np.int8)).astype(np.int8)
    else:
        c = rng.choice(np.array([-1, 1], dtype=np.int8), size=(5, N))
    sigma = math.sqrt(10.0 ** (-POOL[code][1] / 10.0) / 0.5 / 2.0)
    y = (c * (1.0 + sigma * rng.standard_normal((5, N)))).astype(PREC[prec][1])
    for T in (0, 1, 2, 30):
        cfg = cfg_of(prec, T)
        pick(ctx, kernel, code, prec, cfg)
        rd, rfr = oracle(code).decode(y, T, c=c, dtype=PREC[prec][1], **FRONT)
        d, fr, _ = ctx.decode(y, cfg, c=c)
        assert np.array_equal(d, rd), T
        same(fr, rfr)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("code", [PEG, W1944])
def test_exact_arithmetic_inputs(gpu_ctx_factory, code, kernel):
    """No quantiser, y from {+-0, +-0.5, +-1, +-2}: every memory is a small multiple of 0.5,
    exact in both precisions, and zeros and ties are frequent -- a sign-bit sgn() or a
    padding edge that adds +-0 to `sum - c2s` shows here. fp32 = fp64 = restatement."""
    ctx = gpu_ctx_factory(code)
    N = oracle(code).N
    rng = np.random.default_rng(11)
    n = 96   # magnitudes from {0, 0.5, 1, 2}; frame f flips a share f/n * 8 % of the signs, zeros half of them
    mag = rng.choice(np.array([0.0, 0.5, 1.0, 2.0]), size=(n, N), p=[0.04, 0.3, 0.46, 0.2])
    neg = np.where(mag == 0, rng.random((n, N)) < 0.5, rng.random((n, N)) < np.linspace(0.0, 0.08, n)[:, None])
    y = np.where(neg, -mag, mag)
    assert np.signbit(y[y == 0]).any() and not np.signbit(y[y == 0]).all()
    T = 12
    rd, rfr = oracle(code).decode(y, T)
    assert (rfr["iters"] < T).any() and (rfr["iters"] == T).any()
    for prec in ("f64", "f32"):
        cfg = cfg_of(prec, T, quantize=False, ymax=0.0, qbits=0)
        pick(ctx, kernel, code, prec, cfg)
        d, fr, _ = ctx.decode(y.astype(PREC[prec][1]), cfg)
        assert np.array_equal(d, rd), prec
        same(fr, rfr)
    rd32, rfr32 = oracle(code).decode(y, T, dtype=np.float32)
    assert np.array_equal(rd32, rd) and np.array_equal(rfr32["iters"], rfr["iters"])


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_dvbs2_global_kernel(gpu_ctx_factory, prec):
    ctx = gpu_ctx_factory(DVBS2, 64)
    o = oracle(DVBS2)
    sigma = math.sqrt(10.0 ** (-3.0 / 10.0) / 0.5 / 2.0)
    y = (1.0 + sigma * np.random.default_rng(3).standard_normal((3, o.N))).astype(PREC[prec][1])
    cfg = cfg_of(prec, 5)
    for kernel in KERNELS:
        pick(ctx, kernel, DVBS2, prec, cfg)
        rd, rfr = o.decode(y, 5, dtype=PREC[prec][1], **FRONT)
        d, fr, _ = ctx.decode(y, cfg)
        assert np.array_equal(d, rd)
        same(fr, rfr)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("run", RUNS, ids=[r["name"] for r in RUNS])
def test_golden_replay_through_the_abi(gpu_ctx_factory, run, kernel):
    """glibc noise on the host, fp64 decode on the GPU in batches, the stop rule in frame
    order: the reference's totals and its sequence of frame error weights."""
    import re
    R, snr, T, front = D.run_config(run)
    ctx = gpu_ctx_factory(run["code"])
    cfg = native.DecoderConfig(variant=native.DDBMP, T=T, precision=native.F64, **front)
    pick(ctx, kernel, run["code"], "f64", cfg)

    def decode(y, c):
        _, fr, _ = ctx.decode(y, cfg, c=c, want_decisions=False)
        return fr
    got = D.replay(run, decode, chunk=128)
    m = re.match(r"Final result: (\d+) bit errs in (\d+) words.*Average iterations = ([0-9.e+-]+)\. "
                 r"Uncoded errors = (\d+)", run["final"])
    assert (got["errors"], got["words"], got["uncoded"]) == (int(m.group(1)), int(m.group(2)), int(m.group(4)))
    assert got["ferr_weights"] == run["ferr_weights"]
    assert "%g" % (got["iters"] / got["words"]) == m.group(3)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("code", [PEG, W1944])
def test_sim_trace(gpu_ctx_factory, code, prec, kernel):
    """The samples the fused kernel generated, pushed through the restatement, give its
    decisions and per-frame results; and they are the min-sum path's samples for the same
    (seed, stream_id, first_cw)."""
    ctx = gpu_ctx_factory(code)
    cfg = cfg_of(prec, 30)
    pick(ctx, kernel, code, prec, cfg)
    snr = POOL[code][1]
    y, d, fr, cnt = ctx.sim_trace(snr, 0.5, cfg, seed=77, stream_id=3, first_cw=1000, batch=48)
    rd, rfr = oracle(code).decode(y, 30, dtype=PREC[prec][1], **FRONT)
    assert np.array_equal(d, rd)
    same(fr, rfr)
    assert cnt.as_dict()["iters"] == int(rfr["iters"].sum())
    ms = native.DecoderConfig(variant=native.MS, T=2, precision=PREC[prec][0], **FRONT)
    y_ms, _, _, _ = ctx.sim_trace(snr, 0.5, ms, seed=77, stream_id=3, first_cw=1000, batch=48)
    assert np.array_equal(y, y_ms)


@pytest.mark.parametrize("kernel", KERNELS)
def test_split_invariance(gpu_ctx_factory, kernel):
    ctx = gpu_ctx_factory(PEG)
    cfg = cfg_of("f64", 30)
    pick(ctx, kernel, PEG, "f64", cfg)
    B = 600
    ctx.read_histogram(reset=True)
    fr, cnt = ctx.sim_batch(4.0, 0.5, cfg, seed=5, stream_id=1, first_cw=0, batch=B)
    hist = ctx.read_histogram(reset=True)
    fa, ca = ctx.sim_batch(4.0, 0.5, cfg, seed=5, stream_id=1, first_cw=0, batch=B // 2)
    fb, cb = ctx.sim_batch(4.0, 0.5, cfg, seed=5, stream_id=1, first_cw=B // 2, batch=B // 2)
    hist2 = ctx.read_histogram(reset=True)
    assert np.array_equal(np.concatenate([fa, fb]), fr)
    assert np.array_equal(ca.as_array() + cb.as_array(), cnt.as_array())
    assert np.array_equal(hist, hist2) and hist.sum() == cnt.as_dict()["frame_err"] > 0


@pytest.mark.parametrize("kernel", KERNELS)
def test_codeword_table(gpu_ctx_factory, kernel):
    ctx = gpu_ctx_factory(PEG)
    bits = codes.read_codeword_file(code_path("PEGReg504x1008_data20.enc"), 1008)
    cfg = cfg_of("f64", 30)
    pick(ctx, kernel, PEG, "f64", cfg)
    ctx.set_codewords(bits)
    try:
        y, d, fr, _ = ctx.sim_trace(4.0, 0.5, cfg, seed=9, stream_id=2, first_cw=7, batch=50)
    finally:
        ctx.set_codewords(None)
    c = (1 - 2 * bits[(7 + np.arange(50)) % len(bits)].astype(np.int8)).astype(np.int8)
    assert (np.sign(y) == c).mean() > 0.9          # the table's rows were transmitted
    rd, rfr = oracle(PEG).decode(y, 30, c=c, **FRONT)
    assert np.array_equal(d, rd)
    same(fr, rfr)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_fer_against_the_reference(gpu_ctx_factory, prec, kernel):
    """Philox simulation at the pooled operating point (PEG, 4.0 dB, T 100, Ymax 1.0, Q 3):
    8192 frames against the reference's pooled frame errors, two-proportion z-test, |z| < 3
    (the bound the project uses for every FER comparison)."""
    R, snr, T, front = D.run_config(POOLED)
    ctx = gpu_ctx_factory(PEG, 8192)
    cfg = native.DecoderConfig(variant=native.DDBMP, T=T, precision=PREC[prec][0], **front)
    pick(ctx, kernel, PEG, prec, cfg)
    _, cnt = ctx.sim_batch(snr, R, cfg, seed=2024, stream_id=0, first_cw=0, batch=8192, want_frames=False)
    n1, e1 = 8192, cnt.as_dict()["frame_err"]
    n2, e2 = POOLED["frames"], POOLED["frame_errors"]
    p = (e1 + e2) / (n1 + n2)
    z = (e1 / n1 - e2 / n2) / math.sqrt(p * (1 - p) * (1 / n1 + 1 / n2))
    print(f"FER gpu {e1}/{n1} reference {e2}/{n2} z = {z:.2f}")
    assert abs(z) < 3, (e1, n1, e2, n2, z)
    assert cnt.as_dict()["iters"] < T * n1


def test_refusals_and_accepted_variants(gpu_ctx_factory):
    ctx = gpu_ctx_factory(PEG)
    y = np.ones((1, 1008))
    d, fr, _ = ctx.decode(y, cfg_of("f64", 3))            # variant 4 is accepted
    assert (d == 1).all() and fr["iters"][0] == 0
    with pytest.raises(native.LdpcError) as e:
        ctx.decode(y, native.DecoderConfig(variant=5, T=3))
    assert e.value.code == -1
    with pytest.raises(native.LdpcError) as e:
        ctx.decode(y, native.DecoderConfig(variant=native.DDBMP, T=3, schedule=native.LAYERED))
    assert e.value.code == -4
    with pytest.raises(native.LdpcError) as e:
        ctx.row_sched_info(cfg_of("f64", 3))
    assert e.value.code == -4
    with pytest.raises(native.LdpcError):
        ctx.set_option("ddbmp_kernel", 2)
    assert native.OPTIONS["ddbmp_kernel"] == 22 and native.DDBMP == 4
