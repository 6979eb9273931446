"""The re-decoding NGDBF decoder (ldpc_rgdbf_*; rgdbf.hip) on the GPU against its numpy
restatement (tests/rgdbf_oracle.py, itself pinned to the reference's recorded runs and to the
GDBF oracle by tests/test_rgdbf_oracle.py), against the existing GDBF kernels where the two
decoders coincide, and against the reference's pooled frame error rate.

Option gdbf_kernel picks the kernel here as it does for ldpc_gdbf_*: 0 = rgdbf_rows where
the code fits, 1 = the generic kernels; every test asserts that kernel_info names the kernel
meant. Equality is exact everywhere, in fp64 and in fp32 (each against the restatement in
the same arithmetic)."""
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import rgdbf_oracle as RO
from conftest import ROOT, code_path
from ldpcsimulation_amd import codes, native, sim

pytestmark = pytest.mark.gpu

PEG, W1944, R4000 = "PEGReg504x1008.alist", "80211n_1944_r12.alist", "4000.2000.4.244.alist"
PREC = {"f64": (native.F64, np.float64), "f32": (native.F32, np.float32)}
KERNELS = ("rows", "generic")
FIVE = native.RGDBF_FLAGS
FLAG_SETS = {"five": FIVE, "adapt_noise": native.GDBF_ADAPT | native.GDBF_NOISE}
ALPHA = {PEG: 0.96, "deg1": 0.96, W1944: 1.5, R4000: 1.2, "heavy": 1.2}
# the kernel the rows option gives; codes beyond rgdbf_rows (N > 4096, column degree > 12) stay generic
ROWS = {PEG: "rgdbf_rows", "deg1": "rgdbf_rows", W1944: "rgdbf_rows", R4000: "rgdbf_rows", "heavy": "rgdbf_lds"}
GENERIC = {(R4000, "f64"): "rgdbf_global"}   # 4000.2000 in fp64 is past 64 KB of LDS; every other case rgdbf_lds
# the given-channel frames: 3.0 dB, T 20, maxphase 3, 6 frames of glibc draws from this seed.
# PEG / deg1: seed 3 gives phases [3, 3, 3, 1, 3, 2] in the restatement (fp64 and fp32): a
# frame that succeeds in phase 0, one in a later phase, and frames that exhaust all phases.
# On 1944 no frame of seeds 1..59 succeeds within 3 x 20 iterations at 3.0 dB, and none of
# 4000.2000 (seeds 1..5) or of the heavy-column code: all six frames exhaust the phases there;
# the early stops of those codes are covered by the Philox cross-checks below.
GIVEN = dict(snr=3.0, T=20, maxphase=3, frames=6, seed=3)


@functools.lru_cache(maxsize=None)
def fixtures():
    """The degree-1-check and heavy-column codes of tests/test_checked_build.py."""
    import tempfile
    from test_checked_build import _fixtures
    return _fixtures(tempfile.mkdtemp(prefix="rgdbf_fx_"))


def path_of(code):
    return fixtures()[code] if code in ("deg1", "heavy") else code_path(code)


@functools.lru_cache(maxsize=None)
def oracle(code):
    return RO.Rgdbf(path_of(code))


@functools.lru_cache(maxsize=None)
def given(code):
    y, pert = RO.glibc_frames(oracle(code), 0.5, GIVEN["snr"], 0.75, GIVEN["maxphase"] * GIVEN["T"], GIVEN["seed"],
                              GIVEN["frames"])
    y.setflags(write=False)
    pert.setflags(write=False)
    return y, pert


@functools.lru_cache(maxsize=None)
def given_reference(code, prec, flagset):
    y, pert = given(code)
    return oracle(code).decode(y, pert, T=GIVEN["T"], maxphase=GIVEN["maxphase"], flags=FLAG_SETS[flagset],
                               alpha=ALPHA[code], dtype=PREC[prec][1])


def cfg_of(prec, code=PEG, **kw):
    base = dict(flags=FIVE, T=100, maxphase=3, alpha=ALPHA[code], precision=PREC[prec][0])
    base.update(kw)
    return native.RgdbfConfig(**base)


def pick(ctx, kernel, code, prec, cfg):
    """Set the kernel option and check that kernel_info names the kernel meant."""
    ctx.set_option("gdbf_kernel", kernel)
    want = ROWS[code] if kernel == "rows" else GENERIC.get((code, prec), "rgdbf_lds")
    info = ctx.rgdbf_kernel_info(cfg)
    assert info["kernel"] == want, info
    return info


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("code", [PEG, W1944, R4000, "deg1", "heavy"])
def test_given_channel_equals_restatement(gpu_ctx_factory, code, prec, kernel):
    """Decisions, per-frame results, counters and the error-weight histogram, with the five
    flags of decodeRSMNGDBF and with ADAPT|NOISE alone (weight 1)."""
    ctx = gpu_ctx_factory(path_of(code))
    y, pert = given(code)
    T, maxphase = GIVEN["T"], GIVEN["maxphase"]
    for flagset, flags in FLAG_SETS.items():
        cfg = cfg_of(prec, code, flags=flags, T=T, maxphase=maxphase)
        pick(ctx, kernel, code, prec, cfg)
        rd, rfr = given_reference(code, prec, flagset)
        if code in (PEG, "deg1") and flagset == "five":   # phase 0, a later phase, all phases exhausted
            assert (rfr["phases"] == 1).any() and ((rfr["phases"] > 1) & (rfr["iters"] < maxphase * T)).any() \
                and (rfr["iters"] == maxphase * T).any(), rfr
        ctx.read_histogram(reset=True)
        d, fr, cnt = ctx.rgdbf_decode(y, pert, cfg)
        hist = ctx.read_histogram(reset=True)
        assert np.array_equal(fr["iters"], rfr["iters"]), (flagset, fr["iters"], rfr["iters"])
        assert np.array_equal(d, rd), flagset
        for k in ("bit_err", "uncoded_bit_err", "syndrome_fail"):
            assert np.array_equal(np.asarray(fr[k], dtype=np.int64), rfr[k]), (flagset, k)
        assert np.array_equal(native.rgdbf_phases(fr["iters"], T, maxphase), rfr["phases"])
        c = cnt.as_dict()
        assert c["frames"] == len(y) and c["iters"] == int(rfr["iters"].sum())
        assert c["bit_err"] == int(rfr["bit_err"].sum()) and c["frame_err"] == int((rfr["bit_err"] > 0).sum())
        assert c["uncoded_bit_err"] == int(rfr["uncoded_bit_err"].sum())
        assert c["syndrome_fail"] == int(rfr["syndrome_fail"].sum())
        w = rfr["bit_err"][rfr["bit_err"] > 0]
        assert np.array_equal(hist, np.bincount(w - 1, minlength=oracle(code).N))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_given_channel_with_codewords(gpu_ctx_factory, prec, kernel):
    """c given (rows of the code's codeword file): the front-end counts uncoded errors against
    it and the error weight compares d with it."""
    ctx = gpu_ctx_factory(PEG)
    o = oracle(PEG)
    y1, pert = given(PEG)
    c = (1 - 2 * codes.read_codeword_file(code_path("PEGReg504x1008_data20.enc"), o.N)[:len(y1)].astype(np.int8))
    c = c.astype(np.int8)
    y = c * y1                                   # the same noise on the transmitted codewords
    cfg = cfg_of(prec, T=GIVEN["T"], maxphase=GIVEN["maxphase"])
    pick(ctx, kernel, PEG, prec, cfg)
    rd, rfr = o.decode(y, pert, c=c, T=cfg.T, maxphase=cfg.maxphase, alpha=cfg.alpha, dtype=PREC[prec][1])
    d, fr, _ = ctx.rgdbf_decode(y, pert, cfg, c=c)
    assert np.array_equal(d, rd)
    for k in ("bit_err", "uncoded_bit_err", "syndrome_fail", "iters"):
        assert np.array_equal(np.asarray(fr[k], dtype=np.int64), rfr[k]), k


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_single_phase_without_weight_equals_gdbf(gpu_ctx_factory, prec, kernel):
    """(a) maxphase 1 without WEIGHT is the GDBF decoder: 2048 Philox frames on 1944 at 3.0 dB
    through ldpc_gdbf_sim_batch, and given frames through ldpc_gdbf_decode_batch."""
    ctx = gpu_ctx_factory(W1944)
    flags = FIVE & ~native.GDBF_WEIGHT
    T = 100
    rcfg = cfg_of(prec, W1944, flags=flags, T=T, maxphase=1)
    gcfg = native.GdbfConfig(flags=flags, T=T, theta=rcfg.theta, lambda_=rcfg.lambda_, alpha=rcfg.alpha,
                             noise_scale=rcfg.noise_scale, ymax=rcfg.ymax, windowsize=rcfg.windowsize,
                             precision=rcfg.precision)
    pick(ctx, kernel, W1944, prec, rcfg)
    assert ctx.gdbf_kernel_info(gcfg)["kernel"] == ("gdbf_rows" if kernel == "rows" else "gdbf_lds")
    ctx.read_histogram(reset=True)
    fa, ca = ctx.rgdbf_sim_batch(3.0, 0.5, rcfg, seed=21, stream_id=5, first_cw=300, batch=2048)
    ha = ctx.read_histogram(reset=True)
    fb, cb = ctx.gdbf_sim_batch(3.0, 0.5, gcfg, seed=21, stream_id=5, first_cw=300, batch=2048)
    hb = ctx.read_histogram(reset=True)
    assert np.array_equal(fa, fb) and ca.as_dict() == cb.as_dict() and np.array_equal(ha, hb)
    assert (fa["iters"] < T).any() and (fa["iters"] == T).any()
    y, pert = given(W1944)
    y, pert = y[:, :], pert[:, :20, :]
    rcfg.T = gcfg.T = 20
    da, fa, ca = ctx.rgdbf_decode(y, pert, rcfg)
    db, fb, cb = ctx.gdbf_decode(y, pert, gcfg)
    assert np.array_equal(da, db) and np.array_equal(fa, fb) and ca.as_dict() == cb.as_dict()


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_single_phase_on_a_regular_code_equals_gdbf(gpu_ctx_factory, prec, kernel):
    """(b) On PEG (dv = 3) with WEIGHT, maxphase 1 is the GDBF decoder with alpha' = alpha*ymax/3."""
    ctx = gpu_ctx_factory(PEG)
    T = 100
    rcfg = cfg_of(prec, PEG, T=T, maxphase=1)
    gcfg = native.GdbfConfig(flags=FIVE, T=T, theta=rcfg.theta, lambda_=rcfg.lambda_,
                             alpha=rcfg.alpha * rcfg.ymax / 3, noise_scale=rcfg.noise_scale, ymax=rcfg.ymax,
                             windowsize=rcfg.windowsize, precision=rcfg.precision)
    pick(ctx, kernel, PEG, prec, rcfg)
    fa, ca = ctx.rgdbf_sim_batch(3.5, 0.5, rcfg, seed=22, stream_id=1, first_cw=0, batch=2048)
    fb, cb = ctx.gdbf_sim_batch(3.5, 0.5, gcfg, seed=22, stream_id=1, first_cw=0, batch=2048)
    assert np.array_equal(fa, fb) and ca.as_dict() == cb.as_dict()
    assert 0 < ca.as_dict()["frame_err"] < 2048 and (fa["iters"] < T).any()


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_later_phases_touch_only_failed_frames(gpu_ctx_factory, prec, kernel):
    """(c) A frame satisfied in phase 0 is the same frame at maxphase 1 and at maxphase 4;
    every other frame ran at least the T iterations of its failed phase 0."""
    ctx = gpu_ctx_factory(PEG)
    T = 50
    c1, c4 = cfg_of(prec, PEG, T=T, maxphase=1), cfg_of(prec, PEG, T=T, maxphase=4)
    pick(ctx, kernel, PEG, prec, c4)
    f1, n1 = ctx.rgdbf_sim_batch(3.5, 0.5, c1, seed=23, stream_id=2, first_cw=0, batch=2048)
    f4, n4 = ctx.rgdbf_sim_batch(3.5, 0.5, c4, seed=23, stream_id=2, first_cw=0, batch=2048)
    done = f1["iters"] < T
    assert 100 < done.sum() < 2048
    assert np.array_equal(f1[done], f4[done])
    assert (f4["iters"][~done] >= T).all() and (f4["iters"] <= 4 * T).all()
    assert np.array_equal(f1["uncoded_bit_err"], f4["uncoded_bit_err"])
    assert n1.as_dict()["frame_err"] > 0 and n4.as_dict()["frame_err"] > 0
    assert n4.as_dict()["frame_err"] < n1.as_dict()["frame_err"]      # re-decoding is what it is for
    ph = native.rgdbf_phases(f4["iters"], T, 4)
    assert set(np.unique(ph)) == {1, 2, 3, 4}


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("code,snrs", [(W1944, (3.0, 4.0)), (PEG, (3.0, 3.5)), (R4000, (3.0, 3.6))])
def test_rows_and_generic_kernels_agree(gpu_ctx_factory, code, snrs, prec):
    """2048 Philox frames at two SNRs: per-frame results, counters and histogram."""
    ctx = gpu_ctx_factory(code)
    cfg = cfg_of(prec, code, T=40, maxphase=3)
    out = {}
    for kernel in KERNELS:
        pick(ctx, kernel, code, prec, cfg)
        for snr in snrs:
            ctx.read_histogram(reset=True)
            fr, cnt = ctx.rgdbf_sim_batch(snr, 0.5, cfg, seed=31, stream_id=7, first_cw=10, batch=2048)
            out[(kernel, snr)] = (fr, cnt.as_dict(), ctx.read_histogram(reset=True))
    for snr in snrs:
        a, b = out[("rows", snr)], out[("generic", snr)]
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2]), snr
    assert out[("rows", snrs[0])][1] != out[("rows", snrs[1])][1]
    if code != R4000:
        assert (out[("rows", snrs[1])][0]["iters"] < 40).any()       # early stops at the higher SNR


@pytest.mark.parametrize("kernel", KERNELS)
def test_split_invariance(gpu_ctx_factory, kernel):
    """Results do not depend on how the frames are split over calls (first_cw / batch)."""
    ctx = gpu_ctx_factory(PEG)
    cfg = cfg_of("f64", PEG, T=40, maxphase=3)
    pick(ctx, kernel, PEG, "f64", cfg)
    B = 900
    ctx.read_histogram(reset=True)
    fr, cnt = ctx.rgdbf_sim_batch(3.25, 0.5, cfg, seed=5, stream_id=1, first_cw=40, batch=B)
    hist = ctx.read_histogram(reset=True)
    parts, acc = [], np.zeros(6, dtype=np.int64)
    for first, n in ((0, 1), (1, 299), (300, 600)):
        f, c = ctx.rgdbf_sim_batch(3.25, 0.5, cfg, seed=5, stream_id=1, first_cw=40 + first, batch=n)
        parts.append(f)
        acc += c.as_array()
    hist2 = ctx.read_histogram(reset=True)
    assert np.array_equal(np.concatenate(parts), fr)
    assert np.array_equal(acc, cnt.as_array())
    assert np.array_equal(hist, hist2) and hist.sum() == cnt.as_dict()["frame_err"] > 0


def test_sim_launch_into_a_device_buffer(gpu_ctx_factory):
    import torch
    ctx = gpu_ctx_factory(PEG)
    cfg = cfg_of("f64", PEG, T=40, maxphase=2)
    fr, _ = ctx.rgdbf_sim_batch(3.5, 0.5, cfg, seed=6, stream_id=0, first_cw=0, batch=256)
    dev = torch.empty((256, 4), dtype=torch.int32, device="cuda:0")
    ctx.rgdbf_sim_launch(3.5, 0.5, cfg, 6, 0, 0, 256, dev)
    ctx.synchronize()
    assert np.array_equal(dev.cpu().numpy().view(native.FRAME_DTYPE).reshape(-1), fr)
    with pytest.raises(native.LdpcError) as e:
        ctx.rgdbf_sim_launch(3.5, 0.5, cfg, 6, 1 << 20, 0, 256, dev)
    assert e.value.code == -1


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_fer_against_the_reference(gpu_ctx_factory, prec):
    """Philox simulation at the pooled operating point (PEG, 3.5 dB, T 100, maxphase 3):
    8192 frames against the reference's pooled frame errors, two-proportion z-test, |z| < 3."""
    runs, pooled = RO.golden_runs()
    R, snr, kw, ns = RO.run_config(pooled)
    ctx = gpu_ctx_factory(PEG, 8192)
    cfg = native.RgdbfConfig(flags=FIVE, T=kw["T"], maxphase=kw["maxphase"], theta=kw["theta"], lambda_=kw["lambda_"],
                             alpha=kw["alpha"], noise_scale=ns, ymax=kw["ymax"], windowsize=kw["windowsize"],
                             precision=PREC[prec][0])
    pick(ctx, "rows", PEG, prec, cfg)
    _, cnt = ctx.rgdbf_sim_batch(snr, R, cfg, seed=2024, stream_id=0, first_cw=0, batch=8192, want_frames=False)
    n1, e1 = 8192, cnt.as_dict()["frame_err"]
    n2, e2 = pooled["frames"], pooled["frame_errors"]
    p = (e1 + e2) / (n1 + n2)
    z = (e1 / n1 - e2 / n2) / math.sqrt(p * (1 - p) * (1 / n1 + 1 / n2))
    print(f"FER gpu {e1}/{n1} reference {e2}/{n2} z = {z:.2f}")
    assert abs(z) < 3, (e1, n1, e2, n2, z)
    assert cnt.as_dict()["iters"] < kw["maxphase"] * kw["T"] * n1


def test_sweep_driver_gdbf(tmp_path):
    """sweep --gdbf RSMNGDBF over two points: the totals are those of direct rgdbf_sim_batch
    calls (point k on stream k) under the family's stop rule, and the log line has the
    documented fields SNR BER avgIt FER T theta noiseScale lambda alpha windowsize Ymax maxphase alist."""
    log = tmp_path / "rsm.txt"
    cmd = [sys.executable, "-m", "ldpcsimulation_amd.sweep", code_path(PEG), "--rate", "0.5", "--snr", "3.0", "3.5",
           "-T", "50", "--gdbf", "RSMNGDBF", "--alpha", "0.96", "--ymax", "2.5", "--maxphase", "3", "--batch", "512",
           "--max-frames", "300", "--seed", "3", "--log", str(log), "--json"]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    js = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    lines = log.read_text().splitlines()
    assert len(js) == len(lines) == 2
    ctx = native.Context(native.Graph.from_alist(code_path(PEG)), 0, 512)
    cfg = cfg_of("f64", PEG, T=50, maxphase=3)
    for k, snr in enumerate((3.0, 3.5)):
        fr, _ = ctx.rgdbf_sim_batch(snr, 0.5, cfg, seed=3, stream_id=k, first_cw=0, batch=512)
        raw = np.ascontiguousarray(fr).view(np.int32).reshape(-1, 4)[:300]
        acc, used = sim.exact_cut(np.zeros(6, dtype=np.int64), raw, 50, 200, 20, True)
        assert 0 < used <= 300
        assert [js[k][key] for key in sim.COUNT_KEYS] == [int(x) for x in acc], (k, js[k])
        assert js[k]["kernel"] == "rgdbf_rows" and js[k]["gdbf"] == "RSMNGDBF"
        f = lines[k].split("\t")
        assert len(f) == 13 and f[0] == "%g" % snr and f[4:12] == ["50", "-0.6", "0.75", "0.99", "0.96", "16", "2.5", "3"]
        assert f[12].endswith(PEG)
        assert f[1] == "%g" % (acc[0] / (acc[3] * 1008)) and f[2] == "%g" % (acc[4] / acc[3])
        assert f[3] == "%g" % (acc[1] / acc[3])
