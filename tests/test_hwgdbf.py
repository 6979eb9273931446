"""The fixed-point NGDBF hardware-model decoder (ldpc_hwgdbf_*; hwgdbf.hip) on the GPU against
its numpy restatement (tests/hwgdbf_oracle.py, itself pinned to the reference's recorded runs
by tests/test_hwgdbf_oracle.py) and against the reference's pooled frame error rate.

Option gdbf_kernel picks the instance: 0 = the library's choice for the graph (hwgdbf_wave, a
wavefront per codeword, on 802.3 and N = 1944; hwgdbf_wg, a workgroup per codeword, on PEG),
1 = hwgdbf_wg forced; every test asserts that kernel_info names the instance meant. Equality is exact everywhere, with the fp64 and the fp32 front end (each against the
restatement in the same arithmetic)."""
import functools
import math

import numpy as np
import pytest

import hwgdbf_oracle as HO
from conftest import code_path
from ldpcsimulation_amd import native

pytestmark = pytest.mark.gpu

C802, PEG, W1944 = "802_3_H.alist", "PEGReg504x1008.alist", "80211n_1944_r12.alist"
PREC = {"f64": (native.F64, np.float64), "f32": (native.F32, np.float32)}
# option gdbf_kernel: 0 = the library's choice for the graph, 1 = hwgdbf_wg forced
KERNELS = {"default": 0, "wg": 1}
# the library's choice: the shape that keeps more waves on a CU (PEG's state is small enough
# for six workgroups of four waves; the two larger codes hold more single-wave codewords)
DEFAULT = {"802_3_H.alist": "hwgdbf_wave", "PEGReg504x1008.alist": "hwgdbf_wg", "80211n_1944_r12.alist": "hwgdbf_wave"}
# Eb/N0 (at the reference's hard-coded R = 0.8413) at which about half of 64 frames fail at
# the defaults: the golden runs bracket them (802.3: 28 of 30 fail at 3.5 dB and 9 of 200 at
# 4.0; PEG: 45 of 200 at 6.0; 1944: 5 of 60 at 8.0)
SNR = {C802: 3.75, PEG: 5.8, W1944: 7.7}
R = HO.R_802_3
FRAMES = 64


@functools.lru_cache(maxsize=None)
def oracle(code):
    return HO.HwGdbf(code_path(code))


@functools.lru_cache(maxsize=None)
def given(code, qlen, frames=FRAMES, seed=17):
    y, q = HO.glibc_frames(oracle(code), SNR[code], seed, frames, qlen=qlen)
    y.setflags(write=False)
    q.setflags(write=False)
    return y, q


# name -> cfg fields; qlen as an offset from N where it starts with "+"
CASES = {
    "defaults": dict(),
    "wraps": dict(T=20, maxphase=3, qlen="+7"),    # several wraps per phase, the carry across phases
    "still": dict(T=30, maxphase=2, qlen="+1"),    # the pointer stays 0
    "nq3": dict(T=50, nq=3),
    "nq7": dict(T=50, nq=7),
}


def case_kw(code, case):
    kw = dict(HO.DEFAULTS)
    kw.update(CASES[case])
    if isinstance(kw["qlen"], str):
        kw["qlen"] = oracle(code).N + int(kw["qlen"])
    if kw["qlen"] <= oracle(code).N:
        kw["qlen"] = oracle(code).N + 600
    return kw


def qptr_of(code, kw, frames):
    wrap = kw["qlen"] - oracle(code).N
    return np.random.default_rng(5).integers(0, wrap, size=frames).astype(np.int32)


@functools.lru_cache(maxsize=None)
def reference(code, case, prec):
    kw = case_kw(code, case)
    y, q = given(code, kw["qlen"])
    okw = {k: v for k, v in kw.items() if k != "noise_scale"}
    return oracle(code).decode(y, q, qptr_of(code, kw, len(y)), dtype=PREC[prec][1], **okw)


def cfg_of(kw, prec):
    return native.HwGdbfConfig(precision=PREC[prec][0], **kw)


def pick(ctx, kernel, cfg, code):
    ctx.set_option("gdbf_kernel", KERNELS[kernel])
    info = ctx.hwgdbf_kernel_info(cfg)
    want = "hwgdbf_wg" if kernel == "wg" else DEFAULT[code]
    if cfg.qlen == HO.DEFAULTS["qlen"]:   # the choice depends on the state's size, so on qlen
        assert info["kernel"] == want, info
    assert info["kernel"] in ("hwgdbf_wave", "hwgdbf_wg") and (kernel != "wg" or info["kernel"] == "hwgdbf_wg")
    assert 0 < info["lds_bytes"] <= 160 * 1024
    return info


def assert_equal(got, want, n=None):
    d, fr, run, cnt = got
    rd, rfr = want
    sl = slice(None) if n is None else slice(0, n)
    assert np.array_equal(run, rfr["iters_run"][sl]), (run, rfr["iters_run"][sl])
    for k in ("iters", "bit_err", "uncoded_bit_err", "syndrome_fail"):
        assert np.array_equal(np.asarray(fr[k], dtype=np.int64), rfr[k][sl]), k
    assert np.array_equal(d, rd[sl])
    c = cnt.as_dict()
    assert c["frames"] == len(d) and c["iters"] == int(rfr["iters"][sl].sum())
    assert c["bit_err"] == int(rfr["bit_err"][sl].sum()) and c["frame_err"] == int((rfr["bit_err"][sl] > 0).sum())
    assert c["uncoded_bit_err"] == int(rfr["uncoded_bit_err"][sl].sum())
    assert c["syndrome_fail"] == int(rfr["syndrome_fail"][sl].sum())


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("code", [C802, PEG, W1944])
def test_defaults_equal_restatement(gpu_ctx_factory, code, prec, kernel):
    """T = 600, one phase, the reference's constants; random start pointers."""
    ctx = gpu_ctx_factory(code)
    kw = case_kw(code, "defaults")
    cfg = cfg_of(kw, prec)
    pick(ctx, kernel, cfg, code)
    y, q = given(code, kw["qlen"])
    want = reference(code, "defaults", prec)
    fails = int(want[1]["syndrome_fail"].sum())
    assert FRAMES // 8 <= fails <= FRAMES - FRAMES // 8, fails   # both outcomes well represented
    assert_equal(ctx.hwgdbf_decode(y, q, cfg, qptr0=qptr_of(code, kw, len(y))), want)


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("code,case", [(C802, "wraps"), (W1944, "wraps"), (PEG, "wraps"), (PEG, "still"), (C802, "still"),
                                       (PEG, "nq3"), (C802, "nq3"), (PEG, "nq7"), (C802, "nq7"), (W1944, "nq7")])
def test_cases_equal_restatement(gpu_ctx_factory, code, case, prec, kernel):
    ctx = gpu_ctx_factory(code)
    kw = case_kw(code, case)
    cfg = cfg_of(kw, prec)
    pick(ctx, kernel, cfg, code)
    y, q = given(code, kw["qlen"])
    want = reference(code, case, prec)
    if case == "wraps" and code == C802:   # phases that stop early and phases that run out: the carry differs by frame
        assert len(set(want[1]["iters_run"])) > 1
    assert_equal(ctx.hwgdbf_decode(y, q, cfg, qptr0=qptr_of(code, kw, len(y))), want)


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("n", [1, 7, 13])
def test_batch_sizes(gpu_ctx_factory, kernel, n):
    """A batch of 1 and batches that are no multiple of the codewords per workgroup (16 waves here)."""
    ctx = gpu_ctx_factory(C802)
    kw = case_kw(C802, "wraps")
    cfg = cfg_of(kw, "f64")
    pick(ctx, kernel, cfg, C802)
    y, q = given(C802, kw["qlen"])
    assert_equal(ctx.hwgdbf_decode(y[:n], q[:n], cfg, qptr0=qptr_of(C802, kw, len(y))[:n]), reference(C802, "wraps", "f64"), n)


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_codewords_on_arrival_and_given_codewords(gpu_ctx_factory, prec, kernel):
    """Frames whose channel decision is already the codeword run 0 iterations and advance
    nothing; the transmitted codewords are given (PEG's encoded words), so errors are counted
    against them."""
    ctx = gpu_ctx_factory(PEG)
    oc = oracle(PEG)
    lines = [l for l in open(code_path("PEGReg504x1008_data20.enc")).read().split("\n") if l.strip()]
    n = 12
    c = np.array([[-1 if ch == "1" else 1 for ch in lines[i % len(lines)][:oc.N]] for i in range(n)], dtype=np.int8)
    kw = case_kw(PEG, "wraps")
    y0, q = given(PEG, kw["qlen"])
    y = y0[:n] * c
    y[::3] = c[::3] * 0.9   # noiseless: the decision is the codeword
    cfg = cfg_of(kw, prec)
    pick(ctx, kernel, cfg, PEG)
    okw = {k: v for k, v in kw.items() if k != "noise_scale"}
    want = oc.decode(y, q[:n], None, c=c, dtype=PREC[prec][1], **okw)
    assert (want[1]["iters_run"][::3] == 0).all() and (want[1]["iters_run"] > 0).any()
    got = ctx.hwgdbf_decode(y, q[:n], cfg, c=c)
    assert_equal(got, want)
    assert (got[1]["bit_err"][::3] == 0).all() and np.array_equal(got[0][::3], c[::3])


def test_refusals_with_a_graph(gpu_ctx_factory):
    ctx = gpu_ctx_factory(C802)
    y, q = given(C802, 2648)
    with pytest.raises(native.LdpcError) as e:
        ctx.hwgdbf_decode(y[:2], q[:2, :2048], native.HwGdbfConfig(qlen=2048))
    assert e.value.code == -1 and "qlen" in str(e.value)
    with pytest.raises(native.LdpcError) as e:
        ctx.hwgdbf_decode(y[:2], q[:2], native.HwGdbfConfig(), qptr0=[0, 600])
    assert e.value.code == -1 and "qptr0" in str(e.value)
    with pytest.raises(native.LdpcError) as e:
        ctx.hwgdbf_kernel_info(native.HwGdbfConfig(qlen=70000))
    assert e.value.code == -4 and "65536" in str(e.value)


# ---- the fused simulation ----
SIM = dict(snr=3.75, seed=2024, stream=3)


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_sim_trace_redecodes_and_splits(gpu_ctx_factory, prec, kernel):
    """sim_trace's samples, decoded by decode_batch, give sim_batch's frames; the results do
    not depend on how the frames are split into launches; counts are sums over frames; the
    channel is the min-sum path's."""
    ctx = gpu_ctx_factory(C802)
    cfg = cfg_of(dict(HO.DEFAULTS, T=100), prec)
    pick(ctx, kernel, cfg, C802)
    n = 512
    y, q, d, fr, cnt = ctx.hwgdbf_sim_trace(SIM["snr"], R, cfg, SIM["seed"], SIM["stream"], 0, n)
    fr1, cnt1 = ctx.hwgdbf_sim_batch(SIM["snr"], R, cfg, SIM["seed"], SIM["stream"], 0, n)
    assert np.array_equal(fr, fr1) and cnt.as_dict() == cnt1.as_dict()
    parts = [ctx.hwgdbf_sim_batch(SIM["snr"], R, cfg, SIM["seed"], SIM["stream"], 128 * k, 128)[0] for k in range(4)]
    assert np.array_equal(np.concatenate(parts), fr)
    c = cnt.as_dict()
    assert c["frames"] == n and c["bit_err"] == int(fr["bit_err"].sum()) and c["iters"] == int(fr["iters"].sum())
    assert c["frame_err"] == int((fr["bit_err"] > 0).sum()) and c["syndrome_fail"] == int(fr["syndrome_fail"].sum())
    assert c["uncoded_bit_err"] == int(fr["uncoded_bit_err"].sum())
    assert 0 < c["frame_err"] < n
    d2, fr2, run2, _ = ctx.hwgdbf_decode(y, q, cfg)
    assert np.array_equal(d2, d) and np.array_equal(fr2, fr)
    # the restatement on a few of the drawn frames
    rd, rfr = oracle(C802).decode(y[:8], q[:8], dtype=PREC[prec][1], T=100)
    assert np.array_equal(rd, d[:8]) and np.array_equal(rfr["iters"], fr["iters"][:8])
    ms = native.DecoderConfig(variant=native.MS, T=1, precision=PREC[prec][0])
    yms = ctx.sim_trace(SIM["snr"], R, ms, SIM["seed"], SIM["stream"], 0, 64)[0]
    assert np.array_equal(yms, y[:64])
    # noise statistics: q = noise_scale * sigma * n
    _, nsig = HO.sigmas(SIM["snr"])
    assert abs(q.std() / nsig - 1) < 0.01 and abs(q.mean()) < 0.01 * nsig


def test_fer_against_the_reference_pool(gpu_ctx_factory):
    """65,536 Philox frames on 802.3 at 4.0 dB against the reference's pooled frame errors:
    two-proportion |z| < 3."""
    _, pool = HO.golden_runs()
    ctx = gpu_ctx_factory(C802, 65536)
    cfg = native.HwGdbfConfig(precision=native.F64)
    _, cnt = ctx.hwgdbf_sim_batch(float(pool["snr"]), R, cfg, 99, 1, 0, 65536, want_frames=False)
    n1, k1, n2, k2 = 65536, cnt.as_dict()["frame_err"], pool["frames"], pool["frame_errors"]
    p = (k1 + k2) / (n1 + n2)
    z = (k1 / n1 - k2 / n2) / math.sqrt(p * (1 - p) * (1 / n1 + 1 / n2))
    print(f"FER gpu {k1}/{n1} = {k1 / n1:.5f}, reference {k2}/{n2} = {k2 / n2:.5f}, z = {z:.3f}")
    assert abs(z) < 3, (k1, n1, k2, n2, z)
