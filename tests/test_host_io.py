"""Host-or-device arguments of the C ABI (include/ldpc_hip.h): every decode entry point
takes each of its buffers as host or as device memory and stages the host ones. The
Python wrapper always passes host outputs, so these tests call the library directly:
the same decode with every argument on the host, every argument on the device (outputs
included) and a mix must give bit-identical decisions, frame records and counts.

Shapes are the smallest that reach the real kernels; the Eb/N0 values (0.8 dB min-sum,
2.0 dB GDBF, 1.0 dB EMS, all used by other tests on these codes) leave failing frames,
so the outputs compared are not trivial. The re-decoding, every-attempt and hardware-model
calls run PEG at batch 5 with T 20, two phases / three attempts, in fp64, at their own
tests' Eb/N0 on this code (3.0 dB; NGDBFhw 5.8 dB at its hard-coded rate)."""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import code_path

PEG = "PEGReg504x1008.alist"
GF16 = "gf16_N1000_dv2_dc4.alist"


def _native():
    from ldpcsimulation_amd import native
    return native


def _dev(a):
    """A device copy of a numpy array (None stays None)."""
    import torch
    if a is None:
        return None
    t = torch.from_numpy(a).cuda()
    torch.cuda.synchronize()
    return t


def _dev_out(like):
    import torch
    t = torch.zeros(like.nbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


def _back(t, like):
    return t.cpu().numpy().view(like.dtype).reshape(like.shape)


def _ok(rc):
    native = _native()
    assert rc == 0, native.lib().ldpc_last_error().decode(errors="replace")


def _counts(cnt):
    return tuple(int(getattr(cnt, k)) for k, _ in cnt._fields_)


def _three_ways(call, sync, inputs, outputs, cnt_type, mixed_host=()):
    """call(inputs..., outputs..., byref(counts)) with host, device and mixed arguments;
    `sync` orders the device outputs before they are read back. Returns the host result."""
    native = _native()
    P = native._ptr
    res = []
    for mode in ("host", "device", "mixed"):
        if mode == "host":
            ins = list(inputs.values())
        elif mode == "device":
            ins = [_dev(a) for a in inputs.values()]
        else:
            ins = [a if k in mixed_host else _dev(a) for k, a in inputs.items()]
        outs = [_dev_out(o) if mode == "device" else np.zeros_like(o) for o in outputs]
        cnt = cnt_type()
        _ok(call(*[P(a) for a in ins], *[P(o) for o in outs], C.byref(cnt)))
        sync()
        got = [_back(o, like) if mode == "device" else o for o, like in zip(outs, outputs)]
        res.append((got, _counts(cnt)))
    for other in res[1:]:
        for a, b in zip(res[0][0], other[0]):
            assert np.array_equal(a, b)
        assert res[0][1] == other[1]
    return res[0]


def _channel(shape, ebn0, dtype, seed, R=0.5):
    sigma = math.sqrt(10 ** (-ebn0 / 10) / R / 2)
    rng = np.random.default_rng(seed)
    return (1 + sigma * rng.standard_normal(shape)).astype(dtype), sigma


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_decode_batch_host_device_mixed(gpu_ctx_factory, prec):
    native = _native()
    L = native.lib()
    ctx = gpu_ctx_factory(PEG)
    N, B = ctx.graph.N, 3
    f64 = prec == "f64"
    cfg = native.DecoderConfig(variant=native.MS, T=5, precision=native.F64 if f64 else native.F32)._c()
    y, _ = _channel((B, N), 0.8, np.float64 if f64 else np.float32, seed=1)
    cw = np.ones((B, N), dtype=np.int8)
    d = np.zeros((B, N), dtype=np.int8)
    fr = np.zeros(B, dtype=native.FRAME_DTYPE)

    def call(py, pcw, pd, pfr, pcnt):
        return L.ldpc_decode_batch(ctx._h, py, B, C.byref(cfg), pcw, pd, pfr, pcnt)

    (d, fr), cnt = _three_ways(call, ctx.synchronize, dict(y=y, cw=cw), [d, fr], native.Counts, mixed_host=("cw",))
    assert cnt[3] == B and fr["bit_err"].sum() > 0 and int((d != 1).sum()) == fr["bit_err"].sum() == cnt[0]


@pytest.mark.gpu
@pytest.mark.parametrize("noise", [False, True], ids=["atgdbf", "mngdbf_pert"])
def test_gdbf_decode_batch_host_device_mixed(gpu_ctx_factory, noise):
    native = _native()
    L = native.lib()
    ctx = gpu_ctx_factory(PEG)
    N, B, T = ctx.graph.N, 3, 10
    flags = native.GDBF_VARIANTS["MNGDBF" if noise else "ATGDBF"]
    cfg = native.GdbfConfig(flags=flags, T=T)._c()
    y, sigma = _channel((B, N), 2.0, np.float64, seed=2)
    pert = (0.75 * sigma * np.random.default_rng(3).standard_normal((B, T, N))) if noise else None
    cw = np.ones((B, N), dtype=np.int8)
    d = np.zeros((B, N), dtype=np.int8)
    fr = np.zeros(B, dtype=native.FRAME_DTYPE)

    def call(py, ppert, pcw, pd, pfr, pcnt):
        return L.ldpc_gdbf_decode_batch(ctx._h, py, ppert, B, C.byref(cfg), pcw, pd, pfr, pcnt)

    (d, fr), cnt = _three_ways(call, ctx.synchronize, dict(y=y, pert=pert, cw=cw), [d, fr], native.Counts,
                               mixed_host=("pert", "cw"))
    assert cnt[3] == B and fr["bit_err"].sum() > 0 and int((d != 1).sum()) == fr["bit_err"].sum() == cnt[0]


@pytest.fixture(scope="module")
def nbctx():
    native = _native()
    return native.NbContext(native.NbGraph.from_alist(code_path(GF16)), 0, 8)


@pytest.mark.gpu
def test_ems_decode_batch_host_device_mixed(nbctx):
    native = _native()
    L = native.lib()
    g = nbctx.graph
    B = 2
    cfg = native.EmsConfig(T=2, nm=16)._c()
    y, sigma = _channel((B, g.N * g.m), 1.0, np.float32, seed=4)
    n0 = 2 * sigma * sigma
    cw = np.zeros((B, g.N), dtype=np.uint8)
    d = np.zeros((B, g.N), dtype=np.uint8)
    fr = np.zeros(B, dtype=native.FRAME_DTYPE)

    def call(py, pcw, pd, pfr, pcnt):
        return L.ldpc_ems_decode_batch(nbctx._h, py, B, n0, C.byref(cfg), pcw, pd, pfr, pcnt)

    (d, fr), cnt = _three_ways(call, nbctx.read_counts, dict(y=y, cw=cw), [d, fr], native.NbCounts,
                               mixed_host=("cw",))
    assert cnt[3] == B and fr["bit_err"].sum() > 0 and int((d != 0).sum()) == cnt[6] > 0


def _host_and_device(call, sync, outputs, cnt_type):
    """call(outputs..., byref(counts)) with host and with device outputs."""
    native = _native()
    res = []
    for device in (False, True):
        outs = [_dev_out(o) if device else np.zeros_like(o) for o in outputs]
        cnt = cnt_type()
        _ok(call(*[native._ptr(o) for o in outs], C.byref(cnt)))
        sync()
        res.append(([_back(o, like) if device else o for o, like in zip(outs, outputs)], _counts(cnt)))
    for a, b in zip(res[0][0], res[1][0]):
        assert np.array_equal(a, b)
    assert res[0][1] == res[1][1]
    return res[0]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_sim_trace_host_and_device_outputs(gpu_ctx_factory, prec):
    native = _native()
    L = native.lib()
    ctx = gpu_ctx_factory(PEG)
    N, B = ctx.graph.N, 3
    f64 = prec == "f64"
    cfg = native.DecoderConfig(variant=native.MS, T=5, precision=native.F64 if f64 else native.F32)._c()
    outs = [np.zeros((B, N), dtype=np.float64 if f64 else np.float32), np.zeros((B, N), dtype=np.int8),
            np.zeros(B, dtype=native.FRAME_DTYPE)]

    def call(py, pd, pfr, pcnt):
        return L.ldpc_sim_trace(ctx._h, 0.8, 0.5, C.byref(cfg), 5, 1, 3, B, py, pd, pfr, pcnt)

    (y, d, fr), cnt = _host_and_device(call, ctx.synchronize, outs, native.Counts)
    assert cnt[3] == B and fr["bit_err"].sum() > 0 and int((d != 1).sum()) == cnt[0] and y.std() > 0.5


@pytest.mark.gpu
def test_ems_sim_trace_host_and_device_outputs(nbctx):
    native = _native()
    L = native.lib()
    g = nbctx.graph
    B = 2
    cfg = native.EmsConfig(T=2, nm=16)._c()
    outs = [np.zeros((B, g.N * g.m), dtype=np.float32), np.zeros((B, g.N), dtype=np.uint8),
            np.zeros(B, dtype=native.FRAME_DTYPE)]

    def call(py, pd, pfr, pcnt):
        return L.ldpc_ems_sim_trace(nbctx._h, 1.0, 0.5, C.byref(cfg), 7, 1, 300, B, py, pd, pfr, pcnt)

    (y, d, fr), cnt = _host_and_device(call, nbctx.read_counts, outs, native.NbCounts)
    assert cnt[3] == B and fr["bit_err"].sum() > 0 and int((d != 0).sum()) == cnt[6] and y.std() > 0.5


# ---- the families whose staging no test exercised with device-side arguments
RB, RT, PHASES, ATTEMPTS = 5, 20, 2, 3
HW_R, HW_SNR = 0.8413, 5.8          # NGDBFhw.cpp's hard-coded rate; tests/test_hwgdbf.py's Eb/N0 on PEG


@pytest.mark.gpu
def test_rgdbf_decode_batch_host_device_mixed(gpu_ctx_factory):
    native = _native()
    L = native.lib()
    ctx = gpu_ctx_factory(PEG)
    N = ctx.graph.N
    cfg = native.RgdbfConfig(T=RT, maxphase=PHASES)._c()
    y, sigma = _channel((RB, N), 3.0, np.float64, seed=5)
    pert = 0.75 * sigma * np.random.default_rng(6).standard_normal((RB, PHASES * RT, N))
    cw = np.ones((RB, N), dtype=np.int8)
    outs = [np.zeros((RB, N), dtype=np.int8), np.zeros(RB, dtype=native.FRAME_DTYPE)]

    def call(py, ppert, pcw, pd, pfr, pcnt):
        return L.ldpc_rgdbf_decode_batch(ctx._h, py, ppert, RB, C.byref(cfg), pcw, pd, pfr, pcnt)

    (d, fr), cnt = _three_ways(call, ctx.synchronize, dict(y=y, pert=pert, cw=cw), outs, native.Counts,
                               mixed_host=("pert", "cw"))
    assert cnt[3] == RB and fr["bit_err"].sum() > 0 and int((d != 1).sum()) == fr["bit_err"].sum() == cnt[0]
    assert fr["iters"].max() > RT                                       # a second phase ran


def _rstat_outputs(native, N, M, samples):
    shape = (RB, ATTEMPTS, RT)
    outs = [np.zeros((RB, ATTEMPTS), dtype=native.ATTEMPT_DTYPE), np.zeros(shape, dtype=np.int32),
            np.zeros(shape, dtype=np.int32), np.zeros(shape + (N,), dtype=np.int8), np.zeros(shape + (M,), dtype=np.int8),
            np.zeros((RB, N), dtype=np.int8), np.zeros(RB, dtype=native.FRAME_DTYPE)]
    if samples:
        outs = [np.zeros((RB, N)), np.zeros((RB, ATTEMPTS, RT, N))] + outs
    return outs


def _rstat_asserts(att, err, unsat, dtr, strc, d, fr, cnt):
    assert cnt[3] == RB and fr["bit_err"].sum() > 0 and int((d != 1).sum()) == fr["bit_err"].sum()
    assert (att["iters"].sum(axis=1) == fr["iters"]).all() and (att["bit_err"][:, -1] == fr["bit_err"]).all()
    ran = err >= 0                                                      # -1: the row's iteration did not run
    assert ran.any() and (ran == (unsat >= 0)).all()
    assert (np.abs(dtr).max(axis=3) == ran).all() and (np.abs(strc).max(axis=3) == ran).all()   # +-1 rows / zero rows


@pytest.mark.gpu
def test_rstat_decode_batch_host_device_mixed(gpu_ctx_factory):
    native = _native()
    L = native.lib()
    ctx = gpu_ctx_factory(PEG)
    N, M = ctx.graph.N, ctx.graph.M
    cfg = native.RstatConfig(T=RT, attempts=ATTEMPTS)._c()
    y, sigma = _channel((RB, N), 3.0, np.float64, seed=7)
    pert = 0.75 * sigma * np.random.default_rng(8).standard_normal((RB, ATTEMPTS, RT, N))
    cw = np.ones((RB, N), dtype=np.int8)

    def call(py, ppert, pcw, patt, perr, punsat, pdt, pst, pd, pfr, pcnt):
        tr = native._RstatTrace(perr, punsat, pdt, pst)
        return L.ldpc_rstat_decode_batch(ctx._h, py, ppert, RB, C.byref(cfg), pcw, patt, C.byref(tr), pd, pfr, pcnt)

    outs, cnt = _three_ways(call, ctx.synchronize, dict(y=y, pert=pert, cw=cw), _rstat_outputs(native, N, M, False),
                            native.Counts, mixed_host=("pert", "cw"))
    _rstat_asserts(*outs, cnt)


@pytest.mark.gpu
def test_rstat_sim_trace_host_and_device_outputs(gpu_ctx_factory):
    native = _native()
    L = native.lib()
    ctx = gpu_ctx_factory(PEG)
    N, M = ctx.graph.N, ctx.graph.M
    cfg = native.RstatConfig(T=RT, attempts=ATTEMPTS)._c()

    def call(py, ppert, patt, perr, punsat, pdt, pst, pd, pfr, pcnt):
        tr = native._RstatTrace(perr, punsat, pdt, pst)
        return L.ldpc_rstat_sim_trace(ctx._h, 3.0, 0.5, C.byref(cfg), 9, 1, 3, RB, py, ppert, patt, C.byref(tr), pd, pfr,
                                      pcnt)

    (y, pert, *outs), cnt = _host_and_device(call, ctx.synchronize, _rstat_outputs(native, N, M, True), native.Counts)
    _rstat_asserts(*outs, cnt)
    assert y.std() > 0.5 and pert[:, 0, 0].std() > 0.1                  # the samples drawn came back


def _hw_cfg(native, N):
    return native.HwGdbfConfig(T=RT, maxphase=PHASES, qlen=N + 7)       # tests/test_hwgdbf.py "wraps": T 20, qlen N + 7


@pytest.mark.gpu
def test_hwgdbf_decode_batch_host_device_mixed(gpu_ctx_factory):
    native = _native()
    L = native.lib()
    ctx = gpu_ctx_factory(PEG)
    N = ctx.graph.N
    hw = _hw_cfg(native, N)
    cfg = hw._c()
    y, sigma = _channel((RB, N), HW_SNR, np.float64, seed=10, R=HW_R)
    q = hw.noise_scale * sigma * np.random.default_rng(11).standard_normal((RB, hw.qlen))
    qptr0 = np.array([0, 6, 3, 1, 5], dtype=np.int32)                   # each in [0, qlen - N)
    cw = np.ones((RB, N), dtype=np.int8)
    outs = [np.zeros((RB, N), dtype=np.int8), np.zeros(RB, dtype=native.FRAME_DTYPE), np.zeros(RB, dtype=np.int32)]

    def call(py, pq, pqptr, pcw, pd, pfr, prun, pcnt):
        return L.ldpc_hwgdbf_decode_batch(ctx._h, py, pq, pqptr, RB, C.byref(cfg), pcw, pd, pfr, prun, pcnt)

    (d, fr, run), cnt = _three_ways(call, ctx.synchronize, dict(y=y, q=q, qptr0=qptr0, cw=cw), outs, native.Counts,
                                    mixed_host=("q", "qptr0"))
    assert cnt[3] == RB and fr["bit_err"].sum() > 0 and (d != 1).any()
    assert (run >= fr["iters"]).all() and run.max() > RT                # the sum over the phases; a second phase ran


@pytest.mark.gpu
def test_hwgdbf_sim_trace_host_and_device_outputs(gpu_ctx_factory):
    native = _native()
    L = native.lib()
    ctx = gpu_ctx_factory(PEG)
    N = ctx.graph.N
    hw = _hw_cfg(native, N)
    cfg = hw._c()
    outs = [np.zeros((RB, N)), np.zeros((RB, hw.qlen)), np.zeros((RB, N), dtype=np.int8),
            np.zeros(RB, dtype=native.FRAME_DTYPE)]

    def call(py, pq, pd, pfr, pcnt):
        return L.ldpc_hwgdbf_sim_trace(ctx._h, HW_SNR, HW_R, C.byref(cfg), 12, 1, 3, RB, py, pq, pd, pfr, pcnt)

    (y, q, d, fr), cnt = _host_and_device(call, ctx.synchronize, outs, native.Counts)
    assert cnt[3] == RB and fr["bit_err"].sum() > 0 and (d != 1).any() and y.std() > 0.1 and q.std() > 0.1
