"""Early termination of the min-sum decoders and BP (ldpc_decoder_cfg.early_stop).

The definition every test uses: D(t) is what the fixed-T decoder returns for a frame at
T = t (decisions, bit_err, uncoded_bit_err, syndrome_fail); with early_stop the frame's
result is D(s) for the smallest s in 0..T whose D(s) has syndrome_fail == 0 (s = T when
there is none), frames[].iters = s and counts.iters += s. The expected side is always
built from fixed-T launches (early_stop = 0) of the same context at T = 0..T, and in fp64
also from the CPU oracle; the comparisons are exact.

Samples: y = 1 + sigma_b * n, n from np.random.default_rng(5), sigma_b cycling per frame,
so that every case has frames that stop at 0, frames that stop in between and (the golden
codes, the dc32 / row33 codes) frames that never stop -- asserted from the expected side."""
import functools
import io
import json
import contextlib

import numpy as np
import pytest

from conftest import code_path
from ldpcsimulation_amd import codes, native, sweep
from oracle import oracle as O
from test_gpu_parity import VARIANTS, _oracle_front
from test_shape_matrix import CODES as SYN_CODES
from test_shape_matrix import SHAPES, build_code

pytestmark = pytest.mark.gpu

PEG, W1944, C802, DVB = "PEGReg504x1008.alist", "80211n_1944_r12.alist", "802_3_H.alist", "dvbs2_1_2.alist"
GOLD_SIGMA, GOLD_FRAMES, GOLD_T = (0.3, 0.6, 0.75, 0.9), 48, 12
SYN_SIGMA, SYN_FRAMES, SYN_T = (0.2, 0.45, 0.6, 0.7), 32, 10
PREC = {"f64": (native.F64, np.float64), "f32": (native.F32, np.float32)}
FIELDS = ("bit_err", "uncoded_bit_err", "syndrome_fail")
INVALID, UNSUPPORTED = -1, -4


def samples(N, frames, sigmas, prec):
    n = np.random.default_rng(5).standard_normal((frames, N))
    sig = np.array([sigmas[b % len(sigmas)] for b in range(frames)])[:, None]
    return (1.0 + sig * n).astype(PREC[prec][1])


def cfg_of(prec, v, T, **kw):
    return native.DecoderConfig(T=T, precision=PREC[prec][0], **v, **kw)


def definition(ctx, y, prec, v, T, c=None, **kw):
    """(s, d, frames) of the definition, from this context's fixed-T launches at T = 0..T."""
    runs = [ctx.decode(y, cfg_of(prec, v, t, **kw), c=c) for t in range(T + 1)]
    for t, (_, fr, cnt) in enumerate(runs):   # fixed T: 0 reported, T counted per frame
        assert not fr["iters"].any() and cnt.iters == t * len(y)
    fail = np.stack([fr["syndrome_fail"] for _, fr, _ in runs])            # [T + 1, frames]
    s = np.where((fail == 0).any(axis=0), (fail == 0).argmax(axis=0), T)
    idx = np.arange(len(y))
    d = np.stack([r[0] for r in runs])[s, idx]
    fr = np.empty(len(y), dtype=native.FRAME_DTYPE)
    for k in FIELDS:
        fr[k] = np.stack([r[1][k] for r in runs])[s, idx]
    fr["iters"] = s
    return s, d, fr


def assert_mix(s, T, never):
    assert (s == 0).any() and ((s > 0) & (s < T)).any(), np.bincount(s, minlength=T + 1)
    if never:
        assert (s == T).any()


def assert_result(got, want, where=""):
    """One early-stop call (d, frames, counts) against (s, d, frames) of the definition."""
    d, fr, cnt = got
    s, dw, fw = want
    for k in ("iters",) + FIELDS:
        assert np.array_equal(fr[k], fw[k]), (where, k, np.nonzero(fr[k] != fw[k])[0][:8].tolist())
    assert np.array_equal(d, dw), (where, np.nonzero((d != dw).any(axis=1))[0][:8].tolist())
    assert cnt.iters == int(s.sum()) and cnt.frames == len(s), where
    assert cnt.bit_err == int(fw["bit_err"].sum()) and cnt.frame_err == int((fw["bit_err"] > 0).sum()), where
    assert cnt.uncoded_bit_err == int(fw["uncoded_bit_err"].sum()), where
    assert cnt.syndrome_fail == int(fw["syndrome_fail"].sum()), where


def assert_oracle(path, y, prec, v, T, want):
    """fp64: D(s) is the oracle's decode at T = s, and the oracle's own s agrees."""
    s, d, _ = want
    A, H = O.Alist(path), codes.read_alist(path)
    yq = _oracle_front(y, v, prec == "f32")
    runs = [A.decode(yq, t, O.Cfg(**v)) for t in range(T + 1)]
    ok = np.array([[not any(H.syndrome(row != 1)) for row in r] for r in runs])
    s_or = np.where(ok.any(axis=0), ok.argmax(axis=0), T)
    assert np.array_equal(s_or, s)
    assert np.array_equal(np.stack(runs)[s, np.arange(len(y))], d)


# ------------------------------------------------------------------ 1. the definition
DEFINITION_CASES = {
    "peg_f64_ms": (PEG, "f64", "ms"), "peg_f32_qnms": (PEG, "f32", "qnms"),
    "w1944_f64_nms": (W1944, "f64", "nms"), "w1944_f32_nms": (W1944, "f32", "nms"), "w1944_f64_oms": (W1944, "f64", "oms"),
    "c802_f64_ms": (C802, "f64", "ms"),
}


@pytest.mark.parametrize("case", list(DEFINITION_CASES))
def test_definition(gpu_ctx_factory, case):
    code, prec, vname = DEFINITION_CASES[case]
    v = VARIANTS[vname]
    ctx = gpu_ctx_factory(code, 64)
    y = samples(ctx.graph.N, GOLD_FRAMES, GOLD_SIGMA, prec)
    want = definition(ctx, y, prec, v, GOLD_T)
    assert_mix(want[0], GOLD_T, never=True)
    if prec == "f64":
        assert_oracle(code_path(code), y, prec, v, GOLD_T, want)
    # the 802.3 code (row degree 32, 2048 bits on 384 rows) has no row schedule: "lds" decodes it
    default = "lds" if code == C802 else "rows_es"
    for opt, kernel in (("auto", default), ("lds", "lds"), ("global", "global")):
        ctx.reset_options()
        ctx.set_option("kernel", opt)
        cfg = cfg_of(prec, v, GOLD_T, early_stop=True)
        assert ctx.kernel_info(cfg)["kernel"] == kernel
        assert_result(ctx.decode(y, cfg), want, (case, kernel))
        # T = 0: D(0), no iteration counted
        d0, fr0, cnt0 = ctx.decode(y, cfg_of(prec, v, 0, early_stop=True))
        ctx.reset_options()
        dw, fw, _ = ctx.decode(y, cfg_of(prec, v, 0))
        assert np.array_equal(d0, dw) and cnt0.iters == 0 and not fr0["iters"].any()
        assert all(np.array_equal(fr0[k], fw[k]) for k in FIELDS)


# ------------------------------------------------------------------ 2. every shape
class Syn:
    """One synthetic code of test_shape_matrix: its alist, graph and a device context."""

    def __init__(self, root, name, max_batch=64):
        self.path = str(root / f"{name}.alist")
        build_code(self.path, name)
        self.graph = native.Graph.from_alist(self.path)
        self.ctx = native.Context(self.graph, 0, max_batch)


@pytest.fixture(scope="module")
def syn(tmp_path_factory):
    assert native.device_count() > 0, "no HIP device visible"
    root = tmp_path_factory.mktemp("early_stop")
    return functools.lru_cache(maxsize=None)(lambda name, max_batch=64: Syn(root, name, max_batch))


NEVER = ("dc32_cpt4_rpt1", "dc32_cpt4_rpt2", "row33")   # wide rows: some sigma = 0.7 frames never decode


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("name", [n for n in SYN_CODES if n.startswith("dc")] + ["row33"])
def test_every_shape(syn, name, prec):
    L, v = syn(name), VARIANTS["nms"]
    y = samples(L.graph.N, SYN_FRAMES, SYN_SIGMA, prec)
    want = definition(L.ctx, y, prec, v, SYN_T)
    assert_mix(want[0], SYN_T, never=name in NEVER)
    if prec == "f64":
        assert_oracle(L.path, y, prec, v, SYN_T, want)
    cfg = cfg_of(prec, v, SYN_T, early_stop=True)
    if name == "row33":   # no row schedule
        assert L.ctx.kernel_info(cfg)["kernel"] == "lds"
        with pytest.raises(native.LdpcError) as e:
            L.ctx.row_sched_info(cfg)
        assert e.value.code == UNSUPPORTED
    else:
        i = L.ctx.row_sched_info(cfg)
        assert (i["dc"], i["slots_per_thread"], i["rows_per_thread"], i["threads"]) == SHAPES[name][2:]
        assert i["cw_per_block"] == 1 and L.ctx.kernel_info(cfg)["kernel"] == "rows_es"
    assert_result(L.ctx.decode(y, cfg), want, (name, prec))


# ------------------------------------------------------------------ 3. tickets and independence
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_tickets_and_independence(syn, prec):
    """More frames than blocks (one block per CU): every frame's result is the definition's,
    whatever the call it is decoded in, its neighbours and the order the tickets come in."""
    L, v, frames = syn("dc8_cpt2_rpt1", 600), VARIANTS["nms"], 600
    ctx = L.ctx
    y = samples(L.graph.N, frames, SYN_SIGMA, prec)
    ctx.reset_options()
    s, dw, fw = definition(ctx, y, prec, v, SYN_T)
    assert_mix(s, SYN_T, never=False)
    ctx.set_option("rows_bpc", 1)
    cfg = cfg_of(prec, v, SYN_T, early_stop=True)
    assert ctx.kernel_info(cfg)["kernel"] == "rows_es"
    assert_result(ctx.decode(y, cfg), (s, dw, fw), "one call")
    for lo in range(0, frames, 37):
        hi = min(frames, lo + 37)
        assert_result(ctx.decode(y[lo:hi], cfg), (s[lo:hi], dw[lo:hi], fw[lo:hi]), f"frames {lo}..{hi}")
    r = slice(None, None, -1)
    assert_result(ctx.decode(np.ascontiguousarray(y[r]), cfg), (s[r], dw[r], fw[r]), "reversed")
    for n in (1, 7, 13):
        assert_result(ctx.decode(y[:n], cfg), (s[:n], dw[:n], fw[:n]), f"batch {n}")
    ctx.reset_options()


# ------------------------------------------------------------------ 4. the on-device channel
@pytest.mark.parametrize("code,prec,vname,snr", [(PEG, "f64", "nms", 2.5), (PEG, "f32", "ms", 2.5),
                                                  (W1944, "f64", "oms", 1.8), (W1944, "f32", "nms", 1.8)])
def test_on_device_channel(gpu_ctx_factory, code, prec, vname, snr):
    ctx, v, T = gpu_ctx_factory(code, 256), VARIANTS[vname], GOLD_T
    es, fixed = cfg_of(prec, v, T, early_stop=True), cfg_of(prec, v, T)
    assert ctx.kernel_info(es)["kernel"] == "rows_es"
    y0, _, _, _ = ctx.sim_trace(snr, 0.5, fixed, seed=7, stream_id=3, first_cw=1000, batch=200)
    y, d, fr, cnt = ctx.sim_trace(snr, 0.5, es, seed=7, stream_id=3, first_cw=1000, batch=200)
    assert np.array_equal(y, y0)
    dd, fd, cd = ctx.decode(y, es)
    assert np.array_equal(d, dd) and np.array_equal(fr, fd) and np.array_equal(cnt.as_array(), cd.as_array())
    assert 0 < cnt.iters < T * 200 and cnt.iters == int(fr["iters"].sum())   # frames stop early at this SNR
    fa, ca = ctx.sim_batch(snr, 0.5, es, seed=7, stream_id=3, first_cw=1000, batch=200)
    f1, c1 = ctx.sim_batch(snr, 0.5, es, seed=7, stream_id=3, first_cw=1000, batch=77)
    f2, c2 = ctx.sim_batch(snr, 0.5, es, seed=7, stream_id=3, first_cw=1077, batch=123)
    assert np.array_equal(fa, fr) and np.array_equal(np.concatenate([f1, f2]), fa)
    assert np.array_equal(c1.as_array() + c2.as_array(), ca.as_array())


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_codeword_table(prec):
    """Codeword-file mode: frame f sends row f % rows; the errors are counted against it."""
    g = native.Graph.from_alist(code_path(PEG))
    ctx = native.Context(g, 0, 64)
    bits = codes.read_codeword_file(code_path("PEGReg504x1008_data20.enc"), g.N)
    ctx.set_codewords(bits)
    v, T = VARIANTS["nms"], GOLD_T
    es = cfg_of(prec, v, T, early_stop=True)
    y, d, fr, cnt = ctx.sim_trace(2.0, 0.5, es, seed=11, stream_id=1, first_cw=13, batch=48)
    c = np.where(bits[(13 + np.arange(48)) % len(bits)] != 0, -1, 1).astype(np.int8)
    assert (c == -1).any()
    s, dw, fw = definition(ctx, y, prec, v, T, c=c)
    assert ((s > 0) & (s < T)).any() and (s == T).any()   # 2 dB: no frame is a codeword undecoded
    assert_result((d, fr, cnt), (s, dw, fw), "table")
    assert_result(ctx.decode(y, es, c=c), (s, dw, fw), "given")
    assert np.array_equal(fr["bit_err"], (d != c).sum(axis=1))


# ------------------------------------------------------------------ 5. belief propagation
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("code", [PEG, W1944])
def test_bp(gpu_ctx_factory, code, prec):
    """Exact against the same kernel's fixed-T launches: the same arithmetic, stopped earlier."""
    ctx, T = gpu_ctx_factory(code, 64), 10
    v = dict(variant=native.BP, n0=0.72)
    y = samples(ctx.graph.N, GOLD_FRAMES, GOLD_SIGMA, prec)
    for opt, kernel in (("rows", "bp_rows"), ("generic", "bp_lds")):
        ctx.reset_options()
        ctx.set_option("bp_kernel", opt)
        cfg = cfg_of(prec, v, T, early_stop=True)
        assert ctx.kernel_info(cfg)["kernel"] == kernel
        want = definition(ctx, y, prec, v, T)
        assert_mix(want[0], T, never=True)
        assert_result(ctx.decode(y, cfg), want, (code, prec, kernel))
        assert_result(ctx.decode(y[:7], cfg), tuple(x[:7] for x in want), (code, prec, kernel, 7))
        d0, fr0, cnt0 = ctx.decode(y, cfg_of(prec, v, 0, early_stop=True))
        dw, fw, _ = ctx.decode(y, cfg_of(prec, v, 0))
        assert np.array_equal(d0, dw) and cnt0.iters == 0 and all(np.array_equal(fr0[k], fw[k]) for k in FIELDS)
    ctx.reset_options()


# ------------------------------------------------------------------ 6. refusals, codes beyond LDS
def test_refusals(gpu_ctx_factory):
    ctx, v = gpu_ctx_factory(PEG, 64), VARIANTS["nms"]
    y = samples(ctx.graph.N, 4, GOLD_SIGMA, "f64")

    def code_of(cfg):
        with pytest.raises(native.LdpcError) as e:
            ctx.decode(y, cfg)
        return e.value.code

    assert code_of(cfg_of("f64", v, 4, early_stop=2)) == INVALID
    assert code_of(cfg_of("f64", v, 4, early_stop=-1)) == INVALID
    assert code_of(cfg_of("f64", v, 4, early_stop=True, schedule=native.LAYERED)) == UNSUPPORTED
    ctx.set_option("kernel", "flood")
    assert code_of(cfg_of("f64", v, 4, early_stop=True)) == UNSUPPORTED
    with pytest.raises(native.LdpcError) as e:
        ctx.kernel_info(cfg_of("f64", v, 4, early_stop=True))
    assert e.value.code == UNSUPPORTED
    ctx.decode(y, cfg_of("f64", v, 4))   # the flood kernel itself still decodes
    ctx.reset_options()
    # DD-BMP always stops and does not read the field
    dd = dict(variant=native.DDBMP, quantize=True, ymax=1.0, qbits=3)
    a, b = ctx.decode(y, cfg_of("f64", dd, 20)), ctx.decode(y, cfg_of("f64", dd, 20, early_stop=True))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_dvbs2_on_global(gpu_ctx_factory, prec):
    ctx, v, T = gpu_ctx_factory(DVB, 64), VARIANTS["nms"], 4
    y = samples(ctx.graph.N, 4, (0.3, 0.9), prec)
    cfg = cfg_of(prec, v, T, early_stop=True)
    assert ctx.kernel_info(cfg)["kernel"] == "global"
    want = definition(ctx, y, prec, v, T)
    assert (want[0] < T).any() and (want[0] == T).any()   # sigma 0.3 stops, sigma 0.9 does not
    assert_result(ctx.decode(y, cfg), want, "dvbs2")


# ------------------------------------------------------------------ 7. the sweep
@pytest.mark.parametrize("sync", [False, True])
def test_sweep(gpu_ctx_factory, sync):
    argv = [code_path(PEG), "--rate", "0.5", "--variant", "nms", "--alpha", "1.25", "-T", "20", "--early-stop",
            "--snr", "3.0", "--max-frames", "512", "--batch", "256", "--seed", "1", "--json"] + (["--sync"] if sync else [])
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        assert sweep.main(argv) == 0
    line, js = out.getvalue().strip().split("\n")
    js = json.loads(js)
    assert js["kernel"] == "rows_es" and js["frames"] == 512
    ctx = gpu_ctx_factory(PEG, 512)
    cfg = native.DecoderConfig(variant=native.NMS, alpha=1.25, T=20, early_stop=True)
    fr, cnt = ctx.sim_batch(3.0, 0.5, cfg, seed=1, stream_id=0, first_cw=0, batch=512)
    for k, val in cnt.as_dict().items():
        assert js[k] == val, k
    assert 0 < js["iters"] < 20 * 512 and js["iters"] == int(fr["iters"].sum())
    assert js["avg_iters"] == js["iters"] / 512
    f = line.split("\t")
    assert float(f[2]) == float("%g" % (js["iters"] / 512)) and f[4] == "20"
