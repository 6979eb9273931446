"""Every refusal of the decoder entry points of the C ABI (include/ldpc_hip.h), one call per
entry point and fault kind with exactly one fault in it: the status and the message of
ldpc_last_error() are compared with tests/golden/abi_refusals.json, which
tests/golden/make_abi_refusals.py recorded from the library before the entry points were
moved onto the shared launch skeleton (host_rt.h). Every call here is refused before any
launch; the buffers are sized for the largest batch used all the same.

PEG 504x1008 with max_batch = 8 for the binary families, the GF(16) code for EMS. The rows
with a null context, and the cfg-only rows of the *_kernel_info calls, need no device."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLD, code_path
from ldpcsimulation_amd import native

PEG, GF16 = "PEGReg504x1008.alist", "gf16_N1000_dv2_dc4.alist"
N, M = 1008, 504
T, ATT, BMAX = 20, 3, 9                  # buffers hold batch 9, the one past max_batch = 8
QLEN = N + 7
GOLDEN = os.path.join(GOLD, "abi_refusals.json")
SIM = dict(ebn0=3.0, R=0.5, seed=1, stream=0, first=0, batch=2)


def _ref(cfg):
    """None, a *Config dataclass or a ctypes cfg struct as the cfg argument."""
    return None if cfg is None else C.byref(cfg._c() if hasattr(cfg, "_c") else cfg)


def _reserved(cfg):
    c = cfg._c()
    c.reserved = 1
    return c


def table(ctx=None, nb=None):
    """{case id: thunk returning the status}. Without contexts: the rows that need no device."""
    L, P = native.lib(), native._ptr
    h, nh = (ctx._h if ctx else None), (nb._h if nb else None)
    dev = ctx is not None
    f8 = np.zeros((BMAX, N))
    pert = np.zeros((BMAX, ATT * T, N))
    q = np.zeros((BMAX, QLEN))
    fr = np.zeros(BMAX, dtype=native.FRAME_DTYPE)
    att = np.zeros((BMAX, ATT), dtype=native.ATTEMPT_DTYPE)
    tr_host = np.zeros((BMAX, ATT, T), dtype=np.int32)
    ynb = np.zeros((BMAX, 1000 * 4), dtype=np.float32)
    ms = native.DecoderConfig(variant=native.NMS, alpha=1.25, T=5)
    gd = native.GdbfConfig(T=T)                                        # SMNGDBF: NOISE
    gq = native.GdbfConfig(T=T, flags=native.GDBF_VARIANTS["StochasticNGDBF"], qsigma=0.0)
    rg = native.RgdbfConfig(T=T, maxphase=2)
    rs = native.RstatConfig(T=T, attempts=ATT)
    hw = native.HwGdbfConfig(T=T, maxphase=2, qlen=QLEN)
    em = native.EmsConfig(T=2, nm=16)
    out = {}

    def sim_args(kw, cfg):
        a = dict(SIM, cfg=cfg, c=h)
        a.update(kw)
        return (a["c"], a["ebn0"], a["R"], _ref(a["cfg"]), a["seed"], a["stream"], a["first"], a["batch"]), a

    def add(name, call, faults):
        for fault, kw in faults.items():
            if dev or kw.get("c", 0) is None:
                out[f"{name}:{fault}"] = (lambda call=call, kw=kw: call(**kw))

    def sim_faults(stream=True, **more):
        f = {"null_ctx": dict(c=None), "null_cfg": dict(cfg=None), "batch_0": dict(batch=0), "batch_9": dict(batch=9),
             "R_0": dict(R=0.0)}
        if stream:
            f["stream_id_2p20"] = dict(stream=1 << 20)
        f.update(more)
        return {k: v for k, v in f.items() if dev or k == "null_ctx"}

    def dec_faults(**more):
        f = {"null_ctx": dict(c=None), "null_y": dict(y=None), "null_cfg": dict(cfg=None), "batch_0": dict(batch=0),
             "batch_9": dict(batch=9)}
        f.update(more)
        return {k: v for k, v in f.items() if dev or k == "null_ctx"}

    # ---- min-sum family
    def ms_decode(c=h, y=f8, batch=2, cfg=ms):
        return L.ldpc_decode_batch(c, P(y), batch, _ref(cfg), None, None, None, None)

    def ms_launch(frames=None, **kw):
        a, _ = sim_args(kw, ms)
        return L.ldpc_sim_launch(*a, P(frames))

    def ms_batch(**kw):
        a, _ = sim_args(kw, ms)
        return L.ldpc_sim_batch(*a, None, None)

    def ms_trace(**kw):
        a, _ = sim_args(kw, ms)
        return L.ldpc_sim_trace(*a, None, None, None, None)

    def ms_info(c=h, cfg=ms):
        return L.ldpc_ctx_kernel_info(c, _ref(cfg), None, 0, None, None)

    add("ldpc_decode_batch", ms_decode, dec_faults(cfg_bad=dict(cfg=native.DecoderConfig(precision=2))))
    add("ldpc_sim_launch", ms_launch, sim_faults(stream=False, host_frames_dev=dict(frames=fr)))
    add("ldpc_sim_batch", ms_batch, sim_faults(stream=False))
    add("ldpc_sim_trace", ms_trace, sim_faults(stream=False))
    add("ldpc_ctx_kernel_info", ms_info, {"null_ctx": dict(c=None), "null_cfg": dict(cfg=None)} if dev
        else {"null_ctx": dict(c=None)})

    # ---- GDBF, re-decoding NGDBF: decode / sim_launch / sim_batch / kernel_info of one shape
    for fam, good, bad in (("gdbf", gd, native.GdbfConfig(flags=512)), ("rgdbf", rg, native.RgdbfConfig(T=0))):
        fn = {k: getattr(L, f"ldpc_{fam}_{k}") for k in ("decode_batch", "sim_launch", "sim_batch", "kernel_info")}

        def decode(c=h, y=f8, pert=pert, batch=2, cfg=good, fn=fn):
            return fn["decode_batch"](c, P(y), P(pert), batch, _ref(cfg), None, None, None, None)

        def launch(frames=None, good=good, fn=fn, **kw):
            a, _ = sim_args(kw, good)
            return fn["sim_launch"](*a, P(frames))

        def batch(good=good, fn=fn, **kw):
            a, _ = sim_args(kw, good)
            return fn["sim_batch"](*a, None, None)

        def info(c=h, cfg=good, fn=fn):
            return fn["kernel_info"](c, _ref(cfg), None, 0, None)

        more = dict(noise_without_pert=dict(pert=None), cfg_bad=dict(cfg=bad))
        if fam == "gdbf":
            more["qprob_qsigma_0"] = dict(cfg=gq)
        add(f"ldpc_{fam}_decode_batch", decode, dec_faults(**more))
        add(f"ldpc_{fam}_sim_launch", launch, sim_faults(host_frames_dev=dict(frames=fr), cfg_bad=dict(cfg=bad)))
        add(f"ldpc_{fam}_sim_batch", batch, sim_faults(cfg_bad=dict(cfg=bad)))
        add(f"ldpc_{fam}_kernel_info", info, {"null_ctx": dict(c=None), "null_cfg": dict(cfg=None), "cfg_bad": dict(cfg=bad),
                                              "null_cfg_no_ctx": dict(cfg=None, c=None),
                                              "cfg_bad_no_ctx": dict(cfg=bad, c=None)})

    # ---- every attempt of every frame
    def trace_of(a):
        return None if a is None else C.byref(native._RstatTrace(None, P(a), None, None))

    def rs_decode(c=h, y=f8, pert=pert, batch=2, cfg=rs):
        return L.ldpc_rstat_decode_batch(c, P(y), P(pert), batch, _ref(cfg), None, None, None, None, None, None)

    def rs_launch(frames=None, attempts=None, trace=None, **kw):
        a, _ = sim_args(kw, rs)
        return L.ldpc_rstat_sim_launch(*a, P(attempts), trace_of(trace), P(frames))

    def rs_batch(**kw):
        a, _ = sim_args(kw, rs)
        return L.ldpc_rstat_sim_batch(*a, None, None, None, None)

    def rs_trace(**kw):
        a, _ = sim_args(kw, rs)
        return L.ldpc_rstat_sim_trace(*a, None, None, None, None, None, None, None)

    def rs_info(c=h, cfg=rs):
        return L.ldpc_rstat_kernel_info(c, _ref(cfg), 0, None, 0, None)

    rbad = native.RstatConfig(attempts=0)
    past = dict(first=(1 << 32) - 1, batch=2)                           # first_cw + batch = 2^32 + 1
    add("ldpc_rstat_decode_batch", rs_decode, dec_faults(noise_without_pert=dict(pert=None), cfg_bad=dict(cfg=rbad)))
    add("ldpc_rstat_sim_launch", rs_launch,
        sim_faults(host_frames_dev=dict(frames=fr), host_attempts_dev=dict(attempts=att), host_trace=dict(trace=tr_host),
                   first_cw_past_2p32=past, cfg_bad=dict(cfg=rbad)))
    add("ldpc_rstat_sim_batch", rs_batch, sim_faults(first_cw_past_2p32=past, cfg_bad=dict(cfg=rbad)))
    add("ldpc_rstat_sim_trace", rs_trace, sim_faults(first_cw_past_2p32=past, cfg_bad=dict(cfg=rbad)))
    add("ldpc_rstat_kernel_info", rs_info, {"null_ctx": dict(c=None), "null_cfg": dict(cfg=None), "cfg_bad": dict(cfg=rbad),
                                            "null_cfg_no_ctx": dict(cfg=None, c=None),
                                            "cfg_bad_no_ctx": dict(cfg=rbad, c=None)})

    # ---- fixed-point NGDBF hardware model (its cfg check needs the context for N)
    def hw_decode(c=h, y=f8, q=q, qptr0=None, batch=2, cfg=hw):
        return L.ldpc_hwgdbf_decode_batch(c, P(y), P(q), P(qptr0), batch, _ref(cfg), None, None, None, None, None)

    def hw_launch(frames=None, **kw):
        a, _ = sim_args(kw, hw)
        return L.ldpc_hwgdbf_sim_launch(*a, P(frames))

    def hw_batch(**kw):
        a, _ = sim_args(kw, hw)
        return L.ldpc_hwgdbf_sim_batch(*a, None, None)

    def hw_trace(**kw):
        a, _ = sim_args(kw, hw)
        return L.ldpc_hwgdbf_sim_trace(*a, None, None, None, None, None)

    def hw_info(c=h, cfg=hw):
        return L.ldpc_hwgdbf_kernel_info(c, _ref(cfg), None, 0, None)

    short = native.HwGdbfConfig(T=T, maxphase=2, qlen=N)
    hw_more = dict(qlen_le_N=dict(cfg=short), reserved_nonzero=dict(cfg=_reserved(hw)))
    add("ldpc_hwgdbf_decode_batch", hw_decode,
        dec_faults(null_q=dict(q=None), qptr0_out_of_range=dict(qptr0=np.array([0, 7], dtype=np.int32)), **hw_more))
    add("ldpc_hwgdbf_sim_launch", hw_launch, sim_faults(host_frames_dev=dict(frames=fr), **hw_more))
    add("ldpc_hwgdbf_sim_batch", hw_batch, sim_faults(**hw_more))
    add("ldpc_hwgdbf_sim_trace", hw_trace, sim_faults(**hw_more))
    add("ldpc_hwgdbf_kernel_info", hw_info, {"null_ctx": dict(c=None), "null_cfg": dict(cfg=None),
                                             "null_cfg_no_ctx": dict(cfg=None, c=None),
                                             "reserved_nonzero_no_ctx": dict(cfg=_reserved(hw), c=None), **hw_more})

    # ---- EMS over GF(16)
    def em_decode(c=nh, y=ynb, batch=2, n0=0.5, cfg=em):
        return L.ldpc_ems_decode_batch(c, P(y), batch, n0, _ref(cfg), None, None, None, None)

    def em_sim(fn, tail):
        def call(frames=None, **kw):
            kw.setdefault("c", nh)
            a, _ = sim_args(kw, em)
            return fn(*a, *([P(frames)] if tail is None else tail))
        return call

    add("ldpc_ems_decode_batch", em_decode, dec_faults(n0_0=dict(n0=0.0), cfg_bad=dict(cfg=native.EmsConfig(nm=0))))
    add("ldpc_ems_sim_launch", em_sim(L.ldpc_ems_sim_launch, None),
        sim_faults(stream=False, host_frames_dev=dict(frames=fr), cfg_bad=dict(cfg=native.EmsConfig(nm=0))))
    add("ldpc_ems_sim_batch", em_sim(L.ldpc_ems_sim_batch, [None, None]), sim_faults(stream=False))
    add("ldpc_ems_sim_trace", em_sim(L.ldpc_ems_sim_trace, [None, None, None, None]), sim_faults(stream=False))
    add("ldpc_ems_kernel_info", lambda c=nh: L.ldpc_ems_kernel_info(c, None, 0, None), {"null_ctx": dict(c=None)})
    return out


def run(cases):
    """{case id: [status, message]}; every case must be a refusal."""
    L = native.lib()
    got = {}
    for name, thunk in cases.items():
        rc = thunk()
        got[name] = [rc, L.ldpc_last_error().decode(errors="replace") if rc else ""]
    return got


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _compare(got, want):
    assert all(rc < 0 for rc, _ in want.values())                      # the table holds refusals only
    assert sorted(got) == sorted(want)
    diff = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not diff, diff


def test_refusals_that_need_no_device():
    gold = _golden()
    host = table()
    assert len(host) >= 30
    _compare(run(host), {k: gold[k] for k in host})


@pytest.mark.gpu
def test_refusals_of_every_entry_point(gpu_ctx_factory):
    ctx = gpu_ctx_factory(PEG, 8)
    assert (ctx.graph.N, ctx.graph.M, ctx.max_batch) == (N, M, 8)
    nb = native.NbContext(native.NbGraph.from_alist(code_path(GF16)), 0, 8)
    before = ctx.read_counts().as_dict()
    gold = _golden()
    assert len(gold) >= 150
    _compare(run(table(ctx, nb)), gold)
    assert ctx.read_counts().as_dict() == before                        # nothing ran
