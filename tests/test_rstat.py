"""The every-attempt decoders (ldpc_rstat_*; rstat.hip) on the GPU against their numpy
restatement (tests/rstat_oracle.py, itself pinned to the reference's recorded
redecodeStatistics and replayGDBF runs by tests/test_rstat_oracle.py) and against the
re-decoding kernels where the two coincide (attempt 0 is ldpc_rgdbf_sim_* with maxphase 1).

Option gdbf_kernel picks the shape as it does for ldpc_rgdbf_*: 0 = rstat_rows where the code
fits (the codes rgdbf_rows takes; 802.3 with row degree 32 does not), 1 = rstat_wg; every test
asserts that kernel_info names the kernel meant. Equality is exact everywhere, in fp64 and in
fp32 (each against the restatement in the same arithmetic). The given-noise inputs are the
recorded runs' frames, drawn in the reference's order: the rows of iterations that did not run
are zero."""
import numpy as np
import pytest

import rstat_oracle as SO
from ldpcsimulation_amd import native

pytestmark = pytest.mark.gpu

PEG, W1944, E8023, R4000 = "PEGReg504x1008.alist", "80211n_1944_r12.alist", "802_3_H.alist", "4000.2000.4.244.alist"
PREC = {"f64": (native.F64, np.float64), "f32": (native.F32, np.float32)}
SHAPES = ("rows", "wg")
ROWS = {PEG: "rstat_rows", W1944: "rstat_rows", E8023: "rstat_wg", R4000: "rstat_rows"}   # what option 0 gives
RUNS, REPLAYS = SO.golden()
RUN = {r["code"] if not r["cwfile"] else "cw": r for r in RUNS}
ATT_KEYS = ("bit_err", "iters", "syndrome_fail", "smoothing_used")


def cfg_of(prec, kw, attempts, **more):
    base = dict(flags=kw["flags"], T=kw["T"], attempts=attempts, theta=kw["theta"], lambda_=kw["lambda_"],
                alpha=kw["alpha"], ymax=kw["ymax"], windowsize=kw["windowsize"], precision=PREC[prec][0])
    base.update(more)
    return native.RstatConfig(**base)


def pick(ctx, shape, code, cfg, trace=False):
    """Set the kernel option and check that kernel_info names the kernel meant."""
    ctx.set_option("gdbf_kernel", shape if shape == "rows" else "generic")
    info = ctx.rstat_kernel_info(cfg, with_trace=trace)
    assert info["kernel"] == (ROWS[code] if shape == "rows" and not trace else "rstat_wg"), info
    return info


def both_outcomes(out):
    """The batch holds an attempt that ends with outcome 0 and one with outcome > 0: the early
    stop and the smoothed output both run."""
    o = out["attempts_out"][:, :, 0]
    assert (o == 0).any() and (o > 0).any(), o


def check_given(ctx, out, cfg, c=None, trace=False):
    att, d, fr, cnt, tr = ctx.rstat_decode(out["y"], out["pert"], cfg, c=c, want_trace=trace)
    want = out["attempts_out"]
    for k, key in enumerate(ATT_KEYS):
        assert np.array_equal(np.asarray(att[key], dtype=np.int64), want[:, :, k]), (key, att[key], want[:, :, k])
    assert np.array_equal(d, out["d"])
    for key in ("bit_err", "uncoded_bit_err", "syndrome_fail", "iters"):
        assert np.array_equal(np.asarray(fr[key], dtype=np.int64), out["frames"][key]), key
    f, n = out["frames"], cnt.as_dict()
    assert n == dict(bit_err=int(f["bit_err"].sum()), frame_err=int((f["bit_err"] > 0).sum()),
                     uncoded_bit_err=int(f["uncoded_bit_err"].sum()), frames=len(out["y"]), iters=int(f["iters"].sum()),
                     syndrome_fail=int(f["syndrome_fail"].sum())), n
    return tr


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("code", [PEG, W1944, E8023])
def test_given_noise_equals_restatement(gpu_ctx_factory, code, prec, shape):
    """The recorded runs: PEG 3.0 dB T 50 NR 6, N = 1944 4.0 dB T 100 NR 5 (column degree 11),
    802.3 3.6 dB T 100 NR 5 (row degree 32)."""
    run = RUN[code]
    _, _, _, attempts, _, kw = SO.run_config(run)
    out = SO.replay_run(run, PREC[prec][1])
    both_outcomes(out)
    ctx = gpu_ctx_factory(code)
    cfg = cfg_of(prec, kw, attempts)
    pick(ctx, shape, code, cfg)
    check_given(ctx, out, cfg)


def test_given_noise_in_a_global_slot(gpu_ctx_factory):
    """4000.2000 in fp64 is past 64 KB of LDS per attempt: rstat_wg keeps its state in a global
    slot (and rstat_rows, which takes the code, in registers). 1 frame x 2 attempts at T 20;
    4.0 dB and glibc seed 9 give one attempt that stops at iteration 17 and one that fails."""
    code = SO.code_of(R4000)
    kw = dict(T=20, theta=-0.6, lambda_=0.99, alpha=1.2, windowsize=16, ymax=2.5, flags=SO.ALL)
    out = SO.glibc_run(code, 0.5, 4.0, 0.75, 9, 1, 2, **kw)
    both_outcomes(out)
    ctx = gpu_ctx_factory(R4000)
    cfg = cfg_of("f64", kw, 2)
    for shape in SHAPES:
        info = pick(ctx, shape, R4000, cfg)
        assert (info["lds_bytes"] == 0) == (shape == "wg"), info
        check_given(ctx, out, cfg)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("frames,attempts", [(1, 6), (7, 3), (13, 2)])
def test_given_noise_batch_sizes(gpu_ctx_factory, frames, attempts, prec, shape):
    """Batches of 1, 7 and 13 frames of the PEG run's stream."""
    R, snr, ns, _, _, kw = SO.run_config(RUN[PEG])
    out = SO.glibc_run(SO.code_of(PEG), R, snr, ns, 5, frames, attempts, dtype=PREC[prec][1], **kw)
    both_outcomes(out)
    ctx = gpu_ctx_factory(PEG)
    cfg = cfg_of(prec, kw, attempts)
    pick(ctx, shape, PEG, cfg)
    check_given(ctx, out, cfg)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_given_noise_with_codewords(gpu_ctx_factory, prec, shape):
    """The recorded run with PEGReg504x1008_data20.enc: frame f sends the file's line f."""
    run = RUN["cw"]
    _, _, _, attempts, _, kw = SO.run_config(run)
    out = SO.replay_run(run, PREC[prec][1])
    both_outcomes(out)
    assert (out["c"] < 0).any()
    ctx = gpu_ctx_factory(PEG)
    cfg = cfg_of(prec, kw, attempts)
    pick(ctx, shape, PEG, cfg)
    check_given(ctx, out, cfg, c=out["c"])


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_given_noise_with_the_window_open_from_the_start(gpu_ctx_factory, prec, shape):
    """windowsize > T: it > T - windowsize holds from iteration 0, so dsum sums every iteration."""
    R, snr, ns, _, _, kw = SO.run_config(RUN[PEG])
    kw = dict(kw, windowsize=kw["T"] + 10)
    out = SO.glibc_run(SO.code_of(PEG), R, snr, ns, 5, 4, 4, dtype=PREC[prec][1], **kw)
    both_outcomes(out)
    assert (out["attempts_out"][:, :, 3] == 1).all()      # every attempt ends inside the window
    ctx = gpu_ctx_factory(PEG)
    cfg = cfg_of(prec, kw, 4)
    pick(ctx, shape, PEG, cfg)
    check_given(ctx, out, cfg)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("which", [0, 1])
def test_traces_equal_the_restatement(gpu_ctx_factory, which, prec):
    """The recorded replays of a PEG frame and a 1944 frame through rstat_wg: the four traces
    equal the restatement's rows; every row past an attempt's iters is -1 / 0."""
    run = REPLAYS[which]
    _, _, _, attempts, _, kw = SO.run_config(run)
    out = SO.replay_run(run, PREC[prec][1])
    both_outcomes(out)
    code = SO.code_of(run["code"])
    ctx = gpu_ctx_factory(run["code"])
    cfg = cfg_of(prec, kw, attempts)
    pick(ctx, "rows", run["code"], cfg, trace=True)        # a trace forces rstat_wg
    tr = check_given(ctx, out, cfg, trace=True)
    want = code.traces(out["att"], kw["T"])
    for key in ("err_trace", "unsat_trace", "d_trace", "s_trace"):
        assert np.array_equal(tr[key], want[key]), key
    it = out["attempts_out"][0, :, 1]
    assert (it < kw["T"]).any()
    for a in range(attempts):
        assert (tr["err_trace"][0, a, it[a]:] == -1).all() and (tr["unsat_trace"][0, a, it[a]:] == -1).all()
        assert not tr["d_trace"][0, a, it[a]:].any() and not tr["s_trace"][0, a, it[a]:].any()
        assert (tr["err_trace"][0, a, :it[a]] >= 0).all() and (tr["unsat_trace"][0, a, :it[a]] > 0).all()


def test_an_attempt_satisfied_at_its_first_check_has_no_row(gpu_ctx_factory):
    """At 12 dB the channel decision of the frame is a codeword: no iteration runs, no row."""
    R, _, ns, _, _, kw = SO.run_config(RUN[PEG])
    out = SO.glibc_run(SO.code_of(PEG), R, 12.0, ns, 5, 1, 2, **kw)
    assert (out["attempts_out"][:, :, 1] == 0).all()
    ctx = gpu_ctx_factory(PEG)
    cfg = cfg_of("f64", kw, 2)
    pick(ctx, "wg", PEG, cfg, trace=True)
    tr = check_given(ctx, out, cfg, trace=True)
    assert (tr["err_trace"] == -1).all() and (tr["unsat_trace"] == -1).all()
    assert not tr["d_trace"].any() and not tr["s_trace"].any()


def rgdbf_cfg(cfg):
    return native.RgdbfConfig(flags=cfg.flags, T=cfg.T, maxphase=1, theta=cfg.theta, lambda_=cfg.lambda_, alpha=cfg.alpha,
                              noise_scale=cfg.noise_scale, ymax=cfg.ymax, windowsize=cfg.windowsize,
                              precision=cfg.precision)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("code,snr,R", [(PEG, 3.0, 0.5), (E8023, 3.6, 0.8125)])
def test_philox_attempt_0_is_the_single_phase_decoder(gpu_ctx_factory, code, snr, R, prec, shape):
    """Attempt 0 of rstat_sim equals rgdbf_sim_batch with maxphase 1, frame by frame."""
    _, _, _, _, _, kw = SO.run_config(RUN[code])
    ctx = gpu_ctx_factory(code)
    cfg = cfg_of(prec, kw, 3, noise_scale=0.8)
    pick(ctx, shape, code, cfg)
    att, fr, cnt, _ = ctx.rstat_sim(snr, R, cfg, seed=41, stream_id=3, first_cw=77, batch=64)
    ref, _ = ctx.rgdbf_sim_batch(snr, R, rgdbf_cfg(cfg), seed=41, stream_id=3, first_cw=77, batch=64)
    for key in ("bit_err", "iters", "syndrome_fail"):
        assert np.array_equal(att[key][:, 0], ref[key]), key
    assert np.array_equal(fr["uncoded_bit_err"], ref["uncoded_bit_err"])
    assert (ref["iters"] < cfg.T).any() and (ref["iters"] == cfg.T).any()
    # the other attempts draw other noise: some frame's outcome differs from attempt 0's
    assert (att["iters"][:, 1] != att["iters"][:, 0]).any()
    assert np.array_equal(fr["iters"], att["iters"].sum(axis=1)) and np.array_equal(fr["bit_err"], att["bit_err"][:, -1])
    assert cnt.as_dict()["frames"] == 64 and cnt.as_dict()["iters"] == int(att["iters"].sum())


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_philox_samples_replay_through_the_given_path(gpu_ctx_factory, prec, shape):
    """y_out / pert_out of rstat_sim_trace, fed to rstat_decode and to the restatement, give
    rstat_sim's attempts_out, attempts >= 1 included; rows that were not drawn are zero."""
    R, snr, _, _, _, kw = SO.run_config(RUN[PEG])
    ctx = gpu_ctx_factory(PEG)
    cfg = cfg_of(prec, kw, 3)
    pick(ctx, shape, PEG, cfg)
    att, fr, cnt, _ = ctx.rstat_sim(snr, R, cfg, seed=7, stream_id=1, first_cw=5, batch=6)
    y, pert, att2, d, fr2, cnt2, _ = ctx.rstat_sim_trace(snr, R, cfg, seed=7, stream_id=1, first_cw=5, batch=6)
    assert np.array_equal(att, att2) and np.array_equal(fr, fr2) and cnt.as_dict() == cnt2.as_dict()
    assert (att["bit_err"] == 0).any() and (att["bit_err"] > 0).any()
    for b in range(6):
        for a in range(3):
            n = att["iters"][b, a]
            assert not pert[b, a, n:].any() and pert[b, a, :n].any(axis=1).all()
    att3, d3, fr3, _, _ = ctx.rstat_decode(y, pert, cfg)
    assert np.array_equal(att, att3) and np.array_equal(d, d3) and np.array_equal(fr, fr3)
    out = SO.code_of(PEG).decode(y, pert, 3, dtype=PREC[prec][1], **kw)
    for k, key in enumerate(ATT_KEYS):
        assert np.array_equal(np.asarray(att[key], dtype=np.int64), out["attempts_out"][:, :, k]), key
    assert np.array_equal(d, out["d"])


@pytest.mark.parametrize("shape", SHAPES)
def test_philox_attempt_ranges_and_batch_splits(gpu_ctx_factory, shape):
    """Attempts [2, 5) through first_attempt equal that slice of a full run; a batch split into
    launches equals one launch."""
    R, snr, _, _, _, kw = SO.run_config(RUN[PEG])
    ctx = gpu_ctx_factory(PEG)
    full = cfg_of("f64", kw, 5)
    pick(ctx, shape, PEG, full)
    att, fr, cnt, _ = ctx.rstat_sim(snr, R, full, seed=11, stream_id=2, first_cw=100, batch=40)
    part = cfg_of("f64", kw, 3, first_attempt=2)
    att_p, fr_p, _, _ = ctx.rstat_sim(snr, R, part, seed=11, stream_id=2, first_cw=100, batch=40)
    assert np.array_equal(att_p, att[:, 2:5])
    assert np.array_equal(fr_p["iters"], att["iters"][:, 2:5].sum(axis=1))
    assert np.array_equal(fr_p["bit_err"], fr["bit_err"]) and np.array_equal(fr_p["uncoded_bit_err"], fr["uncoded_bit_err"])
    parts, acc = [], np.zeros(6, dtype=np.int64)
    for first, n in ((0, 1), (1, 12), (13, 27)):
        a, f, c, _ = ctx.rstat_sim(snr, R, full, seed=11, stream_id=2, first_cw=100 + first, batch=n)
        parts.append((a, f))
        acc += c.as_array()
    assert np.array_equal(np.concatenate([p[0] for p in parts]), att)
    assert np.array_equal(np.concatenate([p[1] for p in parts]), fr)
    assert np.array_equal(acc, cnt.as_array())


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("code,snr,R,frames", [(PEG, 3.0, 0.5, 64), (W1944, 4.0, 0.5, 64), (E8023, 3.6, 0.8125, 64),
                                               (PEG, 3.0, 0.5, 600)])
def test_the_two_shapes_agree(gpu_ctx_factory, code, snr, R, frames, prec):
    """64 frames x 8 attempts: per-attempt results, per-frame results and counters; and 600 x 8,
    more items than the persistent grid of rstat_rows holds, so that items go out by ticket."""
    _, _, _, _, _, kw = SO.run_config(RUN[code])
    ctx = gpu_ctx_factory(code)
    cfg = cfg_of(prec, kw, 8)
    res = {}
    for shape in SHAPES:
        pick(ctx, shape, code, cfg)
        att, fr, cnt, _ = ctx.rstat_sim(snr, R, cfg, seed=13, stream_id=4, first_cw=0, batch=frames)
        res[shape] = (att, fr, cnt.as_dict())
    a, b = res["rows"], res["wg"]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert (a[0]["bit_err"] == 0).any() and (a[0]["bit_err"] > 0).any()


def test_sim_launch_into_device_buffers(gpu_ctx_factory):
    import torch
    R, snr, _, _, _, kw = SO.run_config(RUN[PEG])
    ctx = gpu_ctx_factory(PEG)
    cfg = cfg_of("f64", kw, 4)
    att, fr, _, _ = ctx.rstat_sim(snr, R, cfg, seed=6, stream_id=0, first_cw=0, batch=32)
    adev = torch.empty((32, 4, 4), dtype=torch.int32, device="cuda:0")
    fdev = torch.empty((32, 4), dtype=torch.int32, device="cuda:0")
    ctx.rstat_sim_launch(snr, R, cfg, 6, 0, 0, 32, adev, fdev)
    ctx.synchronize()
    assert np.array_equal(adev.cpu().numpy().view(native.ATTEMPT_DTYPE).reshape(32, 4), att)
    assert np.array_equal(fdev.cpu().numpy().view(native.FRAME_DTYPE).reshape(-1), fr)
    for bad in (dict(stream_id=1 << 20, first_cw=0), dict(stream_id=0, first_cw=(1 << 32) - 31)):
        with pytest.raises(native.LdpcError) as e:
            ctx.rstat_sim_launch(snr, R, cfg, 6, bad["stream_id"], bad["first_cw"], 32, adev, fdev)
        assert e.value.code == -1
    with pytest.raises(native.LdpcError) as e:       # an asynchronous launch takes device pointers only
        ctx.rstat_sim_launch(snr, R, cfg, 6, 0, 0, 32, np.empty((32, 4), dtype=native.ATTEMPT_DTYPE), fdev)
    assert e.value.code == -1


def test_sim_launch_with_device_traces(gpu_ctx_factory):
    """The asynchronous launch writes the traces into device tensors: they equal rstat_sim's
    host traces, and rows that did not run hold -1 / 0 (the launch puts them there)."""
    import torch
    R, snr, _, _, _, kw = SO.run_config(RUN[PEG])
    ctx = gpu_ctx_factory(PEG)
    cfg = cfg_of("f64", kw, 3)
    g = ctx.graph
    att, fr, _, tr = ctx.rstat_sim(snr, R, cfg, seed=8, stream_id=2, first_cw=3, batch=5, want_trace=True)
    assert (att["iters"] < cfg.T).any() and (att["iters"] == cfg.T).any()
    shape = (5, 3, cfg.T)
    dev = {"err_trace": torch.full(shape, 7, dtype=torch.int32, device="cuda:0"),
           "unsat_trace": torch.full(shape, 7, dtype=torch.int32, device="cuda:0"),
           "d_trace": torch.full(shape + (g.N,), 7, dtype=torch.int8, device="cuda:0"),
           "s_trace": torch.full(shape + (g.M,), 7, dtype=torch.int8, device="cuda:0")}
    adev = torch.empty((5, 3, 4), dtype=torch.int32, device="cuda:0")
    ctx.rstat_sim_launch(snr, R, cfg, 8, 2, 3, 5, adev, None, trace_dev=dev)
    ctx.synchronize()
    assert np.array_equal(adev.cpu().numpy().view(native.ATTEMPT_DTYPE).reshape(5, 3), att)
    for key, t in dev.items():
        assert np.array_equal(t.cpu().numpy(), tr[key]), key
    only = {"unsat_trace": torch.full(shape, 7, dtype=torch.int32, device="cuda:0")}   # any subset
    ctx.rstat_sim_launch(snr, R, cfg, 8, 2, 3, 5, None, None, trace_dev=only)
    ctx.synchronize()
    assert np.array_equal(only["unsat_trace"].cpu().numpy(), tr["unsat_trace"])
    with pytest.raises(native.LdpcError) as e:       # host memory is refused
        ctx.rstat_sim_launch(snr, R, cfg, 8, 2, 3, 5, None, None, trace_dev={"err_trace": np.empty(shape, np.int32)})
    assert e.value.code == -1
