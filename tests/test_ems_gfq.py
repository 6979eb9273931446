"""Extended Min-Sum over GF(4) and GF(8) on the GPU (nb.hip k_ems<4, 2, ...> and <8, 3, ...>, and
the schedule-from-global instance ems_global_sched) against the CPU oracle (oracle/ems_oracle.c,
DESIGN.md §11), bit for bit: decided symbols, iteration counts, syndrome flags, error counts and
counters, on the smallest codes that reach each path and on the reference's own two codes
(SystemC/NB-LDPC/codes/GF4/q4.sp.9000.6000.4500.1 and GF8/q8.sp.6000.4000.3000.1)."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import ems_gfq_common as G
import philox_channel as P
import philox_channel_gfq as PQ
from conftest import ROOT, code_path
from oracle import oracle as O

REF = {4: "q4.sp.9000.6000.4500.1.alist", 8: "q8.sp.6000.4000.3000.1.alist"}
REF_KERNEL = {4: "ems_global_sched", 8: "ems_global"}
# What the oracle gives at T = 8, full vectors, early stop (eight frames at 2.0 dB): a run in which
# every frame stops, or every frame fails, exercises half the control flow.
MIX = {(8, 120): dict(iters=[8, 8, 8, 8, 4, 8, 2, 8], fails=6), (4, 90): dict(iters=[5, 8, 8, 4, 8, 8, 6, 8], fails=3),
       (8, 96): dict(fails=3), (4, 120): dict(fails=2), (4, 96): dict(fails=0)}


def _native():
    from ldpcsimulation_amd import native
    return native


def _ctx(H, max_batch=64):
    native = _native()
    return native.NbContext(native.NbGraph.from_lists(H.N, H.M, H.q, H.cols, H.rows), 0, max_batch)


def assert_mix(q, N, its, sf):
    want = MIX.get((q, N))
    if want is None:
        return
    assert int(sf.sum()) == want["fails"], (q, N, sf)
    if "iters" in want:
        assert its.tolist() == want["iters"], (q, N, its)
    if (q, N) == (4, 96):
        assert its.min() >= 3 and its.max() <= 7, its


# ------------------------------------------------------------------ CPU tier
@pytest.mark.parametrize("q,N", sorted(MIX))
def test_oracle_gives_the_mix_of_stopped_and_failed_frames(q, N):
    shape = [s for s in G.SHAPES if s[0] == N][0]
    H, A, y, n0 = G.small_case(*shape, q)
    _, its, sf = G.oracle_decode((shape, q), A, y, n0, 8, **G.ems_cfgs(q)[0])
    assert_mix(q, N, its, sf)
    assert {len(r) for r in H.rows} == {(96, 48, 2): {4}, (120, 40, 2): {6}, (90, 60, 3): {4, 5}}[shape]


def test_restated_channel_at_four_bits_is_the_gf16_one():
    a = PQ.ems_channel_noise(0xC0FFEE123, 0x1234, (1 << 32) - 2, 3, 50, 4)
    assert np.array_equal(a, P.ems_channel_noise(0xC0FFEE123, 0x1234, (1 << 32) - 2, 3, 50))
    for m in (2, 3):   # the first m normals of the same call, the others dropped
        n = PQ.ems_channel_noise(0xC0FFEE123, 0x1234, (1 << 32) - 2, 3, 50, m)
        assert n.shape == (3, 50 * m) and np.array_equal(n.reshape(3, 50, m), a.reshape(3, 50, 4)[:, :, :m])


def test_native_rejects_samples_of_the_wrong_width():
    """NbContext.decode sizes y as N * m; the check needs no device (it comes before the call)."""
    native = _native()
    H = G.peg_code(96, 48, 2, 8)
    ctx = native.NbContext.__new__(native.NbContext)
    ctx.graph = native.NbGraph.from_lists(H.N, H.M, H.q, H.cols, H.rows)
    assert ctx.graph.m == 3
    for shape in ((2, 96 * 4), (2, 96 * 2), (96 * 3 + 1,), (0, 96 * 3)):
        with pytest.raises(ValueError):
            ctx.decode(np.ones(shape, dtype=np.float32), 1.0, native.EmsConfig(T=1))
    with pytest.raises(ValueError):
        ctx.decode(np.ones((2, 96 * 3), dtype=np.float32), 1.0, native.EmsConfig(T=1), c=np.zeros((2, 95), dtype=np.uint8))


# ------------------------------------------------------------------ GPU tier
@pytest.mark.gpu
@pytest.mark.parametrize("shape", G.SHAPES, ids=["dc4", "dc8", "dv3_irregular", "more_symbols_padded_stride"])
@pytest.mark.parametrize("q", G.QS)
def test_exact_against_the_oracle(q, shape):
    native = _native()
    H, A, y, n0 = G.small_case(*shape, q)
    ctx = _ctx(H)
    assert ctx.kernel_info()["kernel"] == "ems_lds"
    for ci, cfg in enumerate(G.ems_cfgs(q)):
        for T in (0, 1, 3, 8):
            _, its, sf = G.assert_equals_oracle(native, ctx, A, (shape, q), y, n0, T, cfg)
            if ci == 0 and T == 8:
                assert_mix(q, shape[0], its, sf)


@pytest.mark.gpu
@pytest.mark.parametrize("q", G.QS)
def test_given_nonzero_codewords_accounting(q):
    native = _native()
    shape = (96, 48, 2)
    H, A, _, _ = G.small_case(*shape, q)
    m = A.m
    c = np.random.default_rng(9 + q).integers(0, q, size=(4, H.N), dtype=np.uint8)   # accounting only: any symbols
    y, n0 = G.frames(H.N, m, 4, 2.0, 11 + q, 0.5, c=c)
    ctx = _ctx(H)
    d, fr, cnt = ctx.decode(y, n0, native.EmsConfig(T=5, nm=q), c=c)
    want, its, _ = A.decode(y, n0, 5, nm=q)
    assert np.array_equal(d, want) and np.array_equal(fr["iters"], its)
    bits = lambda s: (s[:, :, None] >> np.arange(m)) & 1
    assert np.array_equal(fr["bit_err"], (bits(want) != bits(c)).sum(axis=(1, 2)))
    lam = np.stack([A.front(r, n0) for r in y]).reshape(4, H.N, m)
    unc = ((lam < 0) != bits(c)).sum(axis=(1, 2))
    assert np.array_equal(fr["uncoded_bit_err"], unc) and cnt.uncoded_bit_err == int(unc.sum())
    assert cnt.symbol_err == int((want != c).sum()) and cnt.frame_err == int((want != c).any(axis=1).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("q", G.QS)
def test_on_device_channel(q):
    from test_philox_channel import assert_normals
    native = _native()
    shape = (96, 48, 2)
    H, A, _, _ = G.small_case(*shape, q)
    ctx = _ctx(H, 4096)
    cfg = native.EmsConfig(T=8, nm=q)
    seed, stream_id, first_cw, batch = 0xC0FFEE123, 0x1234, (1 << 32) - 3, 8
    y, d, fr, cnt = ctx.sim_trace(2.0, 0.5, cfg, seed=seed, stream_id=stream_id, first_cw=first_cw, batch=batch)
    assert y.shape == (batch, H.N * A.m)
    assert_normals(f"ems_lds_gf{q}", y, PQ.ems_channel_noise(seed, stream_id, first_cw, batch, H.N, A.m), P.sigma_of(2.0, 0.5))
    n0 = 10 ** (-2.0 / 10) / 0.5
    want, its, sf = A.decode(y, n0, 8, nm=q)
    assert np.array_equal(d, want) and np.array_equal(fr["iters"], its) and np.array_equal(fr["syndrome_fail"], sf)
    # a launch of 300 frames is launches of 100 and 200
    full, _ = ctx.sim_batch(2.0, 0.5, cfg, seed=5, stream_id=0, first_cw=0, batch=300)
    a, _ = ctx.sim_batch(2.0, 0.5, cfg, seed=5, stream_id=0, first_cw=0, batch=100)
    b, _ = ctx.sim_batch(2.0, 0.5, cfg, seed=5, stream_id=0, first_cw=100, batch=200)
    assert np.array_equal(full, np.concatenate([a, b]))
    # more codewords than blocks: past the first grid they come from the ticket counter
    full, cf = ctx.sim_batch(2.0, 0.5, cfg, seed=8, stream_id=2, first_cw=0, batch=3000)
    a, ca = ctx.sim_batch(2.0, 0.5, cfg, seed=8, stream_id=2, first_cw=0, batch=1100)
    b, cb = ctx.sim_batch(2.0, 0.5, cfg, seed=8, stream_id=2, first_cw=1100, batch=1900)
    assert np.array_equal(full, np.concatenate([a, b]))
    assert cf.frames == 3000 and cf.iters == ca.iters + cb.iters and len(set(full["iters"].tolist())) > 3


@pytest.mark.gpu
@pytest.mark.parametrize("q,N", [(4, 5000), (8, 2500)])
def test_messages_beyond_lds(q, N):
    """A random regular (2, 4) code with a 256 KB message array: ems_global; equal to the oracle, and
    byte-equal with the plain layout and with 512 threads."""
    native = _native()
    H = G.random_nb_code([2] * N, [4] * (N // 2), q, seed=N + q)
    A = O.NbCode(H)
    y, n0 = G.frames(H.N, A.m, 2, 2.0, N + q, 0.5)
    ctx = _ctx(H, 8)
    info = ctx.kernel_info()
    assert info["kernel"] == "ems_global", info
    cfg = dict(nm=q, offset=0.0, early_stop=True)
    base = {}
    for T in (1, 4):
        G.assert_equals_oracle(native, ctx, A, ("global", q), y, n0, T, cfg)
        base[T] = ctx.decode(y, n0, native.EmsConfig(T=T, **cfg))
    for name, value in (("ems_swizzle", 1), ("ems_threads", 512)):
        other = _ctx(H, 8)
        other.set_option(name, value)
        assert other.kernel_info()["kernel"] == "ems_global"
        for T in (1, 4):
            d, fr, cnt = other.decode(y, n0, native.EmsConfig(T=T, **cfg))
            assert d.tobytes() == base[T][0].tobytes() and fr.tobytes() == base[T][1].tobytes(), (name, T)
            assert bytes(cnt) == bytes(base[T][2]), (name, T)


@pytest.mark.gpu
@pytest.mark.parametrize("q", G.QS)
def test_reference_codes(q):
    """The reference's own codes: the GF(4) code on the schedule-from-global instance (its tables
    exceed LDS), the GF(8) code on ems_global. Two frames at 3.0 dB: decoded within 20 iterations
    to the all-zero word as the oracle does, and symbol for symbol after 3 iterations, where the
    oracle has not converged."""
    native = _native()
    from ldpcsimulation_amd import codes
    H = codes.read_nb_alist(code_path(REF[q]))
    ctx = native.NbContext(native.NbGraph.from_alist(code_path(REF[q])), 0, 8)
    assert ctx.kernel_info()["kernel"] == REF_KERNEL[q]
    A = O.NbCode(H)
    y, n0 = G.frames(H.N, A.m, 2, 3.0, q, 1 - H.M / H.N)
    cfg = dict(nm=q, offset=0.0, early_stop=True)
    want, its, sf = G.assert_equals_oracle(native, ctx, A, ("ref", q), y, n0, 20, cfg)
    assert (want == 0).all() and (its < 20).all() and (sf == 0).all()
    want, its, sf = G.assert_equals_oracle(native, ctx, A, ("ref", q), y, n0, 3, cfg)
    assert (its == 3).all() and (sf == 1).all() and (want != 0).any()


@pytest.mark.gpu
def test_refusals():
    native = _native()
    for q in (2, 32):
        H = G.random_nb_code([2] * 24, [4] * 12, q, seed=q)
        g = native.NbGraph.from_lists(H.N, H.M, H.q, H.cols, H.rows)
        with pytest.raises(native.LdpcError) as e:
            native.NbContext(g, 0, 8)
        assert e.value.code == -4, e.value                       # LDPC_ERR_UNSUPPORTED
        assert all(w in str(e.value) for w in ("GF(4)", "GF(8)", "GF(16)", "q=%d" % q)), str(e.value)
    H = G.peg_code(96, 48, 2, 8)
    ctx = _ctx(H)
    with pytest.raises(ValueError):
        ctx.decode(np.ones((2, 96 * 4), dtype=np.float32), 1.0, native.EmsConfig(T=1))


@pytest.mark.gpu
def test_sweep_ems_on_a_gf8_alist(tmp_path):
    """sweep --ems on the q = 8 (96, 48) code: the point's totals are sim_batch's over the same frames
    (stream 0 of the seed, from frame 0)."""
    native = _native()
    from ldpcsimulation_amd import codes
    H = G.peg_code(96, 48, 2, 8)
    path, log = tmp_path / "gf8.alist", tmp_path / "ems.txt"
    path.write_text(codes.nb_alist_text(H))
    p = subprocess.run([sys.executable, "-m", "ldpcsimulation_amd.sweep", str(path), "--ems", "--rate", "0.5", "--snr", "2.0",
                        "-T", "8", "--nm", "8", "--batch", "512", "--seed", "3", "--max-frames", "2048", "--log", str(log),
                        "--json"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    js = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")][0]
    f = log.read_text().split("\t")
    assert len(f) == 8 and f[0] == "2" and f[4] == "8" and f[5] == "8"          # SNR BER avgIt FER T nm offset alist
    ctx = _ctx(H, 4096)
    fr, cnt = ctx.sim_batch(2.0, 0.5, native.EmsConfig(T=8, nm=8), seed=3, stream_id=0, first_cw=0, batch=js["frames"])
    assert js["frames"] > 0 and cnt.frames == js["frames"]   # the sweep stops at the frame that meets its stop rule
    assert (cnt.bit_err, cnt.frame_err, cnt.iters) == (js["bit_err"], js["frame_err"], js["iters"])
    assert 0 < cnt.frame_err < cnt.frames
