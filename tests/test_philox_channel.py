"""Every sample the kernels draw on the device against an independent restatement.

tests/philox_channel.py restates Philox4x32-10, the fp32 uniforms, Box-Muller and the counter
layout of every stream in numpy. The CPU tier pins that restatement: to the
CPU oracle's Philox (itself pinned to the Random123 known answers by test_oracle.py), to the
layout's injectivity, to the edges of the uniforms and to the Gaussian moments. The GPU tier
then recovers n = (y / c - 1) / sigma (or p / noise_sigma) from what each kernel returns and
compares every sample with the restatement's, for every channel site and every perturbation
draw, at seeds, streams and codeword numbers that use every bit of the counter and the key.

The tolerance is set from what the test must tell apart, not from what the kernels give:
|n_dev - n_ref| <= 2^-12 in units of one standard normal, plus 2^-22 |v| / scale for the
rounding of an fp32 output v. A sample from any other counter, key, round count or with cos
and sin swapped is an independent normal and lands in that window with probability about
2e-4; every sample is asserted, so no wrong stream passes. DESIGN.md §5a records what the
hardware log / sqrt / sin / cos actually deviate by (the module prints it, see MEASURED).

The gdbf.hip draws are pinned through two tests that exist: rstat attempt 0 equals rgdbf with
maxphase 1 frame by frame (test_rstat.test_philox_attempt_0_is_the_single_phase_decoder), and
rgdbf with maxphase 1 without WEIGHT equals gdbf_sim_batch of the same NOISE flags on the same
seed, frame by frame, on both kernels
(test_rgdbf.test_single_phase_without_weight_equals_gdbf); gdbf_rows equals gdbf_lds by
test_gdbf.test_gdbf_rows_kernel_equals_generic_kernel."""
import functools
import math

import numpy as np
import pytest

import philox_channel as P
import test_shape_matrix as SM
from conftest import code_path
from ldpcsimulation_amd import codes, native
from oracle import oracle as O

gpu = pytest.mark.gpu

KAT = [   # Random123 kat_vectors, philox4x32 10
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
     [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
]


# ------------------------------------------------------------------ CPU tier: the restatement
def test_philox_equals_the_oracle():
    """The three Random123 vectors, and 1,000 random counters and keys (a few words forced to
    0 and 2^32 - 1) against oracle/ldpc_oracle.c's orc_philox4x32_10."""
    for ctr, key, want in KAT:
        assert [int(x) for x in P.philox(*ctr, *key)] == want
        assert O.philox4x32_10(ctr, key) == want
    w = np.random.default_rng(2026).integers(0, 1 << 32, size=(1000, 6), dtype=np.uint64)
    w[:60] = np.where(np.arange(60)[:, None] % 6 == np.arange(6)[None, :], np.uint64(0), w[:60])
    w[60:120] = np.where(np.arange(60)[:, None] % 6 == np.arange(6)[None, :], np.uint64(P.M32), w[60:120])
    got = np.stack(P.philox(*w.T), axis=1)
    want = np.array([O.philox4x32_10(r[:4], r[4:]) for r in w.tolist()], dtype=np.uint64)
    assert np.array_equal(got, want)


def test_layout_keeps_the_streams_apart():
    """The draws of (stream s, cw), (s + 1, cw), (s, cw + 1), (s, cw + 2^32), the seed with bit
    32 flipped or its halves swapped, and perturbation rows 0, 1 and 4093 of the same (s, cw)
    share no sample. A perturbation's counter word 3 is at least 2^20, which no channel of
    stream_id < 2^20 has -- and the channel of the stream_id that equals that word is the same
    draw, so the refusal of stream_id >= 2^20 is what keeps the two apart."""
    N, seed, s, cw = 64, 0x00C0FFEE12345678, 5, 1000
    draws = {
        "base": P.channel_noise(seed, s, cw, 1, N)[0],
        "stream + 1": P.channel_noise(seed, s + 1, cw, 1, N)[0],
        "cw + 1": P.channel_noise(seed, s, cw + 1, 1, N)[0],
        "cw + 2^32": P.channel_noise(seed, s, cw + (1 << 32), 1, N)[0],
        "seed ^ 1 << 32": P.channel_noise(seed ^ (1 << 32), s, cw, 1, N)[0],
        "seed halves swapped": P.channel_noise(P.lo32(seed) << 32 | P.hi32(seed), s, cw, 1, N)[0],
    }
    for row in (0, 1, 4093):
        draws[f"perturbation row {row}"] = P.perturbation(seed, s, P.lo32(cw), P.hi32(cw), row, N, 1.0)
    names = list(draws)
    for i, a in enumerate(names):
        assert draws[a].shape == (N,) and np.isfinite(draws[a]).all()
        for b in names[:i]:
            assert not (draws[a] == draws[b]).any(), (a, b)
    assert np.array_equal(P.channel_noise(seed, s, cw, 3, N)[1], draws["cw + 1"])   # frame b of a batch is cw + b
    for stream in (0, 1, P.STREAM20):
        for row in (0, 1, 4093):
            word = int(P.perturbation_word(stream, row))
            assert word == stream | (row + 1) << 20 and 1 << 20 <= word <= P.M32
            assert np.array_equal(P.channel_noise(seed, word, cw, 1, N)[0],
                                  P.perturbation(seed, stream, P.lo32(cw), P.hi32(cw), row, N, 1.0))
    # the every-attempt decoders: attempt a of frame f draws what attempt 0 of frame f + (a << 32) draws
    assert P.rstat_words(cw, 2) == (P.lo32(cw + (2 << 32)), P.hi32(cw + (2 << 32)))
    # the NGDBFhw queue is perturbation row 0's word at counter word 0 = k // 4
    assert np.array_equal(P.hw_queue(seed, s, cw, 1, N, 0.5)[0], P.perturbation(seed, s, P.lo32(cw), P.hi32(cw), 0, N, 0.5))
    # the EMS channel: symbol v's four normals are group v of the binary channel's
    assert np.array_equal(P.ems_channel_noise(seed, s, cw, 2, N // 4), P.channel_noise(seed, s, cw, 2, N))


def test_codeword_table_row_is_taken_in_64_bits():
    """2^32 % 3 = 1: from first_cw = 2^32 - 3 the rows run 1, 2, 0, 1, 2; a 32-bit sum would
    start over at 0 after the boundary."""
    assert P.codeword_rows((1 << 32) - 3, 5, 3) == [1, 2, 0, 1, 2]
    c = np.array([[1, -1], [-1, 1], [-1, -1]])
    y = P.channel(3, 0, (1 << 32) - 3, 5, 2, 0.0, c)
    assert np.array_equal(y, c[[1, 2, 0, 1, 2]])


def test_uniforms_edges():
    """(0, 1] in fp32 with a round-to-nearest-even conversion; u = 2^32 - 1 gives r = 1 exactly
    and n = 0, u = 0 gives 2^-33 and the largest normal, sqrt(66 ln 2) = 6.764."""
    u = P.uniforms([0, 1, 0x01000001, 0x01000003, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFF])
    assert u.dtype == np.float32
    assert u[0] == np.float32(2.0 ** -33) and u[1] == np.float32(2.0 ** -32 + 2.0 ** -33)
    assert u[2] == np.float32(2.0 ** -8 + 2.0 ** -33) and u[3] == np.float32((2 ** 24 + 4) * 2.0 ** -32 + 2.0 ** -33)   # ties to even
    assert u[4] == np.float32(1 - 2.0 ** -24) and u[5] == 1.0 and u[6] == 1.0
    w = np.random.default_rng(5).integers(0, 1 << 32, size=200000, dtype=np.uint64)
    r = P.uniforms(w)
    assert (r > 0).all() and (r <= 1).all()
    ones, zeros = np.full(len(w), P.M32, dtype=np.uint64), np.zeros(len(w), dtype=np.uint64)
    assert not P.normals((w, ones, w[::-1], ones)).any()
    n = P.normals((w, zeros, w[::-1], zeros))
    assert np.isfinite(n).all() and np.abs(n).max() <= 6.77
    assert np.allclose(np.hypot(n[:, 0], n[:, 1]), math.sqrt(66 * math.log(2)), rtol=1e-12)
    assert np.isfinite(P.normals((zeros, w, ones, w))).all()


def gaussian_moments(n):
    """The assertions of test_gpu_parity.test_channel_noise_statistics."""
    m = n.size
    assert abs(n.mean()) < 5 / math.sqrt(m)
    assert abs(n.var() - 1) < 5 * math.sqrt(2 / m)
    for t in (1.0, 2.0, 3.0):
        p = math.erfc(t / math.sqrt(2))
        got = float((np.abs(n) > t).mean())
        assert abs(got - p) < 6 * math.sqrt(p * (1 - p) / m), (t, got, p)
    assert abs(np.corrcoef(n[:-1], n[1:])[0, 1]) < 5 / math.sqrt(m)


def test_restated_normals_are_gaussian():
    n = P.channel_noise(11, 0, 0, 512, 2048).ravel()
    assert n.size == 1 << 20
    gaussian_moments(n)
    assert abs(float(np.mean(n[0::4] * n[1::4]))) < 5 / math.sqrt(n.size / 4)   # the cos and sin of one radius


# ------------------------------------------------------------------ GPU tier: the comparison
CAP = 2.0 ** -12
PRECS = ("f64", "f32")
PREC = SM.PREC
W1944, PEG, R4000, C802, GF16 = ("80211n_1944_r12.alist", "PEGReg504x1008.alist", "4000.2000.4.244.alist",
                                 "802_3_H.alist", "gf16_N1000_dv2_dc4.alist")
BASE = dict(seed=0xC0FFEE123, stream_id=0x1234, first_cw=7)
# (site, precision) -> [largest |n_dev - n_ref|, the same in units of 2^-23 max(1, |n|), samples]; printed at the end
MEASURED = {}


@pytest.fixture(scope="module", autouse=True)
def report_measured():
    yield
    for (site, prec), (dev, ulps, count) in sorted(MEASURED.items()):
        print(f"\nmax deviation {site:<16} {prec}: {dev:.3e} = {ulps:8.2f} x 2^-23 max(1, |n|) over {count} samples", end="")
    if MEASURED:
        print()


def assert_normals(site, out, n_ref, scale, offset=1.0, c=None, drawn=None):
    """Every sample of `out` = c (offset + scale n), an array the device wrote in fp64 or fp32,
    against n_ref; drawn (a mask) leaves out rows the decoder never drew."""
    f32 = out.dtype == np.float32
    assert out.dtype == (np.float32 if f32 else np.float64) and out.shape == n_ref.shape, (site, out.shape, n_ref.shape)
    v = out.astype(np.float64)
    s = float(np.float32(scale)) if f32 else scale        # the kernels convert sigma to their precision once
    n_dev = ((v / c if c is not None else v) - offset) / s
    tol = CAP + (2.0 ** -22 * np.abs(v) / s if f32 else 0.0)
    dev = np.abs(n_dev - n_ref)
    ok = dev <= tol                                        # a NaN fails
    if drawn is not None:
        ok, dev = ok[drawn], dev[drawn]
        n_ref = n_ref[drawn]
    assert ok.size > 0, site
    m = MEASURED.setdefault((site, "f32" if f32 else "f64"), [0.0, 0.0, 0])
    m[0] = max(m[0], float(np.nanmax(dev)))
    m[1] = max(m[1], float(np.nanmax(dev / (2.0 ** -23 * np.maximum(1.0, np.abs(n_ref))))))
    m[2] += ok.size
    assert ok.all(), (f"{site}: {np.count_nonzero(~ok)} of {ok.size} samples are not the restatement's, "
                      f"the first at {np.argwhere(~ok)[0].tolist()}, largest deviation {np.nanmax(dev):.3g}")


@functools.lru_cache(maxsize=256)
def channel_ref(seed, stream_id, first_cw, batch, N):
    n = P.channel_noise(seed, stream_id, first_cw, batch, N)
    n.setflags(write=False)
    return n


class Site:
    """One place that draws on the device: prepare() selects its kernel and asserts
    kernel_info names it, draw() returns [(label, device output, n_ref, scale, offset, takes the
    codeword, mask of drawn rows or None)]."""
    stream_bits = 32
    batch = 5
    cw_limit = 1 << 64      # first_cw + batch may reach this

    def streams(self):
        return (0, 0xFFFFF) + ((0xFFFFFFFF,) if self.stream_bits == 32 else ())


class MinSumSite(Site):
    """Context.sim_trace: MS / BP / DD-BMP at T = 1."""

    def __init__(self, name, ctx, opts, cfg, batch=5, inreg=None):
        self.name, self.ctx, self.opts, self.cfg, self.batch, self.inreg = name, ctx, opts, cfg, batch, inreg
        self.sigma = P.sigma_of(1.0, 0.5)

    def prepare(self):
        self.ctx.reset_options()
        self.ctx.set_options(self.opts)
        info = self.ctx.kernel_info(self.cfg)
        assert info["kernel"] == self.name, (self.name, self.opts, info)
        if self.inreg is not None:
            assert self.ctx.pp_inreg_info(self.cfg)["inreg_bits"] == self.inreg

    def trace(self, seed, stream_id, first_cw, batch):
        return self.ctx.sim_trace(1.0, 0.5, self.cfg, seed, stream_id, first_cw, batch)

    def draw(self, seed, stream_id, first_cw, batch):
        y = self.trace(seed, stream_id, first_cw, batch)[0]
        return [("y", y, channel_ref(seed, stream_id, first_cw, batch, self.ctx.graph.N), self.sigma, 1.0, True, None)]


class RstatSite(Site):
    """rstat_sim_trace: y_out and pert_out of 3 attempts of T = 6 iterations."""
    stream_bits, batch, cw_limit = 20, 3, 1 << 32
    EBN0, RATE, T, ATTEMPTS = 3.0, 0.5, 6, 3

    def __init__(self, shape, ctx, prec, first_attempt=0):
        self.name, self.ctx = "rstat_" + shape, ctx
        self.cfg = native.RstatConfig(T=self.T, attempts=self.ATTEMPTS, first_attempt=first_attempt, noise_scale=0.8,
                                      precision=PREC[prec][0])
        self.sigma = P.sigma_of(self.EBN0, self.RATE)

    def prepare(self):
        self.ctx.reset_options()
        self.ctx.set_option("gdbf_kernel", "rows" if self.name == "rstat_rows" else "generic")
        assert self.ctx.rstat_kernel_info(self.cfg)["kernel"] == self.name

    def draw(self, seed, stream_id, first_cw, batch):
        N, cfg = self.ctx.graph.N, self.cfg
        y, pert, att, _, _, _, _ = self.ctx.rstat_sim_trace(self.EBN0, self.RATE, cfg, seed, stream_id, first_cw, batch)
        ref = np.empty((batch, cfg.attempts, cfg.T, N))
        for b in range(batch):
            for a in range(cfg.attempts):
                c1, c2 = P.rstat_words(first_cw + b, cfg.first_attempt + a)
                ref[b, a] = P.perturbation(seed, stream_id, c1, c2, np.arange(cfg.T), N, 1.0)
        drawn = np.arange(cfg.T)[None, None, :] < att["iters"][:, :, None]
        assert drawn.any() and not pert[~drawn].any()
        return [("y", y, channel_ref(seed, stream_id, first_cw, batch, N), self.sigma, 1.0, True, None),
                ("pert", pert, ref, self.sigma * cfg.noise_scale, 0.0, False, drawn)]


class HwSite(Site):
    """hwgdbf_sim_trace: y_out and the noise queue q_out."""
    stream_bits, batch = 20, 4
    EBN0, RATE = 3.75, 0.8413

    def __init__(self, kernel, ctx, prec):
        self.name, self.ctx = kernel, ctx
        self.cfg = native.HwGdbfConfig(T=2, precision=PREC[prec][0])
        self.sigma = P.sigma_of(self.EBN0, self.RATE)

    def prepare(self):
        self.ctx.reset_options()
        self.ctx.set_option("gdbf_kernel", 1 if self.name == "hwgdbf_wg" else 0)
        assert self.ctx.hwgdbf_kernel_info(self.cfg)["kernel"] == self.name

    def draw(self, seed, stream_id, first_cw, batch):
        y, q, _, _, _ = self.ctx.hwgdbf_sim_trace(self.EBN0, self.RATE, self.cfg, seed, stream_id, first_cw, batch)
        qref = P.hw_queue(seed, stream_id, first_cw, batch, self.cfg.qlen, 1.0)
        return [("y", y, channel_ref(seed, stream_id, first_cw, batch, self.ctx.graph.N), self.sigma, 1.0, True, None),
                ("q", q, qref, self.sigma * self.cfg.noise_scale, 0.0, False, None)]


class EmsSite(Site):
    """NbContext.sim_trace (fp32 only; the all-zero codeword)."""
    batch = 4

    def __init__(self, kernel, ctx):
        self.name, self.ctx, self.cfg = kernel, ctx, native.EmsConfig(T=1)
        self.sigma = P.sigma_of(1.5, 0.5)

    def prepare(self):
        assert self.ctx.kernel_info()["kernel"] == self.name

    def draw(self, seed, stream_id, first_cw, batch):
        y = self.ctx.sim_trace(1.5, 0.5, self.cfg, seed, stream_id, first_cw, batch)[0]
        return [("y", y, P.ems_channel_noise(seed, stream_id, first_cw, batch, self.ctx.graph.N), self.sigma, 1.0, False, None)]


def verify(site, seed, stream_id, first_cw, batch=None, table=None):
    """Draw once and compare every sample; table: a 0/1 codeword table the frames send rows of."""
    batch = batch or site.batch
    site.prepare()
    c = None
    if table is not None:
        site.ctx.set_codewords(table)
        c = (1 - 2 * table.astype(np.int8))[P.codeword_rows(first_cw, batch, len(table))]
    try:
        outs = site.draw(seed, stream_id, first_cw, batch)
    finally:
        if table is not None:
            site.ctx.set_codewords(None)
    for label, out, n_ref, scale, offset, coded, drawn in outs:
        assert_normals(site.name if label == "y" else f"{site.name} {label}", out, n_ref, scale, offset,
                       c if coded else None, drawn)
    return outs


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    """Contexts of test_shape_matrix's synthetic codes (max_batch 64)."""
    assert native.device_count() > 0, "no HIP device visible"
    root = tmp_path_factory.mktemp("philox")

    @functools.lru_cache(maxsize=None)
    def make(name):
        path = str(root / f"{name}.alist")
        SM.build_code(path, name)
        return native.Context(native.Graph.from_alist(path), 0, 64)
    return make


@pytest.fixture(scope="module")
def nbctx():
    assert native.device_count() > 0, "no HIP device visible"

    @functools.lru_cache(maxsize=None)
    def make(kernel):
        if kernel == "ems_lds":
            g = native.NbGraph.from_alist(code_path(GF16))
        else:
            H = codes.peg_nb_code(2000, 1000, 2, 16, seed=3000)
            g = native.NbGraph.from_lists(H.N, H.M, H.q, H.cols, H.rows)
        return native.NbContext(g, 0, 64)
    return make


def minsum_sites(ctx, name, prec):
    """Every min-sum kernel selection of a synthetic code (test_shape_matrix.selections: the row
    kernels, lds, flood in both modes, global) and the two layered kernels, at T = 1."""
    sites = [MinSumSite(kernel, ctx, opts, SM.cfg_of(prec, "ms", 1)) for opts, kernel, _, _ in SM.selections(name, prec, "ms")]
    lay = SM.cfg_of(prec, "ms", 1, schedule=native.LAYERED)
    return sites + [MinSumSite("layered_lds", ctx, {}, lay), MinSumSite("layered_global", ctx, dict(kernel="global"), lay)]


def pp_site(ctx, prec):
    """The ping-pong kernel on N = 1944: fp64 with its 486 in-register bits (two codewords a
    step), fp32 pairs with every bit in LDS (four codewords a step); batches that leave slots
    of the last step empty."""
    cfg = native.DecoderConfig(variant=native.NMS, alpha=1.25, T=1, precision=PREC[prec][0])
    return MinSumSite("rows_pp", ctx, {}, cfg, batch=5 if prec == "f64" else 7, inreg=486 if prec == "f64" else 0)


def family_cfg(family, prec):
    if family == "bp":
        return native.DecoderConfig(variant=native.BP, T=1, precision=PREC[prec][0])
    return native.DecoderConfig(variant=native.DDBMP, T=1, precision=PREC[prec][0], quantize=True, ymax=1.0, qbits=3)


# ------------------------------------------------------------------ GPU tier: every site
TINY = ("dc8_cpt2_rpt1", "dc8_cpt4_rpt2", "dc8_cpt4_rpt1")   # N = 126, 1037, 252: two, one, no bit short in the last group


@gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", TINY)
def test_minsum_kernels(tiny, name, prec):
    """rows, rows_fast (fp32: the pair instance), lds, flood in both modes, global, layered_lds
    and layered_global; batch 5, so the fp32 pair kernels' last pair lacks its partner."""
    ran = []
    for site in minsum_sites(tiny(name), name, prec):
        verify(site, **BASE)
        ran.append(site.name)
    assert sorted(ran) == sorted(["rows", "rows_fast", "lds", "flood", "flood", "global", "layered_lds", "layered_global"])


@gpu
@pytest.mark.parametrize("prec,batches", [("f64", (5, 6)), ("f32", (7,))])
def test_ping_pong_kernel(gpu_ctx_factory, prec, batches):
    site = pp_site(gpu_ctx_factory(W1944, 64), prec)
    for batch in batches:
        verify(site, batch=batch, **BASE)


# (code, precision) -> {family: (kernel by default, kernel with the family's option at "generic")}
FAMILY_KERNELS = {
    ("dc16_cpt4_rpt1", "f64"): dict(bp=("bp_lds", "bp_lds"), ddbmp=("ddbmp_lds", "ddbmp_lds")),
    ("dc16_cpt4_rpt1", "f32"): dict(bp=("bp_lds", "bp_lds"), ddbmp=("ddbmp_lds", "ddbmp_lds")),
    (W1944, "f64"): dict(bp=("bp_rows", "bp_lds"), ddbmp=("ddbmp_rows", "ddbmp_lds")),
    (W1944, "f32"): dict(bp=("bp_rows", "bp_lds"), ddbmp=("ddbmp_rows", "ddbmp_lds")),
    (PEG, "f64"): dict(bp=("bp_rows", "bp_lds"), ddbmp=("ddbmp_rows", "ddbmp_lds")),
    (PEG, "f32"): dict(bp=("bp_rows", "bp_lds"), ddbmp=("ddbmp_rows", "ddbmp_lds")),
    (R4000, "f64"): dict(bp=("bp_global", "bp_global"), ddbmp=("ddbmp_rows", "ddbmp_global")),   # past 160 KB of LDS
}


def family_sites(ctx, code, prec):
    out = []
    for family, names in FAMILY_KERNELS[(code, prec)].items():
        for name, choice in zip(names, ("rows", "generic")):
            out.append(MinSumSite(name, ctx, {family + "_kernel": choice}, family_cfg(family, prec), batch=3 if code == R4000 else 5))
    return out


@gpu
@pytest.mark.parametrize("code,prec", list(FAMILY_KERNELS))
def test_bp_and_ddbmp_kernels(gpu_ctx_factory, tiny, code, prec):
    """Every kernel name BP and DD-BMP report: bp_lds / ddbmp_lds at row degree 16, the rows and
    lds kernels on N = 1944 and PEG, the global kernels on 4000.2000 in fp64."""
    ctx = tiny(code) if code.startswith("dc") else gpu_ctx_factory(code, 64)
    for site in family_sites(ctx, code, prec):
        verify(site, **BASE)


def rstat_sites(ctx, prec, first_attempt=0):
    return [RstatSite(shape, ctx, prec, first_attempt) for shape in ("rows", "wg")]


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_ngdbf_perturbations(gpu_ctx_factory, prec):
    """y_out and the drawn rows of pert_out of rstat_rows and rstat_wg (ngdbf_draw), attempts
    0..2 and 2..4 (the attempt in counter word 2)."""
    for first_attempt in (0, 2):
        for site in rstat_sites(gpu_ctx_factory(PEG, 64), prec, first_attempt):
            verify(site, **BASE)


def hw_sites(ctx, prec):
    return [HwSite(k, ctx, prec) for k in ("hwgdbf_wave", "hwgdbf_wg")]


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_ngdbfhw_channel_and_queue(gpu_ctx_factory, prec):
    for site in hw_sites(gpu_ctx_factory(C802, 64), prec):
        verify(site, **BASE)


@gpu
@pytest.mark.parametrize("kernel", ["ems_lds", "ems_global"])
def test_ems_channel(nbctx, kernel):
    verify(EmsSite(kernel, nbctx(kernel)), **BASE)


# ------------------------------------------------------------------ GPU tier: the edges of the counter and the key
SEEDS = (0, 0x00C0FFEE00000000, 0xFFFFFFFFFFFFFFFF)
FIRST_CWS = (0, (1 << 32) - 3, (1 << 40) + 5)    # the middle one: the batch crosses 2^32
EDGE_SITES = ["rows", "rows_fast", "rows_pp", "lds", "flood", "layered_lds", "bp_rows", "ddbmp_lds", "rstat_rows", "rstat_wg",
              "hwgdbf_wave", "hwgdbf_wg", "ems_lds"]


@pytest.fixture
def edge_site(gpu_ctx_factory, tiny, nbctx):
    def make(name, prec):
        if name == "ems_lds":
            return EmsSite(name, nbctx(name))
        if name == "rows_pp":
            return pp_site(gpu_ctx_factory(W1944, 64), prec)
        if name.startswith("rstat"):
            return [s for s in rstat_sites(gpu_ctx_factory(PEG, 64), prec) if s.name == name][0]
        if name.startswith("hwgdbf"):
            return [s for s in hw_sites(gpu_ctx_factory(C802, 64), prec) if s.name == name][0]
        if name in ("bp_rows", "ddbmp_lds"):
            return [s for s in family_sites(gpu_ctx_factory(PEG, 64), PEG, prec) if s.name == name][0]
        return [s for s in minsum_sites(tiny("dc8_cpt4_rpt1"), "dc8_cpt4_rpt1", prec) if s.name == name][0]
    return make


def edge_cases():
    return [(n, p) for n in EDGE_SITES for p in PRECS if not (n == "ems_lds" and p == "f64")]


@gpu
@pytest.mark.parametrize("name,prec", edge_cases())
def test_edges_of_seed_stream_and_codeword_number(edge_site, name, prec):
    """seed x stream_id x first_cw at the ends of their ranges. The every-attempt decoders keep
    the attempt in the high word of the codeword number and refuse first_cw + batch > 2^32
    (asserted here): their batch of 3 ends at 2^32 exactly."""
    site = edge_site(name, prec)
    for seed in SEEDS:
        for stream_id in site.streams():
            for first_cw in FIRST_CWS:
                if first_cw + site.batch <= site.cw_limit:
                    verify(site, seed, stream_id, first_cw)
                    continue
                site.prepare()
                with pytest.raises(native.LdpcError) as e:
                    site.draw(seed, stream_id, first_cw, site.batch)
                assert e.value.code == -1


@gpu
@pytest.mark.parametrize("name,prec", [c for c in edge_cases() if c[0] != "ems_lds"])
def test_codeword_table_across_the_32_bit_boundary(edge_site, name, prec):
    """Three rows of random bits from first_cw = 2^32 - 3: frames send rows 1, 2, 0, 1, 2."""
    site = edge_site(name, prec)
    table = np.random.default_rng(33).integers(0, 2, size=(3, site.ctx.graph.N), dtype=np.uint8)
    verify(site, 0x00C0FFEE00000000, 0xFFFFF, (1 << 32) - 3, table=table)


@gpu
@pytest.mark.parametrize("name,prec", edge_cases())
def test_frame_b_of_a_launch_is_frame_0_of_a_launch_b_later(edge_site, name, prec):
    site = edge_site(name, prec)
    first_cw = (1 << 32) - 3
    site.prepare()
    full = site.draw(7, 3, first_cw, site.batch)
    for b in range(site.batch):
        one = site.draw(7, 3, first_cw + b, 1)
        for (label, out, *_), (_, out1, *_) in zip(full, one):
            assert np.array_equal(out[b], out1[0]), (label, b)


@gpu
@pytest.mark.parametrize("name,prec", [(n, p) for n in ("rows", "rows_fast", "rows_pp") for p in PRECS])
def test_straight_line_channel_step_counts_what_the_traced_one_does(edge_site, name, prec):
    """sim_batch asks for no samples and, where N is a multiple of 4, takes the row kernels'
    straight-line channel step: a second copy of the counter. Its per-frame records (the uncoded
    errors are the signs of y) equal those of sim_trace, whose y is compared above, below 2^32,
    across it and past 2^40."""
    site = edge_site(name, prec)
    site.prepare()
    assert site.ctx.graph.N % 4 == 0
    for first_cw in FIRST_CWS:
        for batch in (6, 8):
            y, _, fr, cnt = site.trace(0x00C0FFEE00000000, 0xFFFFFFFF, first_cw, batch)
            fr2, cnt2 = site.ctx.sim_batch(1.0, 0.5, site.cfg, 0x00C0FFEE00000000, 0xFFFFFFFF, first_cw, batch)
            assert np.array_equal(fr["uncoded_bit_err"], (y <= 0).sum(axis=1)) and len(set(fr["uncoded_bit_err"])) > 1
            assert np.array_equal(fr, fr2) and np.array_equal(cnt.as_array(), cnt2.as_array()), (first_cw, batch)


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_every_binary_family_draws_the_same_channel(gpu_ctx_factory, prec):
    """y of flooding min-sum (the default kernel, lds, flood, global), layered min-sum, BP and
    DD-BMP on both of their kernels, for one (seed, stream_id, first_cw, precision): equal."""
    ctx = gpu_ctx_factory(W1944, 64)
    ms = native.DecoderConfig(T=1, precision=PREC[prec][0])
    lay = native.DecoderConfig(T=1, precision=PREC[prec][0], schedule=native.LAYERED)
    sites = [pp_site(ctx, prec), MinSumSite("lds", ctx, dict(kernel="lds"), ms), MinSumSite("flood", ctx, dict(kernel="flood"), ms),
             MinSumSite("global", ctx, dict(kernel="global"), ms), MinSumSite("layered_lds", ctx, {}, lay),
             MinSumSite("layered_global", ctx, dict(kernel="global"), lay)] + family_sites(ctx, W1944, prec)
    ys = []
    for site in sites:
        site.prepare()
        ys.append(site.trace(0xFFFFFFFFFFFFFFFF, 0xFFFFF, (1 << 32) - 3, 5)[0])
    for site, y in zip(sites[1:], ys[1:]):
        assert np.array_equal(y, ys[0]), site.name
    ctx.reset_options()


@gpu
def test_gdbf_families_refuse_stream_ids_of_more_than_20_bits(gpu_ctx_factory):
    """Counter word 3 holds the perturbation row above bit 20: stream_id = 2^20 is LDPC_ERR_INVALID
    in every family that draws perturbations; 2^20 - 1 runs."""
    ctx = gpu_ctx_factory(PEG, 64)
    ctx.reset_options()
    calls = {
        "gdbf": lambda s: ctx.gdbf_sim_batch(3.0, 0.5, native.GdbfConfig(T=2), 1, s, 0, 4),
        "rgdbf": lambda s: ctx.rgdbf_sim_batch(3.0, 0.5, native.RgdbfConfig(T=2, maxphase=2), 1, s, 0, 4),
        "rstat": lambda s: ctx.rstat_sim(3.0, 0.5, native.RstatConfig(T=2, attempts=2), 1, s, 0, 4),
        "hwgdbf": lambda s: ctx.hwgdbf_sim_batch(3.0, 0.5, native.HwGdbfConfig(T=2), 1, s, 0, 4),
    }
    for name, call in calls.items():
        call((1 << 20) - 1)
        for stream_id in (1 << 20, 0xFFFFFFFF):
            with pytest.raises(native.LdpcError) as e:
                call(stream_id)
            assert e.value.code == -1, name
