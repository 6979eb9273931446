"""In-register bits of the ping-pong kernel (rows_pp.hip k_rows_ppi, graph.h pp_pair_rows).

A degree-2 bit whose two check rows are the two rows of one check thread never passes
through LDS: the thread forms (yq + c2v_first) + c2v_second -- the bit node's sum in nlist
order, decodeMinSum.cpp:452-476 -- from its own registers, and the bit's decision, error
weight and syndrome share at the end. Every output must equal the same schedule with every
bit in LDS (pp_slots=split_lds, the kernel before this one), the one-codeword kernel
(rows64=fast) and the fp64 / fp32 oracle: sim_trace's (y, decisions, per-frame records) and
the counters, compared with np.array_equal.
"""
import numpy as np
import pytest

from conftest import code_path
from oracle import oracle as O

CODE = "80211n_1944_r12.alist"
NMS125 = dict(variant=1, alpha=1.25)


def _same(a, b, what):
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y), what
    assert a[3].as_dict() == b[3].as_dict(), what


def _trace(ctx, cfg, batch, ebn0=1.5):
    out = ctx.sim_trace(ebn0, 0.5, cfg, seed=91, stream_id=3, first_cw=17, batch=batch)
    return out, ctx.redo_count()


@pytest.mark.gpu
def test_bench_code_pairs_every_row_and_keeps_the_plan(gpu_ctx_factory):
    from ldpcsimulation_amd import native
    ctx = gpu_ctx_factory(CODE)
    ctx.reset_options()
    for prec in (native.F64, native.F32):
        cfg = native.DecoderConfig(T=50, precision=prec, **NMS125)
        assert ctx.kernel_info(cfg)["kernel"] == "rows_pp"
        if prec == native.F64:
            assert ctx.pp_inreg_info(cfg) == {"inreg_bits": 486, "lds_check_edges": 6400, "bit_slot_edges": 6208,
                                              "slots_per_thread": 3}
        else:   # fp32 pairs measured slower with in-register bits: they keep every bit in LDS
            assert ctx.pp_inreg_info(cfg) == {"inreg_bits": 0, "lds_check_edges": 7424, "bit_slot_edges": 7232,
                                              "slots_per_thread": 4}
        si = ctx.row_sched_info(cfg)   # still the split schedule it is derived from
        assert (si["e_pad"], si["dc_low"], si["issued_check_edges"], si["lds_bytes"]) == (7232, 7, 7424, 148864)
        for slots in ("split_lds", "plain"):
            ctx.set_option("pp_slots", slots)
            info = ctx.pp_inreg_info(cfg)
            assert info["inreg_bits"] == 0 and info["bit_slot_edges"] == 7232
            assert info["lds_check_edges"] == (7424 if slots == "split_lds" else 8192)
            assert ctx.kernel_info(cfg)["kernel"] == "rows_pp"
        ctx.reset_options()


@pytest.mark.gpu
@pytest.mark.parametrize("batch,T,v", [
    (515, 50, NMS125),
    (257, 7, dict(variant=2, delta=0.15)),
    (64, 1, dict(variant=1, alpha=1.1)),
    (3, 0, NMS125),
    (1, 13, dict(variant=0)),
])
def test_bench_code_fp64_equals_lds_schedule_fast_kernel_and_oracle(gpu_ctx_factory, batch, T, v):
    from ldpcsimulation_amd import native
    ctx = gpu_ctx_factory(CODE)
    ctx.reset_options()
    cfg = native.DecoderConfig(T=T, precision=native.F64, **v)
    assert ctx.pp_inreg_info(cfg)["inreg_bits"] == 486
    got, redo = _trace(ctx, cfg, batch)
    assert redo == 0
    ctx.set_option("pp_slots", "split_lds")
    lds, redo = _trace(ctx, cfg, batch)
    assert redo == 0
    ctx.reset_options()
    ctx.set_option("rows64", "fast")
    assert ctx.kernel_info(cfg)["kernel"] == "rows_fast"
    fast, _ = _trace(ctx, cfg, batch)
    ctx.reset_options()
    _same(got, lds, "split_lds")
    _same(got, fast, "rows_fast")
    n = min(batch, 64)
    want = O.Alist(code_path(CODE)).decode(got[0][:n], T, O.Cfg(**v), workers=16)
    assert int((got[1][:n] != want).sum()) == 0
    assert np.array_equal(got[2]["bit_err"][:n], (want != 1).sum(axis=1))


@pytest.mark.gpu
@pytest.mark.parametrize("batch,T,v", [(515, 50, NMS125), (3, 0, dict(variant=0))])
def test_bench_code_fp32_pairs_equal_lds_schedule_and_row_kernel(gpu_ctx_factory, batch, T, v):
    from ldpcsimulation_amd import native
    ctx = gpu_ctx_factory(CODE)
    ctx.reset_options()
    cfg = native.DecoderConfig(T=T, precision=native.F32, **v)
    assert ctx.pp_inreg_info(cfg)["inreg_bits"] == 0      # fp32 pairs keep every bit in LDS (measured slower otherwise)
    got, redo = _trace(ctx, cfg, batch)
    assert redo == 0
    ctx.set_option("pp_slots", "split_lds")
    lds, _ = _trace(ctx, cfg, batch)
    ctx.reset_options()
    ctx.set_option("rows32", "rows")
    assert ctx.kernel_info(cfg)["kernel"] == "rows"
    rows, _ = _trace(ctx, cfg, batch)
    ctx.reset_options()
    _same(got, lds, "split_lds")
    _same(got, rows, "rows")
    n = min(batch, 64)
    want = O.Alist(code_path(CODE)).decode(got[0][:n], T, O.Cfg(**v), workers=16)
    assert int((got[1][:n] != want).sum()) == 0


def _random_code(tmp_path, name, N, M, row_deg, seed, extra_bits=()):
    """tests/test_rows_pp.py's recipe -- a random code with the given row degrees in which every
    bit is in at least one check (the first N edge slots take a permutation of the bits, the rest
    random bits, redrawn on a duplicate within the row) -- plus bits N, N + 1, ... of degree 2:
    extra_bits[i] = the two rows of bit N + i."""
    from ldpcsimulation_amd import codes
    rng = np.random.default_rng(seed)
    assert sum(row_deg) >= N
    pool = list(rng.permutation(N)) + list(rng.integers(0, N, size=sum(row_deg) - N))
    rows, at = [], 0
    for j in range(M):
        r = []
        for _ in range(row_deg[j]):
            v = int(pool[at])
            at += 1
            while v in r:
                v = int(rng.integers(N))
            r.append(v)
        rows.append(sorted(r))
    for i, (a, b) in enumerate(extra_bits):
        rows[a].append(N + i)
        rows[b].append(N + i)
    path = str(tmp_path / name)
    codes.write_alist(codes.ParityCheck.from_rows(N + len(extra_bits), rows), path)
    return path


@pytest.mark.gpu
@pytest.mark.parametrize("low_rows", [False, True])
def test_random_code_with_a_few_pairs(tmp_path, low_rows):
    """950 random rows and 45 added degree-2 bits, most check threads without a pair (check waves
    that mix paired lanes with lanes holding real edges at the last position):
    rows 0..59 pair up as (0,1), (2,3), ...; rows 100..103 form a star (row 101 touches three
    degree-2 bits, one pairs); rows 200..219 are ten pairs with a degree-8 row, first in the
    bit's nlist (the lower row index) in five of them and second in the others; rows 300..304
    are a path of odd length. low_rows adds a degree-1 row and a degree-2 row whose edges are
    paired bits: their messages are +-inf, then NaN (tests/test_shape_matrix.py), so every
    frame is re-decoded on the exact path."""
    from ldpcsimulation_amd import native
    M, N0 = 950, 1800
    deg = [6] * M
    extra = [(2 * i, 2 * i + 1) for i in range(30)]
    deg[101] = 5
    extra += [(100, 101), (101, 102), (101, 103)]
    for i in range(10):
        a, b = 200 + 2 * i, 201 + 2 * i
        deg[a if i < 5 else b] = 7           # 7 + the added bit: degree 8
        extra.append((a, b))
    extra += [(300, 301), (301, 302), (302, 303), (303, 304)]
    if low_rows:
        deg[400], deg[402] = 0, 1
        extra += [(400, 401), (402, 403)]
    path = _random_code(tmp_path, "pairs.alist", N0, M, deg, seed=12, extra_bits=extra)
    ctx = native.Context(native.Graph.from_alist(path), 0, 128)
    cfg = native.DecoderConfig(T=20, precision=native.F64, **NMS125)
    assert ctx.kernel_info(cfg)["kernel"] == "rows_pp"
    info = ctx.pp_inreg_info(cfg)
    # 30 + 1 (the star) + 10 + 2 (the 5-row path) pairs at least; the random bits of degree 2 add more
    assert info["inreg_bits"] >= 43 + (2 if low_rows else 0), info
    got, redo = _trace(ctx, cfg, 96, ebn0=3.0)
    assert redo == (96 if low_rows else 0)
    ctx.set_option("pp_slots", "split_lds")
    assert ctx.pp_inreg_info(cfg)["inreg_bits"] == 0
    lds, redo_lds = _trace(ctx, cfg, 96, ebn0=3.0)
    assert redo_lds == redo
    _same(got, lds, "split_lds")
    want = O.Alist(path).decode(got[0][:64], 20, O.Cfg(**NMS125), workers=16)
    assert int((got[1][:64] != want).sum()) == 0
    assert np.array_equal(got[2]["bit_err"][:64], (want != 1).sum(axis=1))


@pytest.mark.gpu
def test_code_without_degree_2_bits_runs_the_lds_schedule(tmp_path):
    from ldpcsimulation_amd import native
    path = _random_code(tmp_path, "d8.alist", 1900, 950, [8] * 950, seed=8)
    g = native.Graph.from_alist(path)
    ctx = native.Context(g, 0, 128)
    cfg = native.DecoderConfig(T=10, precision=native.F64, **NMS125)
    assert ctx.kernel_info(cfg)["kernel"] == "rows_pp"
    assert ctx.pp_inreg_info(cfg)["inreg_bits"] == 0
    got, _ = _trace(ctx, cfg, 66, ebn0=3.0)
    ctx.set_option("pp_slots", "plain")
    plain, _ = _trace(ctx, cfg, 66, ebn0=3.0)
    _same(got, plain, "plain")


@pytest.mark.gpu
def test_given_samples_and_premise_breaks_at_in_register_bits(gpu_ctx_factory):
    """ctx.decode returns the in-register bits' decisions, and the premise-break frames of
    tests/test_rows_pp.py (1e305, 1e-305, inf, NaN, 2^995, -0.0), with the single bad samples
    also at in-register bit positions (bits 1053..1133 join block rows 0 and 1), equal the
    oracle; the re-decode list holds the same frames as with every bit in LDS."""
    from test_rows_pp import _glibc_frames
    from ldpcsimulation_amd import native
    ctx = gpu_ctx_factory(CODE)
    ctx.reset_options()
    N = ctx.graph.N
    y = _glibc_frames(N, 14, 1.5, 0.5, seed=4246)
    y[1] *= 1e305
    y[2] *= 1e-305
    y[3, 5] = np.inf
    y[4, 7] = np.nan
    y[5] *= 2.0 ** 995
    y[6, ::3] = -0.0
    y[7] = np.where(np.arange(N) % 2 == 0, 0.5, -1.0)
    y[8, 1060] = np.inf          # in-register bits
    y[9, 1133] = np.nan
    y[10, 1053:1134] = -0.0
    y[11, 1100] = 1e305
    y[12, 1101] = -np.inf
    A = O.Alist(code_path(CODE))
    for T in (0, 1, 7, 30):
        cfg = native.DecoderConfig(T=T, precision=native.F64, **NMS125)
        assert ctx.pp_inreg_info(cfg)["inreg_bits"] == 486
        d, fr, cnt = ctx.decode(y, cfg)
        redo = ctx.redo_count()
        ctx.set_option("pp_slots", "split_lds")
        d2, fr2, cnt2 = ctx.decode(y, cfg)
        redo2 = ctx.redo_count()
        ctx.reset_options()
        assert redo == redo2 and np.array_equal(d, d2) and np.array_equal(fr, fr2) and cnt.as_dict() == cnt2.as_dict()
        want = A.decode(y, T, O.Cfg(**NMS125), workers=8)
        mism = (d != want).sum(axis=1)
        assert int(mism.sum()) == 0, f"T={T}: mismatching frames {np.nonzero(mism)[0].tolist()}"
        assert np.array_equal(fr["bit_err"], (want != 1).sum(axis=1))
        assert redo >= 7      # frames 1, 3, 4, 8, 9, 11, 12 always


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_codeword_table_sample_output_and_sent_words(gpu_ctx_factory, prec):
    """Error weights against a sent word that is not all-zero: the in-register bits count
    d != c like every other bit. A codeword table of three rows (the library takes the rows
    as they are: one is the zero word, two are random words, so their frames do not
    converge) with the samples written out, in a batch whose last step has empty slots; and
    given samples with the sent words given."""
    from ldpcsimulation_amd import native
    ctx = native.Context(native.Graph.from_alist(code_path(CODE)), 0, 64)
    N = ctx.graph.N
    rng = np.random.default_rng(3)
    table = rng.integers(0, 2, size=(3, N)).astype(np.uint8)
    table[1] = 0
    ctx.set_codewords(table)
    P = native.F64 if prec == "f64" else native.F32
    other = ("rows64", "fast") if prec == "f64" else ("rows32", "rows")
    for T in (0, 6):
        cfg = native.DecoderConfig(T=T, precision=P, **NMS125)
        assert ctx.pp_inreg_info(cfg)["inreg_bits"] == (486 if prec == "f64" else 0)
        got, _ = _trace(ctx, cfg, 37)
        ctx.set_option("pp_slots", "split_lds")
        lds, _ = _trace(ctx, cfg, 37)
        ctx.reset_options()
        ctx.set_option(*other)
        ref, _ = _trace(ctx, cfg, 37)
        ctx.reset_options()
        _same(got, lds, "split_lds")
        _same(got, ref, other[1])
        assert got[3].bit_err > 0
        # the same frames as given samples with their sent words: first_cw 17, row (17 + b) % 3
        c = np.where(table[(17 + np.arange(37)) % 3] == 1, -1, 1).astype(np.int8)
        d, fr, cnt = ctx.decode(got[0], cfg, c=c)
        assert np.array_equal(d, got[1]) and np.array_equal(fr["bit_err"], got[2]["bit_err"])
        assert cnt.bit_err == got[3].bit_err
    ctx.set_codewords(None)
