"""The ping-pong kernel's 12-wave block (rows_pp.hip k_rows_ppw: the 8 check waves of k_rows_ppi,
4 bit waves that each take the bit slots of two schedule threads, the channel of a plain step
spread over all 768 threads, the fixed-stride LDS layout with the slot in the instructions'
offset field and the check rows' LDS addresses kept in registers) computes what the 16-wave
k_rows_ppi (pp_slots=split_w16), the one-codeword kernel (rows64=fast) and the fp64 oracle
compute, on the 802.11n N=1944 code -- the bundled code with row pairs and both check-wave
shapes. Inputs, references and the premise-break construction are those of
tests/test_rows_pp_stream.py (shared, computed once).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import test_rows_pp_stream as S
from conftest import ROOT, code_path
from oracle import oracle as O

CODE = S.CODE
CHECKED = os.path.join(ROOT, "ldpcsimulation_amd", "lib", "checked", "libldpc_hip_checked.so")
# pp_slots value -> threads of the block that must run
SHAPES = {"split": 768, "split_w16": 1024}
# the fixed-stride layout (rows_pp.hip pp_slots FIX), restated: app[0], app[1] 16 KiB apart; behind them per slot a
# +0 word and a c2v array of at most 65520 bytes, slot 1's 65528 bytes behind slot 0's (a ds offset field holds 16
# bits); then red[] (240 ints)
APP_STRIDE, C2V_STRIDE, ZERO_WORD, RED_BYTES, LDS_MAX = 16384, 65520, 8, 240 * 4, 160 * 1024


def _set_shape(ctx, cfg, shape):
    ctx.set_option("rows64", "pp")
    ctx.set_option("pp_slots", shape)
    assert ctx.kernel_info(cfg)["kernel"] == "rows_pp"
    assert ctx.pp_inreg_info(cfg)["inreg_bits"] == 486
    assert ctx.pp_block_info(cfg)["threads"] == SHAPES[shape]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("vname", list(S.VARIANTS))
def test_w12_equals_rows_fast_and_oracle(gpu_ctx_factory, vname, shape):
    """Decisions, per-frame records, counters and the re-decode list on every frame: batches 5 and 6
    (the last step's slot 1 empty / full), T = 0..3, given samples and Philox noise."""
    from ldpcsimulation_amd import native
    ctx = gpu_ctx_factory(CODE)
    try:
        for source in ("given", "philox"):
            for batch in S.BATCHES:
                for T in S.TS:
                    (y0, d0, f0, c0, r0), want = S._reference(ctx, native, vname, source, batch, T)
                    cfg = native.DecoderConfig(T=T, precision=native.F64, **S.VARIANTS[vname])
                    _set_shape(ctx, cfg, shape)
                    y1, d1, f1, c1, r1 = S._run(ctx, cfg, source, batch)
                    at = f"{source} batch={batch} T={T}"
                    assert np.array_equal(y0, y1), at
                    assert np.array_equal(d1, d0) and np.array_equal(f1, f0), at
                    assert c1.as_dict() == c0.as_dict(), at
                    assert np.array_equal(r1, r0), at
                    assert int((d1 != want).sum()) == 0, at
                    w = (want != 1).sum(axis=1)
                    assert np.array_equal(f1["bit_err"], w), at
                    assert c1.frames == batch and c1.bit_err == int(w.sum()) and c1.iters == T * batch, at
                    assert c1.frame_err == int((w > 0).sum()), at
    finally:
        ctx.reset_options()


@pytest.mark.gpu
def test_w12_bit_role_remap_places_every_group(gpu_ctx_factory):
    """Frames of +1 samples with one strongly negative sample per group of 64 bits (another lane of
    the group in every frame): after one iteration the decisions differ from the all-positive
    frame's exactly around those bits, so a bit wave that took a wrong (wave, slot) -> group of the
    schedule, or wrote a sum to another bit, cannot reproduce the oracle's decisions."""
    from ldpcsimulation_amd import native
    ctx = gpu_ctx_factory(CODE)
    N, batch = 1944, 5
    y = np.ones((batch, N))
    for f in range(batch):
        for g in range((N + 63) // 64):
            v = 64 * g + (7 * g + 13 * f + 5) % 64
            if v < N:
                y[f, v] = -(2.5 + 0.25 * (g % 5))
    cfg = native.DecoderConfig(T=1, precision=native.F64, variant=native.NMS, alpha=1.25)
    want = S._alist().decode(y, 1, O.Cfg(variant=1, alpha=1.25), workers=8)
    assert (want == -1).any(axis=1).all() and (want == 1).any(axis=1).all()
    try:
        for shape in SHAPES:
            _set_shape(ctx, cfg, shape)
            d, fr, cnt = ctx.decode(y, cfg)
            assert ctx.redo_list().size == 0, shape
            assert int((d != want).sum()) == 0, shape
            assert np.array_equal(fr["bit_err"], (want != 1).sum(axis=1)), shape
    finally:
        ctx.reset_options()


@pytest.mark.gpu
def test_w12_channel_samples_do_not_depend_on_the_thread_that_draws_them(gpu_ctx_factory):
    """sim_trace's y of 5 frames at a non-zero first_cw, byte for byte: 768 threads draw a plain
    step's Philox groups in the 12-wave block, 512 in the 16-wave one; a trace step (samples
    written out) is drawn by the bit waves alone, 256 threads against 512."""
    from ldpcsimulation_amd import native
    ctx = gpu_ctx_factory(CODE)
    cfg = native.DecoderConfig(T=2, precision=native.F64, variant=native.NMS, alpha=1.25)
    got = {}
    try:
        for shape in SHAPES:
            _set_shape(ctx, cfg, shape)
            y, d, fr, cnt = ctx.sim_trace(1.5, 0.5, cfg, seed=4711, stream_id=3, first_cw=1000003, batch=5)
            fr2, cnt2 = ctx.sim_batch(1.5, 0.5, cfg, seed=4711, stream_id=3, first_cw=1000003, batch=5)[:2]
            # the plain step (no sample output) decodes the same samples: same per-frame records
            assert np.array_equal(np.asarray(fr2), np.asarray(fr)), shape
            got[shape] = (np.asarray(y), np.asarray(d), np.asarray(fr), cnt.as_dict())
    finally:
        ctx.reset_options()
    a, b = got["split"], got["split_w16"]
    assert a[0].dtype == np.float64 and a[0].shape == (5, 1944)
    assert a[0].tobytes() == b[0].tobytes()
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]


@pytest.mark.gpu
@pytest.mark.parametrize("frame", [2, 3], ids=["slot0", "slot1"])
@pytest.mark.parametrize("r", [0, 1], ids=["row0", "row1"])
def test_w12_premise_break_in_one_row_is_redecoded(gpu_ctx_factory, r, frame):
    """tests/test_rows_pp_stream.py's one-row break (every input below 2^1000, row r of one check
    thread past it at iteration 1) in an older-wave thread (5) and a younger-wave one (300), in a
    codeword of slot 0 and of slot 1: the re-decode list is that frame alone, as k_rows_fast lists
    it, and every frame equals k_rows_fast's and the oracle's."""
    from ldpcsimulation_amd import codes, native
    ctx = gpu_ctx_factory(CODE)
    H = codes.read_alist(code_path(CODE))
    v = S.VARIANTS["nms_fma"]
    cfg = native.DecoderConfig(T=2, precision=native.F64, **v)
    try:
        for t in (5, 300):
            _set_shape(ctx, cfg, "split")
            rows = S._thread_rows(ctx, cfg, H, t)
            y = S._given(6)
            y[frame] = S._one_row_break(H, y[frame], rows[r], rows[1 - r])
            assert np.abs(y).max() < S.BOUND
            assert S._premise_model(H, y[frame], 2, v) == [(1, rows[r])], t
            _, d1, f1, c1, r1 = S._run(ctx, cfg, "given", 6, y)
            assert r1.tolist() == [frame], t
            ctx.set_option("rows64", "fast")
            _, d0, f0, c0, r0 = S._run(ctx, cfg, "given", 6, y)
            assert r0.tolist() == [frame], t
            assert np.array_equal(d1, d0) and np.array_equal(f1, f0) and c1.as_dict() == c0.as_dict(), t
            want = S._alist().decode(y, 2, O.Cfg(**v), workers=8)
            assert int((d1 != want).sum()) == 0, t
    finally:
        ctx.reset_options()


def _e_pad(path):
    """Padded edge slots of the row schedule's bit layout (graph.cpp build_row_schedule): bits in
    decreasing degree, groups of 64, every group padded to its largest degree; at least N."""
    from ldpcsimulation_amd import codes
    H = codes.read_alist(path)
    deg = sorted((len(c) for c in H.cols), reverse=True)
    return H.N, max(H.N, 64 * sum(max(deg[i:i + 64]) for i in range(0, len(deg), 64)))


def _bytes(e_pad):
    return 2 * APP_STRIDE + 2 * ZERO_WORD + C2V_STRIDE + (e_pad + 64) * 8 + RED_BYTES


def _fits(N, e_pad):
    return ((N + 3) * 8 <= APP_STRIDE and (e_pad + 64) * 8 <= C2V_STRIDE
            and _bytes(e_pad) <= LDS_MAX)


def test_w12_support_rule_on_the_host():
    """No device: the layout rule (ldpc_pp_block_layout) holds exactly when both stride conditions
    and the 160 KB bound hold -- on the bundled codes and at each bound's edge."""
    from ldpcsimulation_amd import native
    shapes = {c: _e_pad(code_path(c)) for c in (CODE, "PEGReg504x1008.alist", "dvbs2_1_2.alist")}
    assert shapes[CODE] == (1944, 7232) and shapes["PEGReg504x1008.alist"][0] == 1008
    assert _fits(*shapes[CODE]) and _fits(*shapes["PEGReg504x1008.alist"]) and not _fits(*shapes["dvbs2_1_2.alist"])
    e_lds = (LDS_MAX - _bytes(0)) // 8   # the largest e_pad within 160 KB
    assert e_lds < C2V_STRIDE // 8 - 64      # the 160 KB bound binds before the offset field does
    cases = list(shapes.values()) + [(2045, 7232), (2046, 7232), (1944, e_lds), (1944, e_lds + 1),
                                     (1944, C2V_STRIDE // 8 - 64), (1944, C2V_STRIDE // 8 - 63), (0, 0)]
    for N, e_pad in cases:
        got = native.pp_block_layout(N, e_pad)
        assert got["fits"] == _fits(N, e_pad), (N, e_pad)
        assert got["launch_lds_bytes"] == _bytes(e_pad), (N, e_pad)
    assert native.pp_block_layout(*shapes[CODE]) == {"fits": True, "launch_lds_bytes": 157632}
    assert native.option_value("pp_slots", "split_w16") == 3


@pytest.mark.gpu
def test_w12_plan_picks_the_block_by_the_rule(gpu_ctx_factory):
    """The plan: 768 threads exactly where the in-register schedule runs and the layout holds the
    code (the bench code, fp64, pp_slots at its default), the 16-wave block otherwise; the reported
    decoder-state LDS does not move."""
    from ldpcsimulation_amd import native
    for code in (CODE, "PEGReg504x1008.alist", "dvbs2_1_2.alist"):
        ctx = gpu_ctx_factory(code)
        N, e_pad = _e_pad(code_path(code))
        for prec in (native.F64, native.F32):
            for slots in ("split", "split_w16", "split_lds", "plain"):
                ctx.reset_options()
                ctx.set_option("pp_slots", slots)
                cfg = native.DecoderConfig(T=3, precision=prec, variant=native.NMS, alpha=1.25)
                if ctx.kernel_info(cfg)["kernel"] != "rows_pp":
                    with pytest.raises(native.LdpcError):
                        ctx.pp_block_info(cfg)
                    continue
                bi, state = ctx.pp_block_info(cfg), ctx.kernel_info(cfg)["lds_bytes"]
                ii = ctx.pp_inreg_info(cfg)
                w12 = ii["inreg_bits"] > 0 and ii["slots_per_thread"] == 3 and slots == "split" and _fits(N, e_pad)
                assert bi["threads"] == (768 if w12 else 1024), (code, prec, slots)
                assert bi["launch_lds_bytes"] == (native.pp_block_layout(N, e_pad)["launch_lds_bytes"] if w12 else state)
                assert state == ctx.row_sched_info(cfg)["lds_bytes"]
        ctx.reset_options()
    ctx = gpu_ctx_factory(CODE)
    cfg = native.DecoderConfig(T=3, precision=native.F64, variant=native.NMS, alpha=1.25)
    assert ctx.pp_block_info(cfg) == {"threads": 768, "launch_lds_bytes": 157632}
    assert ctx.kernel_info(cfg)["lds_bytes"] == 148864


def run_cases(lib, out):
    """Child process: NMS, batch 5, T = 2, given samples and Philox noise with library `lib` on the
    12-wave block; results to `out` (npz)."""
    from ldpcsimulation_amd import native
    native.use_library(lib)
    ctx = native.Context(native.Graph.from_alist(code_path(CODE)), 0, 64)
    cfg = native.DecoderConfig(variant=native.NMS, alpha=1.25, T=2, precision=native.F64)
    info = [ctx.kernel_info(cfg)["kernel"], ctx.pp_inreg_info(cfg)["inreg_bits"], ctx.pp_block_info(cfg)["threads"]]
    res = {}
    for source in ("given", "philox"):
        y, d, fr, cnt, redo = S._run(ctx, cfg, source, 5)
        res[source + "__y"] = np.asarray(y)
        res[source + "__d"] = np.asarray(d)
        res[source + "__frames"] = np.asarray(fr).view(np.int32).reshape(len(fr), -1)
        res[source + "__counts"] = cnt.as_array()
        res[source + "__redo"] = np.asarray(redo)
    np.savez(out, **res)
    with open(out + ".json", "w") as f:
        json.dump(info, f)


def _child(lib, out):
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_rows_pp_w12 as t; "
            "t.run_cases(%r, %r)" % (ROOT, os.path.join(ROOT, "tests"), lib, out))
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)


@pytest.mark.gpu
def test_w12_checked_build_equals_product(tmp_path):
    """The bounds-checked library (`make checked`, check.h) on the 12-wave block: the gather and
    scatter addresses go through LDPC_CHK once, where they are formed, the bit waves' reads and
    writes at every access. No violation (an LdpcError would fail the child) and the product's
    results, as tests/test_pp_inreg_checked.py does for k_rows_ppi."""
    from ldpcsimulation_amd import native
    assert os.path.exists(CHECKED), "run `make checked`"
    a, b = str(tmp_path / "product.npz"), str(tmp_path / "checked.npz")
    pa = _child(native.LIB_PATH, a)
    assert pa.returncode == 0, pa.stderr[-3000:]
    pb = _child(CHECKED, b)
    assert pb.returncode == 0, pb.stderr[-3000:]
    assert json.load(open(a + ".json")) == json.load(open(b + ".json")) == ["rows_pp", 486, 768]
    ra, rb = np.load(a), np.load(b)
    assert sorted(ra.files) == sorted(rb.files)
    for k in ra.files:
        assert np.array_equal(ra[k], rb[k]), k
    assert ra["given__counts"][3] == 5 and ra["philox__counts"][3] == 5
