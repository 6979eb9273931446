"""The host side of the workgroup-per-codeword kernel of layered fixed-point min-sum
(fxlms_wg.hip), without a GPU: the layer-at-a-time restatement the GPU tests use
(tests/fxlms_layer_oracle.py) against the row-serial one in the same order, the kernel instances
the library carries, the ABI that did not move, the launch planner (a stand-alone program under
AddressSanitizer and UBSan), and the sweep driver's --fx-kernel."""
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import fxlms_layer_oracle as LO
import fxlms_oracle as FL
from conftest import GOLD, ROOT, code_path
from ldpcsimulation_amd import native, sweep

PEG, W1944, C802, C4000, DVBS2 = ("PEGReg504x1008.alist", "80211n_1944_r12.alist", "802_3_H.alist", "4000.2000.4.244.alist",
                                  "dvbs2_1_2.alist")
BASE = [code_path(PEG), "--rate", "0.5", "--snr", "2.0", "-T", "20"]
LDS = 160 * 1024
RED = 256   # bytes of reduction and ticket words before the APPs (fxlms_layout.h kFxlmsWgRed)


# code, frames, sigma from..to, T, (variant, msg_bits, app_bits, num, shift, beta)
PINS = [(PEG, 8, (0.55, 0.95), 4, (FL.NMS, 8, 8, 3, 2, 0)), (PEG, 8, (0.55, 0.95), 4, (FL.OMS, 6, 7, 1, 0, 1)),
        (W1944, 8, (0.55, 0.95), 4, (FL.NMS, 8, 9, 3, 2, 0)), (C802, 8, (0.38, 0.60), 4, (FL.MS, 12, 13, 1, 0, 0)),
        (C802, 8, (0.38, 0.60), 4, (FL.NMS, 6, 6, 3, 2, 0)), (DVBS2, 2, (0.70, 0.85), 2, (FL.NMS, 8, 8, 3, 2, 0))]


@pytest.mark.parametrize("code,frames,sigma,T,cfg", PINS, ids=["%s-%d_%d_%d" % (p[0][:6], *p[4][:3]) for p in PINS])
def test_layer_restatement_equals_the_row_serial_one(code, frames, sigma, T, cfg):
    """Every decision after every iteration, the peaks before both clamps and the count of clamped
    values per iteration and frame, and the stop iteration. (The row-serial restatement returns
    no APPs: their signs after every iteration and the per-iteration peaks stand for them.)"""
    path = code_path(code)
    fx = LO.LayerFxlms(path)
    order, ptr = native.Graph.from_alist(path).layers()
    y = 1.0 + np.linspace(*sigma, frames)[:, None] * np.random.default_rng(23).standard_normal((frames, fx.N))
    Y = FL.front(y, 31 / 16, 5)
    variant, mb, ab, num, shift, beta = cfg
    a = fx.trajectory(Y, variant, T, mb, ab, num, shift, beta, order=order, ptr=ptr)
    b = FL.Fxlms.trajectory(fx, Y, variant, T, mb, ab, num, shift, beta, order=order)
    for k in b:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["dneg"][T], a["app"] <= 0) and np.abs(a["app"]).max() <= (1 << (ab - 1)) - 1
    assert b["clamped"][1:].sum() > 0 and (b["dneg"][T] != b["dneg"][0]).any()   # the clamps act, decisions move
    ra, rb = fx.result(a, T, True), fx.result(b, T, True)
    assert np.array_equal(ra["s"], rb["s"]) and np.array_equal(ra["d"], rb["d"]) and np.array_equal(ra["frames"], rb["frames"])


def test_library_carries_the_eight_instances_and_the_old_ones():
    syms = subprocess.run(["nm", "-C", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    got = sorted(set(re.findall(r"ldpc::k_fxlms_wg<([^>]*)>", syms)))
    assert got == sorted(f"{f}, {m}, {s}" for f in ("double", "float") for m in ("signed char", "short") for s in (0, 1)), got
    assert len(set(re.findall(r"ldpc::k_fxlms<([^>]*)>", syms))) == 16 and len(set(re.findall(r"ldpc::k_fxms<([^>]*)>", syms))) == 16


def test_abi_and_options_did_not_move():
    txt = open(os.path.join(ROOT, "include", "ldpc_hip.h")).read()
    assert "#define LDPC_ABI_VERSION 11" in txt and "#define LDPC_OPT_COUNT 23" in txt
    assert native.lib().ldpc_abi_version() == 11 and max(native.OPTIONS.values()) == 22
    assert "LDPC_OPT_KERNEL = 4" in txt and "fxlms_wg" in txt


def want_wg(N, M, dcs, app_bits):
    """fxlms_wg_plan and fxlms_wg_layout, restated."""
    wide = app_bits > 8
    need = RED + N * (2 if wide else 1)
    al = lambda x: (x + 255) & ~255
    s1 = al(4 * M)
    mg = s1 + (al(4 * M) if dcs > 26 else 0)
    slot = mg + al(M * (4 if wide else 2))
    if need > LDS:
        return ["-", 0, 0, 0, need, 0, 0, 1, 0, s1, mg, int(dcs > 26)]
    lds = (need + 15) & ~15
    threads = max(64, (1024 // (LDS // lds)) & ~63)
    return ["fxlms_wg_i16" if wide else "fxlms_wg_i8", threads, 1, lds, need, 0, 0, 1, slot, s1, mg, int(dcs > 26)]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_planner_under_asan_ubsan(tmp_path):
    """fxlms_wg_plan on the five test codes at both widths and on sizes at the LDS bound, the slot
    with and without S1; and the 75 recorded rows of the wave-per-codeword planners, which share
    its headers, unchanged."""
    exe, qfile = str(tmp_path / "fxlms_wg_plan_host"), str(tmp_path / "queries.txt")
    subprocess.run(["g++", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-std=c++17", "-I" + os.path.join(ROOT, "ldpcsimulation_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "native", "fxlms_wg_plan_host.cpp")],
                   check=True, capture_output=True, text=True)
    with open(os.path.join(GOLD, "wave_cw_choices.json")) as f:
        table = json.load(f)
    assert len(table) == 75
    sizes = {c: (g.N, g.M, max(g.maxdc, 1), g.E) for c in (PEG, W1944, C802, C4000, DVBS2)
             for g in [native.Graph.from_alist(code_path(c))]}
    wg = [(s, ab) for s in sizes.values() for ab in (8, 9)]
    # the LDS bound: the last N that fits and the first that does not, at one byte and at two
    wg += [((LDS - RED, 100, 8, 0), 8), ((LDS - RED + 1, 100, 8, 0), 8), (((LDS - RED) // 2, 100, 8, 0), 16),
           (((LDS - RED) // 2 + 1, 100, 8, 0), 16)]
    # S1 exists from row degree 27; a row count that is no multiple of the slot's alignment
    wg += [((2048, 389, 26, 0), 8), ((2048, 389, 27, 0), 8), ((2048, 389, 26, 0), 12), ((2048, 389, 27, 0), 12)]
    with open(qfile, "w") as f:
        for r in table:
            f.write("%s %d %d %d %d %d %d\n" % (r["family"], r["N"], r["M"], r["dcs"], r["E"], r["arg"], r["opt"]))
        for (N, M, dcs, E), ab in wg:
            f.write("fxlms_wg %d %d %d %d %d 0\n" % (N, M, dcs, E, ab))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe, qfile], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
    out = [ln.split() for ln in p.stdout.splitlines()]
    assert len(out) == len(table) + len(wg)
    for r, got in zip(table, out):
        want = [r["name"] or "-", r["threads"], r["cw_per_block"], r["lds_bytes"], r["cw_bytes"], r["staged"], r["wave"], 0, 0, 0, 0, 0]
        assert got == [str(x) for x in want], (r, got)
    for ((N, M, dcs, E), ab), got in zip(wg, out[len(table):]):
        assert got == [str(x) for x in want_wg(N, M, dcs, ab)], (N, M, dcs, ab, got)
    res = {(q[0][0], q[0][2], q[1]): g for q, g in zip(wg, out[len(table):])}
    # DVB-S2: two workgroups of 512 threads a CU at one byte, one of 1024 at two; 194,816 and 259,584 bytes of slot
    N, M, dcs, _ = sizes[DVBS2]
    assert (N, M, dcs) == (64800, 32400, 7)
    assert res[N, dcs, 8][:4] == ["fxlms_wg_i8", "512", "1", "65056"] and res[N, dcs, 8][8] == "194816"
    assert res[N, dcs, 9][:4] == ["fxlms_wg_i16", "1024", "1", "129856"] and res[N, dcs, 9][8] == "259584"
    for c in (PEG, W1944, C802, C4000):   # the small codes: one wavefront a codeword
        assert res[sizes[c][0], sizes[c][2], 8][1] == res[sizes[c][0], sizes[c][2], 9][1] == "64"
    assert res[LDS - RED, 8, 8][:4] == ["fxlms_wg_i8", "1024", "1", str(LDS)] and res[LDS - RED + 1, 8, 8][0] == "-"
    assert res[(LDS - RED) // 2, 8, 16][:4] == ["fxlms_wg_i16", "1024", "1", str(LDS)] and res[(LDS - RED) // 2 + 1, 8, 16][0] == "-"
    assert res[LDS - RED + 1, 8, 8][4] == str(LDS + 1)   # what the refusal reports
    assert res[2048, 26, 8][8:] == ["2816", "1792", "1792", "0"] and res[2048, 27, 8][8:] == ["4608", "1792", "3584", "1"]
    assert res[2048, 26, 12][8] == "3584" and res[2048, 27, 12][8] == "5376"


def test_sweep_fx_kernel_argument():
    a = sweep.parse(BASE + ["--fxlms"])
    assert a.fx_kernel == "auto"
    a = sweep.parse(BASE + ["--fxlms", "--fx-kernel", "wg", "--variant", "nms"])
    assert a.fx_kernel == "wg" and a.fxlms
    assert sweep.parse(BASE + ["--fxlms", "--fx-kernel", "auto"]).fx_kernel == "auto"
    assert sweep.parse(BASE + ["--fx-kernel", "auto"]).fx_kernel == "auto"   # the default, spelled out
    for bad, word in ((["--fx-kernel", "wg"], "--fx-kernel belongs to --fxlms"),
                      (["--fxms", "--fx-kernel", "wg"], "--fx-kernel belongs to --fxlms"),
                      (["--gdbf", "SMNGDBF", "--fx-kernel", "wg"], "--fx-kernel belongs to --fxlms"),
                      (["--schedule", "layered", "--fx-kernel", "wg"], "--fx-kernel belongs to --fxlms"),
                      (["--fxlms", "--fx-kernel", "wave"], "invalid choice"), (["--fxlms", "--fx-kernel"], "expected one argument")):
        p = subprocess.run([sys.executable, "-m", "ldpcsimulation_amd.sweep"] + BASE + bad, cwd=ROOT,
                           capture_output=True, text=True, timeout=120)
        assert p.returncode == 2 and word in p.stderr, (bad, p.stderr[-300:])


def test_fx_kernel_is_no_checkpoint_setting():
    """The kernel does not change a point's result: the settings with --fx-kernel wg are those without
    it, and the key sets of the other sweeps are what they were."""
    nms = ["--fxlms", "--variant", "nms", "--msg-bits", "8", "--app-bits", "9", "--early-stop"]
    base = sweep._checkpoint_config(sweep.parse(BASE + nms))
    assert sweep._checkpoint_config(sweep.parse(BASE + nms + ["--fx-kernel", "wg"])) == base
    assert sweep._checkpoint_config(sweep.parse(BASE + nms + ["--fx-kernel", "auto"])) == base
    keys = {"alist", "alist_md5", "rate", "snr", "T", "variant", "alpha", "delta", "quantize", "saturate",
            "precision", "schedule", "min_bit_errors", "min_frame_errors", "max_frames", "codewords_md5", "ems",
            "nm", "offset", "early_stop"}
    fxms = {"fxms", "ymax", "qbits", "msg_bits", "nms_num", "nms_shift", "beta"}
    assert set(sweep._checkpoint_config(sweep.parse(BASE + ["--variant", "nms", "--alpha", "1.25"]))) == keys
    assert set(sweep._checkpoint_config(sweep.parse(BASE + ["--fxms", "--variant", "nms"]))) == keys | fxms
    assert set(base) == keys | fxms | {"fxlms", "app_bits", "min_sum_early_stop"}
