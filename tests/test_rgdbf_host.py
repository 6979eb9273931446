"""The host side of the re-decoding NGDBF decoder, without a GPU: the ABI additions, the cfg
refusals (made before any device call), the kernel instances the library carries, the CLI up
to its first device call and the sweep driver's --gdbf argument rules."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

import rgdbf_oracle as RO
from conftest import ROOT, code_path
from ldpcsimulation_amd import native, sweep

EXE = os.path.join(ROOT, "bin", "decodeRSMNGDBF")
PEG = "PEGReg504x1008.alist"
NAMES = ["ldpc_rgdbf_decode_batch", "ldpc_rgdbf_sim_launch", "ldpc_rgdbf_sim_batch", "ldpc_rgdbf_kernel_info"]


def test_abi_additions_in_header_and_binding():
    txt = open(os.path.join(ROOT, "include", "ldpc_hip.h")).read()
    assert "#define LDPC_ABI_VERSION 11" in txt and "#define LDPC_OPT_COUNT 23" in txt   # purely additive
    for n in NAMES:
        assert re.search(r"\b%s\(" % n, txt) and n in native.EXPORTED and hasattr(native.lib(), n)
    m = re.search(r"typedef struct \{([^}]*)\} ldpc_rgdbf_cfg;", txt)
    fields = re.findall(r"(int32_t|double)\s+(\w+);", m.group(1))
    ctype = {C.c_int32: "int32_t", C.c_double: "double"}
    assert fields == [(ctype[t], n.rstrip("_")) for n, t in native._RgdbfCfg._fields_]
    assert [n for _, n in fields] == ["flags", "precision", "T", "maxphase", "windowsize", "reserved", "theta",
                                      "lambda", "alpha", "noise_scale", "ymax"]
    cfg = native.RgdbfConfig()
    assert cfg.precision == native.F64 and cfg.flags == native.RGDBF_FLAGS == 31
    assert native.RGDBF_FLAGS == native.GDBF_VARIANTS["SMNGDBF"]


def _info(cfg, ctx=None):
    rc = native.lib().ldpc_rgdbf_kernel_info(ctx, C.byref(cfg._c()), None, 0, None)
    return rc, native.lib().ldpc_last_error().decode()


def test_cfg_refusals_without_a_device():
    """ldpc_rgdbf_kernel_info with a NULL context checks the cfg first and never reaches the
    device: every refusal below is the cfg's, and a good cfg is refused for the context."""
    ok = native.RgdbfConfig(T=100, maxphase=3)
    assert _info(ok) == (-1, "ctx is null")
    for flag in (native.GDBF_QUANTIZE, native.GDBF_SEQUENTIAL, native.GDBF_MODESWITCH, native.GDBF_QPROB):
        rc, msg = _info(native.RgdbfConfig(flags=native.RGDBF_FLAGS | flag))
        assert rc == -4 and "NOISE|ADAPT|WEIGHT|SMOOTH|SATURATE" in msg, (flag, msg)
    assert _info(native.RgdbfConfig(flags=512))[0] == -1                # an unknown bit
    assert _info(native.RgdbfConfig(T=0))[0] == -1 and "T must be >= 1" in _info(native.RgdbfConfig(T=0))[1]
    assert _info(native.RgdbfConfig(maxphase=0))[0] == -1
    assert _info(native.RgdbfConfig(T=1365, maxphase=3))[0] == -1       # 4095 > 4094
    assert "4094" in _info(native.RgdbfConfig(T=1365, maxphase=3))[1]
    assert _info(native.RgdbfConfig(T=2047, maxphase=2)) == (-1, "ctx is null")   # 4094 passes the cfg check
    assert _info(native.RgdbfConfig(precision=2))[0] == -1
    assert _info(native.RgdbfConfig(ymax=0.0))[0] == -1
    assert _info(native.RgdbfConfig(flags=native.GDBF_ADAPT, ymax=0.0)) == (-1, "ctx is null")
    for fn, args in (("ldpc_rgdbf_sim_batch", (None, 3.0, 0.5, C.byref(ok._c()), 1, 0, 0, 1, None, None)),
                     ("ldpc_rgdbf_sim_launch", (None, 3.0, 0.5, C.byref(ok._c()), 1, 0, 0, 1, None)),
                     ("ldpc_rgdbf_decode_batch", (None, None, None, 1, C.byref(ok._c()), None, None, None, None))):
        assert getattr(native.lib(), fn)(*args) == -1, fn


def test_library_carries_the_rgdbf_kernels():
    """rgdbf_rows in both precisions and sources, register schedules of 4 and 12 edges, 512 and
    1024 threads -- the instances of gdbf_rows -- and the two generic kernels."""
    syms = subprocess.run(["nm", "-C", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    rows = sorted(set(re.findall(r"ldpc::k_rgdbf_rows<([^>]*)>", syms)))
    want = sorted(f"{f}, {s}, {dvm}, {nt}" for f in ("double", "float") for s in (0, 1) for dvm in (4, 12)
                  for nt in (512, 1024))
    assert rows == want, rows
    assert rows == sorted(set(re.findall(r"ldpc::k_gdbf_rows<([^>]*)>", syms)))
    for k in ("k_rgdbf_lds", "k_rgdbf_global"):
        assert len(set(re.findall(r"ldpc::%s<([^>]*)>" % k, syms))) == 4, k


def test_cli_parameter_block_and_dry_run(tmp_path):
    p = subprocess.run([EXE], capture_output=True, text=True)
    assert p.returncode == 0
    assert p.stdout == ("Usage: %s alist R SNR T theta logfilename noiseScale lambda alpha windowsize Ymax maxphase "
                        "[codeword filename]\n" % EXE)
    env = {k: v for k, v in os.environ.items() if not k.startswith("LDPC_")}
    env["LDPC_DRY_RUN"] = "1"
    log = tmp_path / "log.txt"
    run = RO.golden_runs()[0][0]
    args = [str(log) if x == "@LOG@" else x for x in run["args"]]
    p = subprocess.run([EXE, code_path(PEG)] + args, env=env, capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    assert p.stderr.strip() == "ldpc: rng=glibc precision=f64 batch=1 device=0"
    # the reference's preamble, byte for byte (RNGDBF.cpp:121-176, the maxphase line included)
    want = run["stdout"].split("Ferr with")[0].replace("@ALIST@", code_path(PEG)).replace("@LOGFILE@", str(log))
    assert " maxphase = \t4\n" in want and p.stdout == want
    assert not log.exists()
    # T * maxphase beyond the 12-bit iteration field is refused before any device call
    bad = [("2000" if i == 2 else x) for i, x in enumerate(args)]
    p = subprocess.run([EXE, code_path(PEG)] + bad, env=env, capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "4094" in p.stderr


def test_sweep_arguments():
    base = [code_path(PEG), "--rate", "0.5", "--snr", "3.5", "-T", "100"]
    for name in list(native.GDBF_VARIANTS) + ["RSMNGDBF"]:
        assert sweep.parse(base + ["--gdbf", name]).gdbf == name
    a = sweep.parse(base + ["--gdbf", "RSMNGDBF", "--theta", "-0.7", "--lam", "0.98", "--noise-scale", "0.8",
                            "--window", "8", "--maxphase", "4", "--alpha", "0.96", "--ymax", "2.25"])
    assert sweep._gdbf_settings(a) == {"theta": -0.7, "lam": 0.98, "noise_scale": 0.8, "window": 8, "nq": 16,
                                       "maxphase": 4, "ymax": 2.25}
    a = sweep.parse(base + ["--gdbf", "SMNGDBF", "--saturate", "2.0", "--nq", "8"])
    assert sweep._gdbf_settings(a) == {"theta": -0.6, "lam": 0.99, "noise_scale": 0.75, "window": 16, "nq": 8,
                                       "ymax": 2.0}
    for bad in (["--gdbf", "RSMNGDBF", "--ems"], ["--gdbf", "RSMNGDBF", "--schedule", "layered"],
                ["--gdbf", "SMNGDBF", "--variant", "nms"], ["--gdbf", "RSMNGDBF", "--variant", "ddbmp"],
                ["--gdbf", "NGDBF"], ["--gdbf", "SMNGDBF", "--maxphase", "2"], ["--theta", "-0.6"],
                ["--maxphase", "3"]):
        p = subprocess.run([sys.executable, "-m", "ldpcsimulation_amd.sweep"] + base + bad, cwd=ROOT,
                           capture_output=True, text=True, timeout=120)
        assert p.returncode == 2 and "gdbf" in p.stderr, (bad, p.stderr[-300:])


def test_checkpoint_config_unchanged_without_gdbf():
    """A sweep without --gdbf keeps the checkpoint settings it had before the flag existed
    (so its checkpoints still match); with --gdbf the new settings are part of them."""
    base = [code_path(PEG), "--rate", "0.5", "--snr", "3.5", "-T", "100"]
    keys = {"alist", "alist_md5", "rate", "snr", "T", "variant", "alpha", "delta", "quantize", "saturate",
            "precision", "schedule", "min_bit_errors", "min_frame_errors", "max_frames", "codewords_md5", "ems",
            "nm", "offset", "early_stop"}
    assert set(sweep._checkpoint_config(sweep.parse(base + ["--variant", "nms", "--alpha", "1.25"]))) == keys
    assert set(sweep._checkpoint_config(sweep.parse(base + ["--variant", "ddbmp", "--ymax", "1", "--qbits", "3"]))) \
        == keys | {"ymax", "qbits"}
    g = sweep._checkpoint_config(sweep.parse(base + ["--gdbf", "RSMNGDBF", "--maxphase", "2"]))
    assert set(g) == keys | {"gdbf", "theta", "lam", "noise_scale", "window", "nq", "maxphase", "ymax"}
    assert g["gdbf"] == "RSMNGDBF" and g["maxphase"] == 2
    g2 = sweep._checkpoint_config(sweep.parse(base + ["--gdbf", "RSMNGDBF", "--maxphase", "3"]))
    assert g2 != g
