"""The host side of the fixed-point NGDBF hardware-model decoder, without a GPU: the ABI
additions, the cfg refusals (made before any device call), the kernel instances the library
carries and the CLI up to its first device call."""
import ctypes as C
import os
import re
import subprocess

import hwgdbf_oracle as HO
from conftest import ROOT, code_path
from ldpcsimulation_amd import native

EXE = os.path.join(ROOT, "bin", "NGDBFhw")
C802 = "802_3_H.alist"
NAMES = ["ldpc_hwgdbf_decode_batch", "ldpc_hwgdbf_sim_launch", "ldpc_hwgdbf_sim_batch", "ldpc_hwgdbf_sim_trace",
         "ldpc_hwgdbf_kernel_info"]


def test_abi_additions_in_header_and_binding():
    txt = open(os.path.join(ROOT, "include", "ldpc_hip.h")).read()
    assert "#define LDPC_ABI_VERSION 11" in txt and "#define LDPC_OPT_COUNT 23" in txt   # purely additive
    assert native.lib().ldpc_abi_version() == 11 and max(native.OPTIONS.values()) == 22   # ids 1..22 of 23
    for n in NAMES:
        assert re.search(r"\b%s\(" % n, txt) and n in native.EXPORTED and hasattr(native.lib(), n)
    m = re.search(r"typedef struct \{([^}]*)\} ldpc_hwgdbf_cfg;", txt)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for typ, names in re.findall(r"(int32_t|double)\s+([\w\s,]+);", body):
        fields += [(typ, n.strip()) for n in names.split(",")]
    ctype = {C.c_int32: "int32_t", C.c_double: "double"}
    assert fields == [(ctype[t], n) for n, t in native._HwGdbfCfg._fields_]
    assert [n for _, n in fields] == ["precision", "T", "maxphase", "nq", "qlen", "reserved", "w", "ymax", "noise_scale",
                                      "theta0"]
    cfg = native.HwGdbfConfig()
    got = {k: getattr(cfg, k) for k in HO.DEFAULTS}
    assert got == HO.DEFAULTS and cfg.precision == native.F64


def _info(cfg, ctx=None):
    rc = native.lib().ldpc_hwgdbf_kernel_info(ctx, C.byref(cfg._c()), None, 0, None)
    return rc, native.lib().ldpc_last_error().decode()


def test_cfg_refusals_without_a_device():
    """ldpc_hwgdbf_kernel_info with a NULL context checks the cfg first and never reaches the
    device: every refusal below is the cfg's, and a good cfg is refused for the context."""
    ok = native.HwGdbfConfig()
    assert _info(ok) == (-1, "ctx is null")
    for bad, word in ((dict(T=0), "T must be >= 1"), (dict(maxphase=0), "maxphase"), (dict(nq=1), "nq"),
                      (dict(nq=8), "nq"), (dict(qlen=0), "qlen"), (dict(qlen=-5), "qlen"), (dict(w=0.0), "w must"),
                      (dict(w=-1.0), "w must"), (dict(ymax=0.0), "ymax"), (dict(precision=2), "precision")):
        rc, msg = _info(native.HwGdbfConfig(**bad))
        assert rc == -1 and word in msg, (bad, msg)
    raw = ok._c()
    raw.reserved = 1
    assert native.lib().ldpc_hwgdbf_kernel_info(None, C.byref(raw), None, 0, None) == -1
    assert "reserved" in native.lib().ldpc_last_error().decode()
    for nq in (2, 7):
        assert _info(native.HwGdbfConfig(nq=nq)) == (-1, "ctx is null")
    c = C.byref(ok._c())
    for fn, args in (("ldpc_hwgdbf_sim_batch", (None, 4.0, 0.8413, c, 1, 0, 0, 1, None, None)),
                     ("ldpc_hwgdbf_sim_launch", (None, 4.0, 0.8413, c, 1, 0, 0, 1, None)),
                     ("ldpc_hwgdbf_sim_trace", (None, 4.0, 0.8413, c, 1, 0, 0, 1, None, None, None, None, None)),
                     ("ldpc_hwgdbf_decode_batch", (None, None, None, None, 1, c, None, None, None, None, None))):
        assert getattr(native.lib(), fn)(*args) == -1, fn


def test_library_carries_both_kernel_shapes():
    """k_hwgdbf<front-end type, sample source, wavefront-per-codeword, graph-in-LDS> in every combination."""
    syms = subprocess.run(["nm", "-C", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    got = sorted(set(re.findall(r"ldpc::k_hwgdbf<([^>]*)>", syms)))
    assert got == sorted(f"{f}, {s}, {w}, {g}" for f in ("double", "float") for s in (0, 1) for w in ("false", "true")
                         for g in ("false", "true")), got


def _env():
    env = {k: v for k, v in os.environ.items() if not k.startswith("LDPC_")}
    env["LDPC_DRY_RUN"] = "1"
    return env


def test_cli_usage_and_dry_run(tmp_path):
    usage = "Usage: %s alist SNR numFrames seed logfilename [codeword filename]\n" % EXE
    for args in ([], ["a", "b", "c", "d"], ["a"] * 7):
        p = subprocess.run([EXE] + args, capture_output=True, text=True)
        assert p.returncode == 0 and p.stdout == usage
    log = tmp_path / "log.txt"
    run = HO.golden_runs()[0][0]
    alist = code_path(run["code"])
    p = subprocess.run([EXE, alist, run["snr"], str(run["frames"]), str(run["seed"]), str(log)], env=_env(),
                       capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    assert p.stderr.strip() == "ldpc: rng=glibc precision=f64 batch=1 device=0"
    # the reference's preamble, byte for byte (NGDBFhw.cpp:499-510, :123, :136-137)
    want = run["stdout"].split("Ferr with")[0].replace("@ALIST@", alist).replace("@LOGFILE@", str(log))
    assert "R=0.8413, dv=6, dc=32" in want and p.stdout == want
    assert not log.exists()
    env = dict(_env(), LDPC_RNG="philox", LDPC_PRECISION="f32", LDPC_BATCH="4096")
    p = subprocess.run([EXE, alist, "4.0", "100000", "1", str(log)], env=env, capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stderr.strip() == "ldpc: rng=philox precision=f32 batch=4096 device=0"


def test_cli_refuses_the_codeword_file(tmp_path):
    """The reference streams a null pointer into cout there and prints nothing more; the CLI
    prints the reference's text up to that point and fails."""
    log = tmp_path / "log.txt"
    alist = code_path(C802)
    p = subprocess.run([EXE, alist, "4.0", "10", "1", str(log), code_path("PEGReg504x1008_data20.enc")], env=_env(),
                       capture_output=True, text=True, timeout=60)
    assert p.returncode != 0
    assert p.stdout == ("PARAMETERS: \n alist = \t%s\n SNR = \t4\nSimulating for 10 frames.\nUsing random seed 1\n"
                        " log = \t%s\n\nUsing codewords from " % (alist, log))
    assert len(p.stderr.strip().splitlines()) == 1 and "codeword file" in p.stderr
    assert not log.exists()
