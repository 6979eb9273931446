"""The host side of the every-attempt decoders, without a GPU: the ABI additions, the cfg
refusals (made before any device call), the kernel instances the library carries, and both
CLIs up to their first device call."""
import ctypes as C
import os
import re
import subprocess

import rstat_oracle as SO
from conftest import ROOT, code_path
from ldpcsimulation_amd import native

STAT = os.path.join(ROOT, "bin", "redecodeStatistics")
REPLAY = os.path.join(ROOT, "bin", "replayGDBF")
PEG = "PEGReg504x1008.alist"
NAMES = ["ldpc_rstat_decode_batch", "ldpc_rstat_sim_launch", "ldpc_rstat_sim_batch", "ldpc_rstat_sim_trace",
         "ldpc_rstat_kernel_info"]


def test_abi_additions_in_header_and_binding():
    txt = open(os.path.join(ROOT, "include", "ldpc_hip.h")).read()
    assert "#define LDPC_ABI_VERSION 11" in txt and "#define LDPC_OPT_COUNT 23" in txt   # purely additive
    for n in NAMES:
        assert re.search(r"\b%s\(" % n, txt) and n in native.EXPORTED and hasattr(native.lib(), n)
    ctype = {C.c_int32: "int32_t", C.c_double: "double", C.c_void_p: "pointer"}

    def fields(name):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, txt).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        out = []
        for decl in body.split(";"):
            m = re.match(r"\s*(int32_t|double|int8_t\s*\*|int32_t\s*\*)\s*(.*)", decl.strip(), flags=re.S)
            if m:
                t = "pointer" if "*" in m.group(1) or m.group(2).lstrip().startswith("*") else m.group(1)
                out += [(t, n.strip().lstrip("*")) for n in m.group(2).split(",")]
        return out

    assert fields("ldpc_rstat_cfg") == [(ctype[t], n.rstrip("_")) for n, t in native._RstatCfg._fields_]
    assert [n for _, n in fields("ldpc_rstat_cfg")] == ["flags", "precision", "T", "attempts", "windowsize",
                                                        "first_attempt", "theta", "lambda", "alpha", "noise_scale", "ymax"]
    assert fields("ldpc_attempt_result") == [("int32_t", n) for n in native.ATTEMPT_DTYPE.names]
    assert native.ATTEMPT_DTYPE.itemsize == 16 and C.sizeof(native._RstatCfg) == 64
    assert fields("ldpc_rstat_trace") == [(ctype[t], n) for n, t in native._RstatTrace._fields_]
    cfg = native.RstatConfig()
    assert cfg.precision == native.F64 and cfg.flags == native.RGDBF_FLAGS == 31 and cfg.first_attempt == 0


def _info(cfg, ctx=None):
    rc = native.lib().ldpc_rstat_kernel_info(ctx, C.byref(cfg._c()), 0, None, 0, None)
    return rc, native.lib().ldpc_last_error().decode()


def test_cfg_refusals_without_a_device():
    """ldpc_rstat_kernel_info with a NULL context checks the cfg first and never reaches the
    device: every refusal below is the cfg's, and a good cfg is refused for the context."""
    ok = native.RstatConfig(T=100, attempts=5)
    assert _info(ok) == (-1, "ctx is null")
    for flag in (native.GDBF_QUANTIZE, native.GDBF_SEQUENTIAL, native.GDBF_MODESWITCH, native.GDBF_QPROB):
        rc, msg = _info(native.RstatConfig(flags=native.RGDBF_FLAGS | flag))
        assert rc == -4 and "NOISE|ADAPT|WEIGHT|SMOOTH|SATURATE" in msg, (flag, msg)
    assert _info(native.RstatConfig(flags=512))[0] == -1                # an unknown bit
    assert _info(native.RstatConfig(T=0))[0] == -1 and "T must be in 1..4094" in _info(native.RstatConfig(T=0))[1]
    assert _info(native.RstatConfig(T=4095))[0] == -1
    assert _info(native.RstatConfig(T=4094)) == (-1, "ctx is null")
    assert _info(native.RstatConfig(attempts=0))[0] == -1 and "attempts" in _info(native.RstatConfig(attempts=0))[1]
    assert _info(native.RstatConfig(first_attempt=-1))[0] == -1
    assert _info(native.RstatConfig(first_attempt=2 ** 31 - 5, attempts=5))[0] == -1      # 2^31 > 2^31 - 1
    assert "2^31 - 1" in _info(native.RstatConfig(first_attempt=2 ** 31 - 5, attempts=5))[1]
    assert _info(native.RstatConfig(first_attempt=2 ** 31 - 6, attempts=5)) == (-1, "ctx is null")
    # a frame's iterations summed over its attempts stay an int32: 4094 * 524545 > 2^31 - 1 >= 4094 * 524544
    assert _info(native.RstatConfig(T=4094, attempts=524545))[0] == -1
    assert "attempts * T" in _info(native.RstatConfig(T=4094, attempts=524545))[1]
    assert _info(native.RstatConfig(T=4094, attempts=524544)) == (-1, "ctx is null")
    assert _info(native.RstatConfig(precision=2))[0] == -1
    assert _info(native.RstatConfig(ymax=0.0))[0] == -1
    L = native.lib()
    cfg = C.byref(ok._c())
    assert L.ldpc_rstat_sim_batch(None, 3.0, 0.5, cfg, 1, 0, 0, 1, None, None, None, None) == -1
    assert L.ldpc_rstat_sim_trace(None, 3.0, 0.5, cfg, 1, 0, 0, 1, None, None, None, None, None, None, None) == -1
    assert L.ldpc_rstat_sim_launch(None, 3.0, 0.5, cfg, 1, 0, 0, 1, None, None, None) == -1
    assert L.ldpc_rstat_decode_batch(None, None, None, 1, cfg, None, None, None, None, None, None) == -1


def test_library_carries_the_rstat_kernels():
    """Both shapes in both precisions and sources: rstat_rows in the instances of rgdbf_rows,
    rstat_wg and its global-slot form with and without traces."""
    syms = subprocess.run(["nm", "-C", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    rows = sorted(set(re.findall(r"ldpc::k_rstat_rows<([^>]*)>", syms)))
    assert rows == sorted(set(re.findall(r"ldpc::k_rgdbf_rows<([^>]*)>", syms))) and len(rows) == 16, rows
    want = sorted(f"{f}, {s}, {t}" for f in ("double", "float") for s in (0, 1) for t in ("false", "true"))
    for k in ("k_rstat_wg", "k_rstat_wg_global"):
        assert sorted(set(re.findall(r"ldpc::%s<([^>]*)>" % k, syms))) == want, k
    assert "ldpc::k_rstat_account" in syms


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if not k.startswith("LDPC_")}
    env.update(kw)
    return env


def test_cli_usage_texts():
    for exe, args in ((STAT, "alist R SNR T NR NF theta logfilename"), (REPLAY, "alist R SNR T NR theta statefilename logfilename")):
        p = subprocess.run([exe], capture_output=True, text=True)
        assert p.returncode == 0
        first, rest = p.stdout.split("\n", 1)
        assert first == "Usage: %s %s noiseScale lambda alpha windowsize Ymax [codeword filename]" % (exe, args)
        assert "GSL" in rest and "seed" in rest and "position" in rest     # the state file is the project's own


def test_cli_parameter_blocks_and_dry_run(tmp_path):
    """The reference's preamble, byte for byte, from both programs; no device call, no file."""
    runs, replays = SO.golden()
    (tmp_path / "tmp").mkdir()
    for exe, run in ((STAT, runs[0]), (REPLAY, replays[0])):
        args = ["log.txt" if x == "@LOG@" else "frame.state" if x == "@STATE@" else x for x in run["args"]]
        p = subprocess.run([exe, code_path(PEG)] + args, env=_env(LDPC_DRY_RUN="1"), cwd=tmp_path, capture_output=True,
                           text=True, timeout=60)
        assert p.returncode == 0, p.stderr
        assert p.stderr.strip() == "ldpc: rng=glibc precision=f64 batch=1 device=0"
        end = "Completed phase with" if exe == REPLAY else "Ferr with"
        want = run["stdout"].split(end)[0].replace("@ALIST@", code_path(PEG))
        assert "\tsigma\t" in want and p.stdout == want
        assert not (tmp_path / "log.txt").exists() and not list((tmp_path / "tmp").iterdir())
    # T beyond the 12-bit iteration field of the Philox stream word is refused before any device call
    bad = [("5000" if i == 2 else "log.txt" if x == "@LOG@" else x) for i, x in enumerate(runs[0]["args"])]
    p = subprocess.run([STAT, code_path(PEG)] + bad, env=_env(LDPC_DRY_RUN="1"), cwd=tmp_path, capture_output=True,
                       text=True, timeout=60)
    assert p.returncode == 1 and "4094" in p.stderr


def test_cli_without_tmp_exits_before_decoding(tmp_path):
    """The reference writes through a null FILE* there; these programs say so and exit 1."""
    runs, replays = SO.golden()
    for exe, run in ((STAT, runs[0]), (REPLAY, replays[0])):
        args = ["log.txt" if x == "@LOG@" else "frame.state" if x == "@STATE@" else x for x in run["args"]]
        p = subprocess.run([exe, code_path(PEG)] + args, env=_env(), cwd=tmp_path, capture_output=True, text=True,
                           timeout=60)
        assert p.returncode == 1 and "tmp/" in p.stderr, p.stderr
        assert not (tmp_path / "log.txt").exists()
