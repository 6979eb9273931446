"""The host side of the GF(4) / GF(8) EMS kernels, without a GPU: a stand-alone program
(tests/native/nb_gfq_host.cpp over nb_graph.cpp and nb_layout.h) under AddressSanitizer and UBSan
checks the message layout for q = 4, 8, 16 (q = 16 against a table of the values it always had),
the GF products and the packed schedule, and prints the kernel choice of the shapes the GPU tests
use and of both reference codes; the library carries the new instances; the ABI did not move."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
from ldpcsimulation_amd import native

CSRC = os.path.join(ROOT, "ldpcsimulation_amd", "csrc")
LDS = 160 * 1024
# (N, M, E, q, maxdc) -> kernel: the small codes, the (2, 4) codes with 256 KB of messages, the
# reference's GF(4) code (196.5 KB of state and tables) and GF(8) code (155 KB), the GF(16) codes of
# tests/test_ems.py, and shapes no kernel takes (N, maxdc * M, row degree, state beyond LDS)
PLANS = [((96, 48, 192, 4, 4), "ems_lds"), ((120, 40, 240, 8, 6), "ems_lds"), ((90, 60, 270, 4, 5), "ems_lds"),
         ((1300, 600, 2600, 8, 5), "ems_lds"), ((5000, 2500, 10000, 4, 4), "ems_global"),
         ((2500, 1250, 5000, 8, 4), "ems_global"), ((9000, 6000, 22500, 4, 4), "ems_global_sched"),
         ((6000, 4000, 15000, 8, 4), "ems_global"), ((1000, 500, 2000, 16, 4), "ems_lds"),
         ((2000, 1000, 4000, 16, 4), "ems_global"), ((4100, 4097, 12296, 16, 8), "ems_global"),
         ((65536, 100, 400, 4, 4), "-"), ((32770, 16385, 65540, 16, 4), "-"), ((96, 48, 192, 4, 9), "-"),
         ((20000, 10000, 40000, 8, 4), "-")]


def al(x):
    return (x + 15) & ~15


def want_plan(N, M, E, q, maxdc):
    """nb_plan restated."""
    m = q.bit_length() - 1
    state = al(N * m * 4) + al(N) + al((M + 3) // 4 * 4) + 288
    sched = al(M) + al(4 * N) + al(2 * E) + al(E)
    ep = 4
    while ep < maxdc * M:
        ep *= 2
    msg = ep * q * 4
    if maxdc > 8 or state > LDS or maxdc * M > 65535 or N > 65535:
        return "-", 0, 0
    if state + sched + msg <= LDS:
        return "ems_lds", state + sched + msg, 0
    if state + sched <= LDS:
        return "ems_global", state + sched, msg
    return "ems_global_sched", state, msg


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_layout_fields_and_kernel_choice_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "nb_gfq_host")
    subprocess.run(["g++", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-std=c++17", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "native", "nb_gfq_host.cpp"), os.path.join(CSRC, "nb_graph.cpp")],
                   check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    args = [str(x) for shape, _ in PLANS for x in shape]
    p = subprocess.run([exe] + args, capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr and "FAILED" not in p.stdout
    lines = [l.split() for l in p.stdout.splitlines() if l.startswith("plan ")]
    assert len(lines) == len(PLANS)
    for (shape, name), got in zip(PLANS, lines):
        assert want_plan(*shape)[0] == name, shape                        # the restatement agrees with the table
        assert got[7:] == [str(x) for x in want_plan(*shape)], (shape, got)
    # the reference's GF(4) code: 87 296 bytes of LDS and 512 KB of messages; its GF(8) code keeps its tables
    assert want_plan(9000, 6000, 22500, 4, 4) == ("ems_global_sched", 87296, 524288)
    assert want_plan(6000, 4000, 15000, 8, 4) == ("ems_global", 155296, 524288)


def test_library_carries_the_new_instances_and_the_old_ones():
    """k_ems<Q, bits, DC, source, messages global, threads, schedule in LDS>: GF(16) as before (1024
    threads at DC = 4 only) plus its schedule-from-global instances, GF(4) and GF(8) at both sizes."""
    syms = subprocess.run(["nm", "-C", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    got = set(re.findall(r"ldpc::k_ems<([^>]*)>", syms))
    want = set()
    for q, mb in ((4, 2), (8, 3), (16, 4)):
        for dc in (4, 8):
            for src in (0, 1):
                for threads in (512, 1024):
                    if q == 16 and dc == 8 and threads == 1024:
                        continue
                    for gs, sched in (("false", "true"), ("true", "true"), ("true", "false")):
                        want.add(f"{q}, {mb}, {dc}, {src}, {gs}, {threads}, {sched}")
    assert got == want, sorted(got ^ want)


def test_abi_and_options_did_not_move():
    txt = open(os.path.join(ROOT, "include", "ldpc_hip.h")).read()
    assert "#define LDPC_ABI_VERSION 11" in txt and "#define LDPC_OPT_COUNT 23" in txt
    assert native.lib().ldpc_abi_version() == 11 and max(native.OPTIONS.values()) == 22
    assert "ems_global_sched" in txt
