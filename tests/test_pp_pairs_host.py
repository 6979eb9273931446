"""The ping-pong kernel's row pairing and in-register schedule on the host (graph.h
pp_pair_rows, build_pp_inreg_schedule): tests/native/pp_pairs_host.cpp, a stand-alone
program over graph.cpp, compiled with -fsanitize=address,undefined and run directly.
It checks, on the bench code: 486 pairs, each pair's rows exactly the two neighbours of
its bit, every row placed once, degree <= 7 in the capped slots, the first-in-nlist flag
(block pairs (6,7): the degree-8 row at r = 1 comes first; (10,11): the r = 0 row does),
the in-register edge at the last position of both rows and no bit slot for it; on a code
without degree-2 bits: no schedule; on a path of odd length: one row left alone; on the
802.11n code of Z = 54 (N = 1296, M = 648) placed on 512 check threads: 324 pairs and 188
threads without one, runs of pairs across the wave boundaries. (On the device that code's
row schedule has 384 threads, so the one-codeword kernel decodes it, not the ping-pong
kernel: its pairing is checked here only.)"""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT, code_path


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_row_pairing_and_in_register_schedule_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "pp_pairs_host")
    csrc = os.path.join(ROOT, "ldpcsimulation_amd", "csrc")
    subprocess.run(["g++", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                    "-o", exe, os.path.join(ROOT, "tests", "native", "pp_pairs_host.cpp"),
                    os.path.join(csrc, "graph.cpp")], check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    from ldpcsimulation_amd import codes
    z54 = str(tmp_path / "80211n_1296_r12.alist")
    codes.write_alist(codes.ieee80211n_r12(Z=54), z54)
    p = subprocess.run([exe, code_path("80211n_1944_r12.alist"), z54], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "ok (0 failures)" in p.stdout
    assert "bench code: 486 pairs; (6,7) first at r=1: 81, (10,11) first at r=0: 81" in p.stdout
    assert "bench code: e_pad 6208, pure waves 8" in p.stdout
    assert "odd path: 100 pairs of 201 rows" in p.stdout
    assert "Z=54: 324 pairs, 188 empty threads, pure waves 8" in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
