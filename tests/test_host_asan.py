"""Host code under AddressSanitizer + UBSan: `make build/host_asan`
compiles graph.cpp (load_alist, build_graph, the row / flood / layer schedules),
nb_graph.cpp (the NB alist reader of SystemC/NB-LDPC/src/alist.cpp:29-53's format,
the GF tables, the message-slot swizzle search), cli_common.h (the CLIs' codeword
files and alist headers) and the CPU oracle with -fsanitize=address,undefined
-fno-sanitize-recover=all; tests/native/host_asan.cpp drives them over every code
fixture (DVB-S2 included), the reference's own malformed 802.11n alists
(tests/golden/codes/reference_80211n), the GF(q) fixtures, the codeword-file
fixtures, the data files of the reference's SystemC/NB-LDPC/codes/*/ through the NB
reader (tests/golden/codes/reference_nb: binary-format alists, the .pchk / .gen
blobs, the GF(2) code and the first 20 lines of its 3 MB data.enc, stored .xz;
its GF(4) and GF(8) codes are the q4 / q8 fixtures; its three shell scripts are
program text and are not stored), and generated malformed inputs (truncated files,
degree-0 and degree-1 checks, out-of-range indices and coefficients, disagreeing
views, empty / unterminated / binary / CRLF codeword files). Any sanitizer report
fails the run."""
import glob
import lzma
import os
import shutil
import subprocess
import tempfile

import pytest

from conftest import REF_80211N, REF_NB, ROOT, code_path


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_graph_compiler_and_oracle_clean_under_asan_ubsan():
    subprocess.run(["make", "-C", ROOT, "build/host_asan"], check=True, capture_output=True, text=True)
    codes = [code_path(n) for n in ("4000.2000.4.244.alist", "80211n_1944_r12.alist", "PEGReg504x1008.alist",
                                    "dvbs2_1_2.alist")]
    ref_codes = sorted(glob.glob(os.path.join(REF_80211N, "*.alist")))
    assert len(ref_codes) == 2
    codes += ref_codes
    nb = [code_path(n) for n in ("gf16_N1000_dv2_dc4.alist", "q4.sp.9000.6000.4500.1.alist",
                                 "q8.sp.6000.4000.3000.1.alist")]
    cw = [code_path(n) for n in ("PEGReg504x1008_data20.enc", "PEGReg504x1008_data5_noeol.enc")]
    # real files in the wrong format for the NB reader: the binary fixtures and codeword files above ...
    nb += [c for c in codes if "dvbs2" not in c] + cw + [code_path("4000.2000.4.244_data10.enc")]
    ref_nb = sorted(glob.glob(os.path.join(REF_NB, "*.xz")))
    assert len(ref_nb) == 12
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    with tempfile.TemporaryDirectory() as td:
        os.mkdir(os.path.join(td, "ref_nb"))
        for x in ref_nb:   # ... and the reference's own NB-LDPC code directory
            nb.append(os.path.join(td, "ref_nb", os.path.basename(x)[:-3]))
            with lzma.open(x, "rb") as fi, open(nb[-1], "wb") as fo:
                fo.write(fi.read())
        p = subprocess.run([os.path.join(ROOT, "build", "host_asan")] + codes + ["--nb"] + nb + ["--cw"] + cw +
                           ["--tmp", td], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "ok (0 failures)" in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
    assert "blob layout: ok" in p.stdout   # blob.h: the device layouts' section offsets, literal numbers
    # the GF(16) code loads, with swizzles whose XOR over every check is 0 (checked inside)
    assert "gf16_N1000_dv2_dc4.alist: NB N=1000 M=500 q=16 E=2000" in p.stdout
    assert "q4.sp.9000.6000.4500.1.alist: NB N=9000 M=6000 q=4" in p.stdout
    # every --nb input is answered: loaded, or rejected with a message
    assert p.stdout.count(": NB N=") + p.stdout.count(": NB rejected (") == len(nb)
    assert "PegReg4000.alist: NB rejected (" in p.stdout and "PEGReg504x1008.pchk: NB rejected (" in p.stdout
    assert p.stdout.count("bytes of invalid-symbol reports") >= 5 * 7 + 2
