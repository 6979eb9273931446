"""Launch shapes of the wave-per-codeword decoders (hwgdbf, fxms, fxlms) against
tests/golden/wave_cw_choices.json: the kernel name, threads, codewords per workgroup, LDS
bytes, bytes of one codeword and the staged / wave flags that hwgdbf_choose, fxms_choose and
fxlms_choose gave before they shared one planner, for the five codes the decoders' tests use
and for synthetic sizes on each side of every threshold of the choice (arg: msg_bits, app_bits
or qlen; opt: option gdbf_kernel).

On the host: tests/native/wave_cw_host.cpp, a stand-alone program over wave_cw_plan.h and the
*_layout.h headers, compiled with -fsanitize=address,undefined and run directly, compares
every row exactly. On the device: *_kernel_info of the five codes names the table's kernel and
LDS bytes, or refuses where the table has no kernel; no kernel is launched."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import GOLD, ROOT

TABLE = os.path.join(GOLD, "wave_cw_choices.json")
CODES = ("PEGReg504x1008.alist", "80211n_1944_r12.alist", "802_3_H.alist", "4000.2000.4.244.alist", "dvbs2_1_2.alist")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_planner_and_layouts_reproduce_the_table_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "wave_cw_host")
    subprocess.run(["g++", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-std=c++17", "-I" + os.path.join(ROOT, "ldpcsimulation_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "native", "wave_cw_host.cpp")],
                   check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe, TABLE], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    with open(TABLE) as f:
        rows = json.load(f)
    named = sum(1 for r in rows if r["name"])
    assert "%d rows, %d with a kernel: ok (0 failures)" % (len(rows), named) in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
    # the table covers what it is meant to
    for fam, names in (("fxms", {"fxms_i8", "fxms_i16", ""}), ("fxlms", {"fxlms_i8", "fxlms_i16", ""}),
                       ("hwgdbf", {"hwgdbf_wave", "hwgdbf_wg", ""})):
        got = [r for r in rows if r["family"] == fam]
        assert {r["name"] for r in got} == names
        assert {r["staged"] for r in got if r["name"]} == {0, 1}
        assert any("tie" in r["note"] for r in got)
    assert any(r["opt"] == 1 and r["name"] == "hwgdbf_wg" for r in rows)


@pytest.mark.gpu
def test_kernel_info_of_the_real_codes_matches_the_table(gpu_ctx_factory):
    from ldpcsimulation_amd import native
    with open(TABLE) as f:
        rows = json.load(f)
    seen = 0
    for code in CODES:
        ctx = gpu_ctx_factory(code, 8)
        g = ctx.graph
        mine = [r for r in rows if (r["N"], r["M"], r["E"]) == (g.N, g.M, g.E)]
        assert {r["family"] for r in mine} == {"fxms", "fxlms", "hwgdbf"} and len(mine) == 6, code
        for r in mine:
            ctx.set_option("gdbf_kernel", r["opt"])
            if r["family"] == "fxms":
                ask = lambda: ctx.fxms_kernel_info(native.FxmsConfig(msg_bits=r["arg"]))
            elif r["family"] == "fxlms":
                ask = lambda: ctx.fxlms_kernel_info(native.FxlmsConfig(msg_bits=r["arg"], app_bits=r["arg"]))
            else:
                ask = lambda: ctx.hwgdbf_kernel_info(native.HwGdbfConfig(qlen=r["arg"]))
            if r["name"]:
                assert ask() == {"kernel": r["name"], "lds_bytes": r["lds_bytes"]}, (code, r)
            else:
                with pytest.raises(native.LdpcError) as e:
                    ask()
                assert e.value.code == -4 and str(r["cw_bytes"]) in str(e.value), (code, r)
            seen += 1
        ctx.reset_options()
    assert seen == 30
