"""The DD-BMP kernels in the bounds-checked build (`make checked`, check.h): every
schedule-derived LDS or global index of ddbmp.hip -- an edge's flag slot in its row, a
check's parity byte -- goes through LDPC_CHK. As tests/test_checked_build.py does for the
other families, one small batch per kernel is decoded by the checked library and by the
product library, each in a child process of its own (one library per process): no
violation (an LdpcError in the child would fail it), and identical decisions, per-frame
results and counters."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, code_path

CHECKED = os.path.join(ROOT, "ldpcsimulation_amd", "lib", "checked", "libldpc_hip_checked.so")

# name -> (code, precision, ddbmp_kernel option, the kernel meant)
CASES = {
    "peg_rows_f64": ("PEGReg504x1008.alist", "f64", "rows", "ddbmp_rows"),
    "peg_rows_f32": ("PEGReg504x1008.alist", "f32", "rows", "ddbmp_rows"),
    "peg_lds_f64": ("PEGReg504x1008.alist", "f64", "generic", "ddbmp_lds"),
    "w1944_rows_f64": ("80211n_1944_r12.alist", "f64", "rows", "ddbmp_rows"),
    "w1944_rows_f32": ("80211n_1944_r12.alist", "f32", "rows", "ddbmp_rows"),
    "w1944_lds_f32": ("80211n_1944_r12.alist", "f32", "generic", "ddbmp_lds"),
}


def run_cases(lib, out):
    """Child process: decode every case with library `lib`, save the results to `out` (npz)."""
    from ldpcsimulation_amd import native
    native.use_library(lib)
    res, kern = {}, {}
    ctxs = {}
    for name, (code, prec, option, _) in CASES.items():
        if code not in ctxs:
            ctxs[code] = native.Context(native.Graph.from_alist(code_path(code)), 0, 512)
        ctx = ctxs[code]
        ctx.set_option("ddbmp_kernel", option)
        cfg = native.DecoderConfig(variant=native.DDBMP, T=30, quantize=True, ymax=1.0, qbits=3,
                                   precision=native.F64 if prec == "f64" else native.F32)
        _, d, fr, cnt = ctx.sim_trace(4.5, 0.5, cfg, seed=9, stream_id=1, first_cw=100, batch=400)
        kern[name] = ctx.kernel_info(cfg)["kernel"]
        res[name + "__counts"] = cnt.as_array()
        res[name + "__frames"] = np.asarray(fr).view(np.int32).reshape(len(fr), -1)
        res[name + "__d"] = np.asarray(d)
    np.savez(out, **res)
    with open(out + ".json", "w") as f:
        json.dump(kern, f)


def _child(lib, out):
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_ddbmp_checked as t; "
            "t.run_cases(%r, %r)" % (ROOT, os.path.join(ROOT, "tests"), lib, out))
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)


@pytest.mark.gpu
def test_checked_build_equals_product_on_ddbmp(tmp_path):
    from ldpcsimulation_amd import native
    assert os.path.exists(CHECKED), "run `make checked`"
    a, b = str(tmp_path / "product.npz"), str(tmp_path / "checked.npz")
    pa = _child(native.LIB_PATH, a)
    assert pa.returncode == 0, pa.stderr[-3000:]
    pb = _child(CHECKED, b)
    assert pb.returncode == 0, pb.stderr[-3000:]
    ka, kb = json.load(open(a + ".json")), json.load(open(b + ".json"))
    assert ka == kb == {name: c[3] for name, c in CASES.items()}
    ra, rb = np.load(a), np.load(b)
    assert sorted(ra.files) == sorted(rb.files)
    for k in ra.files:
        assert np.array_equal(ra[k], rb[k]), k
    assert ra["peg_rows_f64__counts"][3] == 400 and 0 < ra["peg_rows_f64__counts"][4] < 30 * 400   # early stops
