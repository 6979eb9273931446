"""The re-decoding NGDBF kernels in the bounds-checked build (`make checked`, check.h): the
two schedule-derived LDS indices of rgdbf_rows -- the flag byte a check row gathers, the
parity byte a bit reads or a row writes -- go through LDPC_CHK. As tests/test_ddbmp_checked.py
does, one small batch per kernel is decoded by the checked library and by the product
library, each in a child process of its own (one library per process): no violation (an
LdpcError in the child would fail it), and identical per-frame results and counters."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, code_path

CHECKED = os.path.join(ROOT, "ldpcsimulation_amd", "lib", "checked", "libldpc_hip_checked.so")

# name -> (code, precision, gdbf_kernel option, the kernel meant, Eb/N0)
CASES = {
    "peg_rows_f64": ("PEGReg504x1008.alist", "f64", "rows", "rgdbf_rows", 3.5),
    "peg_rows_f32": ("PEGReg504x1008.alist", "f32", "rows", "rgdbf_rows", 3.5),
    "peg_lds_f64": ("PEGReg504x1008.alist", "f64", "generic", "rgdbf_lds", 3.5),
    "w1944_rows_f64": ("80211n_1944_r12.alist", "f64", "rows", "rgdbf_rows", 4.0),
    "w1944_rows_f32": ("80211n_1944_r12.alist", "f32", "rows", "rgdbf_rows", 4.0),
    "w1944_lds_f32": ("80211n_1944_r12.alist", "f32", "generic", "rgdbf_lds", 4.0),
    "r4000_rows_f64": ("4000.2000.4.244.alist", "f64", "rows", "rgdbf_rows", 3.6),
    "r4000_rows_f32": ("4000.2000.4.244.alist", "f32", "rows", "rgdbf_rows", 3.6),
    "r4000_global_f64": ("4000.2000.4.244.alist", "f64", "generic", "rgdbf_global", 3.6),
}


def run_cases(lib, out):
    """Child process: decode every case with library `lib`, save the results to `out` (npz)."""
    from ldpcsimulation_amd import native
    native.use_library(lib)
    res, kern = {}, {}
    ctxs = {}
    for name, (code, prec, option, _, snr) in CASES.items():
        if code not in ctxs:
            ctxs[code] = native.Context(native.Graph.from_alist(code_path(code)), 0, 512)
        ctx = ctxs[code]
        ctx.set_option("gdbf_kernel", option)
        cfg = native.RgdbfConfig(T=30, maxphase=3, alpha=1.2, precision=native.F64 if prec == "f64" else native.F32)
        fr, cnt = ctx.rgdbf_sim_batch(snr, 0.5, cfg, seed=9, stream_id=1, first_cw=100, batch=400)
        kern[name] = ctx.rgdbf_kernel_info(cfg)["kernel"]
        res[name + "__counts"] = cnt.as_array()
        res[name + "__frames"] = np.asarray(fr).view(np.int32).reshape(len(fr), -1)
    np.savez(out, **res)
    with open(out + ".json", "w") as f:
        json.dump(kern, f)


def _child(lib, out):
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_rgdbf_checked as t; "
            "t.run_cases(%r, %r)" % (ROOT, os.path.join(ROOT, "tests"), lib, out))
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)


@pytest.mark.gpu
def test_checked_build_equals_product_on_rgdbf(tmp_path):
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
    it = ra["peg_rows_f64__frames"][:, 3]
    assert ra["peg_rows_f64__counts"][3] == 400 and (it < 30).any() and (it > 30).any()   # early stops and re-decodes
