"""The NGDBFhw kernels in the bounds-checked build (`make checked`, check.h): the decision
byte a check gathers, the parity byte a bit reads and the noise sample i + qpointer go
through LDPC_CHK. As tests/test_rgdbf_checked.py does, a small batch per case is decoded by
the checked library and by the product library, each in a child process of its own (one
library per process): no violation (an LdpcError in the child would fail it), and identical
per-frame results and counters."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, code_path

CHECKED = os.path.join(ROOT, "ldpcsimulation_amd", "lib", "checked", "libldpc_hip_checked.so")

# name -> (code, precision, gdbf_kernel option, the kernel meant, Eb/N0, cfg fields; qlen None = N + 7)
CASES = {
    "c802_wave_default": ("802_3_H.alist", "f64", 0, "hwgdbf_wave", 3.9, dict()),
    "c802_wg_default": ("802_3_H.alist", "f32", 1, "hwgdbf_wg", 3.9, dict()),
    "c802_wave_wraps": ("802_3_H.alist", "f32", 0, "hwgdbf_wave", 4.2, dict(T=20, maxphase=3, qlen=None)),
    "c802_wg_wraps": ("802_3_H.alist", "f64", 1, "hwgdbf_wg", 4.2, dict(T=20, maxphase=3, qlen=None)),
    "w1944_wave_wraps": ("80211n_1944_r12.alist", "f64", 0, "hwgdbf_wave", 8.0, dict(T=20, maxphase=3, qlen=None)),
}
BATCH = 203   # no multiple of the 4 codewords of a workgroup


def run_cases(lib, out):
    """Child process: decode every case with library `lib`, save the results to `out` (npz)."""
    from ldpcsimulation_amd import native
    native.use_library(lib)
    res, kern, ctxs = {}, {}, {}
    for name, (code, prec, option, _, snr, kw) in CASES.items():
        if code not in ctxs:
            ctxs[code] = native.Context(native.Graph.from_alist(code_path(code)), 0, 512)
        ctx = ctxs[code]
        ctx.set_option("gdbf_kernel", option)
        kw = dict(kw)
        if "qlen" in kw and kw["qlen"] is None:
            kw["qlen"] = ctx.graph.N + 7
        cfg = native.HwGdbfConfig(precision=native.F64 if prec == "f64" else native.F32, **kw)
        fr, cnt = ctx.hwgdbf_sim_batch(snr, 0.8413, cfg, seed=9, stream_id=1, first_cw=100, batch=BATCH)
        kern[name] = ctx.hwgdbf_kernel_info(cfg)["kernel"]
        res[name + "__counts"] = cnt.as_array()
        res[name + "__frames"] = np.asarray(fr).view(np.int32).reshape(len(fr), -1)
    np.savez(out, **res)
    with open(out + ".json", "w") as f:
        json.dump(kern, f)


def _child(lib, out):
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_hwgdbf_checked as t; "
            "t.run_cases(%r, %r)" % (ROOT, os.path.join(ROOT, "tests"), lib, out))
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)


@pytest.mark.gpu
def test_checked_build_equals_product_on_hwgdbf(tmp_path):
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
    it = ra["c802_wave_default__frames"][:, 3]
    assert ra["c802_wave_default__counts"][3] == BATCH and (it < 600).any() and (it == 600).any()
