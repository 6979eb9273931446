"""The workgroup-per-codeword kernel of layered fixed-point min-sum (fxlms_wg.hip) in the
bounds-checked build (`make checked`, check.h): the schedule entry of every row edge, the APP it
gathers and scatters, the layered position of every row (the index of its state words in the
workgroup's global slot) and the slot itself go through LDPC_CHK. As tests/test_fxlms_checked.py
does, a small batch per case is decoded by the checked library and by the product library, each
in a child process of its own (one library per process), with option kernel = global: no
violation (an LdpcError in the child would fail it), and identical samples, codes, decisions,
per-frame results and counters."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, code_path

CHECKED = os.path.join(ROOT, "ldpcsimulation_amd", "lib", "checked", "libldpc_hip_checked.so")
PEG = "PEGReg504x1008.alist"

# name -> (code, precision, the kernel meant, batch, Eb/N0, rate, cfg fields): two-byte APPs on the code
# with rows of degree 32 (two sign words a row), PEG with checks of degree 0, 1 and 2 and a bit of
# degree 0 at one byte, and DVB-S2 at one byte with early stop (workgroups of 512 threads). The
# batches are no multiple of a wavefront, of a CU count or of a grid.
CASES = {
    "c802_wg_i16_oms": ("802_3_H.alist", "f64", "fxlms_wg_i16", 203, 3.7, 0.8413,
                        dict(variant=2, T=8, msg_bits=12, app_bits=13, beta=1, early_stop=True)),
    "edge_wg_i8_nms": ("edge", "f32", "fxlms_wg_i8", 203, 2.0, 0.5,
                       dict(variant=1, T=8, msg_bits=6, app_bits=7, nms_num=3, nms_shift=2, early_stop=True)),
    "dvbs2_wg_i8_nms": ("dvbs2_1_2.alist", "f32", "fxlms_wg_i8", 37, 2.8, 0.5,
                        dict(variant=1, T=8, msg_bits=8, app_bits=8, nms_num=3, nms_shift=2, early_stop=True)),
}


def run_cases(lib, out):
    """Child process: decode every case with library `lib`, save the results to `out` (npz)."""
    from ldpcsimulation_amd import native
    native.use_library(lib)
    import fxlms_oracle as FL
    res, kern = {}, {}
    for name, (code, prec, _, batch, snr, rate, kw) in CASES.items():
        path = FL.write_edge_code(out + ".edge.alist", code_path(PEG)) if code == "edge" else code_path(code)
        g = native.Graph.from_alist(path)
        ctx = native.Context(g, 0, 256)
        ctx.set_option("kernel", "global")
        cfg = native.FxlmsConfig(precision=native.F64 if prec == "f64" else native.F32, **kw)
        y, ycode, d, fr, cnt = ctx.fxlms_sim_trace(snr, rate, cfg, seed=9, stream_id=1, first_cw=100, batch=batch)
        kern[name] = ctx.fxlms_kernel_info(cfg)["kernel"]
        res[name + "__counts"] = cnt.as_array()
        res[name + "__frames"] = np.asarray(fr).view(np.int32).reshape(len(fr), -1)
        res[name + "__d"], res[name + "__ycode"], res[name + "__y"] = d, ycode, y
    np.savez(out, **res)
    with open(out + ".json", "w") as f:
        json.dump(kern, f)


def _child(lib, out):
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_fxlms_wg_checked as t; "
            "t.run_cases(%r, %r)" % (ROOT, os.path.join(ROOT, "tests"), lib, out))
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)


@pytest.mark.gpu
def test_checked_build_equals_product_on_fxlms_wg(tmp_path):
    from ldpcsimulation_amd import native
    assert os.path.exists(CHECKED), "run `make checked`"
    a, b = str(tmp_path / "product.npz"), str(tmp_path / "checked.npz")
    pa = _child(native.LIB_PATH, a)
    assert pa.returncode == 0, pa.stderr[-3000:]
    pb = _child(CHECKED, b)
    assert pb.returncode == 0, pb.stderr[-3000:]
    ka, kb = json.load(open(a + ".json")), json.load(open(b + ".json"))
    assert ka == kb == {name: c[2] for name, c in CASES.items()}
    ra, rb = np.load(a), np.load(b)
    assert sorted(ra.files) == sorted(rb.files)
    for k in ra.files:
        assert np.array_equal(ra[k], rb[k]), k
    for name, c in CASES.items():   # frames that stop early and frames that run to T
        fr = ra[name + "__frames"]
        assert ra[name + "__counts"][3] == c[3] and (fr[:, 3] < 8).any() and (fr[:, 3] == 8).any(), name
