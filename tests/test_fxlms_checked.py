"""The layered fixed-point min-sum kernel in the bounds-checked build (`make checked`, check.h):
the schedule entry of every row edge, the APP it gathers and scatters and the packed state of a
layer's row go through LDPC_CHK. As tests/test_fxms_checked.py does, a small batch per case is
decoded by the checked library and by the product library, each in a child process of its own
(one library per process): no violation (an LdpcError in the child would fail it), and
identical per-frame results and counters."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, code_path

CHECKED = os.path.join(ROOT, "ldpcsimulation_amd", "lib", "checked", "libldpc_hip_checked.so")
PEG = "PEGReg504x1008.alist"

# name -> (code, precision, the kernel meant, schedule staged, Eb/N0, rate, cfg fields): two-byte APPs on
# the code with rows of degree 32 (two sign words a row), generated (4, 8)-regular codes that read the
# schedule from global memory, and PEG with checks of degree 0, 1 and 2 and a bit of degree 0
CASES = {
    "c802_i16_oms": ("802_3_H.alist", "f64", "fxlms_i16", True, 3.7, 0.8413,
                     dict(variant=2, T=8, msg_bits=12, app_bits=13, beta=1, early_stop=True)),
    "r8000_i8_global": (8000, "f32", "fxlms_i8", False, 2.2, 0.5,
                        dict(variant=1, T=8, msg_bits=8, app_bits=8, nms_num=3, nms_shift=2, early_stop=True)),
    "r6400_i16_global": (6400, "f64", "fxlms_i16", False, 2.2, 0.5, dict(variant=2, T=6, msg_bits=12, app_bits=13, beta=1)),
    "edge_i8_nms": ("edge", "f32", "fxlms_i8", True, 2.0, 0.5,
                    dict(variant=1, T=8, msg_bits=6, app_bits=7, nms_num=3, nms_shift=2, early_stop=True)),
}
BATCH = 203   # no multiple of the codewords of a workgroup


def run_cases(lib, out):
    """Child process: decode every case with library `lib`, save the results to `out` (npz)."""
    from ldpcsimulation_amd import native
    native.use_library(lib)
    import fxlms_oracle as FL
    res, kern = {}, {}
    for name, (code, prec, _, _, snr, rate, kw) in CASES.items():
        if isinstance(code, int):
            path = FL.write_regular_code(out + ".r%d.alist" % code, code)
        elif code == "edge":
            path = FL.write_edge_code(out + ".edge.alist", code_path(PEG))
        else:
            path = code_path(code)
        g = native.Graph.from_alist(path)
        ctx = native.Context(g, 0, 512)
        cfg = native.FxlmsConfig(precision=native.F64 if prec == "f64" else native.F32, **kw)
        y, ycode, d, fr, cnt = ctx.fxlms_sim_trace(snr, rate, cfg, seed=9, stream_id=1, first_cw=100, batch=BATCH)
        info = ctx.fxlms_kernel_info(cfg)
        cw, sched = FL.cw_bytes(g.N, g.M, g.maxdc, kw["app_bits"]), FL.sched_bytes(g.M, g.maxdc)
        kern[name] = [info["kernel"], info["lds_bytes"] % cw != 0 and (info["lds_bytes"] - sched) % cw == 0]
        res[name + "__counts"] = cnt.as_array()
        res[name + "__frames"] = np.asarray(fr).view(np.int32).reshape(len(fr), -1)
        res[name + "__d"], res[name + "__ycode"] = d, ycode
    np.savez(out, **res)
    with open(out + ".json", "w") as f:
        json.dump(kern, f)


def _child(lib, out):
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_fxlms_checked as t; "
            "t.run_cases(%r, %r)" % (ROOT, os.path.join(ROOT, "tests"), lib, out))
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)


@pytest.mark.gpu
def test_checked_build_equals_product_on_fxlms(tmp_path):
    from ldpcsimulation_amd import native
    assert os.path.exists(CHECKED), "run `make checked`"
    a, b = str(tmp_path / "product.npz"), str(tmp_path / "checked.npz")
    pa = _child(native.LIB_PATH, a)
    assert pa.returncode == 0, pa.stderr[-3000:]
    pb = _child(CHECKED, b)
    assert pb.returncode == 0, pb.stderr[-3000:]
    ka, kb = json.load(open(a + ".json")), json.load(open(b + ".json"))
    assert ka == kb == {name: [c[2], c[3]] for name, c in CASES.items()}
    ra, rb = np.load(a), np.load(b)
    assert sorted(ra.files) == sorted(rb.files)
    for k in ra.files:
        assert np.array_equal(ra[k], rb[k]), k
    fr = ra["c802_i16_oms__frames"]
    assert ra["c802_i16_oms__counts"][3] == BATCH and (fr[:, 3] < 8).any() and (fr[:, 3] == 8).any()
