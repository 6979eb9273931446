"""The fixed-point min-sum kernels in the bounds-checked build (`make checked`, check.h): the
message slot of every check and bit edge and the decision byte a check gathers go through
LDPC_CHK. As tests/test_hwgdbf_checked.py does, a small batch per case is decoded by the
checked library and by the product library, each in a child process of its own (one library
per process): no violation (an LdpcError in the child would fail it), and identical per-frame
results and counters."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, code_path

CHECKED = os.path.join(ROOT, "ldpcsimulation_amd", "lib", "checked", "libldpc_hip_checked.so")

# name -> (code, precision, the kernel meant, Eb/N0, rate, cfg fields): one-byte messages on the
# code with column degree 11, two-byte messages on the code with rows of degree 32
CASES = {
    "w1944_i8_nms": ("80211n_1944_r12.alist", "f32", "fxms_i8", 1.6, 0.5,
                     dict(variant=1, T=20, msg_bits=6, nms_num=3, nms_shift=2, early_stop=True)),
    "c802_i16_oms": ("802_3_H.alist", "f64", "fxms_i16", 3.7, 0.8413, dict(variant=2, T=12, msg_bits=12, beta=1)),
    # generated (4, 8)-regular codes whose graph copy does not fit beside a codeword: the instances that
    # take the slot of an edge and the bits of a check from global memory (tests/test_fxms.py)
    "r8000_i8_global": (8000, "f32", "fxms_i8", 2.2, 0.5,
                        dict(variant=1, T=12, msg_bits=6, nms_num=3, nms_shift=2, early_stop=True)),
    "r6400_i16_global": (6400, "f64", "fxms_i16", 2.2, 0.5, dict(variant=2, T=8, msg_bits=12, beta=1)),
}
BATCH = 203   # no multiple of the codewords of a workgroup


def run_cases(lib, out):
    """Child process: decode every case with library `lib`, save the results to `out` (npz)."""
    from ldpcsimulation_amd import native
    native.use_library(lib)
    import fxms_oracle as FO
    res, kern = {}, {}
    for name, (code, prec, _, snr, rate, kw) in CASES.items():
        path = FO.write_regular_code(out + ".r%d.alist" % code, code) if isinstance(code, int) else code_path(code)
        ctx = native.Context(native.Graph.from_alist(path), 0, 512)
        cfg = native.FxmsConfig(precision=native.F64 if prec == "f64" else native.F32, **kw)
        y, ycode, d, fr, cnt = ctx.fxms_sim_trace(snr, rate, cfg, seed=9, stream_id=1, first_cw=100, batch=BATCH)
        info = ctx.fxms_kernel_info(cfg)
        kern[name] = info["kernel"]
        if isinstance(code, int):   # whole codeword states and no graph copy in the workgroup's LDS
            assert info["lds_bytes"] % FO.cw_bytes(code, code // 2, 8, kw["msg_bits"]) == 0, info
        res[name + "__counts"] = cnt.as_array()
        res[name + "__frames"] = np.asarray(fr).view(np.int32).reshape(len(fr), -1)
        res[name + "__d"], res[name + "__ycode"] = d, ycode
    np.savez(out, **res)
    with open(out + ".json", "w") as f:
        json.dump(kern, f)


def _child(lib, out):
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_fxms_checked as t; "
            "t.run_cases(%r, %r)" % (ROOT, os.path.join(ROOT, "tests"), lib, out))
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)


@pytest.mark.gpu
def test_checked_build_equals_product_on_fxms(tmp_path):
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
    fr = ra["w1944_i8_nms__frames"]
    assert ra["w1944_i8_nms__counts"][3] == BATCH and (fr[:, 3] < 20).any() and (fr[:, 3] == 20).any()
    assert 0 < (ra["c802_i16_oms__frames"][:, 0] > 0).sum() < BATCH
