"""k_rows_ppi in the bounds-checked build (`make checked`, check.h): the schedule-derived
LDS indices of the in-register schedule -- the app entries a check row gathers (the staged
sample of its in-register bit among them), the c2v slots it scatters to, the slots a bit
reads, the app entry it writes, the per-thread pair flags -- go through LDPC_CHK. As
tests/test_early_stop_checked.py does, the checked library and the product library each
decode the same frames in a child process of their own: no violation (an LdpcError in the
child would fail it) and identical channel samples, decisions, per-frame results and
counters. Bench code, batch 64, T 5, fp64 (k_rows_ppi) and fp32 pairs (k_rows_pp: the fp32
pairs measured slower with in-register bits and keep every bit in LDS)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, code_path

CHECKED = os.path.join(ROOT, "ldpcsimulation_amd", "lib", "checked", "libldpc_hip_checked.so")
CODE = "80211n_1944_r12.alist"


def run_cases(lib, out):
    """Child process: decode both precisions with library `lib`, save the results to `out` (npz)."""
    from ldpcsimulation_amd import native
    native.use_library(lib)
    ctx = native.Context(native.Graph.from_alist(code_path(CODE)), 0, 64)
    res, info = {}, {}
    for name, prec in (("f64", native.F64), ("f32", native.F32)):
        cfg = native.DecoderConfig(variant=native.NMS, alpha=1.25, T=5, precision=prec)
        info[name] = [ctx.kernel_info(cfg)["kernel"], ctx.pp_inreg_info(cfg)["inreg_bits"]]
        y, d, fr, cnt = ctx.sim_trace(1.5, 0.5, cfg, seed=41, stream_id=1, first_cw=7, batch=64)
        res[name + "__y"] = np.asarray(y)
        res[name + "__d"] = np.asarray(d)
        res[name + "__frames"] = np.asarray(fr).view(np.int32).reshape(len(fr), -1)
        res[name + "__counts"] = cnt.as_array()
    np.savez(out, **res)
    with open(out + ".json", "w") as f:
        json.dump(info, f)


def _child(lib, out):
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_pp_inreg_checked as t; "
            "t.run_cases(%r, %r)" % (ROOT, os.path.join(ROOT, "tests"), lib, out))
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)


@pytest.mark.gpu
def test_checked_build_equals_product_on_rows_ppi(tmp_path):
    from ldpcsimulation_amd import native
    assert os.path.exists(CHECKED), "run `make checked`"
    a, b = str(tmp_path / "product.npz"), str(tmp_path / "checked.npz")
    pa = _child(native.LIB_PATH, a)
    assert pa.returncode == 0, pa.stderr[-3000:]
    pb = _child(CHECKED, b)
    assert pb.returncode == 0, pb.stderr[-3000:]
    ia, ib = json.load(open(a + ".json")), json.load(open(b + ".json"))
    assert ia == ib == {"f64": ["rows_pp", 486], "f32": ["rows_pp", 0]}   # fp32 pairs keep every bit in LDS
    ra, rb = np.load(a), np.load(b)
    assert sorted(ra.files) == sorted(rb.files)
    for k in ra.files:
        assert np.array_equal(ra[k], rb[k]), k
    assert ra["f64__counts"][3] == 64 and ra["f32__counts"][3] == 64
