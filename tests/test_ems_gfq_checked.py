"""The GF(4) / GF(8) EMS instances (nb.hip) in the bounds-checked build (`make checked`, check.h):
every message slot of a check or symbol edge goes through LDPC_CHK. As tests/test_fxlms_wg_checked.py
does, each case is decoded by the checked library and by the product library, each in a child
process of its own (one library per process): no violation (an LdpcError in the child would fail
it), the same kernels, and identical samples, decisions, per-frame results and counters."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, code_path

CHECKED = os.path.join(ROOT, "ldpcsimulation_amd", "lib", "checked", "libldpc_hip_checked.so")
REF_GF4 = "q4.sp.9000.6000.4500.1.alist"
# name -> (code, q, kernel, batch, T, cfg): both fields on the DC = 4 and the DC = 8 build, full and
# truncated vectors, and the reference's GF(4) code on the schedule-from-global instance
CASES = {}
for _q in (4, 8):
    CASES[f"gf{_q}_dc4"] = ((96, 48, 2), _q, "ems_lds", 37, 8, dict(nm=_q, offset=0.0, early_stop=True))
    CASES[f"gf{_q}_dc8_trunc"] = ((120, 40, 2), _q, "ems_lds", 37, 8, dict(nm=_q // 2, offset=0.5, early_stop=True))
CASES["ref_gf4"] = (REF_GF4, 4, "ems_global_sched", 3, 2, dict(nm=4, offset=0.0, early_stop=True))


def run_cases(lib, out):
    """Child process: decode every case with library `lib`, save the results to `out` (npz)."""
    from ldpcsimulation_amd import native
    native.use_library(lib)
    import ems_gfq_common as G
    res, kern = {}, {}
    for name, (code, q, _, batch, T, kw) in CASES.items():
        if isinstance(code, str):
            g, rate = native.NbGraph.from_alist(code_path(code)), 1 / 3
        else:
            H = G.peg_code(*code, q)
            g, rate = native.NbGraph.from_lists(H.N, H.M, H.q, H.cols, H.rows), 1 - code[1] / code[0]
        ctx = native.NbContext(g, 0, 64)
        y, d, fr, cnt = ctx.sim_trace(2.0, rate, native.EmsConfig(T=T, **kw), seed=9, stream_id=1, first_cw=100, batch=batch)
        kern[name] = ctx.kernel_info()["kernel"]
        res[name + "__counts"] = np.frombuffer(bytes(cnt), dtype=np.int64)
        res[name + "__frames"] = np.asarray(fr).view(np.int32).reshape(len(fr), -1)
        res[name + "__d"], res[name + "__y"] = d, y
    np.savez(out, **res)
    with open(out + ".json", "w") as f:
        json.dump(kern, f)


def _child(lib, out):
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_ems_gfq_checked as t; "
            "t.run_cases(%r, %r)" % (ROOT, os.path.join(ROOT, "tests"), lib, out))
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)


@pytest.mark.gpu
def test_checked_build_equals_product_on_gf4_and_gf8(tmp_path):
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
    for name, c in CASES.items():
        fr = ra[name + "__frames"]
        assert ra[name + "__counts"][3] == c[3], name
        if not isinstance(c[0], str):   # frames that stop early and frames that run to T
            assert (fr[:, 3] < c[4]).any() and (fr[:, 3] == c[4]).any(), (name, fr[:, 3])
