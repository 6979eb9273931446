"""k_rows_es in the bounds-checked build (`make checked`, check.h): every schedule-derived
LDS index of rows_es.hip -- the app entries a check row gathers, the c2v slots it scatters
to, the slots a bit reads and the app entry it writes -- goes through LDPC_CHK. As
tests/test_ddbmp_checked.py does for DD-BMP, the checked library and the product library
each decode the same frames in a child process of their own (one library per process): no
violation (an LdpcError in the child would fail it), and identical decisions, per-frame
results and counters. Cases: test_early_stop's PEG fp64 MS case (DC 8, two rows per thread)
and the widest shape, dc32_cpt4_rpt2 of test_shape_matrix (DC 32, 64-bit row masks)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, code_path

CHECKED = os.path.join(ROOT, "ldpcsimulation_amd", "lib", "checked", "libldpc_hip_checked.so")

# name -> (code, precision, variant of test_gpu_parity.VARIANTS, sigmas, frames, T)
CASES = {
    "peg_f64_ms": ("PEGReg504x1008.alist", "f64", "ms", (0.3, 0.6, 0.75, 0.9), 48, 12),
    "dc32_cpt4_rpt2_f64": ("dc32_cpt4_rpt2", "f64", "nms", (0.2, 0.45, 0.6, 0.7), 32, 10),
    "dc32_cpt4_rpt2_f32": ("dc32_cpt4_rpt2", "f32", "nms", (0.2, 0.45, 0.6, 0.7), 32, 10),
}


def run_cases(lib, out, tmp):
    """Child process: decode every case with library `lib`, save the results to `out` (npz)."""
    from ldpcsimulation_amd import native
    native.use_library(lib)
    from test_early_stop import cfg_of, samples
    from test_gpu_parity import VARIANTS
    from test_shape_matrix import build_code
    res, kern, ctxs = {}, {}, {}
    for name, (code, prec, vname, sigmas, frames, T) in CASES.items():
        if code not in ctxs:
            path = code_path(code) if code.endswith(".alist") else os.path.join(tmp, code + ".alist")
            if not code.endswith(".alist"):
                build_code(path, code)
            ctxs[code] = native.Context(native.Graph.from_alist(path), 0, 64)
        ctx = ctxs[code]
        cfg = cfg_of(prec, VARIANTS[vname], T, early_stop=True)
        d, fr, cnt = ctx.decode(samples(ctx.graph.N, frames, sigmas, prec), cfg)
        kern[name] = ctx.kernel_info(cfg)["kernel"]
        res[name + "__counts"] = cnt.as_array()
        res[name + "__frames"] = np.asarray(fr).view(np.int32).reshape(len(fr), -1)
        res[name + "__d"] = np.asarray(d)
    np.savez(out, **res)
    with open(out + ".json", "w") as f:
        json.dump(kern, f)


def _child(lib, out, tmp):
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_early_stop_checked as t; "
            "t.run_cases(%r, %r, %r)" % (ROOT, os.path.join(ROOT, "tests"), lib, out, tmp))
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)


@pytest.mark.gpu
def test_checked_build_equals_product_on_rows_es(tmp_path):
    from ldpcsimulation_amd import native
    assert os.path.exists(CHECKED), "run `make checked`"
    a, b = str(tmp_path / "product.npz"), str(tmp_path / "checked.npz")
    pa = _child(native.LIB_PATH, a, str(tmp_path))
    assert pa.returncode == 0, pa.stderr[-3000:]
    pb = _child(CHECKED, b, str(tmp_path))
    assert pb.returncode == 0, pb.stderr[-3000:]
    ka, kb = json.load(open(a + ".json")), json.load(open(b + ".json"))
    assert ka == kb == {name: "rows_es" for name in CASES}
    ra, rb = np.load(a), np.load(b)
    assert sorted(ra.files) == sorted(rb.files)
    for k in ra.files:
        assert np.array_equal(ra[k], rb[k]), k
    for name, c in CASES.items():   # early stops: fewer iterations than T per frame, more than none
        cnt = ra[name + "__counts"]
        assert cnt[3] == c[4] and 0 < cnt[4] < c[5] * c[4]
