"""The every-attempt kernels in the bounds-checked build (`make checked`, check.h): the
schedule-derived LDS indices of rstat.hip -- the decision byte a check gathers, the parity
byte a bit reads or a row writes, in both kernel shapes -- go through LDPC_CHK. As tests/test_rgdbf_checked.py does, the given-noise cases are decoded once by the
checked library and once by the product library, each in a child process of its own (one
library per process): no violation (an LdpcError in the child would fail it), and identical
results."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

CHECKED = os.path.join(ROOT, "ldpcsimulation_amd", "lib", "checked", "libldpc_hip_checked.so")

# name -> (recorded run, precision, gdbf_kernel option, the kernel meant, traces)
CASES = {
    "peg_rows_f64": (0, "f64", 0, "rstat_rows", False),
    "peg_rows_f32": (0, "f32", 0, "rstat_rows", False),
    "peg_wg_f64_trace": (0, "f64", 1, "rstat_wg", True),
    "w1944_rows_f64": (1, "f64", 0, "rstat_rows", False),
    "w1944_rows_f32": (1, "f32", 0, "rstat_rows", False),
    "w1944_wg_f64": (1, "f64", 1, "rstat_wg", False),
    "e8023_wg_f64": (2, "f64", 0, "rstat_wg", False),
    "e8023_wg_f32": (2, "f32", 1, "rstat_wg", False),
    "peg_cw_rows_f64": (3, "f64", 0, "rstat_rows", False),
}


def run_cases(lib, out):
    """Child process: decode every case with library `lib`, save the results to `out` (npz)."""
    import rstat_oracle as SO
    from conftest import code_path
    from ldpcsimulation_amd import native
    native.use_library(lib)
    runs, _ = SO.golden()
    res, kern, ctxs = {}, {}, {}
    for name, (k, prec, option, _, trace) in CASES.items():
        run = runs[k]
        _, _, _, attempts, _, kw = SO.run_config(run)
        dtype = np.float64 if prec == "f64" else np.float32
        o = SO.replay_run(run, dtype)
        if run["code"] not in ctxs:
            ctxs[run["code"]] = native.Context(native.Graph.from_alist(code_path(run["code"])), 0, 64)
        ctx = ctxs[run["code"]]
        ctx.set_option("gdbf_kernel", option)
        cfg = native.RstatConfig(flags=kw["flags"], T=kw["T"], attempts=attempts, theta=kw["theta"], lambda_=kw["lambda_"],
                                 alpha=kw["alpha"], ymax=kw["ymax"], windowsize=kw["windowsize"],
                                 precision=native.F64 if prec == "f64" else native.F32)
        att, d, fr, cnt, tr = ctx.rstat_decode(o["y"], o["pert"], cfg, c=o["c"], want_trace=trace)
        kern[name] = ctx.rstat_kernel_info(cfg, with_trace=trace)["kernel"]
        res[name + "__counts"] = cnt.as_array()
        res[name + "__attempts"] = np.asarray(att).view(np.int32).reshape(att.shape + (4,))
        res[name + "__want"] = o["attempts_out"].astype(np.int32)
        res[name + "__d"] = d
        if trace:
            res[name + "__err_trace"] = tr["err_trace"]
    np.savez(out, **res)
    with open(out + ".json", "w") as f:
        json.dump(kern, f)


def _child(lib, out):
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_rstat_checked as t; "
            "t.run_cases(%r, %r)" % (ROOT, os.path.join(ROOT, "tests"), lib, out))
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)


@pytest.mark.gpu
def test_checked_build_equals_product_on_rstat(tmp_path):
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
    for name in CASES:
        assert np.array_equal(rb[name + "__attempts"], rb[name + "__want"]), name
