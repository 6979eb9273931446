"""The launch plan of the binary context, pinned over codes x precision x variant x schedule x option.

What `kernel_info` and `row_sched_info` report (kernel name, dynamic LDS, blocks per CU, the
row schedule's shape) is what bench.py and the kernel-choice assertions of the other tests
read; tests/golden/launch_plan.json is that report as recorded on an MI355X, and a change
to the planner (csrc/kernels.h LaunchPlan, the plan_* of the kernel files) must not move it
unawares. No decoding here: context creation and the two info calls only.

The table holds each distinct {kernel_info, row_sched_info} once ("entries") and, per code,
the entry of every combination in the order KEYS walks them ("codes").

`python tests/test_launch_plan.py OUT.json` records the table (on the device).
"""
import json
import os
import sys

import pytest

from conftest import GOLD, code_path

TABLE = os.path.join(GOLD, "launch_plan.json")
CODES = ["PEGReg504x1008.alist", "80211n_1944_r12.alist", "4000.2000.4.244.alist", "dvbs2_1_2.alist"]
PRECISIONS = ["f32", "f64"]
VARIANTS = ["ms", "nms", "oms", "bp"]
SCHEDULES = ["flooding", "layered"]
OPTION_SETS = [None, ("rows64", "fast"), ("rows64", "rows"), ("rows32", "fast"), ("rows32", "rows"),
               ("pp_slots", "plain"), ("kernel", "lds"), ("kernel", "flood"), ("kernel", "global"),
               ("flood_mode", "persistent"), ("layered_threads", 512), ("bp_kernel", "generic")]
KEYS = [f"{prec}/{variant}/{sched}/{'none' if opt is None else f'{opt[0]}={opt[1]}'}"
        for opt in OPTION_SETS for prec in PRECISIONS for variant in VARIANTS for sched in SCHEDULES]


def _cfg(native, prec, variant, sched):
    v = {"ms": dict(variant=native.MS), "nms": dict(variant=native.NMS, alpha=1.25),
         "oms": dict(variant=native.OMS, delta=0.15), "bp": dict(variant=native.BP, n0=1.0)}[variant]
    return native.DecoderConfig(T=10, precision=native.F64 if prec == "f64" else native.F32,
                                schedule=native.LAYERED if sched == "layered" else native.FLOODING, **v)


def _info(native, call, cfg):
    try:
        return call(cfg)
    except native.LdpcError as e:
        return {"error": e.code}


def collect(code):
    """{"prec/variant/schedule/option": {"kernel_info": ..., "row_sched_info": ...}} of one code."""
    from ldpcsimulation_amd import native
    ctx = native.Context(native.Graph.from_alist(code_path(code)), 0, 4096)
    out = {}
    for opt in OPTION_SETS:
        ctx.reset_options()
        if opt:
            ctx.set_option(*opt)
        oname = "none" if opt is None else f"{opt[0]}={opt[1]}"
        for prec in PRECISIONS:
            for variant in VARIANTS:
                for sched in SCHEDULES:
                    cfg = _cfg(native, prec, variant, sched)
                    out[f"{prec}/{variant}/{sched}/{oname}"] = {
                        "kernel_info": _info(native, ctx.kernel_info, cfg),
                        "row_sched_info": _info(native, ctx.row_sched_info, cfg)}
    return out


@pytest.fixture(scope="module")
def table():
    with open(TABLE) as f:
        t = json.load(f)
    return {code: {k: t["entries"][i] for k, i in zip(KEYS, idx)} for code, idx in t["codes"].items()}


@pytest.mark.gpu
@pytest.mark.parametrize("code", CODES)
def test_launch_plan_is_the_recorded_one(code, table):
    want, got = table[code], collect(code)
    assert list(want) == KEYS and list(got) == KEYS
    diff = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not diff, f"{len(diff)} of {len(want)} entries differ (got, want): {dict(list(diff.items())[:8])}"


if __name__ == "__main__":
    entries, codes = [], {}
    for code in CODES:
        got = collect(code)
        for k in KEYS:
            if got[k] not in entries:
                entries.append(got[k])
        codes[code] = [entries.index(got[k]) for k in KEYS]
    with open(sys.argv[1], "w") as f:
        f.write('{"entries": [\n' + ",\n".join(json.dumps(e, sort_keys=True) for e in entries) + '\n],\n"codes": {\n')
        f.write(",\n".join(f"{json.dumps(c)}: {json.dumps(i, separators=(',', ':'))}" for c, i in codes.items()) + "\n}}\n")
