"""The host side of layered fixed-point min-sum, without a GPU: the ABI additions, the cfg
refusals (made before any device call), the kernel instances the library carries, the sweep
driver's --fxlms argument rules and its checkpoint settings."""
import ctypes as C
import os
import re
import subprocess
import sys

from conftest import ROOT, code_path
from ldpcsimulation_amd import native, sweep

NAMES = ["ldpc_fxlms_decode_batch", "ldpc_fxlms_sim_launch", "ldpc_fxlms_sim_batch", "ldpc_fxlms_sim_trace",
         "ldpc_fxlms_kernel_info"]
PEG = "PEGReg504x1008.alist"
BASE = [code_path(PEG), "--rate", "0.5", "--snr", "2.0", "-T", "20"]


def test_abi_additions_in_header_and_binding():
    txt = open(os.path.join(ROOT, "include", "ldpc_hip.h")).read()
    assert "#define LDPC_ABI_VERSION 11" in txt and "#define LDPC_OPT_COUNT 23" in txt   # purely additive
    assert native.lib().ldpc_abi_version() == 11 and max(native.OPTIONS.values()) == 22
    for n in NAMES:
        assert re.search(r"\b%s\(" % n, txt) and n in native.EXPORTED and hasattr(native.lib(), n)
    m = re.search(r"typedef struct \{([^}]*)\} ldpc_fxlms_cfg;", txt)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for typ, names in re.findall(r"(int32_t|double)\s+([\w\s,]+);", body):
        fields += [(typ, n.strip()) for n in names.split(",")]
    ctype = {C.c_int32: "int32_t", C.c_double: "double"}
    assert fields == [(ctype[t], n) for n, t in native._FxlmsCfg._fields_]
    names = ["variant", "precision", "T", "qbits", "msg_bits", "app_bits", "nms_num", "nms_shift", "beta", "early_stop", "ymax"]
    assert [n for _, n in fields] == names
    # the C layout: ten int32 and a double, no padding
    assert C.sizeof(native._FxlmsCfg) == 48
    assert [getattr(native._FxlmsCfg, n).offset for n in names] == [4 * i for i in range(10)] + [40]
    raw = native.FxlmsConfig(variant=native.OMS, T=7, qbits=4, msg_bits=9, app_bits=11, nms_num=5, nms_shift=3, beta=2,
                             early_stop=True, ymax=1.5, precision=native.F32)._c()
    assert [getattr(raw, n) for n in names] == [2, 0, 7, 4, 9, 11, 5, 3, 2, 1, 1.5]
    # the defaults: FxmsConfig's, and app_bits = msg_bits + 1 capped at 16
    d, f = native.FxlmsConfig(), native.FxmsConfig()
    assert all(getattr(d, k) == getattr(f, k) for k in ("variant", "T", "qbits", "msg_bits", "nms_num", "nms_shift", "beta",
                                                        "early_stop", "ymax", "precision"))
    assert [native.FxlmsConfig(msg_bits=b).app_bits for b in (6, 15, 16)] == [7, 16, 16]
    # ldpc_fxms_cfg is untouched
    assert C.sizeof(native._FxmsCfg) == 48 and native._FxmsCfg.reserved.offset == 36


def _info(ctx=None, **kw):
    rc = native.lib().ldpc_fxlms_kernel_info(ctx, C.byref(native.FxlmsConfig(**kw)._c()), None, 0, None)
    return rc, native.lib().ldpc_last_error().decode()


def test_cfg_refusals_without_a_device():
    """ldpc_fxlms_kernel_info with a NULL context checks the cfg first and never reaches the
    device: every refusal below is the cfg's and names the field, and a good cfg is refused for
    the context."""
    assert _info() == (-1, "ctx is null")
    nms, oms = dict(variant=native.NMS), dict(variant=native.OMS)
    for bad, word in ((dict(T=-1), "T must"), (dict(qbits=1), "qbits"), (dict(qbits=8), "qbits"),
                      (dict(msg_bits=1, app_bits=8), "msg_bits"), (dict(msg_bits=17, app_bits=16), "msg_bits"),
                      (dict(nms, nms_shift=-1), "nms_shift"), (dict(nms, nms_shift=8, nms_num=1), "nms_shift"),
                      (dict(nms, nms_num=0), "nms_num"), (dict(nms, nms_num=5, nms_shift=2), "nms_num"),
                      (dict(oms, beta=-1), "beta"), (dict(ymax=0.0), "ymax"), (dict(ymax=-1.0), "ymax"),
                      (dict(ymax=float("inf")), "ymax"), (dict(ymax=float("nan")), "ymax"), (dict(precision=2), "precision"),
                      (dict(variant=-1), "variant"), (dict(variant=5), "variant"),
                      (dict(msg_bits=6, app_bits=5), "app_bits"), (dict(msg_bits=6, app_bits=17), "app_bits"),
                      (dict(msg_bits=16, app_bits=15), "app_bits"), (dict(msg_bits=2, app_bits=1), "app_bits"),
                      (dict(msg_bits=6, app_bits=0), "app_bits"), (dict(msg_bits=6, app_bits=-3), "app_bits")):
        rc, msg = _info(**bad)
        assert rc == -1 and word in msg, (bad, msg)
    for v in (native.BP, native.DDBMP):   # another ldpc_variant
        rc, msg = _info(variant=v)
        assert rc == -4 and "variant" in msg
    for es in (2, -1):
        raw = native.FxlmsConfig()._c()
        raw.early_stop = es
        assert native.lib().ldpc_fxlms_kernel_info(None, C.byref(raw), None, 0, None) == -1
        assert "early_stop" in native.lib().ldpc_last_error().decode()
    assert native.lib().ldpc_fxlms_kernel_info(None, None, None, 0, None) == -1
    # the bounds themselves, and fields of another rule are not looked at
    for ok in (dict(T=0), dict(qbits=2), dict(qbits=7), dict(msg_bits=2, app_bits=2), dict(msg_bits=2, app_bits=16),
               dict(msg_bits=16, app_bits=16), dict(msg_bits=8, app_bits=8), dict(msg_bits=6, app_bits=6),
               dict(nms, nms_num=128, nms_shift=7), dict(nms, nms_num=1, nms_shift=0), dict(oms, beta=0),
               dict(variant=native.MS, nms_num=0, beta=-3), dict(oms, nms_num=99), dict(early_stop=True)):
        assert _info(**ok) == (-1, "ctx is null"), ok
    c = C.byref(native.FxlmsConfig()._c())
    for fn, args in (("ldpc_fxlms_sim_batch", (None, 2.0, 0.5, c, 1, 0, 0, 1, None, None)),
                     ("ldpc_fxlms_sim_launch", (None, 2.0, 0.5, c, 1, 0, 0, 1, None)),
                     ("ldpc_fxlms_sim_trace", (None, 2.0, 0.5, c, 1, 0, 0, 1, None, None, None, None, None)),
                     ("ldpc_fxlms_decode_batch", (None, None, 1, c, None, None, None, None))):
        assert getattr(native.lib(), fn)(*args) == -1, fn


def test_library_carries_every_instance():
    """k_fxlms<front-end type, APP type, sample source, schedule-in-LDS> in every combination, and
    the pattern that pins the flooding kernel's instances does not see them."""
    syms = subprocess.run(["nm", "-C", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    got = sorted(set(re.findall(r"ldpc::k_fxlms<([^>]*)>", syms)))
    assert got == sorted(f"{f}, {m}, {s}, {g}" for f in ("double", "float") for m in ("signed char", "short")
                         for s in (0, 1) for g in ("false", "true")), got
    assert len(set(re.findall(r"ldpc::k_fxms<([^>]*)>", syms))) == 16


def test_layers_of_every_row_degree():
    """The row order the decoder walks exists for every graph the library loads, past the row
    degree the floating-point layered kernels take: 802.3an has rows of degree 32."""
    g = native.Graph.from_alist(code_path("802_3_H.alist"))
    assert g.maxdc == 32
    order, ptr = g.layers()
    assert sorted(order.tolist()) == list(range(g.M)) and ptr[0] == 0 and ptr[-1] == g.M
    from ldpcsimulation_amd import codes
    rows = codes.read_alist(code_path("802_3_H.alist")).rows
    for l in range(len(ptr) - 1):
        bits = [b for j in order[ptr[l]:ptr[l + 1]] for b in rows[j]]
        assert len(bits) == len(set(bits))   # rows of a layer share no bit


def test_sweep_arguments():
    a = sweep.parse(BASE + ["--fxlms"])
    assert a.fxlms and not a.fxms
    assert sweep._fxlms_settings(a) == {"ymax": 1.9375, "qbits": 5, "msg_bits": 6, "app_bits": 7, "nms_num": 3, "nms_shift": 2,
                                        "beta": 1}
    a = sweep.parse(BASE + ["--fxlms", "--variant", "nms", "--quantize", "1.75", "3", "--msg-bits", "8", "--app-bits", "12",
                            "--scale", "13", "4", "--early-stop", "--precision", "f32"])
    assert sweep._fxlms_settings(a) == {"ymax": 1.75, "qbits": 3, "msg_bits": 8, "app_bits": 12, "nms_num": 13, "nms_shift": 4,
                                        "beta": 1}
    assert sweep._fxlms_settings(sweep.parse(BASE + ["--fxlms", "--variant", "oms", "--beta", "2"]))["beta"] == 2
    assert sweep._fxlms_settings(sweep.parse(BASE + ["--fxlms", "--msg-bits", "16"]))["app_bits"] == 16
    for bad, word in ((["--fxlms", "--fxms"], "fxlms"), (["--fxlms", "--gdbf", "SMNGDBF"], "fxlms"), (["--fxlms", "--hwgdbf"], "fxlms"),
                      (["--fxlms", "--ems"], "fxlms"), (["--fxlms", "--schedule", "layered"], "fxlms"),
                      (["--fxlms", "--variant", "bp"], "fxlms"), (["--fxlms", "--variant", "ddbmp"], "fxlms"),
                      (["--fxlms", "--alpha", "1.25"], "fxlms"), (["--fxlms", "--delta", "0.1"], "fxlms"),
                      (["--fxlms", "--saturate", "2.0"], "fxlms"), (["--fxlms", "--scale", "3", "2"], "fxlms"),
                      (["--fxlms", "--variant", "nms", "--beta", "1"], "fxlms"),
                      (["--app-bits", "7"], "--app-bits belongs to --fxlms"), (["--fxms", "--app-bits", "7"], "--app-bits belongs to --fxlms"),
                      (["--msg-bits", "6"], "fxms"), (["--scale", "3", "2"], "fxms"), (["--beta", "1"], "fxms"),
                      (["--fxms", "--schedule", "layered"], "--fxms excludes --gdbf, --hwgdbf, --ems and --schedule layered")):
        p = subprocess.run([sys.executable, "-m", "ldpcsimulation_amd.sweep"] + BASE + bad, cwd=ROOT,
                           capture_output=True, text=True, timeout=120)
        assert p.returncode == 2 and word in p.stderr, (bad, p.stderr[-300:])


def test_checkpoint_key():
    """Every fxlms field is a checkpoint setting, and sweeps without --fxlms keep the settings
    they had before the switch existed."""
    keys = {"alist", "alist_md5", "rate", "snr", "T", "variant", "alpha", "delta", "quantize", "saturate",
            "precision", "schedule", "min_bit_errors", "min_frame_errors", "max_frames", "codewords_md5", "ems",
            "nm", "offset", "early_stop"}
    fxms = {"fxms", "ymax", "qbits", "msg_bits", "nms_num", "nms_shift", "beta"}
    assert set(sweep._checkpoint_config(sweep.parse(BASE + ["--variant", "nms", "--alpha", "1.25"]))) == keys
    assert set(sweep._checkpoint_config(sweep.parse(BASE + ["--fxms", "--variant", "nms"]))) == keys | fxms
    nms = ["--fxlms", "--variant", "nms"]
    base = sweep._checkpoint_config(sweep.parse(BASE + nms))
    assert set(base) == keys | fxms | {"fxlms", "app_bits"} and base["fxlms"] is True and base["app_bits"] == 7
    others = [nms + ["--msg-bits", "8"], nms + ["--app-bits", "8"], nms + ["--app-bits", "6"], nms + ["--scale", "13", "4"],
              nms + ["--scale", "3", "3"], nms + ["--quantize", "1.9375", "6"], nms + ["--quantize", "2.0", "5"],
              nms + ["--early-stop"], nms + ["--precision", "f32"], ["--fxlms", "--variant", "oms"], ["--fxlms", "--variant", "ms"],
              ["--fxms", "--variant", "nms"], ["--variant", "nms"]]
    cfgs = [sweep._checkpoint_config(sweep.parse(BASE + o)) for o in others]
    assert all(c != base for c in cfgs) and len({repr(sorted(c.items())) for c in cfgs}) == len(cfgs)
