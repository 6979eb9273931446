"""Early termination of the min-sum decoders and BP, the parts that need no GPU: the ABI
keeps its version, option count and struct layout (ldpc_decoder_cfg.reserved became
early_stop at the same offset), DecoderConfig carries the flag, and the sweep takes
--early-stop (not with --schedule layered) and keys its checkpoints with it only when set."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT, code_path
from ldpcsimulation_amd import native, sweep

PEG = "PEGReg504x1008.alist"


def _header():
    return open(os.path.join(ROOT, "include", "ldpc_hip.h")).read()


def test_abi_version_and_option_count_unchanged():
    txt = _header()
    assert re.search(r"#define\s+LDPC_ABI_VERSION\s+11\b", txt)
    assert re.search(r"#define\s+LDPC_OPT_COUNT\s+23\b", txt)
    assert native.lib().ldpc_abi_version() == 11


def test_cfg_layout_unchanged():
    assert C.sizeof(native._Cfg) == 6 * 4 + 3 * 8 + 2 * 4 + 2 * 8
    assert native._Cfg.early_stop.offset == 52 and native._Cfg.early_stop.size == 4
    assert native._Cfg.schedule.offset == 48 and native._Cfg.n0.offset == 56
    assert not hasattr(native._Cfg, "reserved")
    body = re.search(r"typedef struct \{([^}]*)\}\s*ldpc_decoder_cfg;", _header()).group(1)
    names = re.findall(r"^\s*(?:int32_t|double)\s+(\w+);", body, flags=re.M)
    assert names == [n for n, _ in native._Cfg._fields_]


def test_decoder_config_sets_the_field():
    assert native.DecoderConfig().early_stop is False
    assert native.DecoderConfig()._c().early_stop == 0
    assert native.DecoderConfig(variant=native.NMS, alpha=1.25)._c().early_stop == 0
    c = native.DecoderConfig(variant=native.NMS, alpha=1.25, T=50, early_stop=True)._c()
    assert c.early_stop == 1 and c.T == 50 and c.schedule == native.FLOODING


def test_kernel_name_is_documented():
    assert '"rows_es"' in _header()


BASE = [code_path(PEG), "--rate", "0.5", "--snr", "3.0"]


@pytest.mark.parametrize("variant", ["ms", "nms", "oms", "bp"])
def test_sweep_accepts_early_stop(variant):
    a = sweep.parse(BASE + ["--variant", variant, "--early-stop"])
    assert a.early_stop is True
    assert sweep.parse(BASE + ["--variant", variant]).early_stop is False


def test_sweep_refuses_early_stop_with_layered(capsys):
    with pytest.raises(SystemExit) as e:
        sweep.parse(BASE + ["--variant", "nms", "--early-stop", "--schedule", "layered"])
    assert e.value.code == 2
    assert "--early-stop" in capsys.readouterr().err


def test_checkpoint_config_keyed_only_when_set():
    off = sweep._checkpoint_config(sweep.parse(BASE + ["--variant", "nms"]))
    on = sweep._checkpoint_config(sweep.parse(BASE + ["--variant", "nms", "--early-stop"]))
    new = set(on) - set(off)
    assert len(new) == 1 and on[new.pop()] is True
    assert {k: v for k, v in on.items() if k in off} == off
    assert off["early_stop"] is True and on["early_stop"] is True   # the EMS setting's key, as before
    # the families that always stop ignore the flag: their checkpoints do not change
    for extra in (["--variant", "ddbmp", "--ymax", "1.0", "--qbits", "3"], ["--gdbf", "SMNGDBF"], ["--ems"]):
        assert sweep._checkpoint_config(sweep.parse(BASE + extra + ["--early-stop"])) == \
            sweep._checkpoint_config(sweep.parse(BASE + extra))
