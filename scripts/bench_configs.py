#!/usr/bin/env python3
"""One measured line per BASELINE config and decoder, each with a named roofline
(VERDICT r5 item 2). Run on the GPU box:

    python scripts/bench_configs.py [--only NAME ...] [--pmc on|off] [--out FILE] [--pmc-dir DIR]

Per config it (1) times the fused on-device simulation (HIP events around the
library's launch: `ldpc_ctx_last_kernel_ms` / `ldpc_nb_ctx_last_kernel_ms`; inputs
are generated on the device, nothing crosses PCIe), then (2) runs four rocprofv3
`--pmc` passes, one counter set each, over a child process that makes exactly one
launch of the same workload (`--child NAME`), and sums the counters of that
launch's dispatches (`ldpc::k_*`, the once-per-context `k_verify_div` excluded).

Every line carries `roofline = {bound, achieved, peak, unit, frac}` for the resource
the counters show busiest, and the other resources' fractions beside it:

* `lds`   -- `SQ_LDS_IDX_ACTIVE` (LDS-array cycles, bank conflicts included) over
             256 CUs x kernel cycles (2.4 GHz); for the two min-sum row kernels
             (configs 1 and 2) the achieved figure is the algorithmic model of
             bench.py (E gathers + E scatters + E bit reads + N app writes at the
             LDS table's conflict-free costs), as in the headline line;
* `valu`  -- VALU issue cycles per SIMD from the instruction mix
             (`SQ_INSTS_VALU_{ADD,MUL,FMA}_F64` 4 cycles per wave64 instruction,
             `SQ_INSTS_VALU_TRANS_F32` and `_F64` 8, every other VALU instruction 2
             -- MI355X_MICROARCH: a wave64 VALU instruction issues over 2 cycles on a
             SIMD-32; fp64 at half that rate) over 1 024 SIMDs x kernel cycles;
             `fp64_flops` (`SQ_INSTS_VALU_FLOPS_FP64` against the 78.6 TFLOP/s fp64
             vector peak) beside it for the fp64 decoders;
* `hbm`   -- memory-side bytes, FETCH_SIZE x 2 + WRITE_SIZE (MI355X_MICROARCH's
             gfx950 correction) per second against 8.0 TB/s (6.29 TB/s achievable).

Which of these binds is a reading of the counters, not a proof: a kernel whose
largest fraction is well below 1 is latency-bound, and the line says so.
Reference paths: src/decodeMinSum.cpp:247-263 (configs 1-3), src/decodeGDBF.cpp:517-621
(config 4), SystemC/NB-LDPC/inc/nodes.h:195-293 (config 5), src/decodeBP.cpp:353-409,
src/decodeDDBMP.cpp:350-423 (the ddbmp_* lines), src/RNGDBF.cpp:277-400 and :552-577 (the
rsmngdbf_* lines; c4_rgdbf_single_* is rgdbf_rows doing gdbf_rows' work on config 4: one phase,
weight 1, for the A/B of the two kernels), src/NGDBFhw.cpp:280-373 and :546-593 (the hwgdbf_*
lines at the reference's constants and its R = 0.8413; *_wg forces the workgroup-per-codeword
instance for the A/B of the two kernel shapes; where that is the library's own choice, the
wavefront shape is measured with --lib on `make hwgdbfvariant VFLAGS=-DLDPC_HWGDBF_FORCE_WAVE`),
src/newstat.cpp:305-429 (the rstat_* lines: 200 frames x 100 attempts as scripts/redecode_statistics_802.3.sh
runs them; *_wg forces the workgroup-per-attempt kernel). The fxms_* lines (fixed-point min-sum,
fxms.hip) have no reference counterpart; nms_1944_* is the floating-point NMS beside them. The
fxlms_* lines are its row-layered form (fxlms.hip) at app_bits = msg_bits + 1, written to
profiles/fxlms_configs.jsonl beside the fxms_* lines of the same session. The fxlms_wg_* lines
force its workgroup-per-codeword kernel (fxlms_wg.hip, option kernel = global): DVB-S2 N=64800,
which only that kernel holds, at two-byte and at one-byte APPs, and N=1944 beside fxlms_1944_nms_m8;
they are written to profiles/fxlms_wg_configs.jsonl.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CLOCK = 2.4e9            # MI355X max shader clock (MI355X_MICROARCH chip table)
CUS = 256
HBM_PEAK = 8.0e12        # spec; 6.29 TB/s measured achievable
HBM_ACHIEVABLE = 6.29e12
FP64_PEAK = 78.6e12      # fp64 vector FLOP/s (half the fp32 vector 157.3 TF)
LDS_CYC = {"ds_read_b64": 2, "ds_write_b64": 6}

# name -> workload (BASELINE.json configs; the headline is config 2, measured by bench.py)
CONFIGS = {
    "c1_peg1008_ms_f64": dict(kind="minsum", code="PEGReg504x1008.alist", variant="ms", prec="f64", T=10,
                              batch=65536, snr=2.0,
                              what="config 1: smallest H (PEG 504x1008), min-sum 10 iterations, fp64"),
    "c2_80211n_nms_f64": dict(kind="minsum", code="80211n_1944_r12.alist", variant="nms", prec="f64", T=50,
                              batch=65536, snr=1.5,
                              what="config 2 (headline): 802.11n N=1944 R1/2, NMS alpha=1.25, T=50, fp64"),
    "c3_dvbs2_flood_f64": dict(kind="minsum", code="dvbs2_1_2.alist", variant="nms", prec="f64", T=50, batch=2048,
                               snr=1.0, what="config 3: DVB-S2 N=64800 R1/2, flooding NMS, T=50, fp64"),
    "c3_dvbs2_layered_f64": dict(kind="minsum", code="dvbs2_1_2.alist", variant="nms", prec="f64", T=50,
                                 batch=2048, snr=1.0, schedule="layered",
                                 what="config 3: DVB-S2 N=64800 R1/2, layered NMS, T=50, fp64"),
    "c4_smngdbf_f32": dict(kind="gdbf", code="80211n_1944_r12.alist", prec="f32", T=100, batch=65536, snr=3.5,
                           what="config 4: SMNGDBF on 802.11n N=1944, T<=100, fp32"),
    "c4_smngdbf_f64": dict(kind="gdbf", code="80211n_1944_r12.alist", prec="f64", T=100, batch=65536, snr=3.5,
                           what="config 4: SMNGDBF on 802.11n N=1944, T<=100, fp64"),
    "c5_ems_gf16": dict(kind="ems", T=20, nm=16, batch=16384, snr=2.0,
                        what="config 5: GF(16) EMS, N=1000 symbols (4000 bits), nm=16, T<=20"),
    # the reference's own non-binary codes (SystemC/NB-LDPC/codes/GF4, GF8), full vectors
    "ems_ref_gf4": dict(kind="ems", code="q4.sp.9000.6000.4500.1.alist", T=20, nm=4, batch=16384, snr=2.0, rate=0.3333,
                        what="GF(4) EMS on the reference's q4.sp.9000.6000 (18000 bits), nm=4, T<=20"),
    "ems_ref_gf8": dict(kind="ems", code="q8.sp.6000.4000.3000.1.alist", T=20, nm=8, batch=16384, snr=2.0, rate=0.3333,
                        what="GF(8) EMS on the reference's q8.sp.6000.4000 (18000 bits), nm=8, T<=20"),
    "bp_80211n_f64": dict(kind="minsum", code="80211n_1944_r12.alist", variant="bp", prec="f64", T=50,
                          batch=16384, snr=1.5, what="BP (tanh rule) on 802.11n N=1944, T=50, fp64"),
    "bp_80211n_f32": dict(kind="minsum", code="80211n_1944_r12.alist", variant="bp", prec="f32", T=50,
                          batch=16384, snr=1.5, what="BP (tanh rule) on 802.11n N=1944, T=50, fp32"),
    # DD-BMP (src/decodeDDBMP.cpp:350-423), Ymax 1.0, Q 3, at an Eb/N0 where most frames stop early
    "ddbmp_80211n_f32": dict(kind="minsum", code="80211n_1944_r12.alist", variant="ddbmp", prec="f32", T=100,
                             batch=65536, snr=5.0, what="DD-BMP on 802.11n N=1944, T<=100, Ymax 1.0, Q 3, fp32"),
    "ddbmp_80211n_f64": dict(kind="minsum", code="80211n_1944_r12.alist", variant="ddbmp", prec="f64", T=100,
                             batch=65536, snr=5.0, what="DD-BMP on 802.11n N=1944, T<=100, Ymax 1.0, Q 3, fp64"),
    "ddbmp_peg1008_f32": dict(kind="minsum", code="PEGReg504x1008.alist", variant="ddbmp", prec="f32", T=100,
                              batch=65536, snr=4.0, what="DD-BMP on PEG 504x1008, T<=100, Ymax 1.0, Q 3, fp32"),
    "ddbmp_peg1008_f64": dict(kind="minsum", code="PEGReg504x1008.alist", variant="ddbmp", prec="f64", T=100,
                              batch=65536, snr=4.0, what="DD-BMP on PEG 504x1008, T<=100, Ymax 1.0, Q 3, fp64"),
    # re-decoding NGDBF (src/RNGDBF.cpp), T<=100 per phase, maxphase 3, theta -0.6, noiseScale 0.75, lambda 0.99,
    # window 16, Ymax 2.5; alpha 1.5 on N=1944 and 0.96 on PEG (the golden runs' settings)
    "rsmngdbf_1944_f32": dict(kind="rgdbf", code="80211n_1944_r12.alist", prec="f32", T=100, maxphase=3, alpha=1.5,
                              batch=65536, snr=3.5, what="RSMNGDBF on 802.11n N=1944, T<=100 x 3 phases, fp32"),
    "rsmngdbf_1944_f64": dict(kind="rgdbf", code="80211n_1944_r12.alist", prec="f64", T=100, maxphase=3, alpha=1.5,
                              batch=65536, snr=3.5, what="RSMNGDBF on 802.11n N=1944, T<=100 x 3 phases, fp64"),
    "rsmngdbf_peg1008_f32": dict(kind="rgdbf", code="PEGReg504x1008.alist", prec="f32", T=100, maxphase=3,
                                 alpha=0.96, batch=65536, snr=3.5,
                                 what="RSMNGDBF on PEG 504x1008, T<=100 x 3 phases, fp32"),
    "rsmngdbf_peg1008_f64": dict(kind="rgdbf", code="PEGReg504x1008.alist", prec="f64", T=100, maxphase=3,
                                 alpha=0.96, batch=65536, snr=3.5,
                                 what="RSMNGDBF on PEG 504x1008, T<=100 x 3 phases, fp64"),
    "c4_gdbf_noweight_f32": dict(kind="gdbf", code="80211n_1944_r12.alist", prec="f32", T=100, weight=False,
                                 batch=65536, snr=3.5, what="config 4 without WEIGHT (weight 1) through gdbf_rows, fp32"),
    "c4_gdbf_noweight_f64": dict(kind="gdbf", code="80211n_1944_r12.alist", prec="f64", T=100, weight=False,
                                 batch=65536, snr=3.5, what="config 4 without WEIGHT (weight 1) through gdbf_rows, fp64"),
    "c4_rgdbf_single_f32": dict(kind="rgdbf", code="80211n_1944_r12.alist", prec="f32", T=100, maxphase=1, alpha=0.8,
                                weight=False, batch=65536, snr=3.5,
                                what="config 4 through rgdbf_rows: one phase, weight 1 (gdbf_rows' work), fp32"),
    "c4_rgdbf_single_f64": dict(kind="rgdbf", code="80211n_1944_r12.alist", prec="f64", T=100, maxphase=1, alpha=0.8,
                                weight=False, batch=65536, snr=3.5,
                                what="config 4 through rgdbf_rows: one phase, weight 1 (gdbf_rows' work), fp64"),
}
# fixed-point NGDBF hardware model (src/NGDBFhw.cpp) at the reference's constants: T<=600, one phase, NQ 5,
# qlen 2648, R 0.8413; 802.3an at 4.0 dB (the golden runs' operating point), PEG 1008 at 6.0 dB
for _code, _tag, _snr in (("802_3_H.alist", "802_3", 4.0), ("PEGReg504x1008.alist", "peg1008", 6.0)):
    for _prec in ("f32", "f64"):
        for _k, _kname in ((0, ""), (1, "_wg")):
            CONFIGS[f"hwgdbf_{_tag}_{_prec}{_kname}"] = dict(
                kind="hwgdbf", code=_code, prec=_prec, T=600, batch=65536, snr=_snr, rate=0.8413, gdbf_kernel=_k,
                what=f"NGDBFhw on {_tag}, T<=600, {_prec} front end, "
                     f"{'hwgdbf_wg forced' if _k else 'the kernel the library chooses'}")

# fixed-point min-sum (integer messages; no reference counterpart) on the headline workload: NMS 3/4, Ymax 31/16,
# Q 5, T=50 at 1.5 dB, and at 3.0 dB with early stop; msg_bits 6 and 8 are one-byte messages, 12 two-byte ones.
# The nms_1944_* lines are the floating-point NMS (alpha 1.25) beside them.
for _snr, _es, _tag in ((1.5, False, ""), (3.0, True, "_es")):
    for _bits in (6, 8, 12):
        CONFIGS[f"fxms_1944_nms_m{_bits}{_tag}"] = dict(
            kind="fxms", code="80211n_1944_r12.alist", prec="f32", T=50, batch=65536, snr=_snr, msg_bits=_bits,
            early_stop=_es, what=f"fixed-point NMS 3/4 on 802.11n N=1944, msg_bits {_bits}, Q 5, T{'<=' if _es else '='}50")
        CONFIGS[f"fxlms_1944_nms_m{_bits}{_tag}"] = dict(
            kind="fxlms", code="80211n_1944_r12.alist", prec="f32", T=50, batch=65536, snr=_snr, msg_bits=_bits,
            early_stop=_es, what=f"layered fixed-point NMS 3/4 on 802.11n N=1944, msg_bits {_bits}, app_bits {_bits + 1}, "
                                 f"Q 5, T{'<=' if _es else '='}50")
    # the workgroup-per-codeword kernel: DVB-S2 at 8/9 bits (two-byte APPs) and 8/8 (one-byte) -- 8,192 frames, 16 or
    # 32 for each resident workgroup, at config 3's 1.0 dB and with early stop at 1.4 dB -- and N=1944 at 8/9
    _dsnr = 1.4 if _es else 1.0
    for _name, _code, _app, _batch, _wsnr in (("dvbs2_nms_m8", "dvbs2_1_2.alist", 9, 8192, _dsnr),
                                              ("dvbs2_nms_m8a8", "dvbs2_1_2.alist", 8, 8192, _dsnr),
                                              ("1944_nms_m8", "80211n_1944_r12.alist", 9, 65536, _snr)):
        CONFIGS[f"fxlms_wg_{_name}{_tag}"] = dict(
            kind="fxlms", code=_code, prec="f32", T=50, batch=_batch, snr=_wsnr, msg_bits=8, app_bits=_app,
            early_stop=_es, kernel="global",
            what=f"layered fixed-point NMS 3/4 on {_code.split('.')[0]}, msg_bits 8, app_bits {_app}, Q 5, "
                 f"T{'<=' if _es else '='}50, fxlms_wg forced")
    for _prec in ("f32", "f64"):
        CONFIGS[f"nms_1944_{_prec}{_tag}"] = dict(
            kind="minsum", code="80211n_1944_r12.alist", variant="nms", prec=_prec, T=50, batch=65536, snr=_snr,
            early_stop=_es, what=f"NMS alpha=1.25 on 802.11n N=1944, {_prec}, T{'<=' if _es else '='}50")

# every attempt of every frame (src/newstat.cpp, src/replayGDBF.cpp): NF 200 frames x NR 100 attempts, the shape of
# the reference's scripts/redecode_statistics_802.3.sh (802.3an at 4.0 dB, R 0.8125, T 1000, theta -0.525, noiseScale
# 0.92, lambda 1, alpha 0.5, window 64) and N=1944 at 4.0 dB with the golden run's settings; `batch` counts frames
for _code, _tag, _rate, _kw in (
        ("802_3_H.alist", "802_3", 0.8125, dict(T=1000, theta=-0.525, lambda_=1.0, alpha=0.5, noise_scale=0.92, windowsize=64)),
        ("80211n_1944_r12.alist", "1944", 0.5, dict(T=100, theta=-0.6, lambda_=0.99, alpha=1.5, noise_scale=0.75, windowsize=16))):
    for _prec in ("f32", "f64"):
        for _k, _kname in ((0, ""), (1, "_wg")):
            CONFIGS[f"rstat_{_tag}_{_prec}{_kname}"] = dict(
                kind="rstat", code=_code, prec=_prec, T=_kw["T"], batch=200, attempts=100, snr=4.0, rate=_rate, cfg=_kw,
                gdbf_kernel=_k,
                what=f"redecodeStatistics on {_tag}: 200 frames x 100 attempts, T<={_kw['T']}, {_prec}, "
                     f"{'rstat_wg forced' if _k else 'the kernel the library chooses'}; value counts attempts x N bits, "
                     f"avg_iters is per frame (summed over its attempts)")

PMC_PASSES = [
    "SQ_WAVES SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_SALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY "
    "GRBM_GUI_ACTIVE",
    "SQ_LDS_IDX_ACTIVE SQ_LDS_BANK_CONFLICT SQ_WAIT_INST_LDS SQ_INSTS_VALU_ADD_F64 SQ_INSTS_VALU_MUL_F64 "
    "SQ_INSTS_VALU_FMA_F64 SQ_INSTS_VALU_TRANS_F64 SQ_INSTS_VALU_TRANS_F32 GRBM_GUI_ACTIVE",
    "SQ_INSTS_VALU_FLOPS_FP64 SQ_INSTS_VALU_FLOPS_FP32 SQ_INSTS_VALU_INT32 SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS "
    "GRBM_GUI_ACTIVE",
    "FETCH_SIZE GRBM_GUI_ACTIVE",
    "WRITE_SIZE TCC_HIT_sum TCC_MISS_sum GRBM_GUI_ACTIVE",
]


# --latency: the memory pipeline's occupancy and latencies (Little's law per CU)
LATENCY_PASSES = [
    "TCP_TCC_READ_REQ_sum TCP_TCC_READ_REQ_LATENCY_sum TCP_TCC_WRITE_REQ_sum TCP_PENDING_STALL_CYCLES_sum "
    "GRBM_GUI_ACTIVE",
    "TCC_REQ_sum TCC_BUSY_sum TCC_EA0_RDREQ_sum TCC_EA0_RDREQ_LEVEL_sum GRBM_GUI_ACTIVE",
    "SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INST_CYCLES_VMEM_RD SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_BUSY_CYCLES "
    "TA_BUSY_sum TA_ADDR_STALLED_BY_TC_CYCLES_sum GRBM_GUI_ACTIVE",
]


class Workload:
    """One config's context and launch, through the C ABI (native.py)."""

    def __init__(self, name, lib=None):
        from ldpcsimulation_amd import codes, native
        if lib:
            native.use_library(os.path.abspath(lib))
        from conftest import code_path
        self.native, self.name, self.c = native, name, CONFIGS[name]
        c = self.c
        if c["kind"] == "ems":
            self.g = native.NbGraph.from_alist(code_path(c["code"]) if "code" in c else codes.ensure_gf16_code())
            self.ctx = native.NbContext(self.g, 0, c["batch"])
            self.cfg = native.EmsConfig(T=c["T"], nm=c["nm"], offset=0.0, early_stop=True)
            self.bits = self.g.N * self.g.m
            self.launch_fn = self.ctx.sim_launch
            self.kernel = self.ctx.kernel_info()["kernel"]
            return
        self.g = native.Graph.from_alist(code_path(c["code"]))
        self.ctx = native.Context(self.g, 0, c["batch"])
        prec = native.F64 if c["prec"] == "f64" else native.F32
        self.bits = self.g.N
        if c["kind"] == "gdbf":
            self.cfg = native.GdbfConfig(T=c["T"], precision=prec)
            if not c.get("weight", True):
                self.cfg.flags &= ~native.GDBF_WEIGHT
            self.launch_fn = self.ctx.gdbf_sim_launch
            self.kernel = self.ctx.gdbf_kernel_info(self.cfg)["kernel"]
        elif c["kind"] == "rgdbf":
            flags = native.RGDBF_FLAGS if c.get("weight", True) else native.RGDBF_FLAGS & ~native.GDBF_WEIGHT
            self.cfg = native.RgdbfConfig(flags=flags, T=c["T"], maxphase=c["maxphase"], alpha=c["alpha"],
                                          precision=prec)
            self.launch_fn = self.ctx.rgdbf_sim_launch
            self.kernel = self.ctx.rgdbf_kernel_info(self.cfg)["kernel"]
        elif c["kind"] == "rstat":
            self.cfg = native.RstatConfig(attempts=c["attempts"], ymax=2.5, precision=prec, **c["cfg"])
            self.ctx.set_option("gdbf_kernel", c["gdbf_kernel"])
            self.bits = self.g.N * c["attempts"]
            self.launch_fn = self.ctx.rstat_sim_launch
            self.kernel = self.ctx.rstat_kernel_info(self.cfg)["kernel"]
        elif c["kind"] == "hwgdbf":
            self.cfg = native.HwGdbfConfig(T=c["T"], precision=prec)
            self.ctx.set_option("gdbf_kernel", c["gdbf_kernel"])
            self.launch_fn = self.ctx.hwgdbf_sim_launch
            info = self.ctx.hwgdbf_kernel_info(self.cfg)
            self.kernel, self.lds_bytes = info["kernel"], info["lds_bytes"]
        elif c["kind"] == "fxms":
            self.cfg = native.FxmsConfig(variant=native.NMS, T=c["T"], qbits=5, msg_bits=c["msg_bits"], nms_num=3,
                                         nms_shift=2, early_stop=c["early_stop"], ymax=31 / 16, precision=prec)
            self.launch_fn = self.ctx.fxms_sim_launch
            info = self.ctx.fxms_kernel_info(self.cfg)
            self.kernel, self.lds_bytes = info["kernel"], info["lds_bytes"]
        elif c["kind"] == "fxlms":
            if c.get("kernel"):
                self.ctx.set_option("kernel", c["kernel"])
            self.cfg = native.FxlmsConfig(variant=native.NMS, T=c["T"], qbits=5, msg_bits=c["msg_bits"],
                                          app_bits=c.get("app_bits", c["msg_bits"] + 1), nms_num=3, nms_shift=2, early_stop=c["early_stop"],
                                          ymax=31 / 16, precision=prec)
            self.launch_fn = self.ctx.fxlms_sim_launch
            info = self.ctx.fxlms_kernel_info(self.cfg)
            self.kernel, self.lds_bytes = info["kernel"], info["lds_bytes"]
        else:
            v = {"ms": dict(variant=native.MS), "nms": dict(variant=native.NMS, alpha=1.25),
                 "bp": dict(variant=native.BP),
                 "ddbmp": dict(variant=native.DDBMP, quantize=True, ymax=1.0, qbits=3)}[c["variant"]]
            sched = native.LAYERED if c.get("schedule") == "layered" else native.FLOODING
            self.cfg = native.DecoderConfig(T=c["T"], precision=prec, schedule=sched, early_stop=c.get("early_stop", False),
                                            **v)
            self.launch_fn = self.ctx.sim_launch
            self.kernel = self.ctx.kernel_info(self.cfg)["kernel"]

    def launch(self, k, batch=None):
        b = batch or self.c["batch"]
        self.launch_fn(self.c["snr"], self.c.get("rate", 0.5), self.cfg, seed=1, stream_id=0, first_cw=k * self.c["batch"], batch=b)
        return self.ctx.last_kernel_ms()

    def counts(self):
        return self.ctx.read_counts(reset=True)


def lds_edges_cycles(w):
    """bench.py's algorithmic LDS model per launch for the two min-sum row kernels (None otherwise)."""
    if w.c["kind"] != "minsum":
        return None
    try:
        si = w.ctx.row_sched_info(w.cfg)
    except w.native.LdpcError:
        return None
    g = w.g
    per = (2 * g.E * LDS_CYC["ds_read_b64"] + g.E * LDS_CYC["ds_write_b64"] + g.N * LDS_CYC["ds_write_b64"]) / 64
    return per * w.c["T"] * w.c["batch"], si


def timed(name, reps, lib):
    w = Workload(name, lib)
    w.launch(reps + 1, batch=min(w.c["batch"], 1024))   # warm-up (code objects, verify_div)
    w.counts()
    kms = []
    t0 = time.perf_counter()
    for k in range(reps):
        kms.append(w.launch(k))
    wall = time.perf_counter() - t0
    cnt = w.counts()
    d = {k: int(v) for k, v in cnt.as_dict().items()}
    frames = d.get("frames")
    kms_best = min(kms)
    out = {"name": name, "what": w.c["what"], "kernel": w.kernel, "batch": w.c["batch"], "T": w.c["T"],
           "ebn0_db": w.c["snr"], "reps": reps, "kernel_ms": kms, "kernel_ms_best": kms_best,
           "value": w.bits * w.c["batch"] / (kms_best / 1e3) / 1e6, "unit": "Mbit/s (coded bits, kernel time)",
           "wall_mbit_s": w.bits * frames / wall / 1e6 if frames else None,
           "fer": d.get("frame_err", 0) / frames if frames else None,
           "avg_iters": d.get("iters", 0) / frames if frames else None, "frames": frames}
    if w.c["kind"] == "rgdbf":   # the phase split of the first launch's frames (phases follow from a frame's iterations)
        import numpy as np
        out["maxphase"] = w.c["maxphase"]
        fr, _ = w.ctx.rgdbf_sim_batch(w.c["snr"], 0.5, w.cfg, seed=1, stream_id=0, first_cw=0, batch=w.c["batch"])
        ph = w.native.rgdbf_phases(fr["iters"], w.c["T"], w.c["maxphase"])
        out["phase_split"] = [int(x) for x in np.bincount(ph, minlength=w.c["maxphase"] + 1)[1:]]
    if w.c["kind"] in ("hwgdbf", "fxms", "fxlms"):
        out["lds_bytes_per_workgroup"] = w.lds_bytes
    m = lds_edges_cycles(w)
    if m:
        out["lds_model_cycles_per_launch"], out["row_sched"] = m
    return out


def child(name, lib):
    """One launch of the workload (under rocprofv3 --pmc)."""
    w = Workload(name, lib)
    w.launch(0)
    w.counts()


def read_pmc(d):
    """Counters of the launch's decode dispatches, summed (k_verify_div excluded)."""
    tot = {}
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            k = r["Kernel_Name"]
            if "ldpc::k_" not in k or "k_verify_div" in k:
                continue
            tot[r["Counter_Name"]] = tot.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
    return tot


def pmc(name, lib, outdir, passes=None):
    tot = {}
    for i, cs in enumerate(passes or PMC_PASSES):
        d = os.path.join(outdir, name, f"p{i + 1}")
        shutil.rmtree(d, ignore_errors=True)
        cmd = ["rocprofv3", "--pmc"] + cs.split() + ["-d", d, "-o", "pmc", "--output-format", "csv", "--",
                                                      sys.executable, os.path.abspath(__file__), "--child", name]
        if lib:
            cmd += ["--lib", lib]
        p = subprocess.run(["timeout", "-s", "KILL", "120"] + cmd, capture_output=True, text=True,
                           env=dict(os.environ, TMPDIR="/tmp"))
        if p.returncode != 0:
            raise RuntimeError(f"pmc pass {i + 1} of {name}: rc {p.returncode}: {p.stderr[-800:]}")
        got = read_pmc(d)
        grbm = got.pop("GRBM_GUI_ACTIVE", None)
        if grbm:
            tot.setdefault("GRBM_GUI_ACTIVE_passes", []).append(grbm)
        tot.update(got)
    return tot


def fractions(line, c):
    """Resource fractions of one launch from its counters and the timed kernel time."""
    t = line["kernel_ms_best"] / 1e3
    cyc = t * CLOCK
    f = {}
    if "SQ_LDS_IDX_ACTIVE" in c:
        f["lds"] = {"achieved": c["SQ_LDS_IDX_ACTIVE"] / t / 1e9, "peak": CUS * CLOCK / 1e9,
                    "unit": "G LDS-array cycles/s (SQ_LDS_IDX_ACTIVE, conflicts included)",
                    "frac": c["SQ_LDS_IDX_ACTIVE"] / (CUS * cyc),
                    "bank_conflict_share": c.get("SQ_LDS_BANK_CONFLICT", 0) / max(c["SQ_LDS_IDX_ACTIVE"], 1)}
        if "lds_model_cycles_per_launch" in line:
            m = line["lds_model_cycles_per_launch"]
            f["lds_algorithmic"] = {"achieved": m / t / 1e9, "peak": CUS * CLOCK / 1e9,
                                    "unit": "G LDS-cycles/s (E gathers + E scatters + E bit reads + N app writes)",
                                    "frac": m / (CUS * cyc)}
    if "SQ_INSTS_VALU" in c:
        f64 = sum(c.get(k, 0) for k in ("SQ_INSTS_VALU_ADD_F64", "SQ_INSTS_VALU_MUL_F64", "SQ_INSTS_VALU_FMA_F64"))
        tr = c.get("SQ_INSTS_VALU_TRANS_F32", 0) + c.get("SQ_INSTS_VALU_TRANS_F64", 0)
        other = c["SQ_INSTS_VALU"] - f64 - tr
        issue = 2 * other + 4 * f64 + 8 * tr
        f["valu"] = {"achieved": issue / t / 1e9, "peak": CUS * 4 * CLOCK / 1e9,
                     "unit": "G SIMD issue-cycles/s (instruction mix: 2 / fp64 add-mul-fma 4 / transcendental 8)",
                     "frac": issue / (CUS * 4 * cyc),
                     "valu_instr_per_cu_cycle": c["SQ_INSTS_VALU"] / (CUS * cyc),
                     "mix": {"fp64_add_mul_fma": f64, "transcendental": tr, "other": other}}
    if c.get("SQ_INSTS_VALU_FLOPS_FP64"):
        f["fp64_flops"] = {"achieved": c["SQ_INSTS_VALU_FLOPS_FP64"] / t / 1e12, "peak": FP64_PEAK / 1e12,
                           "unit": "TFLOP/s fp64 (SQ_INSTS_VALU_FLOPS_FP64)",
                           "frac": c["SQ_INSTS_VALU_FLOPS_FP64"] / t / FP64_PEAK}
    if "FETCH_SIZE" in c and "WRITE_SIZE" in c:
        b = 2 * c["FETCH_SIZE"] * 1024 + c["WRITE_SIZE"] * 1024   # rocprofv3 reports KB
        f["hbm"] = {"achieved": b / t / 1e9, "peak": HBM_PEAK / 1e9, "unit": "GB/s (FETCH_SIZE x 2 + WRITE_SIZE)",
                    "frac": b / t / HBM_PEAK, "frac_of_achievable": b / t / HBM_ACHIEVABLE, "bytes_per_launch": b}
    if "SQ_WAIT_ANY" in c and "SQ_WAVE_CYCLES" in c:
        f["wait_any_share"] = c["SQ_WAIT_ANY"] / c["SQ_WAVE_CYCLES"]
    g = c.get("GRBM_GUI_ACTIVE_passes")
    if g:
        f["profiled_clock_ghz"] = sum(g) / len(g) / 8 / t / 1e9   # approximate: profiled launch vs timed launch
    return f


def latency(line, c):
    """Little's law per CU from the latency passes: average TCP->TCC read requests in
    flight = sum of their latencies / kernel cycles; bytes per cycle = in flight x 64 B /
    latency (the measured rate, restated); and the occupancy of the units in between."""
    g = c.get("GRBM_GUI_ACTIVE_passes")
    cyc = (sum(g) / len(g) / 8) if g else line["kernel_ms_best"] / 1e3 * CLOCK   # per-XCD cycles of the launch
    out = {"kernel_cycles": cyc}
    rq, lat = c.get("TCP_TCC_READ_REQ_sum"), c.get("TCP_TCC_READ_REQ_LATENCY_sum")
    if rq and lat:
        out["tcp_tcc_read_latency_cycles"] = lat / rq
        out["tcp_tcc_reads_in_flight_per_cu"] = lat / (CUS * cyc)
        out["tcp_tcc_read_req_per_cu_cycle"] = rq / (CUS * cyc)
        out["littles_law_read_bytes_per_cu_cycle_64B"] = out["tcp_tcc_reads_in_flight_per_cu"] * 64 / out[
            "tcp_tcc_read_latency_cycles"]
    if c.get("TCP_TCC_WRITE_REQ_sum"):
        out["tcp_tcc_write_req_per_cu_cycle"] = c["TCP_TCC_WRITE_REQ_sum"] / (CUS * cyc)
    if c.get("TCP_PENDING_STALL_CYCLES_sum") is not None:
        out["tcp_pending_stall_share"] = c["TCP_PENDING_STALL_CYCLES_sum"] / (CUS * cyc)
    if c.get("TCC_EA0_RDREQ_sum") and c.get("TCC_EA0_RDREQ_LEVEL_sum"):
        out["fabric_read_latency_cycles"] = c["TCC_EA0_RDREQ_LEVEL_sum"] / c["TCC_EA0_RDREQ_sum"]
        out["fabric_reads_in_flight_per_xcd"] = c["TCC_EA0_RDREQ_LEVEL_sum"] / (8 * cyc)
    if c.get("TCC_BUSY_sum"):
        out["tcc_busy_share"] = c["TCC_BUSY_sum"] / (128 * cyc)   # 16 channels x 8 XCDs
    if c.get("TCC_REQ_sum"):
        out["tcc_req_per_channel_cycle"] = c["TCC_REQ_sum"] / (128 * cyc)
    if c.get("TA_BUSY_sum"):
        out["ta_busy_share"] = c["TA_BUSY_sum"] / (CUS * cyc)
        out["ta_addr_stalled_by_tc_share"] = c.get("TA_ADDR_STALLED_BY_TC_CYCLES_sum", 0) / (CUS * cyc)
    if c.get("SQ_INSTS_VMEM_RD"):
        out["vmem_rd_instr_per_cu_cycle"] = c["SQ_INSTS_VMEM_RD"] / (CUS * cyc)
        out["vmem_wr_instr_per_cu_cycle"] = c.get("SQ_INSTS_VMEM_WR", 0) / (CUS * cyc)
    if c.get("SQ_WAIT_ANY") and c.get("SQ_WAVE_CYCLES"):
        out["wait_any_share"] = c["SQ_WAIT_ANY"] / c["SQ_WAVE_CYCLES"]
    return out


def roofline(line, f):
    """The binding resource: the largest fraction (LDS kernels keep the algorithmic model)."""
    cand = {k: v for k, v in f.items() if k in ("lds", "valu", "hbm")}
    if not cand:
        return None
    k = max(cand, key=lambda x: cand[x]["frac"])
    r = cand[k]
    if k == "lds" and "lds_algorithmic" in f:
        r = f["lds_algorithmic"]
    out = {"bound": k, "achieved": r["achieved"], "peak": r["peak"], "unit": r["unit"], "frac": r["frac"]}
    if cand[k]["frac"] < 0.7:
        out["note"] = ("no resource above 0.7 of its peak: latency-bound (wait_any_share %.2f)"
                       % f.get("wait_any_share", float("nan")))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pmc", choices=["on", "off"], default="on")
    ap.add_argument("--pmc-dir", default=os.path.join(ROOT, "gpurun_out", "bench_configs_pmc"))
    ap.add_argument("--out", default=None, help="append the JSON lines here too")
    ap.add_argument("--child", default=None)
    ap.add_argument("--lib", default=None, help="A/B only: another build of the decoder library")
    ap.add_argument("--latency", action="store_true", help="also the memory-latency passes (Little's law)")
    a = ap.parse_args()
    if a.child:
        child(a.child, a.lib)
        return 0
    names = a.only or list(CONFIGS)
    for n in names:
        if n not in CONFIGS:
            sys.exit(f"unknown config {n}; known: {', '.join(CONFIGS)}")
    for n in names:
        # the timed run in a child process of its own (one context, one device state per config)
        p = subprocess.run([sys.executable, "-c",
                            "import json,sys; sys.argv=['x']; sys.path.insert(0, %r); import bench_configs as b; "
                            "print(json.dumps(b.timed(%r, %d, %r)))" % (os.path.dirname(os.path.abspath(__file__)),
                                                                         n, a.reps, a.lib)],
                           capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            raise RuntimeError(f"timed run of {n}: {p.stderr[-1500:]}")
        line = json.loads(p.stdout.strip().splitlines()[-1])
        if a.pmc == "on":
            c = pmc(n, a.lib, a.pmc_dir)
            f = fractions(line, c)
            line["fractions"] = f
            line["roofline"] = roofline(line, f)
            line["pmc"] = {k: v for k, v in c.items()}
            line["pmc_source"] = "rocprofv3 --pmc, %d passes over one launch (%s)" % (
                len(PMC_PASSES), os.path.relpath(os.path.join(a.pmc_dir, n), ROOT))
        if a.latency:
            cl = pmc(n, a.lib, os.path.join(a.pmc_dir, "latency"), LATENCY_PASSES)
            line["latency"] = latency(line, cl)
            line["latency_pmc"] = cl
        s = json.dumps(line)
        print(s, flush=True)
        if a.out:
            with open(a.out, "a") as fo:
                fo.write(s + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
