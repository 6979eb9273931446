"""ctypes binding of the C ABI in include/ldpc_hip.h (libldpc_hip.so).

This is the only way the Python side reaches the decoder: there is no CPU
fallback. If the HIP library is missing, importing this module raises.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "lib", "libldpc_hip.so")

LDPC_OK = 0
MS, NMS, OMS, BP, DDBMP = 0, 1, 2, 3, 4
F32, F64 = 0, 1
FLOODING, LAYERED = 0, 1
ABI_VERSION = 11
# Kernel-selection options (include/ldpc_hip.h ldpc_option): tests and A/B runs set
# them per context through the ABI; the library never reads the environment.
OPTIONS = {"rows64": 1, "rows32": 2, "pp_slots": 3, "kernel": 4, "flood_mode": 5, "flood_msg": 6,
           "flood_sps_check": 7, "flood_sps_bit": 8, "flood_resident": 9, "flood_streams": 10, "flood_bpc": 11,
           "layered_bpc": 12, "layered_lds_pos": 13, "layered_rows64": 14, "layered_threads": 15,
           "rows_bpc": 16, "fast_bpc": 17, "bp_kernel": 18, "gdbf_kernel": 19, "ems_threads": 20,
           "ems_swizzle": 21, "ddbmp_kernel": 22}
# options of the GF(q) EMS context only (ldpc_nb_ctx_set_option); the binary context refuses them
EMS_OPTIONS = ("ems_threads", "ems_swizzle")
# symbolic values of the kernel-choice options
OPTION_VALUES = {"rows64": {"pp": 0, "fast": 1, "rows": 2}, "rows32": {"pp": 0, "fast": 1, "rows": 2},
                 "pp_slots": {"split": 0, "plain": 1, "split_lds": 2, "split_w16": 3},
                 "kernel": {"auto": 0, "lds": 1, "flood": 2, "global": 3},
                 "flood_mode": {"phase": 0, "persistent": 1}, "flood_msg": {"packed": 0, "c2v": 1},
                 "bp_kernel": {"rows": 0, "generic": 1}, "gdbf_kernel": {"rows": 0, "generic": 1},
                 "ddbmp_kernel": {"rows": 0, "generic": 1},
                 "ems_swizzle": {"on": 0, "off": 1}}


def option_id(name) -> int:
    return name if isinstance(name, int) else OPTIONS[name]


def option_value(name, value) -> int:
    if isinstance(value, str) and not isinstance(name, int):
        return OPTION_VALUES[name][value]
    return int(value)


def use_library(path: str):
    """Load another build of the library (A/B variants; `bench.py --lib`). Only before
    the first call into the library; the product path is LIB_PATH."""
    global LIB_PATH
    if _lib is not None and os.path.abspath(path) != os.path.abspath(LIB_PATH):
        raise RuntimeError("the decoder library is already loaded")
    LIB_PATH = path
_STATUS = {0: "OK", -1: "INVALID", -2: "NOMEM", -3: "DEVICE", -4: "UNSUPPORTED", -5: "IO", -6: "GRAPH"}


class LdpcError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"ldpc error {code} ({_STATUS.get(code, '?')}): {msg}")
        self.code = code


class Counts(C.Structure):
    _fields_ = [("bit_err", C.c_int64), ("frame_err", C.c_int64), ("uncoded_bit_err", C.c_int64),
                ("frames", C.c_int64), ("iters", C.c_int64), ("syndrome_fail", C.c_int64)]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}

    def as_array(self) -> np.ndarray:
        return np.array([getattr(self, k) for k, _ in self._fields_], dtype=np.int64)


FRAME_DTYPE = np.dtype([("bit_err", np.int32), ("uncoded_bit_err", np.int32),
                        ("syndrome_fail", np.int32), ("iters", np.int32)])


class _Cfg(C.Structure):
    _fields_ = [("variant", C.c_int32), ("precision", C.c_int32), ("T", C.c_int32),
                ("quantize", C.c_int32), ("saturate", C.c_int32), ("qbits", C.c_int32),
                ("ymax", C.c_double), ("alpha", C.c_double), ("delta", C.c_double),
                ("schedule", C.c_int32), ("early_stop", C.c_int32), ("n0", C.c_double), ("max_llr", C.c_double)]


GDBF_NOISE, GDBF_ADAPT, GDBF_WEIGHT, GDBF_SMOOTH, GDBF_SATURATE, GDBF_QUANTIZE = 1, 2, 4, 8, 16, 32
GDBF_SEQUENTIAL, GDBF_MODESWITCH, GDBF_QPROB = 64, 128, 256
# the reference's decodeGDBF.cpp Makefile targets (C_implementations/Makefile:33-53)
GDBF_VARIANTS = {
    "MNGDBF": GDBF_NOISE | GDBF_ADAPT | GDBF_WEIGHT | GDBF_SATURATE,
    "SMNGDBF": GDBF_NOISE | GDBF_ADAPT | GDBF_WEIGHT | GDBF_SMOOTH | GDBF_SATURATE,
    "ATGDBF": GDBF_ADAPT,
    "SATGDBF": GDBF_ADAPT | GDBF_SMOOTH,
    "SMGDBF": GDBF_SMOOTH,
    "SGDBF": GDBF_SEQUENTIAL,
    "MGDBF": GDBF_MODESWITCH,
    "StochasticNGDBF": GDBF_QUANTIZE | GDBF_QPROB | GDBF_WEIGHT | GDBF_SATURATE,
}


class _GdbfCfg(C.Structure):
    _fields_ = [("flags", C.c_int32), ("precision", C.c_int32), ("T", C.c_int32), ("windowsize", C.c_int32),
                ("nq", C.c_int32), ("tswitch", C.c_int32), ("theta", C.c_double), ("lambda_", C.c_double),
                ("alpha", C.c_double), ("noise_scale", C.c_double), ("ymax", C.c_double), ("qsigma", C.c_double)]


@dataclass
class GdbfConfig:
    """GDBF / NGDBF bit flipping (src/decodeGDBF.cpp parallel mode); flags = the -D switches."""
    flags: int = GDBF_VARIANTS["SMNGDBF"]
    T: int = 100
    theta: float = -0.6
    lambda_: float = 0.99
    alpha: float = 0.8
    noise_scale: float = 0.75
    ymax: float = 2.5
    windowsize: int = 16
    nq: int = 16
    precision: int = 1   # F64, the reference's double (decodeGDBF.cpp); F32 = 0 opt-in
    tswitch: int = 0     # MODESWITCH: Tswitch (:51)
    qsigma: float = 0.0  # QPROB, gdbf_decode only: the normalCDF sigma

    def _c(self) -> _GdbfCfg:
        return _GdbfCfg(self.flags, self.precision, self.T, self.windowsize, self.nq, self.tswitch, self.theta,
                        self.lambda_, self.alpha, self.noise_scale, self.ymax, self.qsigma)


RGDBF_FLAGS = GDBF_NOISE | GDBF_ADAPT | GDBF_WEIGHT | GDBF_SMOOTH | GDBF_SATURATE   # decodeRSMNGDBF sets all five


class _RgdbfCfg(C.Structure):
    _fields_ = [("flags", C.c_int32), ("precision", C.c_int32), ("T", C.c_int32), ("maxphase", C.c_int32),
                ("windowsize", C.c_int32), ("reserved", C.c_int32), ("theta", C.c_double), ("lambda_", C.c_double),
                ("alpha", C.c_double), ("noise_scale", C.c_double), ("ymax", C.c_double)]


@dataclass
class RgdbfConfig:
    """Re-decoding NGDBF (src/RNGDBF.cpp, decodeRSMNGDBF): up to maxphase attempts of T
    iterations each, per-bit syndrome weight alpha*ymax/dv; flags a subset of RGDBF_FLAGS."""
    flags: int = RGDBF_FLAGS
    T: int = 100
    maxphase: int = 3
    theta: float = -0.6
    lambda_: float = 0.99
    alpha: float = 0.96
    noise_scale: float = 0.75
    ymax: float = 2.5
    windowsize: int = 16
    precision: int = 1   # F64, the reference's double (RNGDBF.cpp); F32 = 0 opt-in

    def _c(self) -> _RgdbfCfg:
        return _RgdbfCfg(self.flags, self.precision, self.T, self.maxphase, self.windowsize, 0, self.theta,
                         self.lambda_, self.alpha, self.noise_scale, self.ymax)


class _RstatCfg(C.Structure):
    _fields_ = [("flags", C.c_int32), ("precision", C.c_int32), ("T", C.c_int32), ("attempts", C.c_int32),
                ("windowsize", C.c_int32), ("first_attempt", C.c_int32), ("theta", C.c_double),
                ("lambda_", C.c_double), ("alpha", C.c_double), ("noise_scale", C.c_double), ("ymax", C.c_double)]


class _RstatTrace(C.Structure):
    _fields_ = [("err_trace", C.c_void_p), ("unsat_trace", C.c_void_p), ("d_trace", C.c_void_p),
                ("s_trace", C.c_void_p)]


ATTEMPT_DTYPE = np.dtype([("bit_err", np.int32), ("iters", np.int32), ("syndrome_fail", np.int32),
                          ("smoothing_used", np.int32)])


@dataclass
class RstatConfig:
    """Every attempt of every frame (src/newstat.cpp = redecodeStatistics, src/replayGDBF.cpp):
    `attempts` single-phase decodes of T iterations per frame from the same channel samples,
    all of them run; attempt indices start at first_attempt. flags a subset of RGDBF_FLAGS."""
    flags: int = RGDBF_FLAGS
    T: int = 100
    attempts: int = 5
    first_attempt: int = 0
    theta: float = -0.6
    lambda_: float = 0.99
    alpha: float = 0.96
    noise_scale: float = 0.75
    ymax: float = 2.5
    windowsize: int = 16
    precision: int = 1   # F64, the reference's double; F32 = 0 opt-in

    def _c(self) -> _RstatCfg:
        return _RstatCfg(self.flags, self.precision, self.T, self.attempts, self.windowsize, self.first_attempt,
                         self.theta, self.lambda_, self.alpha, self.noise_scale, self.ymax)


class _HwGdbfCfg(C.Structure):
    _fields_ = [("precision", C.c_int32), ("T", C.c_int32), ("maxphase", C.c_int32), ("nq", C.c_int32),
                ("qlen", C.c_int32), ("reserved", C.c_int32), ("w", C.c_double), ("ymax", C.c_double),
                ("noise_scale", C.c_double), ("theta0", C.c_double)]


@dataclass
class HwGdbfConfig:
    """Fixed-point NGDBF hardware model (src/NGDBFhw.cpp): nq-bit sign-magnitude samples, an
    integer energy, and a noise shift register of qlen samples per frame. The defaults are
    the reference's compile-time constants (:48-57)."""
    T: int = 600
    maxphase: int = 1
    nq: int = 5
    qlen: int = 2648
    w: float = 0.185
    ymax: float = 1.625
    noise_scale: float = 0.95
    theta0: float = -0.525
    precision: int = 1   # front end: F64, the reference's double; F32 = 0 opt-in

    def _c(self) -> _HwGdbfCfg:
        return _HwGdbfCfg(self.precision, self.T, self.maxphase, self.nq, self.qlen, 0, self.w, self.ymax,
                          self.noise_scale, self.theta0)


class _FxmsCfg(C.Structure):
    _fields_ = [("variant", C.c_int32), ("precision", C.c_int32), ("T", C.c_int32), ("qbits", C.c_int32),
                ("msg_bits", C.c_int32), ("nms_num", C.c_int32), ("nms_shift", C.c_int32), ("beta", C.c_int32),
                ("early_stop", C.c_int32), ("reserved", C.c_int32), ("ymax", C.c_double)]


@dataclass
class FxmsConfig:
    """Fixed-point min-sum (include/ldpc_hip.h ldpc_fxms_cfg): integer samples of qbits bits,
    saturating integer messages of msg_bits bits, NMS as (m * nms_num) >> nms_shift, OMS as
    max(m - beta, 0). The precision is the front end's only."""
    variant: int = MS
    T: int = 10
    qbits: int = 5
    msg_bits: int = 6
    nms_num: int = 3
    nms_shift: int = 2
    beta: int = 1
    early_stop: bool = False
    ymax: float = 31 / 16
    precision: int = F64

    def _c(self) -> _FxmsCfg:
        return _FxmsCfg(self.variant, self.precision, self.T, self.qbits, self.msg_bits, self.nms_num, self.nms_shift,
                        self.beta, int(self.early_stop), 0, self.ymax)


class _FxlmsCfg(C.Structure):
    _fields_ = [("variant", C.c_int32), ("precision", C.c_int32), ("T", C.c_int32), ("qbits", C.c_int32),
                ("msg_bits", C.c_int32), ("app_bits", C.c_int32), ("nms_num", C.c_int32), ("nms_shift", C.c_int32),
                ("beta", C.c_int32), ("early_stop", C.c_int32), ("ymax", C.c_double)]


@dataclass
class FxlmsConfig:
    """Layered fixed-point min-sum (include/ldpc_hip.h ldpc_fxlms_cfg): FxmsConfig's fields and the
    width of the saturating posteriors, app_bits (None: msg_bits + 1, at most 16, where the APP
    clamp never acts for msg_bits >= qbits)."""
    variant: int = MS
    T: int = 10
    qbits: int = 5
    msg_bits: int = 6
    app_bits: Optional[int] = None
    nms_num: int = 3
    nms_shift: int = 2
    beta: int = 1
    early_stop: bool = False
    ymax: float = 31 / 16
    precision: int = F64

    def __post_init__(self):
        if self.app_bits is None:
            self.app_bits = min(self.msg_bits + 1, 16)

    def _c(self) -> _FxlmsCfg:
        return _FxlmsCfg(self.variant, self.precision, self.T, self.qbits, self.msg_bits, self.app_bits, self.nms_num,
                         self.nms_shift, self.beta, int(self.early_stop), self.ymax)


def rgdbf_phases(iters, T: int, maxphase: int):
    """Phases a frame ran, from its total iterations (int or array): a failed phase runs
    exactly T iterations and a satisfied one fewer, so phases = min(maxphase, iters // T + 1)."""
    return np.minimum(maxphase, np.asarray(iters) // T + 1)


def rgdbf_smoothing_used(iters, T: int, maxphase: int, windowsize: int):
    """Phases of a frame that end with it > T - windowsize (RNGDBF.cpp:388-389, counted per
    phase): every failed phase when windowsize > 0, and the last phase by its own count."""
    iters = np.asarray(iters)
    p = rgdbf_phases(iters, T, maxphase)
    last = iters - (p - 1) * T
    return (p - 1) * int(windowsize > 0) + (last > T - windowsize)


@dataclass
class DecoderConfig:
    """Runtime form of the reference's compile-time decoder switches."""
    variant: int = MS            # MS | NMS (-D normalizedMS) | OMS (-D offsetMS) | BP | DDBMP (decodeDDBMP.cpp)
    T: int = 10                  # iterations (fixed; the maximum with early_stop and for DDBMP)
    precision: int = F64         # F64 = the reference's double (default) | F32 throughput path (opt-in)
    alpha: float = 1.0           # NMS divisor
    delta: float = 0.0           # OMS offset
    quantize: bool = False       # -D quantizeSamples
    saturate: bool = False       # -D saturateSamples
    ymax: float = 0.0
    qbits: int = 0
    schedule: int = FLOODING     # FLOODING (the reference's) | LAYERED (row-serial, config 3)
    n0: float = 0.0              # BP (variant BP): N0 of the LLR front-end 4*y/N0 (decode only)
    max_llr: float = 0.0         # BP: MAXLLR (0 = the reference's 20)
    # MS / NMS / OMS / BP, flooding: stop a frame at the first t in 0..T whose decisions are a codeword and
    # return what T = t returns; frames["iters"] = t (include/ldpc_hip.h ldpc_decoder_cfg.early_stop)
    early_stop: bool = False

    def _c(self) -> _Cfg:
        return _Cfg(self.variant, self.precision, self.T, int(self.quantize), int(self.saturate),
                    self.qbits, self.ymax, self.alpha, self.delta, self.schedule, int(self.early_stop), self.n0,
                    self.max_llr)


class _EmsCfg(C.Structure):
    _fields_ = [("T", C.c_int32), ("nm", C.c_int32), ("early_stop", C.c_int32), ("reserved", C.c_int32),
                ("offset", C.c_double)]


class NbCounts(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("bit_err", "frame_err", "uncoded_bit_err", "frames", "iters",
                                         "syndrome_fail", "symbol_err")]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


@dataclass
class EmsConfig:
    """Extended Min-Sum over GF(q) (include/ldpc_hip.h ldpc_ems_cfg)."""
    T: int = 20
    nm: int = 16                 # message truncation (>= q: full vectors)
    offset: float = 0.0          # fill offset for truncated symbols
    early_stop: bool = True      # stop when H d = 0

    def _c(self) -> _EmsCfg:
        return _EmsCfg(self.T, self.nm, int(self.early_stop), 0, self.offset)


_vp, _i32, _u32, _u64, _dbl = C.c_void_p, C.c_int, C.c_uint32, C.c_uint64, C.c_double
_pi32 = C.POINTER(C.c_int)


def _sim(cfg, *outs):
    """Argument types of a *_sim_* call: ctx, Eb/N0, R, cfg, seed, stream_id, first_cw, batch, then its outputs."""
    return [_vp, _dbl, _dbl, C.POINTER(cfg), _u64, _u32, _u64, _i32, *outs]


def _info(cfg, *more):
    return [_vp, C.POINTER(cfg), *more, C.c_char_p, _i32, _pi32]


# Every symbol include/ldpc_hip.h declares (tests/test_abi.py compares the two): (argument types, result type).
_SIG = {
    "ldpc_abi_version": ([], _i32),
    "ldpc_f64_nms_fast_division": ([_dbl], _i32),
    "ldpc_bp_math_probe": ([_i32, _vp, _i32, _vp, _vp], _i32),
    "ldpc_check_selftest": ([_i32], _i32),
    "ldpc_last_error": ([], C.c_char_p),
    "ldpc_graph_create": ([_i32, _i32, _vp, _vp, _vp, _vp, C.POINTER(_vp)], _i32),
    "ldpc_graph_load_alist": ([C.c_char_p, C.POINTER(_vp)], _i32),
    "ldpc_graph_info": ([_vp] + [_pi32] * 5, _i32),
    "ldpc_graph_destroy": ([_vp], None),
    "ldpc_graph_layers": ([_vp, _vp, _vp, _pi32], _i32),
    "ldpc_device_count": ([_pi32], _i32),
    "ldpc_ctx_create": ([_i32, _vp, _i32, C.POINTER(_vp)], _i32),
    "ldpc_ctx_set_stream": ([_vp, _vp], _i32),
    "ldpc_ctx_synchronize": ([_vp], _i32),
    "ldpc_ctx_destroy": ([_vp], None),
    "ldpc_decode_batch": ([_vp, _vp, _i32, C.POINTER(_Cfg), _vp, _vp, _vp, C.POINTER(Counts)], _i32),
    "ldpc_sim_set_codewords": ([_vp, _vp, _i32], _i32),
    "ldpc_sim_launch": (_sim(_Cfg, _vp), _i32),
    "ldpc_ctx_read_counts": ([_vp, C.POINTER(Counts), _i32], _i32),
    "ldpc_ctx_read_histogram": ([_vp, _vp, _i32], _i32),
    "ldpc_sim_batch": (_sim(_Cfg, _vp, C.POINTER(Counts)), _i32),
    "ldpc_sim_trace": (_sim(_Cfg, _vp, _vp, _vp, C.POINTER(Counts)), _i32),
    "ldpc_ctx_last_kernel_ms": ([_vp, C.POINTER(C.c_float)], _i32),
    "ldpc_ctx_kernel_info": (_info(_Cfg) + [_pi32], _i32),
    "ldpc_ctx_redo_count": ([_vp, C.POINTER(C.c_int64)], _i32),
    "ldpc_ctx_redo_list": ([_vp, _vp, C.c_int64, C.POINTER(C.c_int64)], _i32),
    "ldpc_ctx_pp_row_slots": ([_vp, _vp, _vp, _vp, C.c_int, C.POINTER(C.c_int)], _i32),
    "ldpc_ctx_row_sched_info": ([_vp, C.POINTER(_Cfg), _vp], _i32),
    "ldpc_ctx_pp_inreg_info": ([_vp, C.POINTER(_Cfg), _vp], _i32),
    "ldpc_ctx_pp_block_info": ([_vp, C.POINTER(_Cfg), _vp], _i32),
    "ldpc_pp_block_layout": ([_i32, _i32, _vp], _i32),
    "ldpc_ctx_set_option": ([_vp, _i32, _i32], _i32),
    "ldpc_ctx_get_option": ([_vp, _i32, _pi32], _i32),
    "ldpc_nb_ctx_set_option": ([_vp, _i32, _i32], _i32),
    "ldpc_gdbf_decode_batch": ([_vp, _vp, _vp, _i32, C.POINTER(_GdbfCfg), _vp, _vp, _vp, C.POINTER(Counts)], _i32),
    "ldpc_gdbf_sim_launch": (_sim(_GdbfCfg, _vp), _i32),
    "ldpc_gdbf_sim_batch": (_sim(_GdbfCfg, _vp, C.POINTER(Counts)), _i32),
    "ldpc_gdbf_kernel_info": (_info(_GdbfCfg), _i32),
    "ldpc_rgdbf_decode_batch": ([_vp, _vp, _vp, _i32, C.POINTER(_RgdbfCfg), _vp, _vp, _vp, C.POINTER(Counts)], _i32),
    "ldpc_rgdbf_sim_launch": (_sim(_RgdbfCfg, _vp), _i32),
    "ldpc_rgdbf_sim_batch": (_sim(_RgdbfCfg, _vp, C.POINTER(Counts)), _i32),
    "ldpc_rgdbf_kernel_info": (_info(_RgdbfCfg), _i32),
    "ldpc_rstat_decode_batch": ([_vp, _vp, _vp, _i32, C.POINTER(_RstatCfg), _vp, _vp, C.POINTER(_RstatTrace), _vp,
                                 _vp, C.POINTER(Counts)], _i32),
    "ldpc_rstat_sim_launch": (_sim(_RstatCfg, _vp, C.POINTER(_RstatTrace), _vp), _i32),
    "ldpc_rstat_sim_batch": (_sim(_RstatCfg, _vp, C.POINTER(_RstatTrace), _vp, C.POINTER(Counts)), _i32),
    "ldpc_rstat_sim_trace": (_sim(_RstatCfg, _vp, _vp, _vp, C.POINTER(_RstatTrace), _vp, _vp, C.POINTER(Counts)),
                              _i32),
    "ldpc_rstat_kernel_info": (_info(_RstatCfg, _i32), _i32),
    "ldpc_hwgdbf_decode_batch": ([_vp, _vp, _vp, _vp, _i32, C.POINTER(_HwGdbfCfg), _vp, _vp, _vp, _vp,
                                  C.POINTER(Counts)], _i32),
    "ldpc_hwgdbf_sim_launch": (_sim(_HwGdbfCfg, _vp), _i32),
    "ldpc_hwgdbf_sim_batch": (_sim(_HwGdbfCfg, _vp, C.POINTER(Counts)), _i32),
    "ldpc_hwgdbf_sim_trace": (_sim(_HwGdbfCfg, _vp, _vp, _vp, _vp, C.POINTER(Counts)), _i32),
    "ldpc_hwgdbf_kernel_info": (_info(_HwGdbfCfg), _i32),
    "ldpc_fxms_decode_batch": ([_vp, _vp, _i32, C.POINTER(_FxmsCfg), _vp, _vp, _vp, C.POINTER(Counts)], _i32),
    "ldpc_fxms_sim_launch": (_sim(_FxmsCfg, _vp), _i32),
    "ldpc_fxms_sim_batch": (_sim(_FxmsCfg, _vp, C.POINTER(Counts)), _i32),
    "ldpc_fxms_sim_trace": (_sim(_FxmsCfg, _vp, _vp, _vp, _vp, C.POINTER(Counts)), _i32),
    "ldpc_fxms_kernel_info": (_info(_FxmsCfg), _i32),
    "ldpc_fxlms_decode_batch": ([_vp, _vp, _i32, C.POINTER(_FxlmsCfg), _vp, _vp, _vp, C.POINTER(Counts)], _i32),
    "ldpc_fxlms_sim_launch": (_sim(_FxlmsCfg, _vp), _i32),
    "ldpc_fxlms_sim_batch": (_sim(_FxlmsCfg, _vp, C.POINTER(Counts)), _i32),
    "ldpc_fxlms_sim_trace": (_sim(_FxlmsCfg, _vp, _vp, _vp, _vp, C.POINTER(Counts)), _i32),
    "ldpc_fxlms_kernel_info": (_info(_FxlmsCfg), _i32),
    "ldpc_nb_graph_create": ([_i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_vp)], _i32),
    "ldpc_nb_graph_load_alist": ([C.c_char_p, C.POINTER(_vp)], _i32),
    "ldpc_nb_graph_info": ([_vp] + [_pi32] * 6, _i32),
    "ldpc_nb_graph_destroy": ([_vp], None),
    "ldpc_nb_ctx_create": ([_i32, _vp, _i32, C.POINTER(_vp)], _i32),
    "ldpc_nb_ctx_set_stream": ([_vp, _vp], _i32),
    "ldpc_nb_ctx_destroy": ([_vp], None),
    "ldpc_nb_ctx_read_counts": ([_vp, C.POINTER(NbCounts), _i32], _i32),
    "ldpc_nb_ctx_last_kernel_ms": ([_vp, C.POINTER(C.c_float)], _i32),
    "ldpc_ems_kernel_info": ([_vp, C.c_char_p, _i32, _pi32], _i32),
    "ldpc_ems_decode_batch": ([_vp, _vp, _i32, _dbl, C.POINTER(_EmsCfg), _vp, _vp, _vp, C.POINTER(NbCounts)], _i32),
    "ldpc_ems_sim_launch": (_sim(_EmsCfg, _vp), _i32),
    "ldpc_ems_sim_batch": (_sim(_EmsCfg, _vp, C.POINTER(NbCounts)), _i32),
    "ldpc_ems_sim_trace": (_sim(_EmsCfg, _vp, _vp, _vp, C.POINTER(NbCounts)), _i32),
}
EXPORTED = list(_SIG)

_lib = None


# exports added without an ABI bump: the product library has them, an older A/B build may not
_ADDED_IN_ABI = {"ldpc_ctx_pp_inreg_info", "ldpc_ctx_pp_block_info", "ldpc_pp_block_layout", "ldpc_ctx_redo_list",
                 "ldpc_ctx_pp_row_slots", "ldpc_fxms_decode_batch", "ldpc_fxms_sim_launch", "ldpc_fxms_sim_batch",
                 "ldpc_fxms_sim_trace", "ldpc_fxms_kernel_info", "ldpc_fxlms_decode_batch", "ldpc_fxlms_sim_launch", "ldpc_fxlms_sim_batch", "ldpc_fxlms_sim_trace",
                 "ldpc_fxlms_kernel_info"}


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"HIP decoder library not built: {LIB_PATH} (run __graft_entry__.build() or `make`)")
    # One HIP runtime per process: torch ships its own libamdhip64 (soname
    # libamdhip64.so.7, DT_NEEDED by file name), and loading this library first
    # would map /opt/rocm's copy as well -- two runtimes, and torch.cuda then finds
    # no GPU. Imported first, torch's copy satisfies this library's soname.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    for name, (argt, rest) in _SIG.items():
        if name in _ADDED_IN_ABI and not hasattr(L, name):
            continue   # an A/B library (use_library, bench.py --lib) of this ABI built before the export
        fn = getattr(L, name)
        fn.argtypes = argt
        fn.restype = rest
    if L.ldpc_abi_version() != ABI_VERSION:
        raise ImportError(f"{LIB_PATH}: ABI version {L.ldpc_abi_version()}, this binding needs {ABI_VERSION}")
    _lib = L
    return L


def _check(rc: int):
    if rc != LDPC_OK:
        raise LdpcError(rc, lib().ldpc_last_error().decode(errors="replace"))


def pp_block_layout(n_bits: int, e_pad: int) -> dict:
    """Whether the ping-pong kernel's 768-thread block (its fixed-stride LDS layout) holds a code of
    n_bits bits and e_pad padded edge slots, and that layout's dynamic LDS bytes. Host-only."""
    info = np.zeros(2, dtype=np.int32)
    _check(lib().ldpc_pp_block_layout(int(n_bits), int(e_pad), info.ctypes.data))
    return {"fits": bool(info[0]), "launch_lds_bytes": int(info[1])}


def device_count() -> int:
    n = C.c_int(0)
    rc = lib().ldpc_device_count(C.byref(n))
    return n.value if rc == LDPC_OK else 0


class Graph:
    """Immutable Tanner graph (H matrix) on the host side of the ABI."""

    def __init__(self, handle):
        self._h = handle
        N, M, E, dv, dc = (C.c_int() for _ in range(5))
        _check(lib().ldpc_graph_info(self._h, C.byref(N), C.byref(M), C.byref(E), C.byref(dv), C.byref(dc)))
        self.N, self.M, self.E, self.maxdv, self.maxdc = N.value, M.value, E.value, dv.value, dc.value

    @classmethod
    def from_alist(cls, path: str) -> "Graph":
        h = C.c_void_p()
        _check(lib().ldpc_graph_load_alist(os.fspath(path).encode(), C.byref(h)))
        return cls(h)

    @classmethod
    def from_lists(cls, N: int, M: int, nlist, mlist) -> "Graph":
        """nlist[i]: 1-based checks of bit i; mlist[j]: 1-based bits of check j (alist_struct form)."""
        num_n = (C.c_int * N)(*[len(x) for x in nlist])
        num_m = (C.c_int * M)(*[len(x) for x in mlist])
        keep = [(C.c_int * max(len(x), 1))(*x) for x in nlist] + [(C.c_int * max(len(x), 1))(*x) for x in mlist]
        np_ = (C.c_void_p * N)(*[C.cast(a, C.c_void_p) for a in keep[:N]])
        mp_ = (C.c_void_p * M)(*[C.cast(a, C.c_void_p) for a in keep[N:]])
        h = C.c_void_p()
        _check(lib().ldpc_graph_create(N, M, num_n, np_, num_m, mp_, C.byref(h)))
        return cls(h)

    def layers(self):
        """(row_order [M] int32, layer_ptr [nlayers+1] int32) of the LAYERED schedule."""
        n = C.c_int()
        _check(lib().ldpc_graph_layers(self._h, None, None, C.byref(n)))
        order = np.empty(self.M, dtype=np.int32)
        ptr = np.empty(n.value + 1, dtype=np.int32)
        _check(lib().ldpc_graph_layers(self._h, order.ctypes.data, ptr.ctypes.data, C.byref(n)))
        return order, ptr

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:
            _lib.ldpc_graph_destroy(h)
            self._h = None


def _ptr(a) -> Optional[int]:
    """Address of a numpy array or a torch tensor (host or device)."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        if not a.flags["C_CONTIGUOUS"]:
            raise ValueError("array must be C-contiguous")
        return a.ctypes.data
    if hasattr(a, "data_ptr"):
        if not a.is_contiguous():
            raise ValueError("tensor must be contiguous")
        return a.data_ptr()
    raise TypeError(type(a))


def _given(N: int, cfg, y, c=None):
    """The float inputs of a *_decode call as the library reads them: y as a contiguous
    [batch, N] array of the cfg's precision and the optional bipolar codewords c as
    contiguous int8. Returns (y, batch, c, dtype); further inputs take the same dtype."""
    want = np.float64 if cfg.precision == F64 else np.float32
    y = np.ascontiguousarray(y, dtype=want).reshape(-1, N)
    if c is not None:
        c = np.ascontiguousarray(c, dtype=np.int8)
    return y, y.shape[0], c, want


def _sim_launch(fn, h, ebn0_db, R, cfg, seed, stream_id, first_cw, batch, *outs_dev):
    """An asynchronous *_sim_launch: every output is a device tensor or None."""
    _check(fn(h, ebn0_db, R, C.byref(cfg._c()), seed, stream_id, first_cw, batch, *(_ptr(o) for o in outs_dev)))


def _sim_batch(fn, h, ebn0_db, R, cfg, seed, stream_id, first_cw, batch, *outs, want_frames=True, counts=None):
    """A synchronous *_sim_batch / *_sim_trace: `outs` (host arrays or ctypes arguments, in the
    call's order), then the frame records (None unless wanted) and the counts. Returns (frames, counts)."""
    fr = np.empty(batch, dtype=FRAME_DTYPE) if want_frames else None
    cnt = (counts or Counts)()
    outs = [_ptr(o) if isinstance(o, np.ndarray) else o for o in outs]
    _check(fn(h, ebn0_db, R, C.byref(cfg._c()), seed, stream_id, first_cw, batch, *outs, _ptr(fr), C.byref(cnt)))
    return fr, cnt


def _kernel_info(fn, *args) -> dict:
    name = C.create_string_buffer(32)
    lds = C.c_int()
    _check(fn(*args, name, 32, C.byref(lds)))
    return {"kernel": name.value.decode(), "lds_bytes": lds.value}


class Context:
    """One device context (stream, counters, scratch) bound to a graph."""

    def __init__(self, graph: Graph, device: int = 0, max_batch: int = 65536):
        self.graph = graph
        self.device = device
        self.max_batch = max_batch
        h = C.c_void_p()
        _check(lib().ldpc_ctx_create(device, graph._h, max_batch, C.byref(h)))
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:
            _lib.ldpc_ctx_destroy(h)
            self._h = None

    def set_stream(self, stream_handle: Optional[int]):
        _check(lib().ldpc_ctx_set_stream(self._h, stream_handle))

    def set_option(self, name, value):
        """Override the kernel choice (ldpc_ctx_set_option): name from OPTIONS, value an int
        or a symbolic value from OPTION_VALUES (e.g. set_option("rows64", "fast"))."""
        _check(lib().ldpc_ctx_set_option(self._h, option_id(name), option_value(name, value)))

    def get_option(self, name) -> int:
        v = C.c_int()
        _check(lib().ldpc_ctx_get_option(self._h, option_id(name), C.byref(v)))
        return int(v.value)

    def set_options(self, opts: Optional[dict]):
        for k, v in (opts or {}).items():
            self.set_option(k, v)

    def reset_options(self):
        """Every option back to 0, the library's own kernel choice."""
        for name, k in OPTIONS.items():
            if name not in EMS_OPTIONS:   # those belong to the nb context (NbContext.set_options)
                _check(lib().ldpc_ctx_set_option(self._h, k, 0))

    def synchronize(self):
        _check(lib().ldpc_ctx_synchronize(self._h))

    def decode(self, y, cfg: DecoderConfig, c=None, want_decisions: bool = True, want_frames: bool = True):
        """Decode y[batch, N] (float32 for F32, float64 for F64; numpy or torch, host or device).

        Returns (d [batch,N] int8 or None, frames structured array or None, Counts)."""
        N = self.graph.N
        if isinstance(y, np.ndarray):
            want = np.float64 if cfg.precision == F64 else np.float32
            if y.dtype != want:
                raise TypeError(f"y must be {np.dtype(want)} for this precision, got {y.dtype}")
            y = np.ascontiguousarray(y)
            size = y.size
        else:   # torch tensor: the kernel reads batch*N elements of the precision's width
            want = "torch.float64" if cfg.precision == F64 else "torch.float32"
            if str(y.dtype) != want:
                raise TypeError(f"y must be {want} for this precision, got {y.dtype}")
            size = y.numel()
        if size % N:
            raise ValueError(f"y has {size} elements, not a multiple of N={N}")
        batch = size // N
        if c is not None:
            if isinstance(c, np.ndarray):
                c = np.ascontiguousarray(c, dtype=np.int8)
            elif str(c.dtype) != "torch.int8":
                raise TypeError(f"c must be torch.int8 (bipolar +1/-1), got {c.dtype}")
            csize = c.size if isinstance(c, np.ndarray) else c.numel()
            if csize != batch * N:
                raise ValueError(f"c has {csize} elements, y {batch * N}")
        d = np.empty((batch, N), dtype=np.int8) if want_decisions else None
        fr = np.empty(batch, dtype=FRAME_DTYPE) if want_frames else None
        cnt = Counts()
        _check(lib().ldpc_decode_batch(self._h, _ptr(y), batch, C.byref(cfg._c()), _ptr(c), _ptr(d), _ptr(fr),
                                       C.byref(cnt)))
        return d, fr, cnt

    def set_codewords(self, bits: Optional[np.ndarray]):
        if bits is None:
            _check(lib().ldpc_sim_set_codewords(self._h, None, 0))
            return
        bits = np.ascontiguousarray(bits, dtype=np.uint8).reshape(-1, self.graph.N)
        _check(lib().ldpc_sim_set_codewords(self._h, bits.ctypes.data, bits.shape[0]))

    def sim_launch(self, ebn0_db: float, R: float, cfg: DecoderConfig, seed: int, stream_id: int, first_cw: int,
                   batch: int, frames_dev=None):
        _sim_launch(lib().ldpc_sim_launch, self._h, ebn0_db, R, cfg, seed, stream_id, first_cw, batch, frames_dev)

    def sim_batch(self, ebn0_db: float, R: float, cfg: DecoderConfig, seed: int, stream_id: int, first_cw: int,
                  batch: int, want_frames: bool = True):
        return _sim_batch(lib().ldpc_sim_batch, self._h, ebn0_db, R, cfg, seed, stream_id, first_cw, batch,
                          want_frames=want_frames)

    def sim_trace(self, ebn0_db: float, R: float, cfg: DecoderConfig, seed: int, stream_id: int, first_cw: int,
                  batch: int):
        """sim_batch that also returns the generated channel samples and decisions."""
        N = self.graph.N
        y = np.empty((batch, N), dtype=np.float64 if cfg.precision == F64 else np.float32)
        d = np.empty((batch, N), dtype=np.int8)
        fr, cnt = _sim_batch(lib().ldpc_sim_trace, self._h, ebn0_db, R, cfg, seed, stream_id, first_cw, batch, y, d)
        return y, d, fr, cnt

    def read_counts(self, reset: bool = False) -> Counts:
        cnt = Counts()
        _check(lib().ldpc_ctx_read_counts(self._h, C.byref(cnt), int(reset)))
        return cnt

    def read_histogram(self, reset: bool = False) -> np.ndarray:
        h = np.zeros(self.graph.N, dtype=np.int64)
        _check(lib().ldpc_ctx_read_histogram(self._h, h.ctypes.data, int(reset)))
        return h

    def last_kernel_ms(self) -> float:
        ms = C.c_float()
        _check(lib().ldpc_ctx_last_kernel_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def redo_count(self) -> int:
        """Codewords of the last launch the fast fp64 row kernel re-decoded on the exact path."""
        n = C.c_int64()
        _check(lib().ldpc_ctx_redo_count(self._h, C.byref(n)))
        return int(n.value)

    def redo_list(self) -> np.ndarray:
        """Batch indices of those codewords, sorted (the kernel lists them in any order)."""
        n = C.c_int64()
        out = np.zeros(max(self.redo_count(), 1), dtype=np.uint32)
        _check(lib().ldpc_ctx_redo_list(self._h, out.ctypes.data, out.size, C.byref(n)))
        return np.sort(out[:int(n.value)])

    def row_sched_info(self, cfg: DecoderConfig) -> dict:
        """Shape of the row kernel that decodes cfg (raises LdpcError UNSUPPORTED for other kernels)."""
        info = np.zeros(10, dtype=np.int32)
        _check(lib().ldpc_ctx_row_sched_info(self._h, C.byref(cfg._c()), info.ctypes.data))
        keys = ("threads", "rows_per_thread", "slots_per_thread", "dc", "e_pad", "cw_per_block", "lds_bytes",
                "blocks_per_cu", "dc_low", "issued_check_edges")
        return {k: int(v) for k, v in zip(keys, info)}

    def pp_inreg_info(self, cfg: DecoderConfig) -> dict:
        """The ping-pong kernel's in-register bits for cfg (raises LdpcError UNSUPPORTED for other kernels)."""
        info = np.zeros(4, dtype=np.int32)
        _check(lib().ldpc_ctx_pp_inreg_info(self._h, C.byref(cfg._c()), info.ctypes.data))
        keys = ("inreg_bits", "lds_check_edges", "bit_slot_edges", "slots_per_thread")
        return {k: int(v) for k, v in zip(keys, info)}

    def pp_block_info(self, cfg: DecoderConfig) -> dict:
        """The workgroup the ping-pong kernel launches for cfg (raises LdpcError UNSUPPORTED for other kernels)."""
        info = np.zeros(2, dtype=np.int32)
        _check(lib().ldpc_ctx_pp_block_info(self._h, C.byref(cfg._c()), info.ctypes.data))
        return {"threads": int(info[0]), "launch_lds_bytes": int(info[1])}

    def pp_row_slots(self, cfg: DecoderConfig):
        """(cols [slots, 8] uint16, deg [slots] uint8) of the schedule the ping-pong kernel runs cfg on, from
        the device: slot j is row j // threads of check thread j % threads; entries >= N are padding edges."""
        cols = np.zeros((2048, 8), dtype=np.uint16)
        deg = np.zeros(2048, dtype=np.uint8)
        n = C.c_int()
        _check(lib().ldpc_ctx_pp_row_slots(self._h, C.byref(cfg._c()), cols.ctypes.data, deg.ctypes.data, 2048, C.byref(n)))
        return cols[:n.value], deg[:n.value]

    def kernel_info(self, cfg: DecoderConfig) -> dict:
        name = C.create_string_buffer(32)
        lds, bpc = C.c_int(), C.c_int()
        _check(lib().ldpc_ctx_kernel_info(self._h, C.byref(cfg._c()), name, 32, C.byref(lds), C.byref(bpc)))
        return {"kernel": name.value.decode(), "lds_bytes": lds.value, "blocks_per_cu": bpc.value}

    # ---- GDBF / NGDBF (src/decodeGDBF.cpp) ----
    def _decode(self, fn, y, cfg, c, want_decisions, *ins):
        """A *_decode_batch call with d, frames and counts as its outputs; `ins` follow y."""
        batch = y.shape[0]
        d = np.empty((batch, self.graph.N), dtype=np.int8) if want_decisions else None
        fr = np.empty(batch, dtype=FRAME_DTYPE)
        cnt = Counts()
        _check(fn(self._h, _ptr(y), *(_ptr(a) for a in ins), batch, C.byref(cfg._c()), _ptr(c), _ptr(d), _ptr(fr),
                  C.byref(cnt)))
        return d, fr, cnt

    def gdbf_decode(self, y, pert, cfg: GdbfConfig, c=None, want_decisions: bool = True):
        """Decode raw channel samples y[batch, N] with perturbations pert[batch, T, N] (or None
        without GDBF_NOISE). Returns (d, frames (iters = iterations run), Counts)."""
        y, batch, c, want = _given(self.graph.N, cfg, y, c)
        if pert is not None:
            pert = np.ascontiguousarray(pert, dtype=want).reshape(batch, cfg.T, self.graph.N)
        return self._decode(lib().ldpc_gdbf_decode_batch, y, cfg, c, want_decisions, pert)

    def gdbf_sim_launch(self, ebn0_db: float, R: float, cfg: GdbfConfig, seed: int, stream_id: int, first_cw: int,
                        batch: int, frames_dev=None):
        _sim_launch(lib().ldpc_gdbf_sim_launch, self._h, ebn0_db, R, cfg, seed, stream_id, first_cw, batch, frames_dev)

    def gdbf_sim_batch(self, ebn0_db: float, R: float, cfg: GdbfConfig, seed: int, stream_id: int, first_cw: int,
                       batch: int, want_frames: bool = True):
        return _sim_batch(lib().ldpc_gdbf_sim_batch, self._h, ebn0_db, R, cfg, seed, stream_id, first_cw, batch,
                          want_frames=want_frames)

    def gdbf_kernel_info(self, cfg: GdbfConfig) -> dict:
        return _kernel_info(lib().ldpc_gdbf_kernel_info, self._h, C.byref(cfg._c()))

    # ---- re-decoding NGDBF (src/RNGDBF.cpp) ----
    def rgdbf_decode(self, y, pert, cfg: RgdbfConfig, c=None, want_decisions: bool = True):
        """Decode raw channel samples y[batch, N] with perturbations pert[batch, maxphase*T, N]
        (row phase*T + it; None without GDBF_NOISE). Returns (d, frames, Counts); iters are
        sums over the phases (rgdbf_phases gives the phase count)."""
        y, batch, c, want = _given(self.graph.N, cfg, y, c)
        if pert is not None:
            pert = np.ascontiguousarray(pert, dtype=want).reshape(batch, cfg.maxphase * cfg.T, self.graph.N)
        return self._decode(lib().ldpc_rgdbf_decode_batch, y, cfg, c, want_decisions, pert)

    def rgdbf_sim_launch(self, ebn0_db: float, R: float, cfg: RgdbfConfig, seed: int, stream_id: int, first_cw: int,
                         batch: int, frames_dev=None):
        _sim_launch(lib().ldpc_rgdbf_sim_launch, self._h, ebn0_db, R, cfg, seed, stream_id, first_cw, batch, frames_dev)

    def rgdbf_sim_batch(self, ebn0_db: float, R: float, cfg: RgdbfConfig, seed: int, stream_id: int, first_cw: int,
                        batch: int, want_frames: bool = True):
        return _sim_batch(lib().ldpc_rgdbf_sim_batch, self._h, ebn0_db, R, cfg, seed, stream_id, first_cw, batch,
                          want_frames=want_frames)

    def rgdbf_kernel_info(self, cfg: RgdbfConfig) -> dict:
        return _kernel_info(lib().ldpc_rgdbf_kernel_info, self._h, C.byref(cfg._c()))

    # ---- every attempt of every frame (src/newstat.cpp, src/replayGDBF.cpp) ----
    def _rstat_trace(self, batch: int, cfg: RstatConfig, want: bool):
        """(the ldpc_rstat_trace argument or None, the dict of its numpy arrays or None)."""
        if not want:
            return None, None
        shape = (batch, cfg.attempts, cfg.T)
        tr = {"err_trace": np.empty(shape, dtype=np.int32), "unsat_trace": np.empty(shape, dtype=np.int32),
              "d_trace": np.empty(shape + (self.graph.N,), dtype=np.int8),
              "s_trace": np.empty(shape + (self.graph.M,), dtype=np.int8)}
        return C.byref(_RstatTrace(*(tr[k].ctypes.data for k, _ in _RstatTrace._fields_))), tr

    def rstat_decode(self, y, pert, cfg: RstatConfig, c=None, want_trace: bool = False):
        """Decode raw channel samples y[batch, N] cfg.attempts times each with perturbations
        pert[batch, attempts, T, N] (None without GDBF_NOISE). Returns (attempts, d, frames,
        Counts, trace): attempts[batch, attempts] of ATTEMPT_DTYPE; d, frames' bit_err and
        syndrome_fail are the last attempt's and iters the sum over the attempts; trace is a
        dict of err_trace, unsat_trace, d_trace, s_trace (None unless want_trace)."""
        N = self.graph.N
        y, batch, c, want = _given(N, cfg, y, c)
        if pert is not None:
            pert = np.ascontiguousarray(pert, dtype=want).reshape(batch, cfg.attempts, cfg.T, N)
        att = np.empty((batch, cfg.attempts), dtype=ATTEMPT_DTYPE)
        d = np.empty((batch, N), dtype=np.int8)
        fr = np.empty(batch, dtype=FRAME_DTYPE)
        cnt = Counts()
        targ, tr = self._rstat_trace(batch, cfg, want_trace)
        _check(lib().ldpc_rstat_decode_batch(self._h, _ptr(y), _ptr(pert), batch, C.byref(cfg._c()), _ptr(c),
                                             _ptr(att), targ, _ptr(d), _ptr(fr), C.byref(cnt)))
        return att, d, fr, cnt, tr

    def rstat_sim_launch(self, ebn0_db: float, R: float, cfg: RstatConfig, seed: int, stream_id: int, first_cw: int,
                         batch: int, attempts_dev=None, frames_dev=None, trace_dev: Optional[dict] = None):
        """Asynchronous; every output is a device tensor or None. trace_dev: a dict with any of
        err_trace, unsat_trace [batch, attempts, T] int32 and d_trace [.., N], s_trace [.., M] int8."""
        targ = None
        if trace_dev:
            unknown = set(trace_dev) - {k for k, _ in _RstatTrace._fields_}
            if unknown:
                raise KeyError(f"unknown trace {sorted(unknown)}")
            targ = _RstatTrace(*(_ptr(trace_dev.get(k)) for k, _ in _RstatTrace._fields_))
        _check(lib().ldpc_rstat_sim_launch(self._h, ebn0_db, R, C.byref(cfg._c()), seed, stream_id, first_cw, batch,
                                           _ptr(attempts_dev), targ and C.byref(targ), _ptr(frames_dev)))

    def rstat_sim(self, ebn0_db: float, R: float, cfg: RstatConfig, seed: int, stream_id: int, first_cw: int,
                  batch: int, want_trace: bool = False):
        """Fused Monte-Carlo of batch frames x cfg.attempts attempts: (attempts, frames, Counts, trace)."""
        att = np.empty((batch, cfg.attempts), dtype=ATTEMPT_DTYPE)
        targ, tr = self._rstat_trace(batch, cfg, want_trace)
        fr, cnt = _sim_batch(lib().ldpc_rstat_sim_batch, self._h, ebn0_db, R, cfg, seed, stream_id, first_cw, batch,
                             att, targ)
        return att, fr, cnt, tr

    def rstat_sim_trace(self, ebn0_db: float, R: float, cfg: RstatConfig, seed: int, stream_id: int, first_cw: int,
                        batch: int, want_trace: bool = False):
        """rstat_sim that also returns the samples drawn: (y, pert, attempts, d, frames, Counts,
        trace) with pert[batch, attempts, T, N]; rows that were not drawn are zero."""
        N = self.graph.N
        want = np.float64 if cfg.precision == F64 else np.float32
        y = np.empty((batch, N), dtype=want)
        pert = np.empty((batch, cfg.attempts, cfg.T, N), dtype=want)
        att = np.empty((batch, cfg.attempts), dtype=ATTEMPT_DTYPE)
        d = np.empty((batch, N), dtype=np.int8)
        targ, tr = self._rstat_trace(batch, cfg, want_trace)
        fr, cnt = _sim_batch(lib().ldpc_rstat_sim_trace, self._h, ebn0_db, R, cfg, seed, stream_id, first_cw, batch,
                             y, pert, att, targ, d)
        return y, pert, att, d, fr, cnt, tr

    def rstat_kernel_info(self, cfg: RstatConfig, with_trace: bool = False) -> dict:
        return _kernel_info(lib().ldpc_rstat_kernel_info, self._h, C.byref(cfg._c()), int(with_trace))

    # ---- fixed-point NGDBF hardware model (src/NGDBFhw.cpp) ----
    def hwgdbf_decode(self, y, q, cfg: HwGdbfConfig, qptr0=None, c=None, want_decisions: bool = True):
        """Decode raw channel samples y[batch, N] with the raw noise draws q[batch, qlen]
        (noiseSigma * n) from the start pointers qptr0[batch] (None: 0). Returns (d, frames,
        iters_run, Counts): frames[].bit_err / iters are the least over the phases, iters_run
        the sum of the phases' iterations (what a caller adds to the pointer)."""
        N = self.graph.N
        y, batch, c, want = _given(N, cfg, y, c)
        q = np.ascontiguousarray(q, dtype=want).reshape(batch, cfg.qlen)
        if qptr0 is not None:
            qptr0 = np.ascontiguousarray(qptr0, dtype=np.int32).reshape(batch)
        d = np.empty((batch, N), dtype=np.int8) if want_decisions else None
        fr = np.empty(batch, dtype=FRAME_DTYPE)
        run = np.empty(batch, dtype=np.int32)
        cnt = Counts()
        _check(lib().ldpc_hwgdbf_decode_batch(self._h, _ptr(y), _ptr(q), _ptr(qptr0), batch, C.byref(cfg._c()),
                                              _ptr(c), _ptr(d), _ptr(fr), _ptr(run), C.byref(cnt)))
        return d, fr, run, cnt

    def hwgdbf_sim_launch(self, ebn0_db: float, R: float, cfg: HwGdbfConfig, seed: int, stream_id: int,
                          first_cw: int, batch: int, frames_dev=None):
        _sim_launch(lib().ldpc_hwgdbf_sim_launch, self._h, ebn0_db, R, cfg, seed, stream_id, first_cw, batch, frames_dev)

    def hwgdbf_sim_batch(self, ebn0_db: float, R: float, cfg: HwGdbfConfig, seed: int, stream_id: int, first_cw: int,
                         batch: int, want_frames: bool = True):
        return _sim_batch(lib().ldpc_hwgdbf_sim_batch, self._h, ebn0_db, R, cfg, seed, stream_id, first_cw, batch,
                          want_frames=want_frames)

    def hwgdbf_sim_trace(self, ebn0_db: float, R: float, cfg: HwGdbfConfig, seed: int, stream_id: int, first_cw: int,
                         batch: int):
        """hwgdbf_sim_batch that also returns the samples drawn: (y, q, d, frames, Counts)."""
        N = self.graph.N
        want = np.float64 if cfg.precision == F64 else np.float32
        y = np.empty((batch, N), dtype=want)
        q = np.empty((batch, cfg.qlen), dtype=want)
        d = np.empty((batch, N), dtype=np.int8)
        fr, cnt = _sim_batch(lib().ldpc_hwgdbf_sim_trace, self._h, ebn0_db, R, cfg, seed, stream_id, first_cw, batch,
                             y, q, d)
        return y, q, d, fr, cnt

    def hwgdbf_kernel_info(self, cfg: HwGdbfConfig) -> dict:
        return _kernel_info(lib().ldpc_hwgdbf_kernel_info, self._h, C.byref(cfg._c()))

    # ---- fixed-point min-sum (integer messages) ----
    def fxms_decode(self, y, cfg: FxmsConfig, c=None, want_decisions: bool = True):
        """Decode raw channel samples y[batch, N]. Returns (d, frames, Counts); frames' iters are
        0, or with early_stop the iteration whose decisions are returned."""
        y, batch, c, _ = _given(self.graph.N, cfg, y, c)
        return self._decode(lib().ldpc_fxms_decode_batch, y, cfg, c, want_decisions)

    def fxms_sim_launch(self, ebn0_db: float, R: float, cfg: FxmsConfig, seed: int, stream_id: int, first_cw: int,
                        batch: int, frames_dev=None):
        _sim_launch(lib().ldpc_fxms_sim_launch, self._h, ebn0_db, R, cfg, seed, stream_id, first_cw, batch, frames_dev)

    def fxms_sim_batch(self, ebn0_db: float, R: float, cfg: FxmsConfig, seed: int, stream_id: int, first_cw: int,
                       batch: int, want_frames: bool = True):
        return _sim_batch(lib().ldpc_fxms_sim_batch, self._h, ebn0_db, R, cfg, seed, stream_id, first_cw, batch,
                          want_frames=want_frames)

    def fxms_sim_trace(self, ebn0_db: float, R: float, cfg: FxmsConfig, seed: int, stream_id: int, first_cw: int,
                       batch: int):
        """fxms_sim_batch that also returns the samples drawn and their integer codes:
        (y, ycode, d, frames, Counts)."""
        N = self.graph.N
        y = np.empty((batch, N), dtype=np.float64 if cfg.precision == F64 else np.float32)
        code = np.empty((batch, N), dtype=np.int8)
        d = np.empty((batch, N), dtype=np.int8)
        fr, cnt = _sim_batch(lib().ldpc_fxms_sim_trace, self._h, ebn0_db, R, cfg, seed, stream_id, first_cw, batch,
                             y, code, d)
        return y, code, d, fr, cnt

    def fxms_kernel_info(self, cfg: FxmsConfig) -> dict:
        return _kernel_info(lib().ldpc_fxms_kernel_info, self._h, C.byref(cfg._c()))

    # ---- layered fixed-point min-sum (saturating posteriors, integer messages) ----
    def fxlms_decode(self, y, cfg: FxlmsConfig, c=None, want_decisions: bool = True):
        """Decode raw channel samples y[batch, N] in the order of Graph.layers(). Returns (d, frames,
        Counts); frames' iters are 0, or with early_stop the iteration whose decisions are returned."""
        y, batch, c, _ = _given(self.graph.N, cfg, y, c)
        return self._decode(lib().ldpc_fxlms_decode_batch, y, cfg, c, want_decisions)

    def fxlms_sim_launch(self, ebn0_db: float, R: float, cfg: FxlmsConfig, seed: int, stream_id: int, first_cw: int,
                         batch: int, frames_dev=None):
        _sim_launch(lib().ldpc_fxlms_sim_launch, self._h, ebn0_db, R, cfg, seed, stream_id, first_cw, batch, frames_dev)

    def fxlms_sim_batch(self, ebn0_db: float, R: float, cfg: FxlmsConfig, seed: int, stream_id: int, first_cw: int,
                        batch: int, want_frames: bool = True):
        return _sim_batch(lib().ldpc_fxlms_sim_batch, self._h, ebn0_db, R, cfg, seed, stream_id, first_cw, batch,
                          want_frames=want_frames)

    def fxlms_sim_trace(self, ebn0_db: float, R: float, cfg: FxlmsConfig, seed: int, stream_id: int, first_cw: int,
                        batch: int):
        """fxlms_sim_batch that also returns the samples drawn and their integer codes:
        (y, ycode, d, frames, Counts)."""
        N = self.graph.N
        y = np.empty((batch, N), dtype=np.float64 if cfg.precision == F64 else np.float32)
        code = np.empty((batch, N), dtype=np.int8)
        d = np.empty((batch, N), dtype=np.int8)
        fr, cnt = _sim_batch(lib().ldpc_fxlms_sim_trace, self._h, ebn0_db, R, cfg, seed, stream_id, first_cw, batch,
                             y, code, d)
        return y, code, d, fr, cnt

    def fxlms_kernel_info(self, cfg: FxlmsConfig) -> dict:
        return _kernel_info(lib().ldpc_fxlms_kernel_info, self._h, C.byref(cfg._c()))


# ---- non-binary GF(q) codes, Extended Min-Sum (BASELINE config 5) ----
class NbGraph:
    """GF(q) Tanner graph (NB alist of SystemC/NB-LDPC/src/alist.cpp)."""

    def __init__(self, handle):
        self._h = handle
        N, M, q, E, dv, dc = (C.c_int() for _ in range(6))
        _check(lib().ldpc_nb_graph_info(handle, C.byref(N), C.byref(M), C.byref(q), C.byref(E), C.byref(dv),
                                        C.byref(dc)))
        self.N, self.M, self.q, self.E, self.maxdv, self.maxdc = N.value, M.value, q.value, E.value, dv.value, dc.value
        self.m = self.q.bit_length() - 1

    @classmethod
    def from_alist(cls, path: str) -> "NbGraph":
        h = C.c_void_p()
        _check(lib().ldpc_nb_graph_load_alist(path.encode(), C.byref(h)))
        return cls(h)

    @classmethod
    def from_lists(cls, N: int, M: int, q: int, cols, rows) -> "NbGraph":
        """cols[i] = [(row, h), ...], rows[j] = [(col, h), ...], 0-based (as codes.NbParityCheck)."""
        def arrs(lists, one_based):
            n = (C.c_int * len(lists))(*[len(l) for l in lists])
            idx = [(C.c_int * max(len(l), 1))(*[a + 1 for a, _ in l]) for l in lists]
            val = [(C.c_int * max(len(l), 1))(*[h for _, h in l]) for l in lists]
            pi = (C.POINTER(C.c_int) * len(lists))(*[C.cast(a, C.POINTER(C.c_int)) for a in idx])
            pv = (C.POINTER(C.c_int) * len(lists))(*[C.cast(a, C.POINTER(C.c_int)) for a in val])
            return n, pi, pv, (idx, val)
        nn, ni, nv, keep1 = arrs(cols, True)
        mn, mi, mv, keep2 = arrs(rows, True)
        h = C.c_void_p()
        _check(lib().ldpc_nb_graph_create(N, M, q, nn, ni, nv, mn, mi, mv, C.byref(h)))
        return cls(h)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:
            _lib.ldpc_nb_graph_destroy(h)
            self._h = None


class NbContext:
    """Device context of the EMS decoder: GF(4), GF(8) and GF(16) graphs (other q:
    LdpcError, LDPC_ERR_UNSUPPORTED). A symbol is m = log2(q) channel samples."""

    def __init__(self, graph: NbGraph, device: int = 0, max_batch: int = 65536):
        self.graph = graph
        self.max_batch = max_batch
        h = C.c_void_p()
        _check(lib().ldpc_nb_ctx_create(device, graph._h, max_batch, C.byref(h)))
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:
            _lib.ldpc_nb_ctx_destroy(h)
            self._h = None

    def set_stream(self, stream_handle: Optional[int]):
        _check(lib().ldpc_nb_ctx_set_stream(self._h, stream_handle))

    def set_option(self, name, value):
        """EMS options (ems_threads, ems_swizzle) of ldpc_nb_ctx_set_option."""
        _check(lib().ldpc_nb_ctx_set_option(self._h, option_id(name), option_value(name, value)))

    def decode(self, y, n0: float, cfg: EmsConfig, c=None, want_decisions: bool = True):
        """Decode y[batch, N*m] float32 (numpy or torch, host or device), m = log2(q) samples per symbol,
        bit i of a symbol at column v*m + i. A y of another width is a ValueError. Returns
        (d [batch,N] uint8, frames, NbCounts)."""
        g = self.graph
        width = g.N * g.m
        if isinstance(y, np.ndarray):
            if y.dtype != np.float32:
                raise TypeError(f"y must be float32, got {y.dtype}")
            y = np.ascontiguousarray(y)
            size, shape = y.size, y.shape
        else:
            size, shape = y.numel(), tuple(y.shape)
        if size == 0 or size % width or (len(shape) > 1 and shape[-1] != width):
            raise ValueError(f"y must be [batch, N*m = {width}] (GF({g.q}): {g.m} samples per symbol), got {shape}")
        batch = size // width
        if c is not None and tuple(c.shape) != (batch, g.N):
            raise ValueError(f"c must be [batch, N] = {(batch, g.N)}, got {tuple(c.shape)}")
        if c is not None and isinstance(c, np.ndarray):
            c = np.ascontiguousarray(c, dtype=np.uint8)
        d = np.empty((batch, g.N), dtype=np.uint8) if want_decisions else None
        fr = np.empty(batch, dtype=FRAME_DTYPE)
        cnt = NbCounts()
        _check(lib().ldpc_ems_decode_batch(self._h, _ptr(y), batch, n0, C.byref(cfg._c()), _ptr(c), _ptr(d),
                                           _ptr(fr), C.byref(cnt)))
        return d, fr, cnt

    def sim_launch(self, ebn0_db: float, R: float, cfg: EmsConfig, seed: int, stream_id: int, first_cw: int,
                   batch: int, frames_dev=None):
        _sim_launch(lib().ldpc_ems_sim_launch, self._h, ebn0_db, R, cfg, seed, stream_id, first_cw, batch, frames_dev)

    def sim_batch(self, ebn0_db: float, R: float, cfg: EmsConfig, seed: int, stream_id: int, first_cw: int,
                  batch: int):
        return _sim_batch(lib().ldpc_ems_sim_batch, self._h, ebn0_db, R, cfg, seed, stream_id, first_cw, batch,
                          counts=NbCounts)

    def sim_trace(self, ebn0_db: float, R: float, cfg: EmsConfig, seed: int, stream_id: int, first_cw: int,
                  batch: int):
        """sim_batch that also returns the generated samples y [batch, N*m] (symbol v's bits 0..m-1 at
        columns v*m .. v*m + m - 1) and the decisions d [batch, N]."""
        g = self.graph
        y = np.empty((batch, g.N * g.m), dtype=np.float32)
        d = np.empty((batch, g.N), dtype=np.uint8)
        fr, cnt = _sim_batch(lib().ldpc_ems_sim_trace, self._h, ebn0_db, R, cfg, seed, stream_id, first_cw, batch, y, d,
                             counts=NbCounts)
        return y, d, fr, cnt

    def read_counts(self, reset: bool = False) -> NbCounts:
        cnt = NbCounts()
        _check(lib().ldpc_nb_ctx_read_counts(self._h, C.byref(cnt), int(reset)))
        return cnt

    def last_kernel_ms(self) -> float:
        ms = C.c_float()
        _check(lib().ldpc_nb_ctx_last_kernel_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def kernel_info(self) -> dict:
        return _kernel_info(lib().ldpc_ems_kernel_info, self._h)
