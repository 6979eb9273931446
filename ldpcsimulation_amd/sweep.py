"""SNR sweep on one or more GPUs -- replacement of the reference's sweep scripts.

The reference launches one background process per SNR point, each appending
one line to a shared log (C_implementations/scripts/minsum_example_*.sh:23-27,
decodeMinSum.cpp:313-329). Here every SNR point runs on all ranks at once: the
frames of a point are sharded over the GPUs by global frame index (one process
per GPU, torch.distributed over RCCL, launched with torchrun), the six error
counters are all-reduced per round, and rank 0 appends the reference's log
line for each point.

    python -m ldpcsimulation_amd.sweep ALIST --rate 0.5 --snr 1.0 1.25 1.5 -T 50 \\
        --variant nms --alpha 1.25 --log results.txt
    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 -m ldpcsimulation_amd.sweep ...
    # BASELINE config 3: DVB-S2 N=64800 R1/2, layered NMS, SNR sweep over 8 GPUs
    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 -m ldpcsimulation_amd.sweep dvbs2_1_2.alist \\
        --rate 0.5 --snr 0.8 0.9 1.0 1.1 -T 50 --variant nms --alpha 1.25 --schedule layered --batch 2048
    # early termination (no reference counterpart): every frame stops at its first codeword, avgIt is the true mean
    python -m ldpcsimulation_amd.sweep ALIST --rate 0.5 --snr 2.5 3.0 -T 50 --variant nms --alpha 1.25 --early-stop
    # belief propagation (decodeBP: its stop rule 200 bit / 20|10|5 frame errors)
    python -m ldpcsimulation_amd.sweep ALIST --rate 0.5 --snr 1.5 2.0 -T 50 --variant bp
    # BASELINE config 5: GF(16) EMS on an NB alist (SystemC/NB-LDPC format), early stop
    python -m ldpcsimulation_amd.sweep codes/gf16_N1000_dv2_dc4.alist --ems --rate 0.5 --snr 1.5 2.0 -T 20
    # DD-BMP (decodeDDBMP: the quantiser always on, early stop; the grid of its sweep script
    # scripts/ddbmp_example_4000.2000.4.244.sh is one such call per (Ymax, Q))
    python -m ldpcsimulation_amd.sweep ALIST --rate 0.5 --snr 3.0 3.5 -T 100 --variant ddbmp --ymax 1.0 --qbits 3
    # the GDBF family (decodeMNGDBF ... decodeStochasticNGDBF, and the re-decoding decodeRSMNGDBF):
    # their stop rule 200 bit / 20|10|5 frame errors, early stop
    python -m ldpcsimulation_amd.sweep ALIST --rate 0.5 --snr 3.0 3.5 -T 100 --gdbf SMNGDBF --alpha 0.8 --ymax 2.5
    python -m ldpcsimulation_amd.sweep ALIST --rate 0.5 --snr 3.0 3.5 -T 100 --gdbf RSMNGDBF --alpha 0.96 --ymax 2.5 --maxphase 3
    # the fixed-point NGDBF hardware model (NGDBFhw; its constants are the defaults, R = 0.8413 on 802.3an)
    python -m ldpcsimulation_amd.sweep 802_3_H.alist --rate 0.8413 --snr 4.0 4.25 -T 600 --hwgdbf
    # fixed-point min-sum: integer messages of --msg-bits bits, NMS as (m * NUM) >> SHIFT, OMS as max(m - B, 0)
    python -m ldpcsimulation_amd.sweep ALIST --rate 0.5 --snr 1.5 2.0 -T 50 --fxms --variant nms --scale 3 2 \\
        --quantize 1.9375 5 --msg-bits 6 --early-stop
    # its row-layered form: saturating posteriors of --app-bits bits (default msg-bits + 1), rows in the graph's layer order
    python -m ldpcsimulation_amd.sweep ALIST --rate 0.5 --snr 1.5 2.0 -T 25 --fxlms --variant nms --scale 3 2 \\
        --quantize 1.9375 5 --msg-bits 8 --app-bits 9 --early-stop
    # ... on a code beyond 64 KiB of state (DVB-S2 N=64800): the workgroup-per-codeword kernel, same results
    python -m ldpcsimulation_amd.sweep dvbs2_1_2.alist --rate 0.5 --snr 1.2 1.4 -T 25 --fxlms --fx-kernel wg --variant nms \\
        --scale 3 2 --msg-bits 8 --app-bits 9 --early-stop
Log line: SNR BER avgIt FER T [Ymax] [alpha] [delta] alist (--fxms: SNR BER avgIt FER T Ymax Q msgBits [num shift] [beta] alist; --fxlms: SNR BER avgIt FER T Ymax Q msgBits appBits [num shift] [beta] alist; DD-BMP: SNR BER avgIt FER T Ymax Q alist; EMS: SNR BER avgIt FER T nm offset alist;
BER over coded bits, 4 per GF(16) symbol; --gdbf: SNR BER avgIt FER T theta noiseScale lambda alpha windowsize Ymax
[maxphase] alist, maxphase with RSMNGDBF only -- the reference's own GDBF log lines are the CLIs' job;
--hwgdbf: SNR BER avgIt FER T theta0 noiseScale w Ymax NQ maxphase qlen alist).

--checkpoint FILE appends each point's running totals after a round at most
every --checkpoint-interval seconds (default 10; 0 = every round; checkpoint.py); a sweep restarted with the same FILE and settings takes the
seed from it, skips finished points and resumes the others at their next
frame, with the totals an uninterrupted run gives.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

from . import checkpoint, native, sim

VARIANTS = {"ms": native.MS, "nms": native.NMS, "oms": native.OMS, "bp": native.BP,
            "ddbmp": native.DDBMP}
# --gdbf: the decodeGDBF.cpp targets and the re-decoding decoder (RNGDBF.cpp)
GDBF_NAMES = list(native.GDBF_VARIANTS) + ["RSMNGDBF"]
# --gdbf settings left unset take these (native.GdbfConfig's)
GDBF_DEFAULTS = {"theta": -0.6, "lam": 0.99, "noise_scale": 0.75, "window": 16, "nq": 16, "maxphase": 3, "ymax": 2.5}
# --hwgdbf settings left unset take these (NGDBFhw.cpp:48-57, native.HwGdbfConfig's)
HWGDBF_DEFAULTS = {"w": 0.185, "ymax": 1.625, "noise_scale": 0.95, "theta0": -0.525, "nq": 5, "maxphase": 1,
                   "qlen": 2648}
# --fxms settings left unset take these (--quantize YMAX Q, --msg-bits, --scale NUM SHIFT, --beta)
FXMS_DEFAULTS = {"ymax": 31 / 16, "qbits": 5, "msg_bits": 6, "nms_num": 3, "nms_shift": 2, "beta": 1}


def parse(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("alist")
    p.add_argument("--rate", type=float, required=True)
    p.add_argument("--snr", type=float, nargs="+", required=True, help="Eb/N0 points in dB")
    p.add_argument("-T", "--iterations", type=int, default=10)
    p.add_argument("--variant", choices=list(VARIANTS), default="ms")
    p.add_argument("--alpha", type=float, default=1.0)
    p.add_argument("--delta", type=float, default=0.0)
    p.add_argument("--quantize", nargs=2, metavar=("YMAX", "Q"), help="-D quantizeSamples front-end")
    p.add_argument("--saturate", type=float, metavar="YMAX", help="-D saturateSamples front-end")
    p.add_argument("--ymax", type=float, help="--variant ddbmp: Ymax of its quantiser (required); --gdbf: Ymax "
                                               "(default 2.5; --saturate YMAX is the same setting)")
    p.add_argument("--qbits", type=int, help="--variant ddbmp: Q of its quantiser (required)")
    p.add_argument("--precision", choices=["f32", "f64"], default="f64",
                   help="f64 = the reference's double (default); f32 = the fp32 kernels (opt-in)")
    p.add_argument("--schedule", choices=["flooding", "layered"], default="flooding",
                   help="flooding = the reference's schedule; layered = row-serial (BASELINE config 3)")
    p.add_argument("--batch", type=int, default=65536, help="frames per GPU per round (the largest round)")
    p.add_argument("--first-round", type=int, default=None,
                   help="frames per GPU in the first round; rounds double up to --batch (default min(batch, 1024))")
    p.add_argument("--seed", type=int, default=None, help="noise seed (default: time)")
    p.add_argument("--min-bit-errors", type=int, default=200)
    p.add_argument("--min-frame-errors", type=int, default=None,
                   help="default 40 (decodeMinSum.cpp:189); BP: 20/10/5 by N (decodeBP.cpp:145-147); EMS: 40")
    p.add_argument("--gdbf", choices=GDBF_NAMES, metavar="NAME",
                   help="a decoder of the GDBF family: " + ", ".join(GDBF_NAMES) + " (-T, --alpha, --ymax are reused)")
    p.add_argument("--theta", type=float, help="--gdbf: flip threshold (default -0.6)")
    p.add_argument("--lam", type=float, help="--gdbf: threshold adaptation lambda (default 0.99)")
    p.add_argument("--noise-scale", type=float, help="--gdbf: perturbation sigma / channel sigma (default 0.75)")
    p.add_argument("--window", type=int, help="--gdbf: output smoothing window (default 16)")
    p.add_argument("--nq", type=int, help="--gdbf: quantiser levels NQ (default 16)")
    p.add_argument("--maxphase", type=int, help="--gdbf RSMNGDBF: decoding attempts per frame (default 3)")
    p.add_argument("--hwgdbf", action="store_true",
                   help="the fixed-point NGDBF hardware model (NGDBFhw): -T, --ymax (default 1.625), --noise-scale "
                        "(0.95), --nq (bits per sample, 5) and --maxphase (1) are reused")
    p.add_argument("--w", type=float, help="--hwgdbf: syndrome weight parameter w (default 0.185)")
    p.add_argument("--theta0", type=float, help="--hwgdbf: noise offset theta0 (default -0.525)")
    p.add_argument("--qlen", type=int, help="--hwgdbf: noise samples per frame, > N (default 2648)")
    p.add_argument("--fxms", action="store_true",
                   help="fixed-point min-sum (integer messages): --variant ms|nms|oms, --quantize YMAX Q (default 1.9375 5), "
                        "-T, --precision (of the front end) and --early-stop are reused")
    p.add_argument("--fxlms", action="store_true",
                   help="layered fixed-point min-sum (saturating posteriors, integer messages, the graph's layer order): "
                        "the settings of --fxms and --app-bits")
    p.add_argument("--app-bits", type=int, help="--fxlms: posterior width in bits, msg-bits..16 (default msg-bits + 1)")
    p.add_argument("--fx-kernel", choices=["auto", "wg"], default="auto",
                   help="--fxlms: wg forces the workgroup-per-codeword kernel (option kernel = global), which also holds "
                        "codes beyond 64 KiB of state such as DVB-S2 N=64800; the results do not depend on the kernel")
    p.add_argument("--msg-bits", type=int, help="--fxms / --fxlms: message width in bits, 2..16 (default 6)")
    p.add_argument("--scale", type=int, nargs=2, metavar=("NUM", "SHIFT"),
                   help="--fxms --variant nms: magnitudes become (m * NUM) >> SHIFT (default 3 2)")
    p.add_argument("--beta", type=int, help="--fxms --variant oms: magnitudes become max(m - B, 0) (default 1)")
    p.add_argument("--ems", action="store_true", help="GF(q) Extended Min-Sum on an NB alist (BASELINE config 5)")
    p.add_argument("--nm", type=int, default=16, help="EMS message truncation")
    p.add_argument("--offset", type=float, default=0.0, help="EMS fill offset")
    p.add_argument("--no-early-stop", action="store_true", help="EMS: always run T iterations")
    p.add_argument("--early-stop", action="store_true",
                   help="--variant ms / nms / oms / bp, flooding: stop a frame at the first iteration count whose "
                        "decisions are a codeword (T is the maximum; avgIt becomes the true mean); the other "
                        "decoders always stop early and ignore it")
    p.add_argument("--max-frames", type=int, default=None)
    p.add_argument("--codewords", help="codeword file ('0'/'1' lines), as the reference's optional argument")
    p.add_argument("--log", "--log-file", dest="log",
                   help="append the reference's tab-separated result line per point (--log-file under torchrun, "
                        "whose parser takes --log for a prefix of its own --log-dir)")
    p.add_argument("--json", action="store_true", help="also print one JSON object per point")
    p.add_argument("--sync", action="store_true",
                   help="one blocking round at a time (default: the next round decodes while one is reduced)")
    p.add_argument("--backend", choices=["nccl", "gloo"], default="nccl",
                   help="collective backend for world > 1 (nccl = RCCL over xGMI; gloo: CPU tensors)")
    p.add_argument("--share-device", action="store_true",
                   help="every rank on device 0 (rehearsal of N ranks on one GPU, with --backend gloo)")
    p.add_argument("--checkpoint", metavar="FILE",
                   help="per-round progress file (.partial); an existing one is resumed (same settings)")
    p.add_argument("--checkpoint-interval", type=float, default=10.0, metavar="S",
                   help="seconds between checkpoint records (0 = after every round); each record "
                        "all-reduces the point's error-weight histogram")
    a = p.parse_args(argv)
    if a.early_stop and a.schedule == "layered":
        p.error("--early-stop is not supported with --schedule layered")
    if a.fxms and a.fxlms:
        p.error("--fxms and --fxlms exclude each other")
    if a.fxms or a.fxlms:
        fx = "--fxlms" if a.fxlms else "--fxms"
        if a.gdbf or a.hwgdbf or a.ems or a.schedule != "flooding":
            p.error(fx + " excludes --gdbf, --hwgdbf, --ems and --schedule layered")
        if a.variant not in ("ms", "nms", "oms"):
            p.error(fx + " is --variant ms, nms or oms")
        if a.saturate is not None or a.ymax is not None or a.qbits is not None or a.alpha != 1.0 or a.delta != 0.0:
            p.error(fx + " takes its settings from --quantize YMAX Q, --msg-bits, --scale NUM SHIFT and --beta")
        if (a.scale is not None and a.variant != "nms") or (a.beta is not None and a.variant != "oms"):
            p.error(fx + ": --scale belongs to --variant nms and --beta to --variant oms")
    else:
        for n in ("msg_bits", "scale", "beta"):
            if getattr(a, n) is not None:
                p.error("--" + n.replace("_", "-") + " belongs to --fxms / --fxlms")
    if a.app_bits is not None and not a.fxlms:
        p.error("--app-bits belongs to --fxlms")
    if a.fx_kernel != "auto" and not a.fxlms:
        p.error("--fx-kernel belongs to --fxlms")
    gdbf_only = [n for n in ("theta", "lam", "noise_scale", "window", "nq", "maxphase") if getattr(a, n) is not None]
    if a.hwgdbf:
        if a.gdbf or a.ems or a.schedule != "flooding" or a.variant != "ms":
            p.error("--hwgdbf excludes --gdbf, --ems, --variant and --schedule layered")
        if a.quantize or a.qbits is not None or a.saturate is not None:
            p.error("--hwgdbf takes its front-end from --ymax, --w and --nq")
        for n in ("theta", "lam", "window"):
            if getattr(a, n) is not None:
                p.error("--" + n + " belongs to --gdbf, not to --hwgdbf")
        return a
    for n in ("w", "theta0", "qlen"):
        if getattr(a, n) is not None:
            p.error("--" + n + " belongs to --hwgdbf")
    if a.gdbf:
        if a.ems or a.schedule != "flooding" or a.variant != "ms":
            p.error("--gdbf excludes --ems, --schedule layered and --variant")
        if a.quantize or a.qbits is not None:
            p.error("--gdbf takes its front-end from --ymax and --nq")
        if a.maxphase is not None and a.gdbf != "RSMNGDBF":
            p.error("--maxphase belongs to --gdbf RSMNGDBF")
        if a.ymax is not None and a.saturate is not None and a.ymax != a.saturate:
            p.error("--ymax and --saturate are the same setting with --gdbf")
        return a
    if gdbf_only:
        p.error("--" + gdbf_only[0].replace("_", "-") + " belongs to --gdbf")
    if a.variant == "ddbmp":
        if a.ymax is None or a.qbits is None:
            p.error("--variant ddbmp needs --ymax and --qbits (decodeDDBMP: alist R SNR T Ymax Q log)")
        if a.quantize or a.saturate is not None or a.schedule != "flooding" or a.ems:
            p.error("--variant ddbmp takes its front-end from --ymax / --qbits and is flooding only")
    elif a.ymax is not None or a.qbits is not None:
        p.error("--ymax / --qbits belong to --variant ddbmp (min-sum: --quantize YMAX Q)")
    return a


def _checkpoint_config(a) -> dict:
    """Every setting that changes a point's result (not the batch or round sizes,
    the GPU count or the log options: exact_stop makes totals independent of them)."""
    ddbmp = {"ymax": a.ymax, "qbits": a.qbits} if a.variant == "ddbmp" else {}
    if getattr(a, "gdbf", None):   # only then, so that checkpoints written before --gdbf existed still match
        ddbmp = {"gdbf": a.gdbf, **_gdbf_settings(a)}
    if getattr(a, "hwgdbf", False):   # likewise
        ddbmp = {"hwgdbf": True, **_hwgdbf_settings(a)}
    if getattr(a, "fxms", False):   # likewise: every field of the cfg, so another width is another sweep
        ddbmp = {"fxms": True, **_fxms_settings(a)}
    if getattr(a, "fxlms", False):   # likewise: the fxms keys, the switch and the posterior width
        ddbmp = {"fxms": False, "fxlms": True, **_fxlms_settings(a)}
    if _min_sum_early_stop(a):   # likewise (the "early_stop" key below is the EMS setting)
        ddbmp = {**ddbmp, "min_sum_early_stop": True}
    return {**ddbmp, "alist": os.path.basename(a.alist), "alist_md5": checkpoint.file_digest(a.alist), "rate": a.rate,
            "snr": list(a.snr), "T": a.iterations, "variant": a.variant, "alpha": a.alpha, "delta": a.delta,
            "quantize": a.quantize, "saturate": a.saturate, "precision": a.precision, "schedule": a.schedule,
            "min_bit_errors": a.min_bit_errors, "min_frame_errors": a.min_frame_errors, "max_frames": a.max_frames,
            "codewords_md5": checkpoint.file_digest(a.codewords), "ems": a.ems, "nm": a.nm, "offset": a.offset,
            "early_stop": not a.no_early_stop}


def _min_sum_early_stop(a) -> bool:
    """--early-stop where it means something: the min-sum variants and BP (the other families always stop)."""
    return bool(getattr(a, "early_stop", False)) and not (a.ems or getattr(a, "gdbf", None) or getattr(a, "hwgdbf", False)) \
        and a.variant in ("ms", "nms", "oms", "bp")


def _gdbf_settings(a) -> dict:
    """The --gdbf settings with their defaults filled in."""
    s = {k: (getattr(a, k) if getattr(a, k) is not None else v) for k, v in GDBF_DEFAULTS.items()}
    if a.ymax is None and a.saturate is not None:
        s["ymax"] = a.saturate
    if a.gdbf != "RSMNGDBF":
        del s["maxphase"]
    return s


def _hwgdbf_settings(a) -> dict:
    """The --hwgdbf settings with their defaults filled in."""
    return {k: (getattr(a, k) if getattr(a, k) is not None else v) for k, v in HWGDBF_DEFAULTS.items()}


def _fxms_settings(a) -> dict:
    """The --fxms settings with their defaults filled in."""
    s = dict(FXMS_DEFAULTS)
    if a.quantize:
        s["ymax"], s["qbits"] = float(a.quantize[0]), int(a.quantize[1])
    if a.msg_bits is not None:
        s["msg_bits"] = a.msg_bits
    if a.scale is not None:
        s["nms_num"], s["nms_shift"] = a.scale
    if a.beta is not None:
        s["beta"] = a.beta
    return s


def _fxlms_settings(a) -> dict:
    """The --fxlms settings with their defaults filled in: --fxms's and app_bits."""
    s = _fxms_settings(a)
    s["app_bits"] = a.app_bits if a.app_bits is not None else min(s["msg_bits"] + 1, 16)
    return s


def _run_points(a, ck, rank, n_hist, run_point):
    """run_point(k, snr, resume, on_round) -> (result, log line, json dict) for each
    point not finished in the checkpoint; rank 0 logs and records each point.
    n_hist: the points' histogram length (bits per frame)."""
    for k, snr in enumerate(a.snr):
        done = ck.done_line(k, snr) if ck else None
        if done is not None:
            if rank == 0:
                print(done, flush=True)   # appended to the log by the run that finished it
            continue
        resume = ck.point_state(k, snr, n_hist) if ck else None
        on_round = (lambda st, k=k, snr=snr: ck.save_round(k, snr, st)) if ck else None
        res, line, js = run_point(k, snr, resume, on_round)
        if rank == 0:
            if a.log:
                with open(a.log, "a") as f:
                    f.write(line + "\n")
            print(line, flush=True)
            if a.json:
                js["resumed_from_frame"] = resume.next_frame if resume else 0
                print(json.dumps(js), flush=True)
        if ck:
            ck.save_done(k, snr, line)


def main(argv=None) -> int:
    a = parse(argv)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    device = local if world > 1 and not a.share_device else 0
    # under torchrun (WORLD_SIZE set) a process group always exists, one rank included:
    # the counters then go through the collective backend exactly as at 8 ranks
    distributed = "WORLD_SIZE" in os.environ
    if distributed:
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(device)
        if a.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", device))
        else:
            dist.init_process_group("gloo")
    ck = checkpoint.SweepCheckpoint(a.checkpoint, _checkpoint_config(a), writer=rank == 0) if a.checkpoint else None
    if ck and ck.seed is not None:
        if a.seed is not None and a.seed != ck.seed:
            raise checkpoint.CheckpointMismatch(f"--seed {a.seed} != the checkpoint's seed {ck.seed}")
        a.seed = ck.seed          # every rank read the same file
    seed = a.seed if a.seed is not None else int(time.time())
    if distributed and a.seed is None:
        # every rank must key its noise with rank 0's seed (ranks may start in different seconds)
        import torch
        import torch.distributed as dist
        t = torch.tensor([seed], dtype=torch.int64, device=f"cuda:{device}" if a.backend == "nccl" else "cpu")
        dist.broadcast(t, src=0)
        seed = int(t.item())
    if os.environ.get("LDPC_SWEEP_REPORT_SEED"):   # tests: every rank reports the seed it keys its noise with
        print(json.dumps({"rank": rank, "seed": seed}), file=sys.stderr, flush=True)
    if ck:
        ck.start(seed)
    if a.ems:
        return _ems_sweep(a, seed, world, rank, device, ck)
    if a.gdbf or a.hwgdbf:
        return _gdbf_sweep(a, seed, world, rank, device, ck)
    if a.fxms or a.fxlms:
        return _fxms_sweep(a, seed, world, rank, device, ck)
    cfg = native.DecoderConfig(variant=VARIANTS[a.variant], T=a.iterations, alpha=a.alpha, delta=a.delta,
                               precision=native.F64 if a.precision == "f64" else native.F32,
                               schedule=native.LAYERED if a.schedule == "layered" else native.FLOODING,
                               early_stop=_min_sum_early_stop(a))
    stops = a.variant == "ddbmp" or cfg.early_stop   # early stop: frames report their iterations
    extra = []
    if a.quantize:
        cfg.quantize, cfg.ymax, cfg.qbits = True, float(a.quantize[0]), int(a.quantize[1])
        extra.append(cfg.ymax)
    elif a.saturate is not None:
        cfg.saturate, cfg.ymax = True, a.saturate
        extra.append(cfg.ymax)
    if a.variant == "ddbmp":   # decodeDDBMP.cpp:255-264: ... T Ymax Q alist
        cfg.quantize, cfg.ymax, cfg.qbits = True, a.ymax, a.qbits
        extra += [cfg.ymax, cfg.qbits]
    if a.variant == "nms":
        extra.append(a.alpha)
    elif a.variant == "oms":
        extra.append(a.delta)
    g = native.Graph.from_alist(a.alist)
    ctx = native.Context(g, device, a.batch)
    min_fe = a.min_frame_errors
    if min_fe is None:
        min_fe = (5 if g.N > 50000 else 10 if g.N > 10000 else 20) if a.variant == "bp" else 40
    if a.codewords:
        from .codes import read_codeword_file
        ctx.set_codewords(read_codeword_file(a.codewords, g.N))
    def run_point(k, snr, resume, on_round):
        def run_batch(first, n):
            fr, _ = ctx.sim_batch(snr, a.rate, cfg, seed, k, first, n)
            return fr

        launcher = None
        if not a.sync:
            # rounds run ahead: round k+1 decodes while round k is reduced (sim.AsyncLauncher)
            def run_launch(first, n, frames_dev):
                ctx.sim_launch(snr, a.rate, cfg, seed, k, first, n, frames_dev)
            launcher = sim.AsyncLauncher(ctx, a.batch, run_launch)
        t0 = time.perf_counter()
        res = sim.simulate_point(run_batch, g.N, a.iterations, snr, a.batch, a.min_bit_errors,
                                 min_fe, a.max_frames, device=device, launcher=launcher, first_round=a.first_round,
                                 iters_in_frames=stops,
                                 resume=resume, on_round=on_round,
                                 on_round_interval=a.checkpoint_interval)
        dt = time.perf_counter() - t0
        c = res.counts
        ran = c["frames"] - (int(resume.acc[3]) if resume else 0)   # frames counted by this run
        return res, res.log_line(a.alist, extra), {
            "ebn0_db": snr, **c, "ber": res.ber, "fer": res.fer, "seconds": dt,
            **({"avg_iters": res.avg_iters} if stops else {}),
            "mbit_s": ran * g.N / dt / 1e6 if dt > 0 else None,
            "n_gpus": world, "wilson95": sim.wilson_interval(c["frame_err"], c["frames"]),
            "precision": a.precision, "schedule": a.schedule, "variant": a.variant,
            "kernel": ctx.kernel_info(cfg)["kernel"], "rounds": res.rounds, "frames_decoded": res.frames_decoded,
            "collectives": res.collectives}

    _run_points(a, ck, rank, g.N, run_point)
    if distributed:
        import torch.distributed as dist
        dist.destroy_process_group()
    return 0


def _ems_sweep(a, seed, world, rank, device, ck=None) -> int:
    """One SNR point after the other on the GF(q) EMS decoder, frames sharded as above."""
    g = native.NbGraph.from_alist(a.alist)
    ctx = native.NbContext(g, device, a.batch)
    cfg = native.EmsConfig(T=a.iterations, nm=a.nm, offset=a.offset, early_stop=not a.no_early_stop)
    bits = g.N * g.m
    def run_point(k, snr, resume, on_round):
        def run_batch(first, n):
            fr, _ = ctx.sim_batch(snr, a.rate, cfg, seed, k, first, n)
            return fr
        t0 = time.perf_counter()
        res = sim.simulate_point(run_batch, bits, a.iterations, snr, a.batch, a.min_bit_errors,
                                 a.min_frame_errors if a.min_frame_errors is not None else 40, a.max_frames,
                                 device=device, iters_in_frames=True, first_round=a.first_round,
                                 resume=resume, on_round=on_round,
                                 on_round_interval=a.checkpoint_interval)
        dt = time.perf_counter() - t0
        c = res.counts
        ran = c["frames"] - (int(resume.acc[3]) if resume else 0)   # frames counted by this run
        return res, res.log_line(a.alist, [float(a.nm), a.offset]), {
            "ebn0_db": snr, **c, "ber": res.ber, "fer": res.fer, "avg_iters": res.avg_iters,
            "seconds": dt, "mbit_s": ran * bits / dt / 1e6 if dt > 0 else None,
            "n_gpus": world, "wilson95": sim.wilson_interval(c["frame_err"], c["frames"]),
            "precision": "f32", "rounds": res.rounds, "frames_decoded": res.frames_decoded}

    _run_points(a, ck, rank, bits, run_point)
    if "WORLD_SIZE" in os.environ:   # a process group exists only under torchrun (torch optional otherwise)
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            dist.destroy_process_group()
    return 0


def _gdbf_sweep(a, seed, world, rank, device, ck=None) -> int:
    """One SNR point after the other on a decoder of the GDBF family (--gdbf NAME) or on the
    fixed-point hardware model (--hwgdbf), frames sharded as above; the family's stop rule
    (decodeGDBF.cpp:216-226) unless --min-frame-errors is given."""
    g = native.Graph.from_alist(a.alist)
    ctx = native.Context(g, device, a.batch)
    prec = native.F64 if a.precision == "f64" else native.F32
    if a.hwgdbf:
        s = _hwgdbf_settings(a)
        cfg = native.HwGdbfConfig(T=a.iterations, maxphase=s["maxphase"], nq=s["nq"], qlen=s["qlen"], w=s["w"],
                                  ymax=s["ymax"], noise_scale=s["noise_scale"], theta0=s["theta0"], precision=prec)
        batch_fn, launch_fn, info_fn = ctx.hwgdbf_sim_batch, ctx.hwgdbf_sim_launch, ctx.hwgdbf_kernel_info
        extra = [s["theta0"], s["noise_scale"], s["w"], s["ymax"], float(s["nq"]), float(s["maxphase"]),
                 float(s["qlen"])]
        return _flip_points(a, seed, world, rank, device, ck, g, ctx, cfg, batch_fn, launch_fn, info_fn, extra,
                            {"gdbf": "NGDBFhw"})
    s = _gdbf_settings(a)
    common = dict(T=a.iterations, theta=s["theta"], lambda_=s["lam"], alpha=a.alpha, noise_scale=s["noise_scale"],
                  ymax=s["ymax"], windowsize=s["window"], precision=prec)
    if a.gdbf == "RSMNGDBF":
        cfg = native.RgdbfConfig(flags=native.RGDBF_FLAGS, maxphase=s["maxphase"], **common)
        batch_fn, launch_fn, info_fn = ctx.rgdbf_sim_batch, ctx.rgdbf_sim_launch, ctx.rgdbf_kernel_info
    else:
        cfg = native.GdbfConfig(flags=native.GDBF_VARIANTS[a.gdbf], nq=s["nq"], **common)
        batch_fn, launch_fn, info_fn = ctx.gdbf_sim_batch, ctx.gdbf_sim_launch, ctx.gdbf_kernel_info
    extra = [s["theta"], s["noise_scale"], s["lam"], a.alpha, float(s["window"]), s["ymax"]]
    if a.gdbf == "RSMNGDBF":
        extra.append(float(s["maxphase"]))
    return _flip_points(a, seed, world, rank, device, ck, g, ctx, cfg, batch_fn, launch_fn, info_fn, extra,
                        {"gdbf": a.gdbf})


def _fxms_sweep(a, seed, world, rank, device, ck=None) -> int:
    """One SNR point after the other on fixed-point min-sum (--fxms) or its layered form (--fxlms),
    frames sharded as above; the min-sum stop rule (decodeMinSum.cpp:189). With --early-stop the
    frames report their iterations."""
    g = native.Graph.from_alist(a.alist)
    ctx = native.Context(g, device, a.batch)
    layered = bool(getattr(a, "fxlms", False))
    if getattr(a, "fx_kernel", "auto") == "wg":   # the same results from another kernel: no checkpoint setting
        ctx.set_option("kernel", "global")
    s = _fxlms_settings(a) if layered else _fxms_settings(a)
    cfg = (native.FxlmsConfig if layered else native.FxmsConfig)(
        variant=VARIANTS[a.variant], T=a.iterations, early_stop=bool(a.early_stop),
        precision=native.F64 if a.precision == "f64" else native.F32, **s)
    extra = [s["ymax"], float(s["qbits"]), float(s["msg_bits"])] + ([float(s["app_bits"])] if layered else [])
    if a.variant == "nms":
        extra += [float(s["nms_num"]), float(s["nms_shift"])]
    elif a.variant == "oms":
        extra.append(float(s["beta"]))
    fns = (ctx.fxlms_sim_batch, ctx.fxlms_sim_launch, ctx.fxlms_kernel_info) if layered else \
        (ctx.fxms_sim_batch, ctx.fxms_sim_launch, ctx.fxms_kernel_info)
    # (--fxlms: the JSON line names the schedule the decoder runs; the checkpoint settings keep --schedule's value,
    # "flooding", which --fxlms requires, and tell the two decoders apart by their "fxlms" key)
    return _flip_points(a, seed, world, rank, device, ck, g, ctx, cfg, *fns, extra,
                        {"decoder": "fxlms" if layered else "fxms", "variant": a.variant,
                         "schedule": "layered" if layered else a.schedule},
                        stops=cfg.early_stop,
                        min_fe=a.min_frame_errors if a.min_frame_errors is not None else 40)


def _flip_points(a, seed, world, rank, device, ck, g, ctx, cfg, batch_fn, launch_fn, info_fn, extra, family, stops=True,
                 min_fe=None) -> int:
    """The points of a sweep of one of the ticket families. stops: the decoder stops early, so the
    frames report their iterations (the bit-flipping decoders always do). min_fe: None = the GDBF
    family's stop rule. family: the keys of the JSON line that name the decoder."""
    if min_fe is None:
        min_fe = a.min_frame_errors
    if min_fe is None:
        min_fe = 5 if g.N > 50000 else 10 if g.N > 10000 else 20
    if a.codewords:
        from .codes import read_codeword_file
        ctx.set_codewords(read_codeword_file(a.codewords, g.N))

    def run_point(k, snr, resume, on_round):
        def run_batch(first, n):
            fr, _ = batch_fn(snr, a.rate, cfg, seed, k, first, n)
            return fr

        launcher = None
        if not a.sync:
            def run_launch(first, n, frames_dev):
                launch_fn(snr, a.rate, cfg, seed, k, first, n, frames_dev)
            launcher = sim.AsyncLauncher(ctx, a.batch, run_launch)
        t0 = time.perf_counter()
        res = sim.simulate_point(run_batch, g.N, a.iterations, snr, a.batch, a.min_bit_errors, min_fe, a.max_frames,
                                 device=device, launcher=launcher, first_round=a.first_round, iters_in_frames=stops,
                                 resume=resume, on_round=on_round, on_round_interval=a.checkpoint_interval)
        dt = time.perf_counter() - t0
        c = res.counts
        ran = c["frames"] - (int(resume.acc[3]) if resume else 0)   # frames counted by this run
        return res, res.log_line(a.alist, extra), {
            "ebn0_db": snr, **c, "ber": res.ber, "fer": res.fer, **({"avg_iters": res.avg_iters} if stops else {}),
            "seconds": dt, "mbit_s": ran * g.N / dt / 1e6 if dt > 0 else None, "n_gpus": world,
            "wilson95": sim.wilson_interval(c["frame_err"], c["frames"]), "precision": a.precision,
            **family, "kernel": info_fn(cfg)["kernel"], "rounds": res.rounds,
            "frames_decoded": res.frames_decoded, "collectives": res.collectives}

    _run_points(a, ck, rank, g.N, run_point)
    if "WORLD_SIZE" in os.environ:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
