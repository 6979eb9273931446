#!/usr/bin/env python3
"""Throughput of the GF(q) EMS decoder (BASELINE config 5: the GF(16) code, the default):
fused on-device AWGN -> EMS -> error count over a batch, one MI355X. Prints one JSON
line per Eb/N0.

    python scripts/bench_ems.py [--batch B --T T --nm NM --ebn0 E --steps K]
    python scripts/bench_ems.py --alist GF4_OR_GF8_OR_GF16.alist --rate 0.3333 ...
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=16384)
    p.add_argument("--T", type=int, default=20)
    p.add_argument("--nm", type=int, default=None, help="message truncation (default: the code's q, full vectors)")
    p.add_argument("--alist", default=None, help="an NB alist with q in {4, 8, 16} (default: the GF(16) code)")
    p.add_argument("--rate", type=float, default=0.5, help="code rate of --alist (Eb/N0 -> N0)")
    p.add_argument("--offset", type=float, default=0.0)
    p.add_argument("--ebn0", type=float, nargs="+", default=[1.5, 2.0])
    p.add_argument("--steps", type=int, default=3)
    p.add_argument("--no-early-stop", action="store_true")
    p.add_argument("--option", action="append", default=[], metavar="NAME=VALUE",
                   help="an EMS option of the context (ems_threads, ems_swizzle), A/B only")
    p.add_argument("--lib", default=None, help="another build of the decoder library (A/B only)")
    a = p.parse_args()
    from ldpcsimulation_amd import codes, native
    if a.lib:
        native.use_library(os.path.abspath(a.lib))
    if a.alist is None and a.rate != 0.5:
        p.error("--rate belongs to --alist")
    g = native.NbGraph.from_alist(a.alist or codes.ensure_gf16_code())
    nm = a.nm if a.nm is not None else g.q
    name = ("%s (N=%d GF(%d) symbols, %d bits, R=%.4g)" % (os.path.basename(a.alist), g.N, g.q, g.N * g.m, a.rate)
            if a.alist else "gf16_N1000_dv2_dc4 (N=1000 GF(16) symbols, 4000 bits, R=1/2)")
    ctx = native.NbContext(g, 0, a.batch)
    for o in a.option:
        k, _, v = o.partition("=")
        ctx.set_option(k, int(v) if v.isdigit() else v)
    cfg = native.EmsConfig(T=a.T, nm=nm, offset=a.offset, early_stop=not a.no_early_stop)
    for ebn0 in a.ebn0:
        ctx.sim_batch(ebn0, a.rate, cfg, seed=1, stream_id=0, first_cw=0, batch=min(a.batch, 1024))   # warm-up
        ctx.read_counts(reset=True)
        kms = []
        t0 = time.perf_counter()
        for k in range(a.steps):
            ctx.sim_launch(ebn0, a.rate, cfg, seed=1, stream_id=0, first_cw=k * a.batch, batch=a.batch)
            kms.append(ctx.last_kernel_ms())
        wall = time.perf_counter() - t0
        c = ctx.read_counts(reset=True)
        bits = c.frames * g.N * g.m
        print(json.dumps({"code": name,
                          "ebn0_db": ebn0, "T_max": a.T, "nm": nm, "offset": a.offset,
                          "early_stop": cfg.early_stop, "batch": a.batch, "steps": a.steps,
                          "kernel": ctx.kernel_info(), "kernel_ms": sum(kms) / len(kms),
                          "coded_mbit_s_kernel": bits / (sum(kms) / 1e3) / 1e6,
                          "coded_mbit_s_wall": bits / wall / 1e6,
                          "fer": c.frame_err / c.frames, "ber": c.bit_err / bits,
                          "avg_iters": c.iters / c.frames, "frames": c.frames}), flush=True)


if __name__ == "__main__":
    main()
