#!/usr/bin/env python3
"""Generate tests/golden/reference_runs_ngdbfhw.json from the REFERENCE's NGDBFhw.

Compiles the unmodified reference sources (ereiss123/LDPCsimulation
C_implementations/src/NGDBFhw.cpp + alist.cpp + r.cpp + nrutil.cpp, -O2; the reference's
Makefile has no target for it, its demo script scripts/demo_NGDBFhw_802_3.sh expects
bin/NGDBFhw) into a temporary directory, runs it and records, as data: the complete stdout,
the log line, the text of <log>_<SNR>_itdist.dat, the per-frame error weights and the final
line of every run. The seed is a command-line argument (no time() is involved). Nothing
compiled is kept.

It also records `fer_pooled`: frames and frame errors of further seeds at one operating
point, the reference side of the two-proportion test of the Philox simulation, and `timing`:
the wall time of run 1 on this machine's CPU (one core).

    python tests/golden/make_golden_ngdbfhw.py REFERENCE_ROOT     (from the repo root;
    REFERENCE_ROOT = the reference's C_implementations directory)
"""
import json
import os
import platform
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLD = os.path.join(ROOT, "tests", "golden")

# (name, code, SNR, numFrames, seed)
RUNS = [
    ("ngdbfhw_802_3_4.0_200_s1234", "802_3_H.alist", "4.0", 200, 1234),
    ("ngdbfhw_802_3_3.5_30_s11", "802_3_H.alist", "3.5", 30, 11),
    ("ngdbfhw_802_3_4.5_400_s5", "802_3_H.alist", "4.5", 400, 5),
    ("ngdbfhw_peg_6.0_200_s7", "PEGReg504x1008.alist", "6.0", 200, 7),
    ("ngdbfhw_1944_8.0_60_s3", "80211n_1944_r12.alist", "8.0", 60, 3),
]
POOL = ("802_3_H.alist", "4.0", 1000, list(range(21, 31)))

PATH_TOKEN = "@ALIST@"
LOG_TOKEN = "@LOGFILE@"


def build(ref, td):
    src, inc = os.path.join(ref, "src"), os.path.join(ref, "inc")
    exe = os.path.join(td, "NGDBFhw")
    subprocess.run(["g++", "-O2", "-w", "-I" + inc, "-o", exe] +
                   [os.path.join(src, f) for f in ("nrutil.cpp", "r.cpp", "alist.cpp", "NGDBFhw.cpp")] + ["-lm"],
                   check=True)
    return exe


def run(exe, td, code, snr, frames, seed):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import code_path
    alist = code_path(code)
    log = os.path.join(td, "log.txt")
    for f in os.listdir(td):
        if f.startswith("log.txt"):
            os.remove(os.path.join(td, f))
    t0 = time.perf_counter()
    p = subprocess.run([exe, alist, snr, str(frames), str(seed), log], capture_output=True, text=True, check=True)
    dt = time.perf_counter() - t0
    stdout = p.stdout.replace(alist, PATH_TOKEN).replace(log, LOG_TOKEN)
    itd = [f for f in os.listdir(td) if f.startswith("log.txt_")]
    assert len(itd) == 1, itd
    return stdout, open(log).read(), itd[0][len("log.txt"):], open(os.path.join(td, itd[0])).read(), dt


def cpu_name():
    try:
        for l in open("/proc/cpuinfo"):
            if l.startswith("model name"):
                return l.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or platform.machine()


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = sys.argv[1]
    out = []
    with tempfile.TemporaryDirectory() as td:
        exe = build(ref, td)
        timing = None
        for name, code, snr, frames, seed in RUNS:
            stdout, logline, suffix, itdist, dt = run(exe, td, code, snr, frames, seed)
            ferr = [int(l.split()[2]) for l in stdout.splitlines() if l.startswith("Ferr with ")]
            final = [l for l in stdout.splitlines() if l.startswith("Final result:")][0]
            out.append({"name": name, "binary": "NGDBFhw", "code": code, "snr": snr, "frames": frames, "seed": seed,
                        "stdout": stdout, "log_line": logline, "itdist_suffix": suffix, "itdist": itdist,
                        "ferr_weights": ferr, "final": final})
            if timing is None:
                from conftest import code_path
                N = int(open(code_path(code)).read().split()[0])
                timing = {"run": name, "seconds": round(dt, 3), "cpu": cpu_name(), "cores": 1,
                          "mbit_per_s": round(frames * N / dt / 1e6, 3)}
            print(f"{name}: {final} ({len(stdout)} bytes, {dt:.2f} s)")
        code, snr, frames, seeds = POOL
        nf = ferrs = 0
        for seed in seeds:
            stdout, *_ = run(exe, td, code, snr, frames, seed)
            nf += frames
            ferrs += sum(1 for l in stdout.splitlines() if l.startswith("Ferr with "))
        pooled = {"code": code, "snr": snr, "seeds": seeds, "frames": nf, "frame_errors": ferrs}
        print("fer_pooled:", pooled, "timing:", timing)
    with open(os.path.join(GOLD, "reference_runs_ngdbfhw.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_golden_ngdbfhw.py",
                   "source": "unmodified reference NGDBFhw.cpp, -O2", "runs": out, "fer_pooled": pooled,
                   "timing": timing}, f, indent=1)


if __name__ == "__main__":
    main()
