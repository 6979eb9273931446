#!/usr/bin/env python3
"""Generate tests/golden/reference_runs_rsmngdbf.json from the REFERENCE's decodeRSMNGDBF.

Compiles the unmodified reference sources (ereiss123/LDPCsimulation
C_implementations/src/RNGDBF.cpp + alist.cpp + r.cpp + nrutil.cpp, -O2, with the switches
of its Makefile target: -D redecode -D addNoise -D thresholdAdaptation -D weightSyndromes
-D outputSmoothing -D saturateSamples) into a temporary directory, with time() wrapped at
link time (oracle/seed_time.c, REF_SEED) so that ran_seed(time(0)) (:219) is reproducible,
runs it, and records the complete stdout, the log line, the per-frame error weights, the
phase histogram and the final line of every run as data, in the format of
reference_runs.json (tests/golden/make_golden.py: the log file sits in the middle of the
arguments, "@LOG@"). Nothing compiled is kept.

It also records `fer_pooled`: frames and frame errors of further seeds at one operating
point, the reference side of the two-proportion test of the Philox simulation.

    python tests/golden/make_golden_rsmngdbf.py REFERENCE_ROOT     (from the repo root;
    REFERENCE_ROOT = the reference's C_implementations directory)
"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLD = os.path.join(ROOT, "tests", "golden")
CODES = os.path.join(GOLD, "codes")
SWITCHES = ["redecode", "addNoise", "thresholdAdaptation", "weightSyndromes", "outputSmoothing", "saturateSamples"]


def args(snr, T, alpha, maxphase):
    """R SNR T theta LOG noiseScale lambda alpha windowsize Ymax maxphase (RNGDBF.cpp:82-105)."""
    return ["0.5", snr, T, "-0.6", "@LOG@", "0.75", "0.99", alpha, "16", "2.5", maxphase]


# (name, code, args after alist, seed, codeword file or None)
RUNS = [
    ("rsmngdbf_peg_3.0_T50_p4_s5", "PEGReg504x1008.alist", args("3.0", "50", "0.96", "4"), 5, None),
    ("rsmngdbf_peg_3.5_T100_p3_s5", "PEGReg504x1008.alist", args("3.5", "100", "0.96", "3"), 5, None),
    ("rsmngdbf_peg_3.5_T100_p1_s4", "PEGReg504x1008.alist", args("3.5", "100", "0.96", "1"), 4, None),
    ("rsmngdbf_peg_cw_3.25_T60_p2_s7", "PEGReg504x1008.alist", args("3.25", "60", "0.96", "2"), 7,
     "PEGReg504x1008_data20.enc"),
    ("rsmngdbf_1944_4.0_T100_p3_s9", "80211n_1944_r12.alist", args("4.0", "100", "1.5", "3"), 9, None),
    ("rsmngdbf_4000_cw_3.0_T40_p2_s13", "4000.2000.4.244.alist", args("3.0", "40", "1.2", "2"), 13,
     "4000.2000.4.244_data10.enc"),
]
# the pooled operating point: PEG 3.5 dB, T 100, maxphase 3 (run 2's)
POOL = ("PEGReg504x1008.alist", args("3.5", "100", "0.96", "3"), list(range(101, 111)))

PATH_TOKEN = "@ALIST@"
CW_TOKEN = "@CWFILE@"
LOG_TOKEN = "@LOGFILE@"


def build(ref, td):
    src, inc = os.path.join(ref, "src"), os.path.join(ref, "inc")
    exe = os.path.join(td, "decodeRSMNGDBF")
    seed_o = os.path.join(td, "seed_time.o")
    subprocess.run(["gcc", "-O2", "-c", "-o", seed_o, os.path.join(ROOT, "oracle", "seed_time.c")], check=True)
    subprocess.run(["g++", "-O2", "-w", "-I" + inc, "-Wl,--wrap=time"] + [x for s in SWITCHES for x in ("-D", s)] +
                   ["-o", exe] + [os.path.join(src, f) for f in ("nrutil.cpp", "r.cpp", "alist.cpp")] +
                   [seed_o, os.path.join(src, "RNGDBF.cpp"), "-lm"], check=True)
    return exe


def run(exe, td, code, a, seed, cw):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import code_path
    alist = code_path(code)
    log = os.path.join(td, "log.txt")
    if os.path.exists(log):
        os.remove(log)
    cmd = [exe, alist] + [log if x == "@LOG@" else x for x in a] + ([os.path.join(CODES, cw)] if cw else [])
    p = subprocess.run(cmd, env=dict(os.environ, REF_SEED=str(seed)), capture_output=True, text=True, check=True)
    stdout = p.stdout.replace(alist, PATH_TOKEN).replace(log, LOG_TOKEN)
    if cw:
        stdout = stdout.replace(os.path.join(CODES, cw), CW_TOKEN)
    return stdout, open(log).read().replace(alist, PATH_TOKEN)


def phase_hist(stdout, maxphase):
    """The final block's histogram: the lines "k:\\tcount" after "Phase histogram:" and an empty line."""
    tail = stdout[stdout.rindex("Phase histogram:\n\n") + len("Phase histogram:\n\n"):]
    h = [0] * maxphase
    for l in tail.splitlines():
        k, n = l.split(":\t")
        h[int(k) - 1] = int(n)
    return h


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = sys.argv[1]
    out = []
    with tempfile.TemporaryDirectory() as td:
        exe = build(ref, td)
        for name, code, a, seed, cw in RUNS:
            stdout, logline = run(exe, td, code, a, seed, cw)
            ferr = [int(l.split()[2]) for l in stdout.splitlines() if l.startswith("Ferr with ")]
            final = [l for l in stdout.splitlines() if l.startswith("Final result:")][0]
            out.append({"name": name, "binary": "decodeRSMNGDBF", "code": code, "args": a, "seed": seed,
                        "cwfile": cw, "stdout": stdout, "log_line": logline, "ferr_weights": ferr,
                        "phase_hist": phase_hist(stdout, int(a[-1])), "final": final})
            print(f"{name}: {final} phases {out[-1]['phase_hist']} ({len(stdout)} bytes)")
        code, a, seeds = POOL
        frames = ferrs = 0
        for seed in seeds:
            stdout, _ = run(exe, td, code, a, seed, None)
            final = [l for l in stdout.splitlines() if l.startswith("Final result:")][0]
            frames += int(final.split()[6])   # "Final result: E bit errs in W words, ..."
            ferrs += sum(1 for l in stdout.splitlines() if l.startswith("Ferr with "))
        pooled = {"code": code, "args": a, "seeds": seeds, "frames": frames, "frame_errors": ferrs}
        print("fer_pooled:", pooled)
    with open(os.path.join(GOLD, "reference_runs_rsmngdbf.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_golden_rsmngdbf.py",
                   "source": "unmodified reference RNGDBF.cpp, -O2, the switches of decodeRSMNGDBF",
                   "runs": out, "fer_pooled": pooled}, f, indent=1)


if __name__ == "__main__":
    main()
