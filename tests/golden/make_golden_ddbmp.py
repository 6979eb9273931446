#!/usr/bin/env python3
"""Generate tests/golden/reference_runs_ddbmp.json from the REFERENCE's decodeDDBMP.

Compiles the unmodified reference sources (ereiss123/LDPCsimulation
C_implementations/src/decodeDDBMP.cpp + alist.cpp + r.cpp + nrutil.cpp, -O2) into a
temporary directory, with time() wrapped at link time (oracle/seed_time.c, REF_SEED) so
that ran_seed(time(0)) (:147) is reproducible, runs it, and records the complete stdout,
the log line, the per-frame error weights and the final line of every run as data, in
the format of reference_runs.json (tests/golden/make_golden.py). Nothing compiled is kept.

It also records `fer_pooled`: frames and frame errors of further seeds at one operating
point, the reference side of the two-proportion test of the Philox simulation.

    python tests/golden/make_golden_ddbmp.py REFERENCE_ROOT     (from the repo root; REFERENCE_ROOT =
    the reference's C_implementations directory)
"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLD = os.path.join(ROOT, "tests", "golden")
CODES = os.path.join(GOLD, "codes")

# (name, code, args after alist: R SNR T Ymax Q, seed, codeword file or None)
RUNS = [
    ("ddbmp_peg_3.0_T100_y1.0_q3_s5", "PEGReg504x1008.alist", ["0.5", "3.0", "100", "1.0", "3"], 5, None),
    ("ddbmp_peg_4.0_T100_y1.0_q3_s5", "PEGReg504x1008.alist", ["0.5", "4.0", "100", "1.0", "3"], 5, None),
    ("ddbmp_peg_6.0_T1_y1.0_q4_s4", "PEGReg504x1008.alist", ["0.5", "6.0", "1", "1.0", "4"], 4, None),
    ("ddbmp_peg_cw_3.5_T50_y1.2_q2_s4", "PEGReg504x1008.alist", ["0.5", "3.5", "50", "1.2", "2"], 4,
     "PEGReg504x1008_data20.enc"),
    ("ddbmp_1944_4.0_T100_y1.0_q3_s9", "80211n_1944_r12.alist", ["0.5", "4.0", "100", "1.0", "3"], 9, None),
    ("ddbmp_4000_cw_3.8_T100_y1.4_q3_s13", "4000.2000.4.244.alist", ["0.5", "3.8", "100", "1.4", "3"], 13,
     "4000.2000.4.244_data10.enc"),
]
# the pooled operating point: PEG 4.0 dB, T 100, Ymax 1.0, Q 3
POOL = ("PEGReg504x1008.alist", ["0.5", "4.0", "100", "1.0", "3"], list(range(101, 111)))

PATH_TOKEN = "@ALIST@"
CW_TOKEN = "@CWFILE@"
LOG_TOKEN = "@LOGFILE@"


def build(ref, td):
    src, inc = os.path.join(ref, "src"), os.path.join(ref, "inc")
    exe = os.path.join(td, "decodeDDBMP")
    seed_o = os.path.join(td, "seed_time.o")
    subprocess.run(["gcc", "-O2", "-c", "-o", seed_o, os.path.join(ROOT, "oracle", "seed_time.c")], check=True)
    subprocess.run(["g++", "-O2", "-w", "-I" + inc, "-Wl,--wrap=time", "-o", exe] +
                   [os.path.join(src, f) for f in ("nrutil.cpp", "r.cpp", "alist.cpp")] +
                   [seed_o, os.path.join(src, "decodeDDBMP.cpp"), "-lm"], check=True)
    return exe


def run(exe, td, code, args, seed, cw):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import code_path
    alist = code_path(code)
    log = os.path.join(td, "log.txt")
    if os.path.exists(log):
        os.remove(log)
    cmd = [exe, alist] + args + [log] + ([os.path.join(CODES, cw)] if cw else [])
    p = subprocess.run(cmd, env=dict(os.environ, REF_SEED=str(seed)), capture_output=True, text=True, check=True)
    stdout = p.stdout.replace(alist, PATH_TOKEN).replace(log, LOG_TOKEN)
    if cw:
        stdout = stdout.replace(os.path.join(CODES, cw), CW_TOKEN)
    return stdout, open(log).read().replace(alist, PATH_TOKEN)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = sys.argv[1]
    out = []
    with tempfile.TemporaryDirectory() as td:
        exe = build(ref, td)
        for name, code, args, seed, cw in RUNS:
            stdout, logline = run(exe, td, code, args, seed, cw)
            ferr = [int(l.split()[2]) for l in stdout.splitlines() if l.startswith("Ferr with ")]
            final = [l for l in stdout.splitlines() if l.startswith("Final result:")][0]
            out.append({"name": name, "binary": "decodeDDBMP", "code": code, "args": args, "seed": seed,
                        "cwfile": cw, "stdout": stdout, "log_line": logline, "ferr_weights": ferr, "final": final})
            print(f"{name}: {final}")
        code, args, seeds = POOL
        frames = ferrs = 0
        for seed in seeds:
            stdout, _ = run(exe, td, code, args, seed, None)
            final = [l for l in stdout.splitlines() if l.startswith("Final result:")][0]
            frames += int(final.split()[6])   # "Final result: E bit errs in W words, ..."
            ferrs += sum(1 for l in stdout.splitlines() if l.startswith("Ferr with "))
        pooled = {"code": code, "args": args, "seeds": seeds, "frames": frames, "frame_errors": ferrs}
        print("fer_pooled:", pooled)
    with open(os.path.join(GOLD, "reference_runs_ddbmp.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_golden_ddbmp.py", "source": "unmodified reference decodeDDBMP.cpp, -O2",
                   "runs": out, "fer_pooled": pooled}, f, indent=1)


if __name__ == "__main__":
    main()
