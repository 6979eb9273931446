#!/usr/bin/env python3
"""Generate tests/golden/reference_runs_redecode.json from the REFERENCE's redecodeStatistics
and replayGDBF.

Compiles the unmodified reference sources (ereiss123/LDPCsimulation C_implementations/src/
newstat.cpp and replayGDBF.cpp + alist.cpp + r.cpp + nrutil.cpp, -O2, with the five switches
of their Makefile targets: -D addNoise -D thresholdAdaptation -D weightSyndromes
-D outputSmoothing -D saturateSamples) into a temporary directory. Both include rand_gsl.h,
which needs GSL; this script writes a stand-in for the few GSL calls they make
(gsl_rng_alloc/set/uniform/uniform_pos/uniform_int/fwrite/fread, gsl_ran_ugaussian) into that
directory: glibc random() and the Box-Muller of the reference's rand.h (the cos operand's
uniform is drawn first), the generator every other recorded run of this project uses. A saved
generator state is the text "seed draws": the seed and the random() calls made since. time()
is wrapped at link time (oracle/seed_time.c, REF_SEED) so that ran_seed(time(0)) is
reproducible; the date in the file names under tmp/ comes from the same call.

The programs run in a directory that has tmp/. Recorded per statistics run: stdout, the log
table and the "seed draws" content of each state file. Per replay run (started from a state
file of a statistics run): stdout, the log line, and per trace file the row count, the
sha-256 of its bytes and per row the number of -1 among the decisions and among the checks.
Nothing compiled is kept.

    python tests/golden/make_golden_redecode.py REFERENCE_ROOT     (from the repo root;
    REFERENCE_ROOT = the reference's C_implementations directory)
"""
import glob
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLD = os.path.join(ROOT, "tests", "golden")
CODES = os.path.join(GOLD, "codes")
SWITCHES = ["addNoise", "thresholdAdaptation", "weightSyndromes", "outputSmoothing", "saturateSamples"]

GSL_RNG_H = r"""
/* Stand-in for <gsl/gsl_rng.h>: glibc random(), state = seed + draws made. */
#ifndef STANDIN_GSL_RNG_H
#define STANDIN_GSL_RNG_H
#include <stdio.h>
#include <stdlib.h>
typedef struct { unsigned long seed, draws; } gsl_rng;
typedef int gsl_rng_type;
static const gsl_rng_type *gsl_rng_taus = 0;
static inline gsl_rng *gsl_rng_alloc(const gsl_rng_type *t) { (void)t; return (gsl_rng *)calloc(1, sizeof(gsl_rng)); }
static inline void gsl_rng_set(gsl_rng *r, unsigned long s) { r->seed = s; r->draws = 0; srandom((unsigned)s); }
static inline long standin_random(gsl_rng *r) { r->draws++; return random(); }
static inline double gsl_rng_uniform(gsl_rng *r) { return (double)standin_random(r) / (1.0 + (double)0x7fffffff); }
static inline double gsl_rng_uniform_pos(gsl_rng *r) { return (1.0 + (double)standin_random(r)) / (2.0 + (double)0x7fffffff); }
static inline unsigned long gsl_rng_uniform_int(gsl_rng *r, unsigned long n) { return (unsigned long)standin_random(r) % n; }
static inline int gsl_rng_fwrite(FILE *f, const gsl_rng *r) { return fprintf(f, "%lu %lu\n", r->seed, r->draws) < 0; }
static inline int gsl_rng_fread(FILE *f, gsl_rng *r)
{
    unsigned long s, n, i;
    if (!f || fscanf(f, "%lu %lu", &s, &n) != 2) return 1;
    gsl_rng_set(r, s);
    for (i = 0; i < n; ++i) (void)standin_random(r);
    return 0;
}
#endif
"""
GSL_RANDIST_H = r"""
/* Stand-in for <gsl/gsl_randist.h>: rand.h's rann(), the cos operand's uniform drawn first. */
#ifndef STANDIN_GSL_RANDIST_H
#define STANDIN_GSL_RANDIST_H
#include <math.h>
#include <gsl/gsl_rng.h>
static inline double gsl_ran_ugaussian(gsl_rng *r)
{
    double u_angle = gsl_rng_uniform(r);
    double u_rad = gsl_rng_uniform(r);
    return cos(2.0 * 3.141592654 * u_angle) * sqrt(-2.0 * log(1.0 - u_rad));
}
#endif
"""


def args(R, snr, T, NR, NF, theta, ns, lam, alpha):
    """R SNR T NR NF theta LOG noiseScale lambda alpha windowsize Ymax (newstat.cpp:92-113)."""
    return [R, snr, T, NR, NF, theta, "@LOG@", ns, lam, alpha, "16", "2.5"]


# (name, code, args after alist, seed, codeword file or None, frame to replay or None)
RUNS = [
    ("redecode_peg_3.0_T50_NR6_s5", "PEGReg504x1008.alist", args("0.5", "3.0", "50", "6", "8", "-0.6", "0.75", "0.99", "0.96"),
     5, None, 3),
    ("redecode_1944_4.0_T100_NR5_s9", "80211n_1944_r12.alist",
     args("0.5", "4.0", "100", "5", "6", "-0.6", "0.75", "0.99", "1.5"), 9, None, 1),
    ("redecode_8023_3.6_T100_NR5_s11", "802_3_H.alist",
     args("0.8125", "3.6", "100", "5", "6", "-0.525", "0.92", "1", "0.5"), 11, None, 4),
    ("redecode_peg_cw_3.0_T50_NR6_s7", "PEGReg504x1008.alist",
     args("0.5", "3.0", "50", "6", "8", "-0.6", "0.75", "0.99", "0.96"), 7, "PEGReg504x1008_data20.enc", None),
]

PATH_TOKEN, CW_TOKEN, LOG_NAME = "@ALIST@", "@CWFILE@", "log.txt"


def build(ref, td):
    src, inc = os.path.join(ref, "src"), os.path.join(ref, "inc")
    os.makedirs(os.path.join(td, "standin", "gsl"))
    for name, text in (("gsl_rng.h", GSL_RNG_H), ("gsl_randist.h", GSL_RANDIST_H)):
        with open(os.path.join(td, "standin", "gsl", name), "w") as f:
            f.write(text)
    seed_o = os.path.join(td, "seed_time.o")
    subprocess.run(["gcc", "-O2", "-c", "-o", seed_o, os.path.join(ROOT, "oracle", "seed_time.c")], check=True)
    exes = {}
    for exe, main in (("redecodeStatistics", "newstat.cpp"), ("replayGDBF", "replayGDBF.cpp")):
        exes[exe] = os.path.join(td, exe)
        subprocess.run(["g++", "-O2", "-w", "-I" + inc, "-I" + os.path.join(td, "standin"), "-Wl,--wrap=time"] +
                       [x for s in SWITCHES for x in ("-D", s)] + ["-o", exes[exe]] +
                       [os.path.join(src, f) for f in ("nrutil.cpp", "r.cpp", "alist.cpp")] +
                       [seed_o, os.path.join(src, main), "-lm"], check=True)
    return exes


def fresh_dir(td, name):
    wd = os.path.join(td, name)
    os.makedirs(os.path.join(wd, "tmp"))
    return wd


def run(exe, wd, alist, a, seed, cw):
    cmd = [exe, alist] + [LOG_NAME if x == "@LOG@" else x for x in a] + ([os.path.join(CODES, cw)] if cw else [])
    p = subprocess.run(cmd, cwd=wd, env=dict(os.environ, REF_SEED=str(seed), TZ="UTC"), capture_output=True, text=True,
                       check=True)
    stdout = p.stdout.replace(alist, PATH_TOKEN)
    if cw:
        stdout = stdout.replace(os.path.join(CODES, cw), CW_TOKEN)
    return stdout, open(os.path.join(wd, LOG_NAME)).read()


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = sys.argv[1]
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import code_path
    stats, replays = [], []
    with tempfile.TemporaryDirectory() as td:
        exes = build(ref, td)
        for name, code, a, seed, cw, replay_frame in RUNS:
            alist = code_path(code)
            wd = fresh_dir(td, name)
            stdout, log = run(exes["redecodeStatistics"], wd, alist, a, seed, cw)
            states = sorted(glob.glob(os.path.join(wd, "tmp", "*_RanState_*.state")),
                            key=lambda p: int(p.rsplit("_", 1)[1].split(".")[0]))
            rec = {"name": name, "binary": "redecodeStatistics", "code": code, "args": a, "seed": seed, "cwfile": cw,
                   "stdout": stdout, "log": log, "state_files": [os.path.basename(p) for p in states],
                   "states": [open(p).read().strip() for p in states],
                   "ferr_weights": [int(l.split()[2]) for l in stdout.splitlines() if l.startswith("Ferr with ")],
                   "final": [l for l in stdout.splitlines() if l.startswith("Final result:")][0]}
            stats.append(rec)
            print(f"{name}: {rec['final']}\n{log}")
            if replay_frame is None:
                continue
            # replayGDBF alist R SNR T NR theta statefilename logfilename ... (replayGDBF.cpp:92-115)
            ra = a[:4] + [a[5], "@STATE@"] + a[6:]
            rwd = fresh_dir(td, name + "_replay")
            state = os.path.join(rwd, "frame.state")
            with open(state, "w") as f:
                f.write(rec["states"][replay_frame] + "\n")
            rout, rlog = run(exes["replayGDBF"], rwd, alist, ["frame.state" if x == "@STATE@" else x for x in ra], seed,
                             None)
            traces = []
            for k in range(int(a[3])):
                (path,) = glob.glob(os.path.join(rwd, "tmp", f"*_{LOG_NAME}_{k}.trace"))
                raw = open(path, "rb").read()
                rows = [l.split("\t\t") for l in raw.decode().splitlines()]
                traces.append({"file": os.path.basename(path), "rows": len(rows), "sha256": hashlib.sha256(raw).hexdigest(),
                               "d_neg": [r[0].split("\t").count("-1") for r in rows],
                               "s_neg": [r[1].split("\t").count("-1") for r in rows]})
            replays.append({"name": name + "_replay", "binary": "replayGDBF", "of": name, "frame": replay_frame,
                            "code": code, "args": ra, "seed": seed, "state": rec["states"][replay_frame],
                            "stdout": rout, "log_line": rlog, "traces": traces})
            print(f"{name} replay of frame {replay_frame}: {rlog.strip()} rows {[t['rows'] for t in traces]}")
    with open(os.path.join(GOLD, "reference_runs_redecode.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_golden_redecode.py",
                   "source": "unmodified reference newstat.cpp and replayGDBF.cpp, -O2, the five switches of "
                             "redecodeStatistics / replayGDBF, glibc stand-in for GSL",
                   "runs": stats, "replays": replays}, f, indent=1)


if __name__ == "__main__":
    main()
