// cli_rstat.cpp -- reference-compatible front-ends of the every-attempt NGDBF decoders.
//
// Drop-ins for redecodeStatistics (C_implementations/src/newstat.cpp) and, with -D replay,
// replayGDBF (src/replayGDBF.cpp) of ereiss123/LDPCsimulation, both as their Makefile
// targets build them (addNoise, thresholdAdaptation, weightSyndromes, outputSmoothing,
// saturateSamples): the same positional CLIs
//   redecodeStatistics alist R SNR T NR NF theta logfilename noiseScale lambda alpha
//                      windowsize Ymax [codewords]
//   replayGDBF         alist R SNR T NR theta statefilename logfilename noiseScale lambda
//                      alpha windowsize Ymax [codewords]
// the same stdout (parameters, "Ferr with k errors." [+ " All checks satisfied."],
// "Incremental result" every round(100e3/N) frames with both histograms, "Final result",
// and in replay "Completed phase with k errors.") and the same files: the log gets one
// appended line per frame (framenum, a tab, the NR outcomes each followed by a tab); the
// statistics program writes tmp/<dd-mm-YYYY>_RanState_<framenum>.state before each frame;
// the replay program writes tmp/<dd-mm-YYYY>_<logfilename>_<attempt>.trace, one line per
// iteration run: N decisions, a tab, M check values, each followed by a tab.
//
// Every frame is decoded NR times from the same channel samples, each attempt up to T
// iterations with perturbations of its own; every attempt runs (ldpc_rstat_*).
//
// Where this differs from the reference, on purpose:
//   * The state file is this project's own small text file (format tag, rng kind, seed,
//     stream, frame number, position: the glibc draws consumed before the frame, or the
//     global frame index for Philox). The reference writes a GSL generator state, which
//     cannot be read without GSL; a state file of one program cannot be read by the other's.
//   * Without tmp/ the reference dereferences a null FILE*; these programs say so and exit 1.
//   * The reference's phase histogram has 7 bins and is indexed by NR - 1 (newstat.cpp:218,
//     :440), out of bounds for NR > 7; here the single line "NR:\tframes" is printed for any NR.
//   * With a codeword file the reference's replay reads the file's first line whatever the
//     frame; here the replay uses the frame's own line (the state file knows the frame
//     number). The outcomes are the same: the decoder is symmetric under a codeword.
//
// Environment (the positional CLI stays identical), as cli_gdbf.cpp:
//   LDPC_RNG       glibc (default): the reference's noise built against glibc random() and
//                  rand.h rann(), drawn on the host in the reference's order (the channel,
//                  then per attempt one row of N perturbations per iteration that passes its
//                  syndrome check); attempts are decoded one at a time in fp64, because an
//                  attempt's rows are known only once the previous attempt's iteration
//                  count is. The verification mode.
//                  philox: channel and perturbations generated on the GPU, LDPC_BATCH frames
//                  x NR attempts per launch. The mode to use.
//   LDPC_SEED, LDPC_PRECISION, LDPC_BATCH, LDPC_DEVICE, LDPC_DRY_RUN as cli_minsum.cpp.
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <algorithm>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include <sys/stat.h>

#include "ldpc_hip.h"
#include "cli_common.h"

using std::cout;
using std::endl;

namespace {

const char *env_or(const char *k, const char *d)
{
    const char *v = std::getenv(k);
    return (v && *v) ? v : d;
}

[[noreturn]] void die(const char *what)
{
    std::cerr << "ldpc: " << what << ": " << ldpc_last_error() << endl;
    std::exit(1);
}

void print_histogram(const std::vector<int> &h)   // printHistogram (newstat.cpp:538-545)
{
    for (size_t i = 0; i < h.size(); ++i)
        if (h[i] > 0) cout << i + 1 << ":\t" << h[i] << endl;
}

const char *const kStateTag = "ldpc-rstat-state 1";

struct State {
    std::string rng;
    long long seed = 0, stream = 0, frame = 0, position = 0;
};

#ifndef replay
bool write_state(const std::string &path, const State &s)
{
    std::ofstream f(path.c_str());
    f << kStateTag << "\nrng " << s.rng << "\nseed " << s.seed << "\nstream " << s.stream << "\nframe " << s.frame
      << "\nposition " << s.position << "\n";
    return (bool)f;
}
#else
bool read_state(const std::string &path, State &s)
{
    std::ifstream f(path.c_str());
    std::string tag, k[5];
    if (!std::getline(f, tag) || tag != kStateTag) return false;
    f >> k[0] >> s.rng >> k[1] >> s.seed >> k[2] >> s.stream >> k[3] >> s.frame >> k[4] >> s.position;
    return (bool)f && k[0] == "rng" && k[1] == "seed" && k[2] == "stream" && k[3] == "frame" && k[4] == "position" &&
           (s.rng == "glibc" || s.rng == "philox") && s.frame >= 0 && s.position >= 0;
}
#endif

}  // namespace

int main(int argc, char *argv[])
{
#ifdef replay
    std::vector<std::string> args = {"alist", "R", "SNR", "T", "NR", "theta", "statefilename", "logfilename"};
#else
    std::vector<std::string> args = {"alist", "R", "SNR", "T", "NR", "NF", "theta", "logfilename"};
#endif
    for (const char *a : {"noiseScale", "lambda", "alpha", "windowsize", "Ymax", "[codeword filename]"}) args.push_back(a);
    if ((size_t)argc != args.size() && (size_t)argc != args.size() + 1) {
        cout << "Usage: " << argv[0];
        for (const auto &a : args) cout << " " << a;
        cout << "\n";
#ifdef replay
        cout << "statefilename: a tmp/<dd-mm-YYYY>_RanState_<framenum>.state file written by this project's "
                "redecodeStatistics (text: format tag, rng, seed, stream, frame, position); a GSL generator state "
                "of the reference cannot be read without GSL.\n";
#else
        cout << "Writes tmp/<dd-mm-YYYY>_RanState_<framenum>.state before each frame in this project's own text "
                "format (format tag, rng, seed, stream, frame, position), which this project's replayGDBF reads; "
                "it is not a GSL generator state.\n";
#endif
        return 0;
    }

    ldpc_rstat_cfg cfg;
    std::memset(&cfg, 0, sizeof cfg);
    cfg.flags = LDPC_GDBF_NOISE | LDPC_GDBF_ADAPT | LDPC_GDBF_WEIGHT | LDPC_GDBF_SMOOTH | LDPC_GDBF_SATURATE;
    int idx = 1;
    ldpc_graph *H = nullptr;
    if (ldpc_graph_load_alist(argv[idx++], &H) != LDPC_OK) die("loading alist");
    int N = 0, M = 0;
    ldpc_graph_info(H, &N, &M, nullptr, nullptr, nullptr);
    cout << "PARAMETERS: \n alist = \t" << argv[1] << endl;   // newstat.cpp:134-169
    const double R = std::atof(argv[idx++]);
    cout << " R = \t" << R << endl;
    const double SNR = std::atof(argv[idx++]);
    cout << " SNR = \t" << SNR << endl;
    const int T = std::atoi(argv[idx++]);
    cout << " T = \t" << T << endl;
    const int NR = std::atoi(argv[idx++]);
    cout << " NR = \t" << NR << endl;
#ifndef replay
    const long NF = std::atol(argv[idx++]);
    cout << " NF = \t" << NF << endl;
#endif
    cfg.theta = std::atof(argv[idx++]);
    cout << " theta = \t" << cfg.theta << endl;
#ifdef replay
    const std::string statefilename(argv[idx++]);
    cout << " state = \t" << statefilename << endl;
#endif
    const std::string logfilename(argv[idx++]);
    cout << " log = \t" << logfilename << endl;
    cfg.noise_scale = std::atof(argv[idx++]);
    cout << " noiseScale = \t" << cfg.noise_scale << endl;
    cfg.lambda = std::atof(argv[idx++]);
    cout << " lambda = \t" << cfg.lambda << endl;
    cfg.alpha = std::atof(argv[idx++]);
    cout << " alpha = \t" << cfg.alpha << endl;
    cfg.windowsize = std::atoi(argv[idx++]);
    cout << "windowsize = \t" << cfg.windowsize << endl;
    cfg.ymax = std::atof(argv[idx++]);
    cout << " Ymax = \t" << cfg.ymax << endl;
    cfg.T = T;
    if (T < 1 || T > 4094 || NR < 1) {
        std::cerr << "ldpc: 1 <= T <= 4094 and NR >= 1 are required" << endl;
        return 1;
    }

    std::vector<std::string> cw_lines;
    const bool use_cw = (size_t)argc == args.size() + 1;
    if (use_cw) {
        cout << "\nUsing codewords from " << argv[idx] << endl;
        cw_lines = reference_codeword_lines(argv[idx]);
    } else {
        cout << "\nUsing all-zero sequence.\n";
    }

    char timeString[80];   // newstat.cpp:184-189
    time_t rawtime;
    time(&rawtime);
    strftime(timeString, sizeof timeString, "%d-%m-%Y", localtime(&rawtime));

    const double N0 = std::pow(10.0, -SNR / 10.0) / R;   // :192-193
    const double sigma = std::sqrt(N0 / 2.0);
    int dv = 0, dc = 0;
    alist_header(argv[1], dv, dc);
    cout << "Simulating GDBF decoding on code with N=" << N << ", M=" << M << ", R=" << R << ", dv=" << dv
         << ", dc=" << dc << endl;
    cout << "\nParameters are:\n\tSNR\t" << SNR << "\n\tN0\t" << N0 << "\n\tsigma\t" << sigma << endl;

    // the reference opens its files under tmp/ without a check and writes through a null FILE*
    struct stat st;
    if (stat("tmp", &st) != 0 || !S_ISDIR(st.st_mode)) {
        std::cerr << "ldpc: the directory tmp/ does not exist here; the state and trace files go there" << endl;
        return 1;
    }

    // ---- GPU setup ----
    std::string rng = env_or("LDPC_RNG", "glibc");
    const std::string prec = env_or("LDPC_PRECISION", "f64");   // the reference's double; f32 opt-in
    cfg.precision = prec == "f32" ? LDPC_F32 : LDPC_F64;
    long long seed = std::atoll(env_or("LDPC_SEED", std::to_string((long long)time(0)).c_str()));
    const int device = std::atoi(env_or("LDPC_DEVICE", "0"));
    long framenum0 = 0;   // the global number of the first frame
#ifdef replay
    State st0;
    const bool dry = std::getenv("LDPC_DRY_RUN") != nullptr;
    if (!dry) {
        if (!read_state(statefilename, st0)) {   // replayGDBF.cpp:251-256
            cout << "Failed to load ran state.\n";
            std::cerr << "ldpc: " << statefilename << " is not a state file of this project's redecodeStatistics" << endl;
            return 1;
        }
        rng = st0.rng;   // the state decides: its position means draws or frames accordingly
        seed = st0.seed;
        framenum0 = (long)st0.frame;
    }
    const long NF = 1;
#endif
    const bool philox = rng == "philox";
    if (!philox && rng != "glibc") {
        std::cerr << "ldpc: LDPC_RNG must be glibc or philox" << endl;
        return 1;
    }
    int batch = philox ? std::atoi(env_or("LDPC_BATCH", "256")) : 1;
    if (batch <= 0) {
        std::cerr << "ldpc: LDPC_BATCH must be > 0" << endl;
        return 1;
    }
#ifdef replay
    batch = 1;
#endif
    if (std::getenv("LDPC_DRY_RUN")) {   // report the GPU settings and stop before any device call
        std::cerr << "ldpc: rng=" << rng << " precision=" << (cfg.precision == LDPC_F64 ? "f64" : "f32")
                  << " batch=" << batch << " device=" << device << endl;
        return 0;
    }
    ldpc_ctx *ctx = nullptr;
    if (ldpc_ctx_create(device, H, batch, &ctx) != LDPC_OK) die("creating device context");

    std::vector<int8_t> c_cur(N, 1);
    auto load_codeword = [&](long frame, std::vector<int8_t> &c) {
        apply_codeword_line(cw_lines[(size_t)(frame % (long)cw_lines.size())], N, c, cout);
    };
    if (philox && use_cw) {
        std::vector<uint8_t> bits((size_t)cw_lines.size() * N);
        for (size_t r = 0; r < cw_lines.size(); ++r) {
            load_codeword((long)r, c_cur);
            for (int i = 0; i < N; ++i) bits[r * N + i] = c_cur[i] < 0 ? 1 : 0;
        }
        if (ldpc_sim_set_codewords(ctx, bits.data(), (int)cw_lines.size()) != LDPC_OK) die("uploading codewords");
    }

    const int reportInterval = (int)std::round(100e3 / N);   // newstat.cpp:468
    long errors = 0, uncodedErrors = 0, totalBits = 0, totalWords = 0, wordErrors = 0, totalIterations = 0;
    std::vector<int> hist(N, 0);
    GlibcRandom g((uint32_t)seed);   // ran_seed(time(0)) (:244)
    long long drawn = 0;             // glibc draws consumed so far (two per normal)
#ifdef replay
    if (!philox) {
        for (long long k = 0; k < st0.position; ++k) (void)g.next();
        drawn = st0.position;
    }
    std::vector<int8_t> dtr((size_t)T * N), str((size_t)T * M);
#endif
    const double noiseSigma = sigma * cfg.noise_scale;   // :336
    std::vector<double> y(N), pert;
    std::vector<float> yf, pf;
    if (!philox) pert.resize((size_t)T * N);
    std::vector<ldpc_attempt_result> att((size_t)batch * NR);
    std::vector<ldpc_frame_result> res(batch);

    // one frame's bookkeeping once its NR outcomes are known (newstat.cpp:421-480)
    auto account = [&](long framenum, const ldpc_attempt_result *a, int uncoded) {
        std::ofstream of(logfilename.c_str(), std::ios::app);
        of << framenum << "\t";
        for (int k = 0; k < NR; ++k) {
            of << a[k].bit_err << "\t";
            totalIterations += a[k].iters;
        }
        of << std::endl;
        of.close();
        const int newErrors = a[NR - 1].bit_err;
        const bool satisfied = a[NR - 1].iters < T;   // of the last attempt
        uncodedErrors += uncoded;
        if (newErrors > 0) {
            cout << "Ferr with " << newErrors << " errors.";
            if (satisfied)
                cout << " All checks satisfied.\n";
            else
                cout << endl;
            errors += newErrors;
            hist[newErrors - 1]++;
            wordErrors++;
        }
        totalBits += N;
        totalWords++;
        if (reportInterval > 0 && (totalWords % reportInterval) == 0) {   // N > 200 000: the reference divides by 0
            cout << "\nIncremental result: " << errors << " bit errs in " << totalWords
                 << " words, BER=" << (double)errors / totalBits
                 << ". Average iterations = " << (double)totalIterations / totalWords << ". Word error=" << wordErrors
                 << ". Uncoded errors = " << uncodedErrors << ", uncBER=" << (double)uncodedErrors / totalBits
                 << "\nError weights:\n";
            print_histogram(hist);
            cout << "Phase histogram:\n" << NR << ":\t" << totalWords << endl;
        }
    };

#ifdef replay
    // the trace file of attempt k (replayGDBF.cpp:315-317, :370-376) and its console line (:401)
    auto finish_attempt = [&](int k) {
        std::ostringstream ss;
        ss << "tmp/" << timeString << "_" << logfilename << "_" << k << ".trace";
        std::ofstream tf(ss.str().c_str(), std::ios::out);
        for (int it = 0; it < att[k].iters; ++it) {
            for (int i = 0; i < N; ++i) tf << (int)dtr[(size_t)it * N + i] << "\t";
            tf << "\t";
            for (int j = 0; j < M; ++j) tf << (int)str[(size_t)it * M + j] << "\t";
            tf << "\n";
        }
        tf.close();
        cout << "Completed phase with " << att[k].bit_err << " errors.\n";
    };
#endif

    for (long done = 0; done < NF;) {
        const int nb = (int)std::min<long>(batch, NF - done);
#ifndef replay
        for (int f = 0; f < nb; ++f) {   // recordRanState (:250, :783-791); Philox frames are independent
            std::ostringstream ss;
            ss << "tmp/" << timeString << "_RanState_" << done + f << ".state";
            State s;
            s.rng = rng;
            s.seed = seed;
            s.frame = done + f;
            s.position = philox ? done + f : drawn;
            if (!write_state(ss.str(), s)) {
                std::cerr << "ldpc: cannot write " << ss.str() << endl;
                return 1;
            }
        }
#endif
        if (philox) {
#ifdef replay
            for (int k = 0; k < NR; ++k) {   // one attempt per launch: its trace is T rows
                ldpc_rstat_cfg c1 = cfg;
                c1.attempts = 1;
                c1.first_attempt = k;
                ldpc_rstat_trace tr{nullptr, nullptr, dtr.data(), str.data()};
                if (ldpc_rstat_sim_batch(ctx, SNR, R, &c1, (uint64_t)seed, (uint32_t)st0.stream, (uint64_t)st0.position, 1,
                                         &att[k], &tr, res.data(), nullptr) != LDPC_OK)
                    die("simulating attempt");
#else
            {
                cfg.attempts = NR;
                cfg.first_attempt = 0;
                if (ldpc_rstat_sim_batch(ctx, SNR, R, &cfg, (uint64_t)seed, 0u, (uint64_t)done, nb, att.data(), nullptr,
                                         res.data(), nullptr) != LDPC_OK)
                    die("simulating batch");
#endif
#ifdef replay
                finish_attempt(k);
#endif
            }
        } else {
            if (use_cw) load_codeword(framenum0 + done, c_cur);
            for (int i = 0; i < N; ++i) y[i] = (double)c_cur[i] * (1.0 + sigma * g.rann());   // :279-281
            drawn += 2ll * N;
            for (int k = 0; k < NR; ++k) {
                GlibcRandom ahead = g;   // the rows this attempt may use, drawn ahead from a copy
                for (size_t q = 0; q < pert.size(); ++q) pert[q] = noiseSigma * ahead.rann();
                const void *yin = y.data(), *pin = pert.data();
                if (cfg.precision == LDPC_F32) {
                    yf.assign(y.begin(), y.end());
                    pf.assign(pert.begin(), pert.end());
                    yin = yf.data();
                    pin = pf.data();
                }
                ldpc_rstat_cfg c1 = cfg;
                c1.attempts = 1;
                c1.first_attempt = k;
#ifdef replay
                ldpc_rstat_trace tr{nullptr, nullptr, dtr.data(), str.data()};
                const ldpc_rstat_trace *trp = &tr;
#else
                const ldpc_rstat_trace *trp = nullptr;
#endif
                if (ldpc_rstat_decode_batch(ctx, yin, pin, 1, &c1, use_cw ? c_cur.data() : nullptr, &att[k], trp, nullptr,
                                            res.data(), nullptr) != LDPC_OK)
                    die("decoding attempt");
                // advance by the rows the attempt drew (one per iteration run, :361-376)
                for (long q = 0; q < (long)N * att[k].iters; ++q) (void)g.rann();
                drawn += 2ll * N * att[k].iters;
#ifdef replay
                finish_attempt(k);
#endif
            }
        }
        for (int f = 0; f < nb; ++f) account(done + f, &att[(size_t)f * NR], res[f].uncoded_bit_err);
        done += nb;
    }

    cout << "\nFinal result: " << errors << " bit errs in " << totalWords << " words, BER=" << (double)errors / totalBits
         << ". Average iterations = " << (double)totalIterations / totalWords << ". Uncoded errors = " << uncodedErrors
         << ", uncBER=" << (double)uncodedErrors / totalBits << endl;
    cout << "Phase histogram:\n" << endl;   // an empty line after the header (:494)
    cout << NR << ":\t" << totalWords << endl;

    ldpc_ctx_destroy(ctx);
    ldpc_graph_destroy(H);
    return 0;
}
