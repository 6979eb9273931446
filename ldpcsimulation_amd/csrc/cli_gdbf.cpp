// cli_gdbf.cpp -- reference-compatible front-end of the MI355X GDBF / NGDBF
// bit-flipping decoders.
//
// Drop-in for the decodeGDBF family of ereiss123/LDPCsimulation
// (C_implementations/src/decodeGDBF.cpp:86-454) in its parallel-flip mode:
// the same positional CLI
//   decodeXGDBF alist R SNR T theta logfilename [noiseScale] [NQ] [lambda]
//               [alpha] [windowsize] [Ymax] [codewordfile]
// with the variant fixed at compile time by the same -D macros (addNoise,
// quantizeSamples, thresholdAdaptation, weightSyndromes, outputSmoothing,
// saturateSamples; Makefile:33-53), the same stdout (parameters, "Ferr with k
// errors." [+ " All checks satisfied."], "Incremental result" every
// round(100e3/N) frames with the histogram, "Final result") and the same
// appended log line (:425-452). Stop rule: errors >= 200 and word errors >=
// 20 (10 for N > 10000, 5 for N > 50000), frame by frame (:221-226).
//
// Environment (the positional CLI stays identical):
//   LDPC_RNG       glibc (default): the reference's noise -- glibc random()
//                  TYPE_3 seeded like ran_seed(seed) and rand.h rann(), drawn
//                  on the host in the reference's order (channel, then one
//                  row of N perturbations per iteration that passes its
//                  syndrome check); frames are decoded one at a time in fp64
//                  on the GPU, so the output equals the reference's.
//                  philox: channel and perturbations generated on the GPU,
//                  batched (LDPC_BATCH frames per launch).
//   LDPC_SEED, LDPC_PRECISION, LDPC_BATCH, LDPC_DEVICE, LDPC_DRY_RUN as cli_minsum.cpp.
//
// With -D redecode this is decodeRSMNGDBF (src/RNGDBF.cpp:79-485): `maxphase` follows
// Ymax on the command line, frames go through ldpc_rgdbf_*, a "Phase histogram:" block
// follows every incremental result and the final one, and the log line counts
// smoothingUsed per phase and ends with maxphase. A frame's glibc perturbation rows are
// contiguous over its phases (a failed phase consumes exactly T rows of N draws).
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

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

void print_histogram(const std::vector<int> &h)   // printHistogram (:465-472)
{
    for (size_t i = 0; i < h.size(); ++i)
        if (h[i] > 0) cout << i + 1 << ":\t" << h[i] << endl;
}

#ifdef redecode
// Phases a frame ran, from its total iterations: a failed phase runs exactly T
// iterations, a satisfied one fewer (native.py rgdbf_phases is the same formula).
int rgdbf_phases(int iters, int T, int maxphase)
{
    const int p = iters / T + 1;
    return p < maxphase ? p : maxphase;
}
// Phases of the frame that end with `it > T - windowsize` (RNGDBF.cpp:388-389): every
// failed phase when windowsize > 0, and the last phase by its own iteration count.
int rgdbf_smoothing_used(int iters, int T, int maxphase, int windowsize)
{
    const int p = rgdbf_phases(iters, T, maxphase);
    const int last = iters - (p - 1) * T;
    return (p - 1) * (windowsize > 0) + (last > T - windowsize);
}
#endif

}  // namespace

int main(int argc, char *argv[])
{
    std::vector<std::string> args = {"alist", "R", "SNR", "T", "theta", "logfilename"};   // :88-113
#if defined(addNoise) || defined(quantizeProbabilities)
    args.push_back("noiseScale");
#endif
#ifdef quantizeSamples
    args.push_back("NQ");
#endif
#ifdef thresholdAdaptation
    args.push_back("lambda");
#endif
#ifdef weightSyndromes
    args.push_back("alpha");
#endif
#ifdef outputSmoothing
    args.push_back("windowsize");
#endif
#ifdef saturateSamples
    args.push_back("Ymax");
#endif
#ifdef redecode
    args.push_back("maxphase");
#endif
    args.push_back("[codeword filename]");
    if ((size_t)argc != args.size() && (size_t)argc != args.size() + 1) {   // :116-123
        cout << "Usage: " << argv[0];
        for (const auto &a : args) cout << " " << a;
        cout << "\n";
        return 0;
    }

    ldpc_gdbf_cfg cfg;
    std::memset(&cfg, 0, sizeof cfg);
    // the reference's defaults (:48-56)
    cfg.lambda = 0.991;
    cfg.alpha = 2.25;
    cfg.ymax = 2.25;
    cfg.windowsize = 64;
    cfg.noise_scale = 1.0;
    cfg.nq = 16;
    int idx = 1;
    ldpc_graph *H = nullptr;
    if (ldpc_graph_load_alist(argv[idx++], &H) != LDPC_OK) die("loading alist");
    int N = 0, M = 0;
    ldpc_graph_info(H, &N, &M, nullptr, nullptr, nullptr);
    cout << "PARAMETERS: \n alist = \t" << argv[1] << endl;   // :128-163
    const double R = std::atof(argv[idx++]);
    cout << " R = \t" << R << endl;
    const double SNR = std::atof(argv[idx++]);
    cout << " SNR = \t" << SNR << endl;
    const int T = std::atoi(argv[idx++]);
    cout << " T = \t" << T << endl;
    cfg.T = T;
    const double theta = std::atof(argv[idx++]);
    cout << " theta = \t" << theta << endl;
    cfg.theta = theta;
    const std::string logfilename(argv[idx++]);
    cout << " log = \t" << logfilename << endl;
#if defined(addNoise) || defined(quantizeProbabilities)
    cfg.noise_scale = std::atof(argv[idx++]);
    cout << " noiseScale = \t" << cfg.noise_scale << endl;
#endif
#ifdef addNoise
    cfg.flags |= LDPC_GDBF_NOISE;
#endif
#ifdef quantizeProbabilities
    cfg.flags |= LDPC_GDBF_QPROB;   // :562-597
#endif
#ifdef sequentialmode
    cfg.flags |= LDPC_GDBF_SEQUENTIAL;   // :285-289
#endif
#ifdef modeswitching
    cfg.flags |= LDPC_GDBF_MODESWITCH;   // :309-345, Tswitch = 0 (:51)
#endif
#ifdef quantizeSamples
    cfg.flags |= LDPC_GDBF_QUANTIZE;
    cfg.nq = std::atoi(argv[idx++]);
    cout << " NQ = \t" << cfg.nq << endl;
#endif
#ifdef thresholdAdaptation
    cfg.flags |= LDPC_GDBF_ADAPT;
    cfg.lambda = std::atof(argv[idx++]);
    cout << " lambda = \t" << cfg.lambda << endl;
#endif
#ifdef weightSyndromes
    cfg.flags |= LDPC_GDBF_WEIGHT;
    cfg.alpha = std::atof(argv[idx++]);
    cout << " alpha = \t" << cfg.alpha << endl;
#endif
#ifdef outputSmoothing
    cfg.flags |= LDPC_GDBF_SMOOTH;
    cfg.windowsize = std::atoi(argv[idx++]);
    cout << "windowsize = \t" << cfg.windowsize << endl;
#endif
#ifdef saturateSamples
    cfg.flags |= LDPC_GDBF_SATURATE;
    cfg.ymax = std::atof(argv[idx++]);
    cout << " Ymax = \t" << cfg.ymax << endl;
#endif
#ifdef redecode
    const int maxphase = std::atoi(argv[idx++]);   // RNGDBF.cpp:153-156
    cout << " maxphase = \t" << maxphase << endl;
    if (T < 1 || maxphase < 1 || (long)T * maxphase > 4094) {
        std::cerr << "ldpc: T >= 1, maxphase >= 1 and maxphase * T <= 4094 are required" << endl;
        return 1;
    }
    const int rows_per_frame = T * maxphase;
#else
    const int rows_per_frame = T > 0 ? T : 1;
#endif

    std::vector<std::string> cw_lines;   // :165-172, :230-249
    const bool use_cw = (size_t)argc == args.size() + 1;
    if (use_cw) {
        cout << "\nUsing codewords from " << argv[idx] << endl;
        cw_lines = reference_codeword_lines(argv[idx]);
    } else {
        cout << "\nUsing all-zero sequence.\n";
    }

    const double N0 = std::pow(10.0, -SNR / 10.0) / R;   // :175-176
    const double sigma = std::sqrt(N0 / 2.0);
    int dv = 0, dc = 0;
    alist_header(argv[1], dv, dc);
    cout << "Simulating GDBF decoding on code with N=" << N << ", M=" << M << ", R=" << R << ", dv=" << dv
         << ", dc=" << dc << endl;
    cout << "\nParameters are:\n\tSNR\t" << SNR << "\n\tN0\t" << N0 << "\n\tsigma\t" << sigma << endl;

    // ---- GPU setup ----
    const std::string rng = env_or("LDPC_RNG", "glibc");
    const bool philox = rng == "philox";
    if (!philox && rng != "glibc") {
        std::cerr << "ldpc: LDPC_RNG must be glibc or philox" << endl;
        return 1;
    }
    const std::string prec = env_or("LDPC_PRECISION", "f64");   // the reference's double; f32 opt-in
    cfg.precision = prec == "f32" ? LDPC_F32 : LDPC_F64;
#ifdef redecode
    ldpc_rgdbf_cfg rcfg;
    std::memset(&rcfg, 0, sizeof rcfg);
    rcfg.flags = cfg.flags;
    rcfg.precision = cfg.precision;
    rcfg.T = T;
    rcfg.maxphase = maxphase;
    rcfg.windowsize = cfg.windowsize;
    rcfg.theta = cfg.theta;
    rcfg.lambda = cfg.lambda;
    rcfg.alpha = cfg.alpha;
    rcfg.noise_scale = cfg.noise_scale;
    rcfg.ymax = cfg.ymax;
    std::vector<int> phase_hist(maxphase, 0);   // RNGDBF.cpp:193
#endif
    const long long seed = std::atoll(env_or("LDPC_SEED", std::to_string((long long)time(0)).c_str()));
    const int batch = philox ? std::atoi(env_or("LDPC_BATCH", "65536")) : 1;
    const int device = std::atoi(env_or("LDPC_DEVICE", "0"));
    if (batch <= 0) {
        std::cerr << "ldpc: LDPC_BATCH must be > 0" << endl;
        return 1;
    }
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

    int minWordErrors = 20;   // :221-223
    if (N > 10000) minWordErrors = 10;
    if (N > 50000) minWordErrors = 5;
    const int reportInterval = (int)std::round(100e3 / N);   // :403
    long errors = 0, uncodedErrors = 0, totalBits = 0, totalWords = 0, wordErrors = 0, totalIterations = 0;
    long smoothingUsed = 0;
    std::vector<int> hist(N, 0);
    std::vector<ldpc_frame_result> res(batch);
    GlibcRandom g((uint32_t)seed);   // ran_seed(time(0)) (:224)
    std::vector<double> y, pert;
    std::vector<float> yf, pf;
    const bool noise = (cfg.flags & LDPC_GDBF_NOISE) != 0;
    const bool qprob = (cfg.flags & LDPC_GDBF_QPROB) != 0;   // ranu() per bit and iteration (:588)
    const double noiseSigma = sigma * cfg.noise_scale;   // :296
    if (!philox) {
        y.resize(N);
        if (noise || qprob) pert.resize((size_t)N * rows_per_frame);
    }
    long generated = 0;
    bool done = false;
    while (!done) {
        if (philox) {
            ldpc_counts tmp{};
#ifdef redecode
            if (ldpc_rgdbf_sim_batch(ctx, SNR, R, &rcfg, (uint64_t)seed, 0u, (uint64_t)generated, batch, res.data(),
                                     &tmp) != LDPC_OK)
#else
            if (ldpc_gdbf_sim_batch(ctx, SNR, R, &cfg, (uint64_t)seed, 0u, (uint64_t)generated, batch, res.data(),
                                    &tmp) != LDPC_OK)
#endif
                die("simulating batch");
        } else {
            if (use_cw) load_codeword(generated, c_cur);
            for (int i = 0; i < N; ++i) y[i] = (double)c_cur[i] * (1.0 + sigma * g.rann());   // :251-253
            if (noise) {   // the rows this frame may use, drawn ahead from a copy
                GlibcRandom ahead = g;
                for (size_t k = 0; k < pert.size(); ++k) pert[k] = noiseSigma * ahead.rann();
            }
            if (qprob) {
                GlibcRandom ahead = g;
                for (size_t k = 0; k < pert.size(); ++k) pert[k] = ahead.ranu();
                cfg.qsigma = noiseSigma;   // symNodeUpdates' sigma (:296, :353)
            }
            const void *yin = y.data(), *pin = (noise || qprob) ? pert.data() : nullptr;
            if (cfg.precision == LDPC_F32) {
                yf.assign(y.begin(), y.end());
                pf.assign(pert.begin(), pert.end());
                yin = yf.data();
                pin = (noise || qprob) ? pf.data() : nullptr;
            }
#ifdef redecode
            if (ldpc_rgdbf_decode_batch(ctx, yin, pin, 1, &rcfg, use_cw ? c_cur.data() : nullptr, nullptr, res.data(),
                                        nullptr) != LDPC_OK)
#else
            if (ldpc_gdbf_decode_batch(ctx, yin, pin, 1, &cfg, use_cw ? c_cur.data() : nullptr, nullptr, res.data(),
                                       nullptr) != LDPC_OK)
#endif
                die("decoding frame");
            if (noise)   // advance by the rows the decoder drew (one per iteration run, :318-333)
                for (long k = 0; k < (long)N * res[0].iters; ++k) (void)g.rann();
            if (qprob)
                for (long k = 0; k < (long)N * res[0].iters; ++k) (void)g.ranu();
        }
        generated += batch;
        for (int f = 0; f < batch; ++f) {
            if (!((errors < 200) || (wordErrors < minWordErrors))) {   // :226
                done = true;
                break;
            }
            const int it = res[f].iters;
#ifdef redecode
            const bool satisfied = it < T * maxphase;   // of the last phase: only a frame whose phases all failed runs them all
            if (cfg.flags & LDPC_GDBF_SMOOTH) smoothingUsed += rgdbf_smoothing_used(it, T, maxphase, cfg.windowsize);
            phase_hist[rgdbf_phases(it, T, maxphase) - 1]++;   // RNGDBF.cpp:403
#else
            const bool satisfied = it < T;
            if ((cfg.flags & LDPC_GDBF_SMOOTH) && it > T - cfg.windowsize) smoothingUsed++;   // :371-375
#endif
            const int newErrors = res[f].bit_err;
            uncodedErrors += res[f].uncoded_bit_err;
            if (newErrors > 0) {   // :380-394
                cout << "Ferr with " << newErrors << " errors.";
                if (satisfied)
                    cout << " All checks satisfied.\n";
                else
                    cout << endl;
                errors += newErrors;
                hist[newErrors - 1]++;
                wordErrors++;
            }
            totalWords++;   // :397-399
            totalBits += N;
            totalIterations += it;
            if ((totalWords % reportInterval) == 0) {   // :403-410
                cout << "\nIncremental result: " << errors << " bit errs in " << totalWords
                     << " words, BER=" << (double)errors / totalBits
                     << ". Average iterations = " << (double)totalIterations / totalWords
                     << ". Word error=" << wordErrors << ". Uncoded errors = " << uncodedErrors
                     << ", uncBER=" << (double)uncodedErrors / totalBits << "\nError weights:\n";
                print_histogram(hist);
#ifdef redecode
                cout << "Phase histogram:\n";   // RNGDBF.cpp:434-437
                print_histogram(phase_hist);
#endif
            }
        }
    }

    cout << "\nFinal result: " << errors << " bit errs in " << totalWords << " words, BER=" << (double)errors / totalBits
         << ". Average iterations = " << (double)totalIterations / totalWords << ". Uncoded errors = " << uncodedErrors
         << ", uncBER=" << (double)uncodedErrors / totalBits << endl;
#ifdef redecode
    cout << "Phase histogram:\n" << endl;   // RNGDBF.cpp:453, an empty line after the header
    print_histogram(phase_hist);
#endif

    std::ofstream of(logfilename.c_str(), std::ios::app);   // :425-452
    const char tab = '\t';
    of << SNR << tab << (double)errors / totalBits << tab << (double)totalIterations / totalWords << tab
       << (double)wordErrors / totalWords << tab << totalBits << tab << totalWords << tab << T << tab << theta << tab;
#if defined(addNoise) || defined(quantizeProbabilities)
    of << cfg.noise_scale << tab;
#endif
#ifdef quantizeSamples
    of << cfg.nq << tab;
#endif
#ifdef thresholdAdaptation
    of << cfg.lambda << tab;
#endif
#ifdef weightSyndromes
    of << cfg.alpha << tab;
#endif
#ifdef outputSmoothing
    of << smoothingUsed << tab << (double)smoothingUsed / totalWords << tab;
    of << cfg.windowsize << tab;
#endif
#ifdef saturateSamples
    of << cfg.ymax << tab;
#endif
#ifdef redecode
    of << maxphase << tab;
#endif
    of << argv[1] << endl;
    of.close();

    ldpc_ctx_destroy(ctx);
    ldpc_graph_destroy(H);
    return 0;
}
