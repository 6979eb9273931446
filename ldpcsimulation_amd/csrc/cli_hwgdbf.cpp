// cli_hwgdbf.cpp -- NGDBFhw: the reference's fixed-point NGDBF hardware model
// (C_implementations/src/NGDBFhw.cpp:97-511, scripts/demo_NGDBFhw_802_3.sh) on the GPU.
//
//   NGDBFhw alist SNR numFrames seed logfilename
//
// Identical positional arguments, stdout (parameter echo :499-510, :123, :136-137; "Ferr
// with k errors." and " BER=..., WER=..." per frame error :381-392; the incremental block
// every 100 frames :426-433; the final line :444-447), appended log line (:449-459) and
// <logfilename>_<SNR>_itdist.dat (:420-421, :464-469). The decoder's constants are the
// reference's compile-time ones (:48-57); R = 0.8413 whatever the code (:49). The seed is
// the argument. The reference's uncodedErrors is never counted for the all-zero word
// (r * c with c = 0, :230), so "Uncoded errors = 0" is printed as it prints it.
//
// The optional sixth argument (a codeword file) is not built: the reference streams
// argv[argc], a null pointer, into cout (:119), which silences all its later output, and
// never reads the file. This program prints the reference's text up to that point and
// fails with a message on stderr.
//
// Environment (the positional CLI stays identical):
//   LDPC_RNG       glibc (default): the reference's noise -- glibc random() TYPE_3 seeded
//                  like ran_seed(seed) and rand.h rann(), drawn on the host in the
//                  reference's order (N channel normals, then qlen noise normals per
//                  frame); frames are decoded one at a time with the fp64 front end and
//                  the noise pointer is carried from frame to frame on the host, so the
//                  output equals the reference's.
//                  philox: channel and noise generated on the GPU, LDPC_BATCH frames per
//                  launch; every frame starts at pointer 0.
//   LDPC_PRECISION, LDPC_BATCH, LDPC_DEVICE, LDPC_DRY_RUN as cli_minsum.cpp.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
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

void print_histogram(const std::vector<int> &h)   // printHistogram (:521-528)
{
    for (size_t i = 0; i < h.size(); ++i)
        if (h[i] > 0) cout << i + 1 << ":\t" << h[i] << endl;
}

}  // namespace

int main(int argc, char *argv[])
{
    if (argc != 6 && argc != 7) {   // :103-110
        cout << "Usage: " << argv[0] << " alist SNR numFrames seed logfilename [codeword filename]\n";
        return 0;
    }
    // The reference's constants (:48-57).
    const int num_iterations = 600, maxPhases = 1, NQ = 5, qlen = 2648;
    const double R = 0.8413, w = 0.185, Ymax = 1.625, noiseScale = 0.95, theta0 = -0.525;

    // ---- parseArguments (:494-511) ----
    ldpc_graph *H = nullptr;
    if (ldpc_graph_load_alist(argv[1], &H) != LDPC_OK) die("loading alist");
    cout << "PARAMETERS: \n alist = \t" << argv[1] << endl;
    const double SNR = std::atof(argv[2]);
    cout << " SNR = \t" << SNR << endl;
    const long numFrames = std::atoi(argv[3]);
    cout << "Simulating for " << numFrames << " frames." << endl;
    const long seed = std::atoi(argv[4]);
    cout << "Using random seed " << seed << endl;
    const std::string logfilename = argv[5];
    cout << " log = \t" << logfilename << endl;

    if (argc == 7) {   // :117-121
        cout << "\nUsing codewords from " << std::flush;
        std::cerr << "ldpc: NGDBFhw: the codeword file argument is not supported (the reference never reads it)" << endl;
        return 2;
    }
    cout << "\nUsing all-zero sequence.\n";

    int N = 0, M = 0, E = 0, gdv = 0, gdc = 0, dv = 0, dc = 0;
    if (ldpc_graph_info(H, &N, &M, &E, &gdv, &gdc) != LDPC_OK) die("graph info");
    alist_header(argv[1], dv, dc);   // biggest_num_n / biggest_num_m as the file declares them
    const double N0 = std::pow(10.0, -SNR / 10.0) / R;   // :127-129
    const double sigma = std::sqrt(N0 / 2.0);
    const double noiseSigma = sigma * noiseScale;
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
    ldpc_hwgdbf_cfg cfg;
    std::memset(&cfg, 0, sizeof cfg);
    const std::string prec = env_or("LDPC_PRECISION", "f64");   // the reference's double; f32 opt-in
    cfg.precision = prec == "f32" ? LDPC_F32 : LDPC_F64;
    cfg.T = num_iterations;
    cfg.maxphase = maxPhases;
    cfg.nq = NQ;
    cfg.qlen = qlen;
    cfg.w = w;
    cfg.ymax = Ymax;
    cfg.noise_scale = noiseScale;
    cfg.theta0 = theta0;
    int batch = philox ? std::atoi(env_or("LDPC_BATCH", "65536")) : 1;
    const int device = std::atoi(env_or("LDPC_DEVICE", "0"));
    if (batch <= 0) {
        std::cerr << "ldpc: LDPC_BATCH must be > 0" << endl;
        return 1;
    }
    if (philox && numFrames > 0 && batch > numFrames) batch = (int)numFrames;
    if (std::getenv("LDPC_DRY_RUN")) {   // report the GPU settings and stop before any device call
        std::cerr << "ldpc: rng=" << rng << " precision=" << (cfg.precision == LDPC_F64 ? "f64" : "f32")
                  << " batch=" << batch << " device=" << device << endl;
        return 0;
    }
    if (N >= qlen) {   // the reference reads qprime out of bounds there (:583)
        std::cerr << "ldpc: NGDBFhw needs N < " << qlen << " (the noise register's length)" << endl;
        return 1;
    }
    ldpc_ctx *ctx = nullptr;
    if (ldpc_ctx_create(device, H, batch, &ctx) != LDPC_OK) die("creating device context");
    // one frame per launch: the workgroup-per-codeword instance has the shorter latency
    if (!philox && ldpc_ctx_set_option(ctx, LDPC_OPT_GDBF_KERNEL, 1) != LDPC_OK) die("setting the kernel option");

    long errors = 0, uncodedErrors = 0, totalBits = 0, totalWords = 0, wordErrors = 0, totalIterations = 0;
    std::vector<int> hist(N, 0);
    std::vector<double> itdist(num_iterations + 1, 0.0);   // the reference writes [T] of a T-vector at it = T (:420)
    std::vector<ldpc_frame_result> res(batch);
    GlibcRandom g((uint32_t)seed);   // ran_seed(seed) (:114)
    std::vector<double> y(philox ? 0 : N), q(philox ? 0 : qlen);
    std::vector<float> yf(philox || cfg.precision == LDPC_F64 ? 0 : N), qf(philox || cfg.precision == LDPC_F64 ? 0 : qlen);
    int32_t qpointer = 0;
    while (totalWords < numFrames) {
        const int nb = (int)std::min<long>(batch, numFrames - totalWords);
        if (philox) {
            ldpc_counts tmp{};
            if (ldpc_hwgdbf_sim_batch(ctx, SNR, R, &cfg, (uint64_t)seed, 0u, (uint64_t)totalWords, nb, res.data(), &tmp) !=
                LDPC_OK)
                die("simulating batch");
        } else {
            for (int i = 0; i < N; ++i) y[i] = 1.0 * (1.0 + sigma * g.rann());       // :220
            for (int k = 0; k < qlen; ++k) q[k] = noiseSigma * g.rann();              // :241
            const void *yp = y.data(), *qp = q.data();
            if (cfg.precision == LDPC_F32) {
                for (int i = 0; i < N; ++i) yf[i] = (float)y[i];
                for (int k = 0; k < qlen; ++k) qf[k] = (float)q[k];
                yp = yf.data();
                qp = qf.data();
            }
            int32_t run = 0;
            if (ldpc_hwgdbf_decode_batch(ctx, yp, qp, &qpointer, 1, &cfg, nullptr, nullptr, res.data(), &run, nullptr) !=
                LDPC_OK)
                die("decoding frame");
            qpointer = (int32_t)(((long)qpointer + run) % (qlen - N));   // :356-358, once per iteration run
        }
        for (int f = 0; f < nb; ++f) {
            const int leastErrors = res[f].bit_err, leastIterations = res[f].iters;
            if (leastErrors > 0) {   // :378-392
                cout << "Ferr with " << leastErrors << " errors.";
                if (!res[f].syndrome_fail)
                    cout << " All checks satisfied.\n";
                else
                    cout << endl;
                errors += leastErrors;
                hist[leastErrors - 1]++;
                wordErrors++;
                cout << " BER=" << (double)errors / (totalBits + N) << ", WER=" << (double)wordErrors / (totalWords + 1)
                     << endl;
            }
            totalWords++;
            totalBits += N;
            totalIterations += leastIterations;
            for (int idx = 0; idx <= leastIterations; idx++)   // :420-421
                itdist[idx] = (double)((totalWords - 1.0) / totalWords) * itdist[idx] + (double)(1.0 / totalWords);
            if ((totalWords % 100) == 0) {   // :426-433
                cout << "\nIncremental result: " << errors << " bit errs in " << totalWords
                     << " words, BER=" << (double)errors / totalBits
                     << ". Average iterations = " << (double)totalIterations / totalWords << ". Word error=" << wordErrors
                     << ". Uncoded errors = " << uncodedErrors << ", uncBER=" << (double)uncodedErrors / totalBits
                     << "\nError weights:\n";
                print_histogram(hist);
            }
        }
    }

    cout << "\nFinal result: " << errors << " bit errs in " << totalWords << " words, BER=" << (double)errors / totalBits
         << ". Average iterations = " << (double)totalIterations / totalWords << ". Uncoded errors = " << uncodedErrors
         << ", uncBER=" << (double)uncodedErrors / totalBits << endl;

    std::ofstream of(logfilename.c_str(), std::ios::app);   // :449-459
    const char tab = '\t';
    of << SNR << tab << errors << tab << wordErrors << tab << (double)errors / totalBits << tab
       << (double)totalIterations / totalWords << tab << (double)wordErrors / totalWords << tab << totalBits << tab
       << totalWords << tab << num_iterations << tab << theta0 << tab;
    of << noiseScale << tab;
    of << w << tab;
    of << Ymax << tab << NQ << tab;
    of << maxPhases << tab << seed;
    of << endl;

    std::stringstream ss;   // :464-469
    ss << logfilename << "_" << SNR << "_itdist.dat";
    std::ofstream ofitdist(ss.str().c_str(), std::ios::trunc);
    for (int idx = 0; idx < num_iterations; idx++) ofitdist << idx << "\t" << itdist[idx] << "\n";
    ofitdist.close();

    ldpc_ctx_destroy(ctx);
    ldpc_graph_destroy(H);
    return 0;
}
