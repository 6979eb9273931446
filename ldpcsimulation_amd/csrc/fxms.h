// fxms.h -- internal launch interface of the fixed-point min-sum kernels (fxms.hip):
// min-sum whose messages are msg_bits-wide saturating integers (no reference
// program computes this, its anchor is fp64 min-sum on samples that sit on the quantiser grid).
#pragma once
#include "kernels.h"

namespace ldpc {

// The front end runs in the cfg's precision F on ymax (rounded to F once); everything after
// it is integer.
struct FxmsArgs {
    int batch, T, variant, src;     // variant: V_MS / V_NMS / V_OMS of minsum_common.h
    int nq1;                        // Nq - 1 = 2^qbits - 1, the largest |Y|
    int vmax;                       // V = 2^(msg_bits - 1) - 1, the message clamp
    int nms_num, nms_shift, beta, early_stop;
    double ymax, sigma;
    const void *y;                  // SRC_GIVEN: raw channel samples [batch][N] (F)
    const int8_t *c;                // SRC_GIVEN: bipolar codewords [batch][N] or null (+1)
    const int8_t *cw_table;         // SRC_PHILOX: codeword table [cw_rows][N] or null
    int cw_rows;
    uint64_t seed, first_cw;
    uint32_t stream_id;
    void *y_out;                    // SRC_PHILOX: the samples drawn [batch][N] (F), or null
    int8_t *ycode_out;              // the integer codes Y [batch][N], or null
    int8_t *d_out;                  // [batch][N] bipolar, or null
    int4 *frame_res;                // [batch] {bit_err, uncoded, syndrome_fail, early_stop ? s : 0} or null
    unsigned long long *counts;     // [6] accumulated (iters: early_stop ? s : T per frame)
    unsigned long long *hist;       // [N] error-weight histogram
    unsigned *ticket;               // codewords past the first grid's are handed out by this counter
};

struct FxmsChoice {
    const char *name = "";          // "fxms_i8" | "fxms_i16"; empty: the state does not fit
    int lds_bytes = 0;              // dynamic LDS of a workgroup
    int cw_bytes = 0;               // state bytes of one codeword
    int threads = 0, cw_per_block = 0;
    bool wide = false;              // int16 messages (msg_bits > 8)
    bool staged = false;            // the graph sits in LDS beside the codewords (lds_bytes includes it)
};

constexpr int kFxmsMaxLds = 64 * 1024;   // one codeword's state must fit (the hwgdbf bound)

// E: the graph's edges.
FxmsChoice fxms_choose(const DevGraph &g, int E, int msg_bits);
hipError_t fxms_launch(const DevGraph &g, const FxmsArgs &a, bool f64, const FxmsChoice &ch, int E, int num_cus,
                       hipStream_t s);

}  // namespace ldpc
