// fxms.h -- internal launch interface of the fixed-point min-sum kernels (fxms.hip):
// min-sum whose messages are msg_bits-wide saturating integers (no reference
// program computes this, its anchor is fp64 min-sum on samples that sit on the quantiser grid).
#pragma once
#include "fxms_layout.h"
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

// fxms_plan of fxms_layout.h on the device graph. E: the graph's edges.
FxmsChoice fxms_choose(const DevGraph &g, int E, int msg_bits);
hipError_t fxms_launch(const DevGraph &g, const FxmsArgs &a, bool f64, const FxmsChoice &ch, int E, int num_cus,
                       hipStream_t s);

}  // namespace ldpc
