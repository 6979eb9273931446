// hwgdbf.h -- internal launch interface of the fixed-point NGDBF hardware-model kernels
// (hwgdbf.hip; src/NGDBFhw.cpp of the reference).
#pragma once
#include "hwgdbf_layout.h"
#include "kernels.h"

namespace ldpc {

// The front end runs in the cfg's precision F on the doubles below (each rounded to F once);
// the decoder itself is integer. lmax, smult and theta are derived on the host in double
// (NGDBFhw.cpp:174-179). The qlen noise normals of the fused path are Philox4x32-10 at
// counter (k / 4, frame, stream_id | 1 << 20) under the seed, through box_muller_hw: the
// key of the GDBF kernels' first perturbation row.
struct HwgdbfArgs {
    int batch, T, maxphase, nq, qlen, src;
    int smult, theta;               // round(NL / lmax); unpack(pack(quantize(2.0), +1))
    double two_w, ymax, lmax, theta0, sigma, noise_sigma;
    const void *y;                  // SRC_GIVEN: raw channel samples [batch][N] (F)
    const void *q;                  // SRC_GIVEN: raw noiseSigma * n draws [batch][qlen] (F)
    const int32_t *qptr0;           // SRC_GIVEN: start pointers [batch] or null (0); SRC_PHILOX: 0
    const int8_t *c;                // SRC_GIVEN: bipolar codewords [batch][N] or null (+1)
    const int8_t *cw_table;         // SRC_PHILOX: codeword table [cw_rows][N] or null
    int cw_rows;
    uint64_t seed, first_cw;
    uint32_t stream_id;
    void *y_out, *q_out;            // SRC_PHILOX: the samples drawn, [batch][N] / [batch][qlen] (F), or null
    int8_t *d_out;                  // [batch][N] bipolar, the last phase's, or null
    int4 *frame_res;                // [batch] {leastErrors, uncoded, last phase unsatisfied, leastIterations} or null
    int32_t *iters_run;             // [batch] sum of `it` over the phases, or null
    unsigned long long *counts;     // [6] accumulated (iters = sum of leastIterations)
    unsigned long long *hist;       // [N] error-weight histogram
    unsigned *ticket;               // codewords past the first grid's are handed out by this counter
};

// hwgdbf_plan of hwgdbf_layout.h on the device graph: the shape that keeps more waves on a CU;
// option LDPC_OPT_GDBF_KERNEL = 1 forces the workgroup-per-codeword instance.
// E: the graph's edges.
HwgdbfChoice hwgdbf_choose(const DevGraph &g, int E, int qlen);
hipError_t hwgdbf_launch(const DevGraph &g, const HwgdbfArgs &a, bool f64, const HwgdbfChoice &ch, int E, int num_cus,
                         hipStream_t s);

}  // namespace ldpc
