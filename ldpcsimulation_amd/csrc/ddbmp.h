// ddbmp.h -- internal launch interface of the DD-BMP kernels (ddbmp.hip): differential
// decoding with binary message passing, variant LDPC_DDBMP of ldpc_decoder_cfg.
#pragma once
#include "kernels.h"

namespace ldpc {

// "ddbmp_rows" (memories in registers, persistent grid with a codeword ticket; N <= 4096,
// row degree <= 8, column degree <= 4, or <= 12 with N <= 2048), "ddbmp_lds" (state in LDS)
// or "ddbmp_global" (a global slot per resident block). in.E: the code's edge count;
// in.maxdv: its largest column degree; in.num_cus sizes the persistent grids.
// LDPC_OPT_DDBMP_KERNEL = 1 forces the generic kernels (tests compare the two).
void plan_ddbmp(const PlanInput &in, LaunchPlan &p);
// ticket: the codeword counter of ddbmp_rows (the launch zeroes it): early stop makes the
// codewords unequal, so those past the first grid's are handed out one by one.
hipError_t launch_ddbmp(const LaunchPlan &p, const DevGraph &g, const DecodeArgs &a, bool f64, int E, void *gscratch,
                        unsigned *ticket, hipStream_t s);

}  // namespace ldpc
