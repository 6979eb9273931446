// bp.h -- internal launch interface of the belief-propagation kernels (bp.hip).
#pragma once
#include "kernels.h"

namespace ldpc {

constexpr int kBpMaxDc = 32;   // row degree bound of the BP check node (per-thread tanh array)

// "bp_rows" (graph in registers, persistent; N <= 4096, row degree <= 8),
// "bp_lds" (state in LDS) or "bp_global" (a global slot per resident block).
// in.E: the code's edge count; in.num_cus sizes the persistent grids.
void plan_bp(const PlanInput &in, LaunchPlan &p);
// ldpc_bp_math_probe: tanh and log of bp_math.h over n device values (verification)
hipError_t bp_math_probe(const double *x, double *t, double *l, int n, hipStream_t s);
// checked builds (LDPC_CHECK): one out-of-range index on purpose (ldpc_check_selftest)
hipError_t check_selftest_launch(hipStream_t s);
// ticket: a word of the context that bp_rows hands codewords out by when a.early_stop is set
// (the launch clears it)
hipError_t launch_bp(const LaunchPlan &p, const DevGraph &g, const DecodeArgs &a, bool f64, int E, void *gscratch,
                     unsigned *ticket, hipStream_t s);

}  // namespace ldpc
