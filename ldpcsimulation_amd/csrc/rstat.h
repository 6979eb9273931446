// rstat.h -- internal launch interface of the every-attempt NGDBF kernels (rstat.hip;
// src/newstat.cpp = redecodeStatistics and src/replayGDBF.cpp of the reference).
#pragma once
#include "gdbf.h"

namespace ldpc {

// GdbfArgs with the attempt loop of src/newstat.cpp (:305-429): every frame is decoded
// `attempts` times from the same channel samples, each attempt one single-phase decode of
// rgdbf.hip (d = r, theta_i = theta, dsum = 0 at its start) with perturbations of its own,
// and every attempt runs whether or not an earlier one succeeded. flags is a subset of
// NOISE | ADAPT | WEIGHT | SMOOTH | SATURATE; `w` is alpha * Ymax. Attempt indices are
// absolute: local attempt ai is attempt first_attempt + ai. pert is
// [batch][attempts][T][N]; with SRC_PHILOX attempt `at` of frame f draws the rows that
// phase 0 of frame f + (at << 32) draws in rgdbf.hip, the channel stays frame f's own.
struct RstatArgs : GdbfArgs {
    int attempts, first_attempt;
    int4 *attempt_res;              // [batch][attempts] {bit_err, iters, syndrome_fail, smoothing_used}
    int *frame_unc;                 // [batch] uncoded bit errors of the frame (written with its last attempt)
    void *y_out;                    // SRC_PHILOX: the channel samples drawn, [batch][N] (F), or null
    void *pert_out;                 // SRC_PHILOX: the rows drawn, [batch][attempts][T][N] (F), or null
    // traces (a launch with a trace goes to rstat_wg), each [batch][attempts][T] rows, any of
    // them null; rows of iterations that did not run keep what the caller put there
    int32_t *err_trace, *unsat_trace;
    int8_t *d_trace, *s_trace;      // [..][N] / [..][M], +-1
};

using RstatChoice = GdbfChoice;     // "rstat_rows" | "rstat_wg" (in LDS, or in a global slot: slot_bytes > 0)

// rstat_rows on the codes rgdbf_rows takes when no trace is wanted (maxdv / maxdc: the code's
// largest column / row degree); option LDPC_OPT_GDBF_KERNEL = 1 forces rstat_wg.
RstatChoice rstat_choose(const DevGraph &g, bool f64, bool trace, int maxdv, int maxdc);
// scratch: slots * choice.slot_bytes bytes for the global-slot instance of rstat_wg; num_cus
// sizes the persistent grid of rstat_rows.
// Queues the attempt kernel and the frame accounting (newstat.cpp:421-465) behind it.
hipError_t rstat_launch(const DevGraph &g, const RstatArgs &a, bool f64, const RstatChoice &ch, void *scratch,
                        int slots, int num_cus, hipStream_t s);

}  // namespace ldpc
