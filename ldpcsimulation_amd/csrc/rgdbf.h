// rgdbf.h -- internal launch interface of the re-decoding NGDBF kernels (rgdbf.hip).
#pragma once
#include "gdbf.h"

namespace ldpc {

// GdbfArgs with the phase loop of src/RNGDBF.cpp (:277-400). flags is a subset of
// NOISE | ADAPT | WEIGHT | SMOOTH | SATURATE; pert is [batch][maxphase * T][N]; `w` is
// alpha * Ymax with GDBF_WEIGHT (bit i adds w / dv_i per check, :564-567), unused without.
struct RgdbfArgs : GdbfArgs {
    int maxphase;
};

constexpr int kRgdbfFlags = GDBF_NOISE | GDBF_ADAPT | GDBF_WEIGHT | GDBF_SMOOTH | GDBF_SATURATE;

using RgdbfChoice = GdbfChoice;     // "rgdbf_rows" | "rgdbf_lds" | "rgdbf_global"

// maxdv / maxdc: the code's largest column / row degree. Option LDPC_OPT_GDBF_KERNEL = 1
// forces the one-workgroup-per-codeword kernels here as it does for gdbf.hip.
RgdbfChoice rgdbf_choose(const DevGraph &g, bool f64, int maxdv, int maxdc);
// scratch: slots * choice.slot_bytes bytes for the global kernel (persistent grid of `slots`);
// num_cus sizes the persistent grid of rgdbf_rows.
hipError_t rgdbf_launch(const DevGraph &g, const RgdbfArgs &a, bool f64, const RgdbfChoice &ch, void *scratch,
                        int slots, int num_cus, hipStream_t s);

}  // namespace ldpc
