// fxlms.h -- internal launch interface of the layered fixed-point min-sum kernels (fxlms.hip: a
// wavefront per codeword, its state in LDS; fxlms_wg.hip: a workgroup per codeword, the APPs in
// LDS and the row state in a global slot, for codes beyond the first's 64 KiB):
// row-layered MS / NMS / OMS with a saturating app_bits-wide posterior per bit and a
// msg_bits-wide message per edge (include/ldpc_hip.h ldpc_fxlms_cfg has the
// definition; no reference program computes this, its anchor is the fp64 layered decoder on
// samples that sit on the quantiser grid).
#pragma once
#include "fxlms_layout.h"
#include "fxms.h"

namespace ldpc {

// The fixed-point min-sum arguments (front end, check-node rule, accounting) and the APP clamp.
struct FxlmsArgs : FxmsArgs {
    int amax;                       // A = 2^(app_bits - 1) - 1
};

// Device copy of the layered row order the kernel walks (graph.h LayerSchedule: the order of
// ldpc_graph_layers), as the kernel reads it: row n is the check at layered position n.
struct FxlmsSched {
    int N = 0, M = 0, dcs = 0, nlayers = 0;
    const int32_t *lptr = nullptr;  // [nlayers + 1] layered positions of each layer
    const int32_t *cols = nullptr;  // [dcs * M] slot-major: bit of edge k of row n at k * M + n (pads: the row's last bit)
    const uint8_t *deg = nullptr;   // [M]
};

// fxlms_plan of fxlms_layout.h on the schedule's sizes.
FxlmsChoice fxlms_choose(const FxlmsSched &sc, int app_bits);
hipError_t fxlms_launch(const FxlmsSched &sc, const FxlmsArgs &a, bool f64, const FxlmsChoice &ch, int num_cus,
                        hipStream_t s);

// fxlms_wg.hip. fxlms_wg_plan of fxlms_layout.h on the schedule's sizes; the workgroups of a
// launch (what the CUs hold, no more than the batch), each of which needs ch.slot_bytes of
// `scratch`; and the launch over `grid` workgroups.
FxlmsChoice fxlms_wg_choose(const FxlmsSched &sc, int app_bits);
int fxlms_wg_grid(const FxlmsArgs &a, bool f64, const FxlmsChoice &ch, int num_cus);
hipError_t fxlms_wg_launch(const FxlmsSched &sc, const FxlmsArgs &a, bool f64, const FxlmsChoice &ch, void *scratch, int grid,
                           hipStream_t s);

}  // namespace ldpc
