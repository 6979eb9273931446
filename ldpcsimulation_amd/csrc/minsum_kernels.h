// minsum_kernels.h -- device helpers and A/B switch defaults shared by the kernel files
// split along the kernel families (kernels.hip, rows.hip, flood.hip, layered.hip).
#pragma once
#include "kernels.h"
#include "device_common.h"
#include "minsum_common.h"

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <type_traits>

namespace ldpc {

// x / alpha for the check-node normalisation (:498). fp32 with a verified
// alpha: reciprocal + one FMA correction (3 VALU instead of ~10); otherwise,
// and for non-finite minima, the IEEE division.
template <typename F>
__device__ __forceinline__ F nms_div(F x, F alpha, const DecodeArgs &a)
{
    return x / alpha;
}
template <>
__device__ __forceinline__ float nms_div<float>(float x, float alpha, const DecodeArgs &a)
{
    if (a.nms_fast && x < __builtin_huge_valf()) {
        const float q = x * a.alpha_rcp;
        return __builtin_fmaf(__builtin_fmaf(-q, alpha, x), a.alpha_rcp, q);
    }
    return x / alpha;
}

// (m1, m2) of the packed check state of the flood and layered kernels.
template <typename F> struct F2T;
template <> struct F2T<float> { using T = float2; };
template <> struct F2T<double> { using T = double2; };

// Progress-ordered wave priorities in k_decode_rows' check phase: s_setprio 3 at the
// phase start, 2 after the first row, 0 for the bit phase (fp32 OMS on N=1944, T=50:
// 13.2 -> 11.6 ms; PEG 1008 fp32 MS T=10 +3 %). 0: none.
// A/B switches of the row kernel's per-step work: block sums with one barrier into LDS
// totals (block_sum_lds, 1) vs block_sum_n_t0 (0); Philox products by v_mad_u64_u32.
// Measured (fp32, 65 536 codewords): block_sum_lds makes PEG 1008 MS T=10 39.6 -> 42.3
// Gbit/s but N=1944 OMS T=50 11.0 -> 10.1 (the same instance; a code-layout effect, not
// the reduction's own cost), so the default stays 0; v_mad_u64_u32 is neutral and kept.
#ifndef LDPC_ROWS_ACCT
#define LDPC_ROWS_ACCT 0
#endif
#ifndef LDPC_ROWS_MAD64
#define LDPC_ROWS_MAD64 1
#endif
#ifndef LDPC_ROWS_PRIOBAL
#define LDPC_ROWS_PRIOBAL 1
#endif
#ifndef LDPC_FLOOD_CPW
#define LDPC_FLOOD_CPW 8
#endif
#ifndef LDPC_FLOOD_XCD
#define LDPC_FLOOD_XCD 1
#endif

}  // namespace ldpc
