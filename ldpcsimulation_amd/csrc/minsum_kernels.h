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

// Check node of the row kernels (rows.hip, rows_es.hip), exact path: the reference's comparisons for any input, incl.
// infinities and NaN (checkNodeUpdates :410-450, applyNormalization :494-499,
// applyOffset :503-515). pv[k].v[c]: in = c2v sent last iteration, out = new c2v.
template <typename F, int C, int DC, typename MT>
__device__ __forceinline__ void cn_exact(const Pack<F, C> (&xin)[DC], int c, Pack<F, C> (&pv)[DC], MT degmask,
                                         const DecodeArgs &a, F alpha, F delta)
{
    F ax[DC];
    F mn1 = dinf<F>(), mn2 = dinf<F>();
    MT sg = 0;
#pragma unroll
    for (int k = 0; k < DC; ++k) {
        const F x = xin[k].v[c] - pv[k].v[c];                       // v2c (:469)
        sg |= (MT)(!(x >= F(0))) << k;                              // sgn(v2c) (:518-523)
        ax[k] = dabs(x);
        // :428-437 -- if (|x| <= m1) {m2 = m1; m1 = |x|} else if (|x| < m2) m2 = |x|
        // (NaN: no comparison holds and fmin returns the other operand).
        const bool le = ax[k] <= mn1;
        mn2 = dmin(mn2, le ? mn1 : ax[k]);
        mn1 = le ? ax[k] : mn1;
    }
    sg &= degmask;
    const MT eff = (__popcll((unsigned long long)sg) & 1) ? (sg ^ degmask) : sg;   // prod*sgn(v2c_k)
    // The argmin edge gets m2, every other edge m1 (:444-447). |x_k| == m1
    // identifies it: on a tie m2 == m1, so which tied edge is "argmin" does not matter.
    if (a.variant != V_OMS) {
        F M1 = mn1, M2 = mn2;
        if (a.variant == V_NMS) {
            M1 = nms_div<F>(mn1, alpha, a);
            M2 = nms_div<F>(mn2, alpha, a);
        }
#pragma unroll
        for (int k = 0; k < DC; ++k) {
            const F mag = (ax[k] == mn1) ? M2 : M1;
            pv[k].v[c] = ((eff >> k) & 1u) ? -mag : mag;
        }
    } else {
        const F t1 = mn1 - delta, t2 = mn2 - delta;
        const bool p1 = t1 > F(0), p2 = t2 > F(0);
        const F M1 = p1 ? t1 : F(0), M2 = p2 ? t2 : F(0);
        // sgn(c2v) maps -0.0 to +1 and a zeroed message is +0
        const MT e1 = (!p1 || mn1 == F(0)) ? (MT)0 : eff;
        const MT e2 = (!p2 || mn2 == F(0)) ? (MT)0 : eff;
#pragma unroll
        for (int k = 0; k < DC; ++k) {
            const bool ism = ax[k] == mn1;
            const F mag = ism ? M2 : M1;
            pv[k].v[c] = (((ism ? e2 : e1) >> k) & 1u) ? -mag : mag;
        }
    }
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
