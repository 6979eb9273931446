// gdbf_front.h -- the sample front-end the GDBF kernels (gdbf.hip) and the re-decoding
// NGDBF kernels (rgdbf.hip) share: decodeGDBF.cpp:254-267 and RNGDBF.cpp:252-275 are the
// same arithmetic.
#pragma once
#include "gdbf.h"

#include <hip/hip_runtime.h>

namespace ldpc {

template <typename F> __device__ __forceinline__ F gabs(F x) { return x < F(0) ? -x : x; }
__device__ __forceinline__ float gfloor(float x) { return __builtin_floorf(x); }
__device__ __forceinline__ double gfloor(double x) { return __builtin_floor(x); }

// Front-end of one sample (:254-267): saturation, hard decision r, quantize()
// (:488-493, whose sgn is y > 0 ? 1 : -1).
template <typename F>
__device__ __forceinline__ F gdbf_front(F y, const GdbfArgs &a, int &r)
{
    F yq = y;
    const F ymax = (F)a.ymax;
    if (a.flags & GDBF_SATURATE)
        if (gabs(yq) > ymax) yq *= ymax / gabs(yq);
    r = yq > F(0) ? 1 : -1;
    if (a.flags & GDBF_QUANTIZE) {
        const F qmax = (F)a.qmax, lmax = ymax / F(2);
        const F s = yq > F(0) ? F(1) : F(-1);
        yq = s * gfloor((gabs(yq) * qmax) / (F(2) * lmax) + F(0.5)) * (F(2) * lmax / qmax);
    }
    return yq;
}

}  // namespace ldpc
