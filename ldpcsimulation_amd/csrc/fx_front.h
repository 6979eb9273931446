// fx_front.h -- what the fixed-point min-sum kernels (fxms.hip, fxlms.hip) share on the device:
// the integer front end and the wavefront-scope helpers of a wave that owns a codeword.
#pragma once
#include "minsum_common.h"

#include <hip/hip_runtime.h>

namespace ldpc {

__device__ __forceinline__ void fx_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ int fx_wave_sum(int x)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// The integer code of one sample.
template <typename F> __device__ __forceinline__ int fx_quant(F y, F ymax, int nq1)
{
    const F a = dabs(y);
    int mag = nq1;
    if (!(a > ymax)) {
        int k = (int)dfloor(a * (F)nq1 / (F(2) * ymax));
        k = max(min(k, nq1 >> 1), 1);   // every a <= ymax is below the upper bound: it only guards (int)floor(NaN)
        mag = 2 * k;
    }
    return y >= F(0) ? mag : -mag;
}

}  // namespace ldpc
