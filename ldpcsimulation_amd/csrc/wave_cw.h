// wave_cw.h -- the skeleton of a decoder whose wavefronts each own a codeword (hwgdbf.hip,
// fxms.hip, fxlms.hip): up to 16 codewords per workgroup, no workgroup barrier
// after staging, persistent waves that take codewords by ticket. A lane owns nodes lane,
// lane + 64, ...; the wave's LDS operations execute in issue order, so a wavefront-scope fence
// (which stops the compiler from moving them) orders a phase's writes before the next reads.
#pragma once
#include "kernels.h"
#include "wave_cw_plan.h"

#include <hip/hip_runtime.h>

namespace ldpc {

static_assert(kWaveCwLds == kMaxLds, "wave_cw_plan.h plans for the LDS a workgroup may use");

__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ int wave_sum(int x)   // in every lane
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}
__device__ __forceinline__ bool wave_any(int x) { return __builtin_amdgcn_ballot_w64(x != 0) != 0; }

// Codewords: the grid's own first, then tickets; the drawing thread (lane 0 of the wave) draws
// the next ticket while the current codeword decodes. `upb`: codewords in flight per workgroup.
struct CwTickets {
    unsigned *ticket;
    int batch, upb;
    bool drawer;
    unsigned nxt = 0;
    __device__ __forceinline__ CwTickets(unsigned *t, int n, int u, bool d) : ticket(t), batch(n), upb(u), drawer(d) { draw(); }
    __device__ __forceinline__ void draw() { if (drawer) nxt = gridDim.x * upb + atomicAdd(ticket, 1u); }
    // The first codeword of the workgroup's slot `slot` (the wave).
    __device__ __forceinline__ int first(int slot) const { return (int)blockIdx.x * upb + slot; }
    // Ends a codeword (the next one's front end rewrites its state) and gives the wave its next.
    __device__ __forceinline__ int next()
    {
        wave_sync();
        return redraw((int)__shfl((int)nxt, 0, 64));
    }
    __device__ __forceinline__ int redraw(int b)
    {
        if (b < batch) draw();
        return b;
    }
};

// One launch of a wave-per-codeword kernel at the shape `ch`: the grid is what the CUs hold,
// no more than the batch needs; the tickets start at 0. pick(f, src) gives the instance
// void (*)(Args, KArgs...) for the precision and sample source tags of for_f_src.
template <typename Args, typename Pick, typename... KArgs>
static hipError_t wave_cw_launch(const Args &a, bool f64, const WaveCwChoice &ch, int num_cus, hipStream_t s, Pick pick,
                                 const KArgs &...rest)
{
    if (a.batch <= 0) return hipSuccess;
    if (!a.ticket || ch.cw_per_block < 1 || (size_t)ch.lds_bytes > kMaxLds) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(a.ticket, 0, sizeof(unsigned), s);
    if (e != hipSuccess) return e;
    return for_f_src(f64, a.src, [&](auto f, auto src) {
        void (*fn)(Args, KArgs...) = pick(f, src);
        int per_cu = occupancy(reinterpret_cast<const void *>(fn), ch.threads, ch.lds_bytes);   // raises the LDS limit
        if (per_cu < 1) per_cu = 1;
        int grid = per_cu * (num_cus > 0 ? num_cus : 1);
        const int need = (a.batch + ch.cw_per_block - 1) / ch.cw_per_block;
        if (grid > need) grid = need;
        hipLaunchKernelGGL(fn, dim3(grid), dim3(ch.threads), ch.lds_bytes, s, a, rest...);
        return hipGetLastError();
    });
}

}  // namespace ldpc
