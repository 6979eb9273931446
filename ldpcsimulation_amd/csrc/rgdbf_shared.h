// rgdbf_shared.h -- the per-bit syndrome weight of src/RNGDBF.cpp (:564-567) and the state
// layouts of one codeword, shared by the re-decoding NGDBF kernels (rgdbf.hip) and the
// every-attempt kernels (rstat.hip; src/newstat.cpp and src/replayGDBF.cpp have the same
// symNodeUpdates). Moving them here changed no register, scratch or occupancy figure of the
// rgdbf.hip kernels (profiles/rstat_shared_header_resources.md).
#pragma once
#include "gdbf.h"

#include <hip/hip_runtime.h>

namespace ldpc {

// w_i of a bit of degree deg (:564-567): alpha*Ymax (a.w, the host's double product)
// divided by dv in double, then rounded to F. A bit without checks adds no term.
template <typename F>
__device__ __forceinline__ F rgdbf_weight(const GdbfArgs &a, int deg)
{
    if (!(a.flags & GDBF_WEIGHT)) return F(1);
    return deg > 0 ? (F)(a.w / (double)deg) : F(0);
}

// w * s_j for the parity bit p of check j (1: s_j = -1): the sign bit of w flipped by p,
// which is what the multiply by +-1 gives, bit for bit.
__device__ __forceinline__ float rgdbf_term(float w, uint32_t p)
{
    return __uint_as_float(__float_as_uint(w) ^ (p << 31));
}
__device__ __forceinline__ double rgdbf_term(double w, uint32_t p)
{
    return __hiloint2double((int)((uint32_t)__double2hiint(w) ^ (p << 31)), __double2loint(w));
}

constexpr int kRgdbfWtab = 64;   // weights by degree kept in LDS; larger degrees divide in place

template <typename F>
__device__ __forceinline__ void rgdbf_fill_wtab(const GdbfArgs &a, F *wtab)
{
    for (int k = threadIdx.x; k < kRgdbfWtab; k += blockDim.x) wtab[k] = rgdbf_weight<F>(a, k);
    __syncthreads();
}

// Byte offsets of one codeword's state: yq[N] | theta[N] | dsum[N] (int16) | d[N] | r[N] | s[M].
struct RgdbfLayout {
    size_t theta, dsum, d, r, s, total;
};
static inline RgdbfLayout rgdbf_layout(int N, int M, size_t fsz)
{
    RgdbfLayout L;
    auto al = [](size_t x) { return (x + 15) & ~(size_t)15; };
    L.theta = al(fsz * N);
    L.dsum = L.theta + al(fsz * N);
    L.d = L.dsum + al(2 * (size_t)N);
    L.r = L.d + al((size_t)N);
    L.s = L.r + al((size_t)N);
    L.total = L.s + al((size_t)M);
    return L;
}

// LDS of the register-schedule kernels (rgdbf_rows, rstat_rows): the d < 0 flag bytes, the
// parity bytes and the double-buffered early-stop flag.
struct RgdbfRowsLayout {
    int np, poff, floff, total;
};
static inline RgdbfRowsLayout rgdbf_rows_layout(int N, int M)
{
    RgdbfRowsLayout L;
    L.np = ((N + 3) & ~3) + 4;                 // d < 0 flags [0..N) + pad; the last word: dummy bits (0)
    L.poff = (L.np + 7) & ~7;
    L.floff = L.poff + ((M + 1 + 7) & ~7);     // parity bytes [0..M), [M]: the dummy check
    L.total = L.floff + 16;                    // flags[2] (+ pad)
    return L;
}

// The codes the register-schedule kernels take: those gdbf_rows takes.
inline bool rgdbf_rows_fits(int N, int M, int maxdv, int maxdc)
{
    return N >= 1 && N <= 4 * 1024 && M <= 2 * 1024 && maxdc <= 8 && maxdv <= 12;
}

}  // namespace ldpc
