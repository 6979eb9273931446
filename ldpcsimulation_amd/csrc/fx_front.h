// fx_front.h -- what the fixed-point min-sum kernels (fxms.hip, fxlms.hip, fxlms_wg.hip) share on
// the device beyond the wave-per-codeword skeleton (wave_cw.h): the integer front end, the
// syndrome of the decisions and the frame's result; and fxlms's check-node rule over four edges.
// What a kernel stores and reads goes in as __forceinline__ lambdas, which also keep its LDPC_CHK
// ids. The loops take the codeword's thread `lane` of `stride`: a wavefront's 64 (the default,
// a constant after inlining) or, in fxlms_wg.hip, the workgroup's threads.
#pragma once
#include "frame.h"
#include "minsum_common.h"
#include "wave_cw.h"

namespace ldpc {

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

// Channel + front end of frame b over the codeword's threads: store(v, Y_v) once per bit; the
// codes go to a.ycode_out. Returns the thread's uncoded errors.
template <typename F, int SRC, typename Args, typename Store>
__device__ __forceinline__ int fx_front_end(const Args &a, int b, int N, int lane, const int8_t *cvec, Store &&store,
                                            int stride = 64)
{
    const F ymax = (F)a.ymax;
    int unc = 0;
    for (int g4 = lane; g4 * 4 < N; g4 += stride) {
        F yv[4];
        channel_group<F, SRC, true>(a, b, g4, N, cvec, a.y_out, yv);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int v = g4 * 4 + q;
            if (v < N) {
                const int yc = fx_quant<F>(yv[q], ymax, a.nq1);
                unc += (yc > 0 ? 0 : 1) != (cvec ? cvec[v] < 0 : 0);
                store(v, yc);
                if (a.ycode_out) a.ycode_out[(size_t)b * N + v] = (int8_t)yc;
            }
        }
    }
    return unc;
}

// Whether the decisions fail a check among the thread's rows lane, lane + stride, ...: row j has
// deg_of(j) edges, its k-th bit is bit_of(k, j), dec_of(i) is 1 where bit i decides -1. Four
// reads in flight; edges past the row read its last edge and count as 0.
template <typename Deg, typename Bit, typename Dec>
__device__ __forceinline__ int fx_syndrome_part(int M, int lane, int stride, Deg &&deg_of, Bit &&bit_of, Dec &&dec_of)
{
    int f = 0;
    for (int j = lane; j < M; j += stride) {
        const int deg = deg_of(j);
        uint32_t p = 0;
        for (int k0 = 0; k0 < deg; k0 += 4)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t dbit = dec_of(bit_of(min(k0 + q, deg - 1), j));
                p ^= k0 + q < deg ? dbit : 0u;
            }
        f |= (int)(p & 1u);
    }
    return f;
}
// ... among all rows, uniform over the wave that owns the codeword.
template <typename Deg, typename Bit, typename Dec>
__device__ __forceinline__ bool fx_syndrome_fails(int M, int lane, Deg &&deg_of, Bit &&bit_of, Dec &&dec_of)
{
    return wave_any(fx_syndrome_part(M, lane, 64, deg_of, bit_of, dec_of));
}

// The check-node rule of a row of deg edges: m1 <= m2 the two smallest magnitudes (V where the
// row has fewer), pos the edge at the minimum, neg the mask of the negative edges. k_fxlms
// uses it; k_fxms keeps the same loop in its own text, where it measured 0.3-2 % faster (§13h).
struct FxMinima {
    const int V, deg;
    int m1, m2, pos;
    uint64_t neg = 0;
    __device__ __forceinline__ FxMinima(int V_, int deg_, int no_pos) : V(V_), deg(deg_), m1(V_), m2(V_), pos(no_pos) {}
    // Edges k0 .. k0 + 3; those past the row count as +V.
    __device__ __forceinline__ void step(int k0, const int (&x)[4])
    {
        uint32_t nb = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int xq = k0 + q < deg ? x[q] : V;
            const int ax = xq < 0 ? -xq : xq;
            nb |= (uint32_t)(xq < 0) << q;
            if (ax < m1) {
                m2 = m1;
                m1 = ax;
                pos = k0 + q;
            } else if (ax < m2) {
                m2 = ax;
            }
        }
        neg |= (uint64_t)nb << k0;
    }
    // f of both minima: identity (MS), (m num) >> shift (NMS), max(m - beta, 0) (OMS).
    template <typename Args> __device__ __forceinline__ void scale(const Args &a)
    {
        if (a.variant == V_NMS) {
            m1 = (m1 * a.nms_num) >> a.nms_shift;
            m2 = (m2 * a.nms_num) >> a.nms_shift;
        } else if (a.variant == V_OMS) {
            m1 = max(m1 - a.beta, 0);
            m2 = max(m2 - a.beta, 0);
        }
    }
};

// The decisions out (dec_of(v) is 1 where bit v decides -1); returns the thread's bit errors.
template <typename Args, typename Dec>
__device__ __forceinline__ int fx_decisions_out(const Args &a, int b, int N, int lane, const int8_t *cvec, Dec &&dec_of,
                                                int stride = 64)
{
    int errs = 0;
    for (int v = lane; v < N; v += stride) {
        const int dbit = dec_of(v);
        errs += dbit != (cvec ? cvec[v] < 0 : 0);
        if (a.d_out) a.d_out[(size_t)b * N + v] = dbit ? -1 : 1;
    }
    return errs;
}
// The record of a frame with `errs` bit errors and `unc` uncoded ones after `it` iterations (one thread).
template <typename Args>
__device__ __forceinline__ void fx_frame_account(const Args &a, int b, int errs, int unc, bool fail, int it)
{
    frame_account(a.counts, a.hist, a.frame_res, b, errs, unc, fail, a.early_stop ? it : a.T, a.early_stop ? it : 0);
}
// The frame's result over the wave that owns it.
template <typename Args, typename Dec>
__device__ __forceinline__ void fx_frame_result(const Args &a, int b, int N, int lane, const int8_t *cvec, int unc,
                                                bool fail, int it, Dec &&dec_of)
{
    const int errs = wave_sum(fx_decisions_out(a, b, N, lane, cvec, dec_of));
    unc = wave_sum(unc);
    if (lane == 0) fx_frame_account(a, b, errs, unc, fail, it);
}

}  // namespace ldpc
