// frame.h -- what a frame is: its transmitted codeword, its channel samples and its
// counters, for the decoder kernels of kernels.hip, flood.hip, layered.hip, bp.hip,
// gdbf.hip, rgdbf.hip and ddbmp.hip. Args is DecodeArgs or GdbfArgs (which has no y_out, so y_out is
// a parameter). rows.hip, rows_fast.hip, rows_pp.hip and nb.hip do not include this: their
// channel steps are staged through LDS and tuned with their kernels.
#pragma once
#include "device_common.h"
#include "kernels.h"

namespace ldpc {

// Row of the transmitted codeword of frame b, or null (all +1).
template <int SRC, typename Args>
__device__ __forceinline__ const int8_t *frame_codeword(const Args &a, int b, int N)
{
    if (SRC == SRC_GIVEN) return a.c ? a.c + (size_t)b * N : nullptr;
    if (!a.cw_table) return nullptr;
    return a.cw_table + (size_t)((a.first_cw + (uint64_t)b) % (uint64_t)a.cw_rows) * N;
}

// The channel samples of bits 4 * g4 .. 4 * g4 + 3 of frame b. SRC_GIVEN: from a.y, 1 past N.
// SRC_PHILOX: y = c (1 + sigma n), n from Philox4x32-10 keyed by the seed at counter
// (g4, lo32(cw), hi32(cw), stream_id) + Box-Muller; written to y_out (may be null) up to N.
// DESIGN §5a has the layout of every stream (it is a contract: checkpoints and sharded
// sweeps rely on it) and tests/test_philox_channel.py compares every sample with it.
// Like MAD64, Y_AFTER is each site's choice and changes no value: the y_out store sits in the
// sample loop, or in a loop after it (layered.hip; bp.hip, its fp64 rows kernel excepted). In
// the sample loop k_bp_global<double, 16> takes 148 VGPRs instead of 127 and the fp64 layered
// DVB-S2 launch measured 0.2 ms of 56 slower; after it the DD-BMP rows kernel takes 1-2 VGPRs more.
template <typename F, int SRC, bool MAD64, bool Y_AFTER = false, typename Args>
__device__ __forceinline__ void channel_group(const Args &a, int b, int g4, int N, const int8_t *cvec, void *y_out,
                                              F (&yv)[4])
{
    if (SRC == SRC_GIVEN) {
        const F *y = reinterpret_cast<const F *>(a.y) + (size_t)b * N;
#pragma unroll
        for (int q = 0; q < 4; ++q) yv[q] = (g4 * 4 + q < N) ? y[g4 * 4 + q] : F(1);
    } else {
        const uint64_t cw = a.first_cw + (uint64_t)b;
        uint32_t u[4];
        philox4x32_10<MAD64>((uint32_t)g4, (uint32_t)cw, (uint32_t)(cw >> 32), a.stream_id, (uint32_t)a.seed,
                             (uint32_t)(a.seed >> 32), u);
        F n[4];
        box_muller(u[0], u[1], n[0], n[1]);
        box_muller(u[2], u[3], n[2], n[3]);
        const F sigma = (F)a.sigma;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int v = g4 * 4 + q;
            yv[q] = (F)(v < N && cvec ? cvec[v] : 1) * (F(1) + sigma * n[q]);
            if (!Y_AFTER && y_out && v < N) reinterpret_cast<F *>(y_out)[(size_t)b * N + v] = yv[q];
        }
        if (Y_AFTER && y_out) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (g4 * 4 + q < N) reinterpret_cast<F *>(y_out)[(size_t)b * N + g4 * 4 + q] = yv[q];
        }
    }
}

// The channel of one frame over the workgroup: bit(v, y_v) once for every bit of the thread,
// per bit for SRC_GIVEN and per Philox group for SRC_PHILOX.
template <typename F, int SRC, bool MAD64, bool Y_AFTER = false, typename Args, typename Bit>
__device__ __forceinline__ void channel_bits(const Args &a, int b, int N, const int8_t *cvec, void *y_out, Bit &&bit)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    if (SRC == SRC_GIVEN) {
        const F *y = reinterpret_cast<const F *>(a.y) + (size_t)b * N;
        for (int v = tid; v < N; v += nt) bit(v, y[v]);
    } else {
        for (int g4 = tid; g4 * 4 < N; g4 += nt) {
            F yv[4];
            channel_group<F, SRC, MAD64, Y_AFTER>(a, b, g4, N, cvec, y_out, yv);
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (g4 * 4 + q < N) bit(g4 * 4 + q, yv[q]);
        }
    }
}

// One decoded frame into the counters (one thread): w bit errors, unc uncoded bit errors.
// iterations_counted goes to counts[4], iterations_reported to frame_res[b].w.
__device__ __forceinline__ void frame_account(unsigned long long *counts, unsigned long long *hist, int4 *frame_res,
                                              int b, int w, int unc, int synd_fail, int iterations_counted,
                                              int iterations_reported)
{
    atomicAdd(&counts[0], (unsigned long long)w);
    atomicAdd(&counts[1], (unsigned long long)(w > 0));
    atomicAdd(&counts[2], (unsigned long long)unc);
    atomicAdd(&counts[3], 1ull);
    atomicAdd(&counts[4], (unsigned long long)iterations_counted);
    atomicAdd(&counts[5], (unsigned long long)synd_fail);
    if (w > 0 && hist) atomicAdd(&hist[w - 1], 1ull);
    if (frame_res) frame_res[b] = make_int4(w, unc, synd_fail, iterations_reported);
}

// The same for a persistent workgroup that decodes T iterations per frame: the six counters
// add up in acc[6] (the block's, zero at its start), and frame_flush adds them once.
__device__ __forceinline__ void frame_account_acc(unsigned long long *acc, unsigned long long *hist, int4 *frame_res,
                                                  int b, int w, int unc, int synd_fail)
{
    acc[0] += (unsigned long long)w;
    acc[1] += (unsigned long long)(w > 0);
    acc[2] += (unsigned long long)unc;
    acc[3] += 1ull;
    acc[5] += (unsigned long long)synd_fail;
    if (w > 0 && hist) atomicAdd(&hist[w - 1], 1ull);
    if (frame_res) frame_res[b] = make_int4(w, unc, synd_fail, 0);
}
__device__ __forceinline__ void frame_flush(unsigned long long *counts, unsigned long long *acc, int T)
{
    if (acc[3] == 0) return;
    acc[4] = acc[3] * (unsigned long long)T;
#pragma unroll
    for (int q = 0; q < 6; ++q) atomicAdd(&counts[q], acc[q]);
}

}  // namespace ldpc
