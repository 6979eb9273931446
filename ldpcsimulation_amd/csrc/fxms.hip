// fxms.hip -- CDNA4 (gfx950) kernels of fixed-point min-sum: flooding MS / NMS / OMS whose
// messages are msg_bits-wide saturating integers (include/ldpc_hip.h has the
// definition). With V = 2^(msg_bits - 1) - 1:
//   front end    in the cfg's precision F, quantize() of decodeMinSum.cpp:480-489 in its order of
//                operations, as the integer code Y = +-(Nq - 1) when |y| > Ymax, else
//                +-2 max(floor(|y| (Nq - 1) / (2 Ymax)), 1); never 0, odd only when saturated
//   start        v2c = clamp(Y, -V, V) on every edge of the bit; decisions r = Y > 0
//   check nodes  m1 <= m2 the two smallest |v2c| of the row (V where the row has fewer), P the
//                product of sgn(v2c), sgn(0) = +1; c2v_k = P sgn(v2c_k) f(k at the minimum ? m2 : m1),
//                f = identity (MS), (m num) >> shift (NMS), max(m - beta, 0) (OMS)
//   bit nodes    S = Y + sum c2v in int32 (the unclamped Y); v2c_k = clamp(S - c2v_k, -V, V);
//                d = S > 0 ? +1 : -1
// T iterations, or with early_stop up to the first t in 0..T whose decisions are a codeword.
//
// One kernel body on the wave-per-codeword skeleton (wave_cw.h); fxms_layout.h has
// the state of a codeword in LDS. A message lives in one slot for both directions -- edge k of
// check j at k * M + j, so the lanes of a wave read consecutive messages in the check phase
// whatever the row degree -- and a check keeps its row's signs in a 64-bit mask between its two
// passes (rows have at most kMaxRowDegree = 58 edges). Every edge loop keeps four LDS reads in
// flight (edges past the node's degree read its last edge and count as +V in a check, as 0 in
// a bit), and a bit keeps its first four messages in registers between the sum and the messages
// back, so only bits of degree above 4 read twice. The graph (template STAGE): where it fits
// beside the codewords every workgroup copies it into LDS once; the iterations then read no
// global memory but col_ptr and row_deg. Without it the indices come from the device copy of
// the graph through the caches.
#include "fxms.h"
#include "fx_front.h"

#include <hip/hip_runtime.h>

namespace ldpc {

template <typename F, typename MT, int SRC, bool STAGE>
__global__ __launch_bounds__(1024) void k_fxms(FxmsArgs a, DevGraph g, FxmsLayout L)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int upb = (int)(blockDim.x >> 6);   // codewords in flight per workgroup
    const uint16_t *gr = reinterpret_cast<const uint16_t *>(smem);             // [dcs][M] bits of the checks
    const uint16_t *gs = reinterpret_cast<const uint16_t *>(smem + L.gcoff);   // [E] slots of the bits' edges
    const int N = g.N, M = g.M, T = a.T, V = a.vmax;
    [[maybe_unused]] const uint32_t slots = (uint32_t)L.slots;   // the bound of LDPC_CHK
    if (STAGE) {   // once per workgroup, before its waves part ways
        uint16_t *wr = reinterpret_cast<uint16_t *>(smem), *wc = reinterpret_cast<uint16_t *>(smem + L.gcoff);
        for (int j = threadIdx.x; j < M; j += blockDim.x)
            for (int k = 0; k < g.dcs; ++k) wr[(size_t)k * M + j] = (uint16_t)g.row_cols[(size_t)j * g.dcs + k];
        for (int e = threadIdx.x; e < L.E; e += blockDim.x) {
            const uint32_t ref = g.col_refs[e];
            wc[e] = (uint16_t)((ref & 63u) * (uint32_t)M + (ref >> 6));
        }
        __syncthreads();
    }
    unsigned char *base = smem + (STAGE ? L.cwoff : 0) + (size_t)wave * L.total;
    MT *msg = reinterpret_cast<MT *>(base);
    int8_t *Y = reinterpret_cast<int8_t *>(base + L.yoff);
    uint8_t *D = base + L.doff;
    const int variant = a.variant, num = a.nms_num, shift = a.nms_shift, beta = a.beta;
    auto slot_of = [&](int e) -> uint32_t {
        uint32_t s;
        if (STAGE) {
            s = gs[e];
        } else {
            const uint32_t ref = g.col_refs[e];
            s = (ref & 63u) * (uint32_t)M + (ref >> 6);
        }
        return LDPC_CHK(s, slots, CHK_FXMS_SLOT);
    };
    auto dec_of = [&](uint32_t i) __attribute__((always_inline)) { return (uint32_t)D[i]; };

    CwTickets tk(a.ticket, a.batch, upb, lane == 0);
    for (int b = tk.first(wave); b < a.batch; b = tk.next()) {
        const int8_t *cvec = frame_codeword<SRC>(a, b, N);
        int unc = fx_front_end<F, SRC>(a, b, N, lane, cvec, [&](int v, int yc) __attribute__((always_inline)) {
            Y[v] = (int8_t)yc;
            D[v] = (uint8_t)(yc > 0 ? 0 : 1);
        });
        wave_sync();   // the front end wrote Y by groups of 4 bits, the start reads it by bit
        for (int v = lane; v < N; v += 64) {
            const int m = min(max((int)Y[v], -V), V);
            for (int e = g.col_ptr[v], e1 = g.col_ptr[v + 1]; e < e1; ++e) msg[slot_of(e)] = (MT)m;
        }
        wave_sync();

        int it = 0;
        bool fail = false;
        for (;;) {
            if (a.early_stop || it == T) {
                fail = fx_syndrome_fails(
                    M, lane, [&](int j) __attribute__((always_inline)) { return (int)g.row_deg[j]; },
                    [&](int k, int j) __attribute__((always_inline)) {
                        const uint32_t i = STAGE ? (uint32_t)gr[(size_t)k * M + j] : (uint32_t)g.row_cols[(size_t)j * g.dcs + k];
                        return LDPC_CHK(i, (uint32_t)N, CHK_FXMS_BIT);
                    },
                    dec_of);
                if (!fail || it == T) break;   // uniform over the wave
            }
            // ---- check nodes: the minima and the signs, then the messages back ----
            for (int j = lane; j < M; j += 64) {
                const int deg = g.row_deg[j];
                int m1 = V, m2 = V, pos = -1;
                uint64_t neg = 0;
                for (int k0 = 0; k0 < deg; k0 += 4) {   // four edges in flight; those past the row count as +V
                    int x[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int k = min(k0 + q, deg - 1);
                        x[q] = msg[LDPC_CHK((uint32_t)(k * M + j), slots, CHK_FXMS_SLOT)];
                    }
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
                if (variant == V_NMS) {
                    m1 = (m1 * num) >> shift;
                    m2 = (m2 * num) >> shift;
                } else if (variant == V_OMS) {
                    m1 = max(m1 - beta, 0);
                    m2 = max(m2 - beta, 0);
                }
                if (__popcll(neg) & 1) neg = ~neg;   // P sgn(v2c_k) < 0
                for (int k0 = 0; k0 < deg; k0 += 4) {
                    const uint32_t nb = (uint32_t)(neg >> k0);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int k = k0 + q, mag = k == pos ? m2 : m1;
                        if (k < deg)
                            msg[LDPC_CHK((uint32_t)(k * M + j), slots, CHK_FXMS_SLOT)] = (MT)(((nb >> q) & 1) ? -mag : mag);
                    }
                }
            }
            wave_sync();
            // ---- bit nodes ----
            for (int v = lane; v < N; v += 64) {
                const int e0 = g.col_ptr[v], e1 = g.col_ptr[v + 1];
                int S = Y[v];
                if (e1 > e0) {
                    // the first four edges stay in registers between the sum and the messages back
                    // (most bits have no more); edges past the bit's count as 0
                    uint32_t s0[4];
                    int c0[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) s0[q] = slot_of(min(e0 + q, e1 - 1));
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        c0[q] = e0 + q < e1 ? (int)msg[s0[q]] : 0;
                        S += c0[q];
                    }
                    for (int e = e0 + 4; e < e1; e += 4) {
                        uint32_t s[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q) s[q] = slot_of(min(e + q, e1 - 1));
#pragma unroll
                        for (int q = 0; q < 4; ++q) S += e + q < e1 ? (int)msg[s[q]] : 0;
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (e0 + q < e1) msg[s0[q]] = (MT)min(max(S - c0[q], -V), V);
                    for (int e = e0 + 4; e < e1; e += 4) {
                        uint32_t s[4];
                        int c[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q) s[q] = slot_of(min(e + q, e1 - 1));
#pragma unroll
                        for (int q = 0; q < 4; ++q) c[q] = msg[s[q]];
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            if (e + q < e1) msg[s[q]] = (MT)min(max(S - c[q], -V), V);
                    }
                }
                D[v] = (uint8_t)(S > 0 ? 0 : 1);
            }
            wave_sync();
            ++it;
        }
        fx_frame_result(a, b, N, lane, cvec, unc, fail, it, dec_of);
    }
}

LDPC_CHECK_TU(fxms)

FxmsChoice fxms_choose(const DevGraph &g, int E, int msg_bits) { return fxms_plan({g.N, g.M, g.dcs, E}, msg_bits); }

hipError_t fxms_launch(const DevGraph &g, const FxmsArgs &a, bool f64, const FxmsChoice &ch, int E, int num_cus,
                       hipStream_t s)
{
    return wave_cw_launch(
        a, f64, ch, num_cus, s,
        [&](auto f, auto src) {
            using F = typename decltype(f)::type;
            constexpr int SRC = decltype(src)::value;
            if (ch.wide) return ch.staged ? k_fxms<F, int16_t, SRC, true> : k_fxms<F, int16_t, SRC, false>;
            return ch.staged ? k_fxms<F, int8_t, SRC, true> : k_fxms<F, int8_t, SRC, false>;
        },
        g, fxms_layout({g.N, g.M, g.dcs, E}, ch.wide));
}

}  // namespace ldpc
