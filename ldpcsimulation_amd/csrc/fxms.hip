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
// One kernel body: a wavefront per codeword, up to 16 per workgroup, no workgroup barrier (the
// shape of hwgdbf_wave: a lane owns checks lane, lane + 64, ... and bits likewise; the wave's
// LDS operations execute in issue order, so a wavefront-scope fence orders a phase's writes
// before the next phase's reads). Waves are persistent and take codewords by ticket, so a
// frame that stops early frees its wave at once. State of a codeword in LDS:
//   msg[dcs * M] (MT = int8 when msg_bits <= 8, else int16) | Y[N] (int8) | D[N] (the decisions)
// A message lives in one slot for both directions -- edge k of check j at k * M + j, so the
// lanes of a wave read consecutive messages in the check phase whatever the row degree -- and
// a check keeps its row's signs in a 64-bit mask between its two passes (rows have at most
// kMaxRowDegree = 58 edges). Every edge loop keeps four LDS reads in flight (edges past the
// node's degree read its last edge and count as +V in a check, as 0 in a bit), and a bit keeps
// its first four messages in registers between the sum and the messages back, so only bits of
// degree above 4 read twice. The graph (template STAGE): where it fits beside the codewords
// every workgroup copies it into LDS once as 16-bit indices, the slot of every column edge and
// the checks' bits slot-major; the iterations then read no global memory but col_ptr and
// row_deg. Without it the indices come from the device copy of the graph through the caches.
#include "fxms.h"
#include "fx_front.h"   // fx_wave_sync, fx_wave_sum, fx_quant: shared with fxlms.hip
#include "frame.h"

#include <hip/hip_runtime.h>

namespace ldpc {

struct FxmsLayout {
    int slots;                 // dcs * M message slots
    int yoff, doff, total;     // of one codeword, bytes
    int E, gcoff, cwoff;       // STAGE: edges, byte offset of the column edges' slots, of the first codeword
};
static FxmsLayout fxms_layout(const DevGraph &g, int E, bool wide)
{
    auto al = [](long long x) { return (x + 15) & ~15ll; };
    auto cap = [](long long x) { return x > 0x7fffffffll ? 0x7fffffff : (int)x; };
    FxmsLayout L;
    const long long slots = (long long)g.M * g.dcs;
    const long long y = al(slots * (wide ? 2 : 1)), d = y + al(g.N), t = d + al(g.N);
    L.slots = cap(slots);
    L.yoff = cap(y);
    L.doff = cap(d);
    L.total = cap(t);
    L.E = E;
    const long long gc = al(2 * slots), cw = gc + al(2ll * E);
    L.gcoff = cap(gc);
    L.cwoff = cap(cw);
    return L;
}

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
    const F ymax = (F)a.ymax;
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

    // Codewords: the grid's own first, then tickets; lane 0 draws the next ticket while the
    // current codeword decodes.
    unsigned nxt = 0;
    if (lane == 0) nxt = gridDim.x * upb + atomicAdd(a.ticket, 1u);
    for (int b = blockIdx.x * upb + wave; b < a.batch;) {
        const int8_t *cvec = frame_codeword<SRC>(a, b, N);
        // ---- channel + front end ----
        int unc = 0;
        for (int g4 = lane; g4 * 4 < N; g4 += 64) {
            F yv[4];
            channel_group<F, SRC, true>(a, b, g4, N, cvec, a.y_out, yv);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int v = g4 * 4 + q;
                if (v < N) {
                    const int yc = fx_quant<F>(yv[q], ymax, a.nq1);
                    const int rbit = yc > 0 ? 0 : 1;
                    unc += rbit != (cvec ? cvec[v] < 0 : 0);
                    Y[v] = (int8_t)yc;
                    D[v] = (uint8_t)rbit;
                    if (a.ycode_out) a.ycode_out[(size_t)b * N + v] = (int8_t)yc;
                }
            }
        }
        fx_wave_sync();   // the front end wrote Y by groups of 4 bits, the start reads it by bit
        for (int v = lane; v < N; v += 64) {
            const int m = min(max((int)Y[v], -V), V);
            for (int e = g.col_ptr[v], e1 = g.col_ptr[v + 1]; e < e1; ++e) msg[slot_of(e)] = (MT)m;
        }
        fx_wave_sync();

        int it = 0;
        bool fail = false;
        for (;;) {
            if (a.early_stop || it == T) {
                // ---- syndrome of the decisions ----
                int f = 0;
                for (int j = lane; j < M; j += 64) {
                    const int deg = g.row_deg[j];
                    const int32_t *rc = g.row_cols + (size_t)j * g.dcs;
                    uint32_t p = 0;
                    for (int k0 = 0; k0 < deg; k0 += 4) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int k = min(k0 + q, deg - 1);
                            const uint32_t i = STAGE ? (uint32_t)gr[(size_t)k * M + j] : (uint32_t)rc[k];
                            const uint32_t dbit = D[LDPC_CHK(i, (uint32_t)N, CHK_FXMS_BIT)];
                            p ^= k0 + q < deg ? dbit : 0u;
                        }
                    }
                    f |= (int)(p & 1u);
                }
                fail = __builtin_amdgcn_ballot_w64(f != 0) != 0;
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
            fx_wave_sync();
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
            fx_wave_sync();
            ++it;
        }
        // ---- the frame's result ----
        int errs = 0;
        for (int v = lane; v < N; v += 64) {
            const int dbit = D[v];
            errs += dbit != (cvec ? cvec[v] < 0 : 0);
            if (a.d_out) a.d_out[(size_t)b * N + v] = dbit ? -1 : 1;
        }
        errs = fx_wave_sum(errs);
        unc = fx_wave_sum(unc);
        if (lane == 0)
            frame_account(a.counts, a.hist, a.frame_res, b, errs, unc, fail, a.early_stop ? it : T, a.early_stop ? it : 0);
        fx_wave_sync();   // the next codeword's front end rewrites Y and D
        b = (int)__shfl((int)nxt, 0, 64);
        if (lane == 0 && b < a.batch) nxt = gridDim.x * upb + atomicAdd(a.ticket, 1u);
    }
}

LDPC_CHECK_TU(fxms)

// Waves per workgroup: the count that keeps most codewords on a CU (each workgroup carries the
// staged graph and 128 bytes of slack), up to 16 waves per workgroup and 28 per CU (7 per
// SIMD at the kernel's 64 VGPRs). A tie goes to the larger workgroup, which stages the graph
// fewer times.
FxmsChoice fxms_choose(const DevGraph &g, int E, int msg_bits)
{
    FxmsChoice ch;
    ch.wide = msg_bits > 8;
    const FxmsLayout L = fxms_layout(g, E, ch.wide);
    ch.cw_bytes = L.total;
    if (L.total > kFxmsMaxLds) return ch;   // name stays empty: the caller reports the bound
    // the 16-bit graph beside the codewords, when the indices fit 16 bits and it leaves room for a codeword
    ch.staged = g.N <= 65535 && (long long)g.M * g.dcs <= 65536 && (size_t)L.cwoff + (size_t)L.total + 128 <= kMaxLds;
    const int gb = ch.staged ? L.cwoff : 0;
    int best_c = 1, best_w = 0;
    for (int c = 1; c <= 16; ++c) {
        const size_t wg = (size_t)gb + (size_t)L.total * c + 128;
        if (wg > kMaxLds) break;
        const int w = std::min((int)(kMaxLds / wg) * c, 28);
        if (w >= best_w) {
            best_w = w;
            best_c = c;
        }
    }
    ch.name = ch.wide ? "fxms_i16" : "fxms_i8";
    ch.cw_per_block = best_c;
    ch.threads = 64 * best_c;
    ch.lds_bytes = gb + L.total * best_c;
    return ch;
}

template <typename F, typename MT, int SRC, bool STAGE>
static hipError_t fxms_launch_w(const DevGraph &g, const FxmsArgs &a, const FxmsChoice &ch, int E, int num_cus,
                                hipStream_t s)
{
    const FxmsLayout L = fxms_layout(g, E, ch.wide);
    auto fn = k_fxms<F, MT, SRC, STAGE>;
    int per_cu = occupancy(reinterpret_cast<const void *>(fn), ch.threads, ch.lds_bytes);   // raises the LDS limit
    if (per_cu < 1) per_cu = 1;
    int grid = per_cu * (num_cus > 0 ? num_cus : 1);
    const int need = (a.batch + ch.cw_per_block - 1) / ch.cw_per_block;
    if (grid > need) grid = need;
    hipLaunchKernelGGL(fn, dim3(grid), dim3(ch.threads), ch.lds_bytes, s, a, g, L);
    return hipGetLastError();
}

hipError_t fxms_launch(const DevGraph &g, const FxmsArgs &a, bool f64, const FxmsChoice &ch, int E, int num_cus,
                       hipStream_t s)
{
    if (a.batch <= 0) return hipSuccess;
    if (!a.ticket || ch.cw_per_block < 1 || (size_t)ch.lds_bytes > kMaxLds) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(a.ticket, 0, sizeof(unsigned), s);
    if (e != hipSuccess) return e;
    return for_f_src(f64, a.src, [&](auto f, auto src) {
        using F = typename decltype(f)::type;
        constexpr int SRC = decltype(src)::value;
        if (ch.wide)
            return ch.staged ? fxms_launch_w<F, int16_t, SRC, true>(g, a, ch, E, num_cus, s)
                             : fxms_launch_w<F, int16_t, SRC, false>(g, a, ch, E, num_cus, s);
        return ch.staged ? fxms_launch_w<F, int8_t, SRC, true>(g, a, ch, E, num_cus, s)
                         : fxms_launch_w<F, int8_t, SRC, false>(g, a, ch, E, num_cus, s);
    });
}

}  // namespace ldpc
