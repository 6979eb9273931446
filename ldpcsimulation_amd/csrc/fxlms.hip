// fxlms.hip -- CDNA4 (gfx950) kernel of layered fixed-point min-sum: row-layered MS / NMS / OMS
// with a saturating app_bits-wide posterior (APP) per bit and a msg_bits-wide message per edge,
// as a hardware layered decoder has them (include/ldpc_hip.h has the definition).
// With V = 2^(msg_bits - 1) - 1 and A = 2^(app_bits - 1) - 1:
//   front end    the fixed-point min-sum front end (fx_front.h): the integer code Y
//   start        app = clamp(Y, -A, A), every c2v = 0
//   row j        in the layered row order: x_k = clamp(app[b_k] - c2v_k, -V, V); m1 <= m2 the two
//                smallest |x_k| (V where the row has fewer), P the product of sgn(x_k);
//                c2v_k = P sgn(x_k) f(k at the minimum ? m2 : m1); app[b_k] = clamp(x_k + c2v_k, -A, A)
//   decision     app > 0 ? +1 : -1
// T iterations, or with early_stop up to the first t in 0..T whose decisions are a codeword.
//
// One kernel body on the wave-per-codeword skeleton (wave_cw.h); fxlms_layout.h
// has the state of a codeword in LDS. The wave walks the layers; a lane owns rows ptr[L] + lane,
// + 64, ... of layer L, and a wavefront-scope fence separates the layers (rows of a layer share
// no bit, so its lanes touch disjoint APPs).
// A check row keeps its messages packed: the two magnitudes after f, f(m1) and f(m2), in MG
// (7 bits each in 16 when AT is int8, else 15 bits each in 32), and in S0 the signs of edges
// 0..25 below the 6-bit position of the minimum; S1 holds the signs of edges 26..57
// (kMaxRowDegree = 58). c2v_k is exactly (sign_k ? -1 : +1) (k at the position ? f(m2) : f(m1)),
// so a row costs three LDS reads and writes of state whatever its degree, and its edges move
// only APPs: a gather for the minima and, past the first eight edges, which stay in
// registers, a second gather before the scatter (the APPs of a row's own bits do not change
// in between). The schedule (template STAGE): where it fits beside the codewords at little
// cost in resident waves (fxlms_choose) every workgroup copies it into LDS once, the rows'
// bits as 16-bit indices slot-major -- edge k of the row at layered position n at k * M + n,
// so the lanes of a wave read consecutive entries whatever the row degree -- and the
// degrees; the iterations then read no global memory but the layer pointers. Without it the
// same arrays come from the device copy through the caches.
#include "fxlms.h"
#include "fx_front.h"

#include <hip/hip_runtime.h>

namespace ldpc {

template <typename AT> struct fxl_mag;   // the packed magnitudes of a row
template <> struct fxl_mag<int8_t> {
    using type = uint16_t;
    static constexpr int shift = 8;
};
template <> struct fxl_mag<int16_t> {
    using type = uint32_t;
    static constexpr int shift = 16;
};

template <typename F, typename AT, int SRC, bool STAGE>
__global__ __launch_bounds__(1024) void k_fxlms(FxlmsArgs a, FxlmsSched sc, FxlmsLayout L)
{
    using MGT = typename fxl_mag<AT>::type;
    constexpr int MSH = fxl_mag<AT>::shift;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int upb = (int)(blockDim.x >> 6);   // codewords in flight per workgroup
    const uint16_t *gc = reinterpret_cast<const uint16_t *>(smem);   // [dcs][M] bits of the rows
    const uint8_t *gd = smem + L.gdoff;                              // [M] their degrees
    const int N = sc.N, M = sc.M, T = a.T, V = a.vmax, A = a.amax;
    const bool hi = L.hi != 0;
    [[maybe_unused]] const uint32_t slots = (uint32_t)L.slots;   // the bound of LDPC_CHK
    if (STAGE) {   // once per workgroup, before its waves part ways
        uint16_t *wc = reinterpret_cast<uint16_t *>(smem);
        uint8_t *wd = smem + L.gdoff;
        for (int e = threadIdx.x; e < L.slots; e += blockDim.x) wc[e] = (uint16_t)sc.cols[e];
        for (int n = threadIdx.x; n < M; n += blockDim.x) wd[n] = sc.deg[n];
        __syncthreads();
    }
    unsigned char *base = smem + (STAGE ? L.cwoff : 0) + (size_t)wave * L.total;
    AT *app = reinterpret_cast<AT *>(base);
    uint32_t *S0 = reinterpret_cast<uint32_t *>(base + L.s0off);
    uint32_t *S1 = reinterpret_cast<uint32_t *>(base + L.s1off);
    MGT *MG = reinterpret_cast<MGT *>(base + L.mgoff);
    // bit of edge k of the row at layered position n
    auto bit_of = [&](int k, int n) -> uint32_t {
        const uint32_t e = LDPC_CHK((uint32_t)(k * M + n), slots, CHK_FXLMS_SCHED);
        const uint32_t i = STAGE ? (uint32_t)gc[e] : (uint32_t)sc.cols[e];
        return LDPC_CHK(i, (uint32_t)N, CHK_FXLMS_BIT);
    };
    auto dec_of = [&](uint32_t i) __attribute__((always_inline)) { return app[i] <= 0 ? 1u : 0u; };
    auto deg_of = [&](uint32_t n) __attribute__((always_inline)) { return STAGE ? (int)gd[n] : (int)sc.deg[n]; };

    CwTickets tk(a.ticket, a.batch, upb, lane == 0);
    for (int b = tk.first(wave); b < a.batch; b = tk.next()) {
        const int8_t *cvec = frame_codeword<SRC>(a, b, N);
        // the start's APPs
        int unc = fx_front_end<F, SRC>(a, b, N, lane, cvec,
                                       [&](int v, int yc) __attribute__((always_inline)) { app[v] = (AT)min(max(yc, -A), A); });
        for (int n = lane; n < M; n += 64) {   // every c2v = 0
            S0[n] = 0u;
            if (hi) S1[n] = 0u;
            MG[n] = (MGT)0;
        }
        wave_sync();   // the start wrote by groups of 4 bits and by row, the layers read by row and edge

        int it = 0;
        bool fail = false;
        for (;;) {
            if (a.early_stop || it == T) {
                fail = fx_syndrome_fails(M, lane, deg_of, bit_of, dec_of);
                if (!fail || it == T) break;   // uniform over the wave
            }
            // ---- the layers, serially; the rows of a layer over the lanes ----
            for (int l = 0; l < sc.nlayers; ++l) {
                const int n1 = sc.lptr[l + 1];
                for (int n = sc.lptr[l] + lane; n < n1; n += 64) {
                    const uint32_t r = LDPC_CHK((uint32_t)n, (uint32_t)M, CHK_FXLMS_ROW);
                    const int deg = deg_of(r);
                    if (deg == 0) continue;
                    // the row's messages of the last iteration
                    const uint32_t w0 = S0[r], w1 = hi ? S1[r] : 0u;
                    const uint32_t omg = MG[r];
                    const int of1 = (int)(omg & ((1u << MSH) - 1u)), of2 = (int)(omg >> MSH), opos = (int)(w0 >> 26);
                    const uint64_t osg = (uint64_t)(w0 & 0x3ffffffu) | ((uint64_t)w1 << 26);
                    // x of four edges (those past the row repeat its last edge)
                    auto gather = [&](int k0, int (&x)[4], uint32_t (&bi)[4]) {
                        int av[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q) bi[q] = bit_of(min(k0 + q, deg - 1), (int)r);
#pragma unroll
                        for (int q = 0; q < 4; ++q) av[q] = app[bi[q]];
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int k = min(k0 + q, deg - 1), mag = k == opos ? of2 : of1;
                            const int c = ((osg >> k) & 1u) ? -mag : mag;
                            x[q] = min(max(av[q] - c, -V), V);
                        }
                    };
                    FxMinima mn(V, deg, 63);
                    // the first eight edges stay in registers between the minima and the APPs back
                    int xa[4], xb[4];
                    uint32_t ba[4], bb[4];
                    gather(0, xa, ba);
                    mn.step(0, xa);
                    if (deg > 4) {
                        gather(4, xb, bb);
                        mn.step(4, xb);
                    }
                    for (int k0 = 8; k0 < deg; k0 += 4) {
                        int x[4];
                        uint32_t bi[4];
                        gather(k0, x, bi);
                        mn.step(k0, x);
                    }
                    mn.scale(a);
                    if (__popcll(mn.neg) & 1) mn.neg ^= (1ull << deg) - 1ull;   // P sgn(x_k) < 0, on the row's edges
                    auto scatter = [&](int k0, const int (&x)[4], const uint32_t (&bi)[4]) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int k = k0 + q, mag = k == mn.pos ? mn.m2 : mn.m1;
                            const int c = ((mn.neg >> k) & 1u) ? -mag : mag;
                            if (k < deg) app[bi[q]] = (AT)min(max(x[q] + c, -A), A);
                        }
                    };
                    scatter(0, xa, ba);
                    if (deg > 4) scatter(4, xb, bb);
                    for (int k0 = 8; k0 < deg; k0 += 4) {   // their APPs are still the ones the minima saw
                        int x[4];
                        uint32_t bi[4];
                        gather(k0, x, bi);
                        scatter(k0, x, bi);
                    }
                    S0[r] = (uint32_t)(mn.neg & 0x3ffffffu) | ((uint32_t)mn.pos << 26);
                    if (hi) S1[r] = (uint32_t)(mn.neg >> 26);
                    MG[r] = (MGT)((uint32_t)mn.m1 | ((uint32_t)mn.m2 << MSH));
                }
                wave_sync();   // the next layer gathers what this one scattered
            }
            ++it;
        }
        fx_frame_result(a, b, N, lane, cvec, unc, fail, it, dec_of);
    }
}

LDPC_CHECK_TU(fxlms)

FxlmsChoice fxlms_choose(const FxlmsSched &sc, int app_bits) { return fxlms_plan({sc.N, sc.M, sc.dcs, 0}, app_bits); }

hipError_t fxlms_launch(const FxlmsSched &sc, const FxlmsArgs &a, bool f64, const FxlmsChoice &ch, int num_cus,
                        hipStream_t s)
{
    if (a.batch > 0 && !sc.lptr) return hipErrorInvalidValue;
    return wave_cw_launch(
        a, f64, ch, num_cus, s,
        [&](auto f, auto src) {
            using F = typename decltype(f)::type;
            constexpr int SRC = decltype(src)::value;
            if (ch.wide) return ch.staged ? k_fxlms<F, int16_t, SRC, true> : k_fxlms<F, int16_t, SRC, false>;
            return ch.staged ? k_fxlms<F, int8_t, SRC, true> : k_fxlms<F, int8_t, SRC, false>;
        },
        sc, fxlms_layout({sc.N, sc.M, sc.dcs, 0}, ch.wide));
}

}  // namespace ldpc
