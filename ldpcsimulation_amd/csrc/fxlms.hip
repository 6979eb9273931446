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
// The shape of k_fxms: a wavefront per codeword, up to 16 per workgroup, no workgroup barrier
// after staging, codewords by ticket. The wave walks the layers; a lane owns rows ptr[L] + lane,
// + 64, ... of layer L, and a wavefront-scope fence separates the layers (rows of a layer share
// no bit, so its lanes touch disjoint APPs). State of a codeword in LDS:
//   app[N] (AT = int8 when app_bits <= 8, else int16) | S0[M] | S1[M] (row degree > 26 only) | MG[M]
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
#include "frame.h"

#include <hip/hip_runtime.h>

namespace ldpc {

struct FxlmsLayout {
    int slots;                       // dcs * M schedule entries
    int s0off, s1off, mgoff, total;  // of one codeword, bytes
    int hi;                          // row degree > 26: S1 exists
    int gdoff, cwoff;                // STAGE: byte offset of the degrees, of the first codeword
};
static FxlmsLayout fxlms_layout(const FxlmsSched &sc, bool wide)
{
    auto al = [](long long x) { return (x + 15) & ~15ll; };
    auto cap = [](long long x) { return x > 0x7fffffffll ? 0x7fffffff : (int)x; };
    FxlmsLayout L;
    const long long slots = (long long)sc.M * sc.dcs;
    L.hi = sc.dcs > 26;
    const long long s0 = al((long long)sc.N * (wide ? 2 : 1)), s1 = s0 + al(4ll * sc.M),
                    mg = s1 + (L.hi ? al(4ll * sc.M) : 0), t = mg + al((long long)sc.M * (wide ? 4 : 2));
    L.slots = cap(slots);
    L.s0off = cap(s0);
    L.s1off = cap(s1);
    L.mgoff = cap(mg);
    L.total = cap(t);
    const long long gd = al(2 * slots), cw = gd + al(sc.M);
    L.gdoff = cap(gd);
    L.cwoff = cap(cw);
    return L;
}

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
    const F ymax = (F)a.ymax;
    const int variant = a.variant, num = a.nms_num, shift = a.nms_shift, beta = a.beta;
    // bit of edge k of the row at layered position n
    auto bit_of = [&](int k, int n) -> uint32_t {
        const uint32_t e = LDPC_CHK((uint32_t)(k * M + n), slots, CHK_FXLMS_SCHED);
        const uint32_t i = STAGE ? (uint32_t)gc[e] : (uint32_t)sc.cols[e];
        return LDPC_CHK(i, (uint32_t)N, CHK_FXLMS_BIT);
    };

    // Codewords: the grid's own first, then tickets; lane 0 draws the next ticket while the
    // current codeword decodes.
    unsigned nxt = 0;
    if (lane == 0) nxt = gridDim.x * upb + atomicAdd(a.ticket, 1u);
    for (int b = blockIdx.x * upb + wave; b < a.batch;) {
        const int8_t *cvec = frame_codeword<SRC>(a, b, N);
        // ---- channel + front end: the start's APPs ----
        int unc = 0;
        for (int g4 = lane; g4 * 4 < N; g4 += 64) {
            F yv[4];
            channel_group<F, SRC, true>(a, b, g4, N, cvec, a.y_out, yv);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int v = g4 * 4 + q;
                if (v < N) {
                    const int yc = fx_quant<F>(yv[q], ymax, a.nq1);
                    unc += (yc > 0 ? 0 : 1) != (cvec ? cvec[v] < 0 : 0);
                    app[v] = (AT)min(max(yc, -A), A);
                    if (a.ycode_out) a.ycode_out[(size_t)b * N + v] = (int8_t)yc;
                }
            }
        }
        for (int n = lane; n < M; n += 64) {   // every c2v = 0
            S0[n] = 0u;
            if (hi) S1[n] = 0u;
            MG[n] = (MGT)0;
        }
        fx_wave_sync();   // the start wrote by groups of 4 bits and by row, the layers read by row and edge

        int it = 0;
        bool fail = false;
        for (;;) {
            if (a.early_stop || it == T) {
                // ---- syndrome of the decisions ----
                int f = 0;
                for (int n = lane; n < M; n += 64) {
                    const int deg = STAGE ? (int)gd[n] : (int)sc.deg[n];
                    uint32_t p = 0;
                    for (int k0 = 0; k0 < deg; k0 += 4) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const uint32_t dbit = app[bit_of(min(k0 + q, deg - 1), n)] <= 0 ? 1u : 0u;
                            p ^= k0 + q < deg ? dbit : 0u;
                        }
                    }
                    f |= (int)(p & 1u);
                }
                fail = __builtin_amdgcn_ballot_w64(f != 0) != 0;
                if (!fail || it == T) break;   // uniform over the wave
            }
            // ---- the layers, serially; the rows of a layer over the lanes ----
            for (int l = 0; l < sc.nlayers; ++l) {
                const int n1 = sc.lptr[l + 1];
                for (int n = sc.lptr[l] + lane; n < n1; n += 64) {
                    const uint32_t r = LDPC_CHK((uint32_t)n, (uint32_t)M, CHK_FXLMS_ROW);
                    const int deg = STAGE ? (int)gd[r] : (int)sc.deg[r];
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
                    int m1 = V, m2 = V, pos = 63;
                    uint64_t neg = 0;
                    auto reduce = [&](int k0, const int (&x)[4]) {   // edges past the row count as +V
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
                    };
                    // the first eight edges stay in registers between the minima and the APPs back
                    int xa[4], xb[4];
                    uint32_t ba[4], bb[4];
                    gather(0, xa, ba);
                    reduce(0, xa);
                    if (deg > 4) {
                        gather(4, xb, bb);
                        reduce(4, xb);
                    }
                    for (int k0 = 8; k0 < deg; k0 += 4) {
                        int x[4];
                        uint32_t bi[4];
                        gather(k0, x, bi);
                        reduce(k0, x);
                    }
                    if (variant == V_NMS) {
                        m1 = (m1 * num) >> shift;
                        m2 = (m2 * num) >> shift;
                    } else if (variant == V_OMS) {
                        m1 = max(m1 - beta, 0);
                        m2 = max(m2 - beta, 0);
                    }
                    if (__popcll(neg) & 1) neg ^= (1ull << deg) - 1ull;   // P sgn(x_k) < 0, on the row's edges
                    auto scatter = [&](int k0, const int (&x)[4], const uint32_t (&bi)[4]) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int k = k0 + q, mag = k == pos ? m2 : m1;
                            const int c = ((neg >> k) & 1u) ? -mag : mag;
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
                    S0[r] = (uint32_t)(neg & 0x3ffffffu) | ((uint32_t)pos << 26);
                    if (hi) S1[r] = (uint32_t)(neg >> 26);
                    MG[r] = (MGT)((uint32_t)m1 | ((uint32_t)m2 << MSH));
                }
                fx_wave_sync();   // the next layer gathers what this one scattered
            }
            ++it;
        }
        // ---- the frame's result ----
        int errs = 0;
        for (int v = lane; v < N; v += 64) {
            const int dbit = app[v] <= 0 ? 1 : 0;
            errs += dbit != (cvec ? cvec[v] < 0 : 0);
            if (a.d_out) a.d_out[(size_t)b * N + v] = dbit ? -1 : 1;
        }
        errs = fx_wave_sum(errs);
        unc = fx_wave_sum(unc);
        if (lane == 0)
            frame_account(a.counts, a.hist, a.frame_res, b, errs, unc, fail, a.early_stop ? it : T, a.early_stop ? it : 0);
        fx_wave_sync();   // the next codeword's front end rewrites the APPs
        b = (int)__shfl((int)nxt, 0, 64);
        if (lane == 0 && b < a.batch) nxt = gridDim.x * upb + atomicAdd(a.ticket, 1u);
    }
}

LDPC_CHECK_TU(fxlms)

// Codewords (waves) a CU holds with `gb` bytes of schedule in every workgroup, and the waves per
// workgroup that reach it: up to 16 waves per workgroup and 32 per CU; each workgroup carries
// 128 bytes of slack. A tie goes to the larger workgroup, which stages the schedule fewer times.
static int fxlms_waves(int gb, int total, int &best_c)
{
    int best_w = 0;
    best_c = 0;
    for (int c = 1; c <= 16; ++c) {
        const size_t wg = (size_t)gb + (size_t)total * c + 128;
        if (wg > kMaxLds) break;
        const int w = std::min((int)(kMaxLds / wg) * c, 32);
        if (w >= best_w) {
            best_w = w;
            best_c = c;
        }
    }
    return best_w;
}

// The schedule goes into LDS when its indices fit 16 bits and the copy costs at most a quarter
// of the waves a CU would hold without it (the kernel hides LDS and instruction latency with
// resident waves only).
FxlmsChoice fxlms_choose(const FxlmsSched &sc, int app_bits)
{
    FxlmsChoice ch;
    ch.wide = app_bits > 8;
    const FxlmsLayout L = fxlms_layout(sc, ch.wide);
    ch.cw_bytes = L.total;
    if (L.total > kFxlmsMaxLds) return ch;   // name stays empty: the caller reports the bound
    int cu = 0, cs = 0;
    const int wu = fxlms_waves(0, L.total, cu);
    const int ws = sc.N <= 65535 && L.cwoff < (int)kMaxLds ? fxlms_waves(L.cwoff, L.total, cs) : 0;
    ch.staged = ws > 0 && 4 * ws >= 3 * wu;
    const int gb = ch.staged ? L.cwoff : 0;
    ch.name = ch.wide ? "fxlms_i16" : "fxlms_i8";
    ch.cw_per_block = ch.staged ? cs : cu;
    ch.threads = 64 * ch.cw_per_block;
    ch.lds_bytes = gb + L.total * ch.cw_per_block;
    return ch;
}

template <typename F, typename AT, int SRC, bool STAGE>
static hipError_t fxlms_launch_w(const FxlmsSched &sc, const FxlmsArgs &a, const FxlmsChoice &ch, int num_cus, hipStream_t s)
{
    const FxlmsLayout L = fxlms_layout(sc, ch.wide);
    auto fn = k_fxlms<F, AT, SRC, STAGE>;
    int per_cu = occupancy(reinterpret_cast<const void *>(fn), ch.threads, ch.lds_bytes);   // raises the LDS limit
    if (per_cu < 1) per_cu = 1;
    int grid = per_cu * (num_cus > 0 ? num_cus : 1);
    const int need = (a.batch + ch.cw_per_block - 1) / ch.cw_per_block;
    if (grid > need) grid = need;
    hipLaunchKernelGGL(fn, dim3(grid), dim3(ch.threads), ch.lds_bytes, s, a, sc, L);
    return hipGetLastError();
}

hipError_t fxlms_launch(const FxlmsSched &sc, const FxlmsArgs &a, bool f64, const FxlmsChoice &ch, int num_cus,
                        hipStream_t s)
{
    if (a.batch <= 0) return hipSuccess;
    if (!a.ticket || !sc.lptr || ch.cw_per_block < 1 || (size_t)ch.lds_bytes > kMaxLds) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(a.ticket, 0, sizeof(unsigned), s);
    if (e != hipSuccess) return e;
    return for_f_src(f64, a.src, [&](auto f, auto src) {
        using F = typename decltype(f)::type;
        constexpr int SRC = decltype(src)::value;
        if (ch.wide)
            return ch.staged ? fxlms_launch_w<F, int16_t, SRC, true>(sc, a, ch, num_cus, s)
                             : fxlms_launch_w<F, int16_t, SRC, false>(sc, a, ch, num_cus, s);
        return ch.staged ? fxlms_launch_w<F, int8_t, SRC, true>(sc, a, ch, num_cus, s)
                         : fxlms_launch_w<F, int8_t, SRC, false>(sc, a, ch, num_cus, s);
    });
}

}  // namespace ldpc
