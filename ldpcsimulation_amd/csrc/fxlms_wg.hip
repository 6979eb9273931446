// fxlms_wg.hip -- layered fixed-point min-sum (fxlms.hip has the definition) for codes whose
// state does not fit the 64 KiB a wavefront's codeword may take: a workgroup per codeword
// (DESIGN §13i). The arithmetic is k_fxlms's -- the same front end (fx_front.h), the same row
// update over the same packed row state (fxl_row below), the same row order -- so a frame's
// result depends on the frame and the cfg only, not on the kernel.
//
// State of a codeword (fxlms_layout.h): in LDS, behind kFxlmsWgRed bytes of reduction and
// ticket words, app[N]; in the workgroup's global slot the packed row state S0[M] | S1[M]
// (row degree > 26 only) | MG[M], indexed by layered position. A thread owns rows
// lptr[l] + tid, + blockDim.x, ... of layer l, in every iteration and for every codeword of
// the workgroup: a state word is read and written by one thread only, consecutive threads
// touch consecutive words, and the slot needs no ordering between threads. The schedule comes
// from the device copy through the caches, as in k_fxlms<..., STAGE = false>.
//
// Every barrier below is reached by every thread of the workgroup: no barrier stands inside a
// loop whose trip count depends on the thread, and each loop that holds one says why its
// bounds are the same in all threads.
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

// The update of the row at layered position r, of deg > 0 edges; bit_of(k, r) is the bit of its
// edge k. This is the text of k_fxlms's row loop (fxlms.hip), which keeps its own: as one
// function under both kernels it moved k_fxlms's registers (93 -> 86 and 95 -> 99 VGPRs, the
// latter a wave per SIMD fewer; profiles/wave_cw_resources.md).
template <typename AT, typename Args, typename Bit>
__device__ __forceinline__ void fxl_row(const Args &a, AT *app, uint32_t *S0, uint32_t *S1, typename fxl_mag<AT>::type *MG,
                                        bool hi, uint32_t r, int deg, int V, int A, Bit &&bit_of)
{
    using MGT = typename fxl_mag<AT>::type;
    constexpr int MSH = fxl_mag<AT>::shift;
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

struct FxlmsWgSlots {
    unsigned char *base;   // [nslots] slots of slot_bytes
    size_t slot_bytes;
    int nslots, s1off, mgoff, hi;
};

// words of the LDS scratch (kFxlmsWgRed bytes)
constexpr int kWgSums = 0, kWgFlags = 32, kWgNext = 48;
static_assert((kWgNext + 1) * 4 <= kFxlmsWgRed, "the scratch words fit");

// Whether x is non-zero in any thread; the same value in every thread. Two barriers: the first
// ends the reads of the last use.
__device__ __forceinline__ bool wg_any(int x, int *flags)
{
    const bool w = wave_any(x);
    const int nw = (int)((blockDim.x + 63) >> 6);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) flags[threadIdx.x >> 6] = w ? 1 : 0;
    __syncthreads();
    int r = 0;
    for (int i = 0; i < nw; ++i) r |= flags[i];
    return r != 0;
}

template <typename F, typename AT, int SRC>
__global__ __launch_bounds__(1024) void k_fxlms_wg(FxlmsArgs a, FxlmsSched sc, FxlmsWgSlots w)
{
    using MGT = typename fxl_mag<AT>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int *red = reinterpret_cast<int *>(smem);
    AT *app = reinterpret_cast<AT *>(smem + kFxlmsWgRed);
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
    const int N = sc.N, M = sc.M, T = a.T, V = a.vmax, A = a.amax;
    const bool hi = w.hi != 0;
    [[maybe_unused]] const uint32_t slots = (uint32_t)sc.dcs * (uint32_t)M;   // the bound of LDPC_CHK
    unsigned char *slot = w.base + (size_t)LDPC_CHK((uint32_t)blockIdx.x, (uint32_t)w.nslots, CHK_FXLMS_WG_SLOT) * w.slot_bytes;
    uint32_t *S0 = reinterpret_cast<uint32_t *>(slot);
    uint32_t *S1 = reinterpret_cast<uint32_t *>(slot + w.s1off);
    MGT *MG = reinterpret_cast<MGT *>(slot + w.mgoff);
    // bit of edge k of the row at layered position n
    auto bit_of = [&](int k, int n) -> uint32_t {
        const uint32_t e = LDPC_CHK((uint32_t)(k * M + n), slots, CHK_FXLMS_WG_SCHED);
        return LDPC_CHK((uint32_t)sc.cols[e], (uint32_t)N, CHK_FXLMS_WG_BIT);
    };
    auto dec_of = [&](uint32_t i) __attribute__((always_inline)) { return app[i] <= 0 ? 1u : 0u; };
    auto deg_of = [&](uint32_t n) __attribute__((always_inline)) { return (int)sc.deg[n]; };

    CwTickets tk(a.ticket, a.batch, 1, tid == 0);
    // b is the same in every thread: the workgroup's index first, then the drawer's ticket
    // through LDS, read after a barrier; so every thread runs this loop equally often.
    for (int b = tk.first(0); b < a.batch;) {
        const int8_t *cvec = frame_codeword<SRC>(a, b, N);
        // the start's APPs
        int unc = fx_front_end<F, SRC>(
            a, b, N, tid, cvec, [&](int v, int yc) __attribute__((always_inline)) { app[v] = (AT)min(max(yc, -A), A); }, nt);
        // every c2v = 0, each thread its own rows. nlayers and lptr are kernel arguments' data:
        // the outer loop is uniform and holds no barrier anyway.
        for (int l = 0; l < sc.nlayers; ++l) {
            const int n1 = sc.lptr[l + 1];
            for (int n = sc.lptr[l] + tid; n < n1; n += nt) {
                const uint32_t r = LDPC_CHK((uint32_t)n, (uint32_t)M, CHK_FXLMS_WG_ROW);
                S0[r] = 0u;
                if (hi) S1[r] = 0u;
                MG[r] = (MGT)0;
            }
        }
        __syncthreads();   // the start wrote by groups of 4 bits, the layers and the syndrome read by row and edge

        int it = 0;
        bool fail = false;
        // Uniform: `it` counts alike in every thread, T and early_stop are kernel arguments, and
        // `fail` is wg_any's value, the same in every thread; so all threads leave together.
        for (;;) {
            if (a.early_stop || it == T) {
                fail = wg_any(fx_syndrome_part(M, tid, nt, deg_of, bit_of, dec_of), red + kWgFlags);
                if (!fail || it == T) break;
            }
            // ---- the layers, serially; the rows of a layer over the threads ----
            // Uniform: nlayers is a kernel argument; the barrier stands outside the row loop,
            // whose trip count is the thread's own.
            for (int l = 0; l < sc.nlayers; ++l) {
                const int n1 = sc.lptr[l + 1];
                for (int n = sc.lptr[l] + tid; n < n1; n += nt) {
                    const uint32_t r = LDPC_CHK((uint32_t)n, (uint32_t)M, CHK_FXLMS_WG_ROW);
                    const int deg = deg_of(r);
                    if (deg == 0) continue;
                    fxl_row<AT>(a, app, S0, S1, MG, hi, r, deg, V, A, bit_of);
                }
                __syncthreads();   // the next layer gathers what this one scattered
            }
            ++it;
        }
        // ---- the frame's result: sums over the workgroup, in its first thread ----
        int sums[2] = {fx_decisions_out(a, b, N, tid, cvec, dec_of, nt), unc};
        block_sum_n_t0<2>(sums, red + kWgSums);
        if (tid == 0) {
            fx_frame_account(a, b, sums[0], sums[1], fail, it);
            red[kWgNext] = (int)tk.nxt;   // the drawer hands its ticket to the workgroup
        }
        __syncthreads();   // also ends the codeword: the next one's front end rewrites the APPs
        b = tk.redraw(red[kWgNext]);   // rewritten only after the next codeword's barriers
    }
}

LDPC_CHECK_TU(fxlms_wg)

FxlmsChoice fxlms_wg_choose(const FxlmsSched &sc, int app_bits) { return fxlms_wg_plan({sc.N, sc.M, sc.dcs, 0}, app_bits); }

using FxlmsWgFn = void (*)(FxlmsArgs, FxlmsSched, FxlmsWgSlots);
static FxlmsWgFn fxlms_wg_fn(bool f64, int src, bool wide)
{
    return for_f_src(f64, src, [&](auto f, auto s) -> FxlmsWgFn {
        using F = typename decltype(f)::type;
        constexpr int SRC = decltype(s)::value;
        return wide ? k_fxlms_wg<F, int16_t, SRC> : k_fxlms_wg<F, int8_t, SRC>;
    });
}

int fxlms_wg_grid(const FxlmsArgs &a, bool f64, const FxlmsChoice &ch, int num_cus)
{
    if (a.batch <= 0 || ch.threads < 64 || (size_t)ch.lds_bytes > kMaxLds) return 0;
    int per_cu = occupancy(reinterpret_cast<const void *>(fxlms_wg_fn(f64, a.src, ch.wide)), ch.threads, ch.lds_bytes);   // raises the LDS limit
    if (per_cu < 1) per_cu = 1;
    const long long grid = (long long)per_cu * (num_cus > 0 ? num_cus : 1);
    return grid < a.batch ? (int)grid : a.batch;
}

hipError_t fxlms_wg_launch(const FxlmsSched &sc, const FxlmsArgs &a, bool f64, const FxlmsChoice &ch, void *scratch, int grid,
                           hipStream_t s)
{
    if (a.batch <= 0) return hipSuccess;
    if (!sc.lptr || !a.ticket || !scratch || grid < 1 || grid > a.batch || !ch.wg || (size_t)ch.lds_bytes > kMaxLds)
        return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(a.ticket, 0, sizeof(unsigned), s);
    if (e != hipSuccess) return e;
    const FxlmsWgLayout L = fxlms_wg_layout({sc.N, sc.M, sc.dcs, 0}, ch.wide);
    const FxlmsWgSlots w{(unsigned char *)scratch, (size_t)ch.slot_bytes, grid, L.s1off, L.mgoff, L.hi};
    hipLaunchKernelGGL(fxlms_wg_fn(f64, a.src, ch.wide), dim3(grid), dim3(ch.threads), ch.lds_bytes, s, a, sc, w);
    return hipGetLastError();
}

}  // namespace ldpc
