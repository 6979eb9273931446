// rgdbf.hip -- CDNA4 (gfx950) kernels of the re-decoding NGDBF decoder
// (src/RNGDBF.cpp built as decodeRSMNGDBF: -D redecode -D addNoise
// -D thresholdAdaptation -D weightSyndromes -D outputSmoothing -D saturateSamples).
//
// A frame is decoded in up to `maxphase` phases (:277-400). Every phase starts
// from the channel hard decision r with theta_i = theta and dsum = 0 and runs up
// to T parallel-flip iterations of decodeGDBF (gdbf.hip):
//   check nodes  s_j = prod_k d_k over mlist[j]; the phase stops when every
//                s_j = +1 (checkNodeUpdates :533-550)
//   bit nodes    E_i = d_i*y_i + sum_j w_i*s_j (nlist order) [+ perturbation]
//                with the per-bit weight w_i = alpha*Ymax/dv_i (:564-567; 1 without
//                WEIGHT); flip d_i when E_i < theta_i, else theta_i *= lambda
//   smoothing    dsum += d when it > T - windowsize; a phase that ended
//                unsatisfied outputs sgn(dsum) (:373-382)
// The phase loop ends after a satisfied phase; the frame's output and error weight
// are the last phase's, its iteration count the sum over its phases (:394). A failed
// phase runs exactly T iterations, so the host derives the phase count from it.
// The perturbation of iteration `it` of phase `ph` is row ph*T + it: given by the
// caller as pert[frame][ph*T + it][bit], or Philox4x32-10 at stream word
// stream_id | (ph*T + it + 1) << 20 -- phase 0 draws what gdbf.hip draws.
// Compiled with -ffp-contract=off; E keeps the reference's operation order, and
// w_i*(+-1) is exactly +-w_i, so the kernels select the sign instead of multiplying.
#include "rgdbf.h"
#include "rgdbf_shared.h"
#include "gdbf_front.h"
#include "frame.h"
#include "minsum_common.h"

#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>

namespace ldpc {

// The per-bit weight (rgdbf_weight, rgdbf_term, the LDS table of weights by degree) and the
// state layout of a codeword are in rgdbf_shared.h, shared with rstat.hip.

// ---------------------------------------------------------------------
// Generic kernels: one workgroup per codeword, its state in LDS (rgdbf_lds) or in
// a global slot (rgdbf_global), as gdbf_lds / gdbf_global.
// ---------------------------------------------------------------------
template <typename F, int SRC>
__device__ __forceinline__ void rgdbf_codeword(const RgdbfArgs &a, const DevGraph &g, int b, F *yq, F *theta,
                                               int16_t *dsum, int8_t *d, int8_t *r8, int8_t *s, int *red,
                                               const F *wtab)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    const int N = g.N, M = g.M, T = a.T;
    const uint64_t cw = a.first_cw + (uint64_t)b;
    const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
    const int8_t *cvec = frame_codeword<SRC>(a, b, N);
    const bool smooth = (a.flags & GDBF_SMOOTH) != 0;
    // ---- channel + front-end (:252-275) ----
    int unc = 0;
    for (int g4 = tid; g4 * 4 < N; g4 += nt) {
        F yv[4];
        channel_group<F, SRC, true>(a, b, g4, N, cvec, nullptr, yv);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int v = g4 * 4 + q;
            if (v < N) {
                int r;
                yq[v] = gdbf_front<F>(yv[q], a, r);
                const int cv = cvec ? cvec[v] : 1;
                unc += (r * cv < 0);
                r8[v] = (int8_t)r;
            }
        }
    }
    const F lambda = (F)a.lambda, nsig = (F)a.noise_sigma;
    int it = 0, total = 0;
    bool sat = false;
    for (int ph = 0; ph < a.maxphase; ++ph) {
        // ---- restart from r (:282-288, :303-306); each thread its own bits ----
        for (int g4 = tid; g4 * 4 < N; g4 += nt)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int v = g4 * 4 + q;
                if (v < N) {
                    d[v] = r8[v];
                    theta[v] = (F)a.theta0;
                    dsum[v] = 0;
                }
            }
        __syncthreads();
        for (it = 0; it < T; ++it) {
            const int gi = ph * T + it;   // the perturbation row
            // ---- check nodes (:533-550) ----
            int fail = 0;
            for (int j = tid; j < M; j += nt) {
                const int deg = g.row_deg[j];
                const int32_t *rc = g.row_cols + (size_t)j * g.dcs;
                int p = 0;
                for (int k = 0; k < deg; ++k) p ^= d[rc[k]] < 0;
                s[j] = (int8_t)p;
                fail |= p;
            }
            sat = !__syncthreads_or(fail);
            if (sat) break;   // :320-321, uniform over the workgroup
            // ---- bit nodes (:552-) ----
            const bool acc_smooth = smooth && it > T - a.windowsize;   // :364
            for (int g4 = tid; g4 * 4 < N; g4 += nt) {
                F pv[4] = {F(0), F(0), F(0), F(0)};
                if (a.flags & GDBF_NOISE) {
                    if (SRC == SRC_GIVEN) {
                        const F *pr = reinterpret_cast<const F *>(a.pert) +
                                      ((size_t)b * ((size_t)a.maxphase * T) + gi) * N;
#pragma unroll
                        for (int q = 0; q < 4; ++q) pv[q] = (g4 * 4 + q < N) ? pr[g4 * 4 + q] : F(0);
                    } else {
                        uint32_t u[4];
                        philox4x32_10<true>((uint32_t)g4, (uint32_t)cw, (uint32_t)(cw >> 32),
                                            (a.stream_id & 0xFFFFFu) | ((uint32_t)(gi + 1) << 20), k0, k1, u);
                        float n[4];
                        box_muller_hw(u[0], u[1], n[0], n[1]);
                        box_muller_hw(u[2], u[3], n[2], n[3]);
#pragma unroll
                        for (int q = 0; q < 4; ++q) pv[q] = nsig * (F)n[q];
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int i = g4 * 4 + q;
                    if (i >= N) break;
                    const int di = d[i];
                    F E = (F)di * yq[i];
                    const int e0 = g.col_ptr[i], e1 = g.col_ptr[i + 1];
                    const int deg = e1 - e0;
                    const F w = deg < kRgdbfWtab ? wtab[deg] : rgdbf_weight<F>(a, deg);
                    for (int e = e0; e < e1; ++e) E += s[g.col_refs[e] >> 6] ? -w : w;   // w_i * s_j
                    if (a.flags & GDBF_NOISE) E += pv[q];
                    const bool flip = E < theta[i];
                    const int dn = flip ? -di : di;
                    if (flip) d[i] = (int8_t)dn;
                    if ((a.flags & GDBF_ADAPT) && !flip) theta[i] *= lambda;
                    if (acc_smooth) dsum[i] = (int16_t)(dsum[i] + dn);
                }
            }
            __syncthreads();
        }
        total += it;   // :394
        if (sat) break;   // :398-399
    }
    if (smooth && !sat)   // :373-382, of the last phase
        for (int g4 = tid; g4 * 4 < N; g4 += nt)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (g4 * 4 + q < N) d[g4 * 4 + q] = dsum[g4 * 4 + q] > 0 ? 1 : -1;
    __syncthreads();

    // ---- error weight (:393), syndrome of the output, accounting ----
    int wgt = 0, synd = 0;
    for (int v = tid; v < N; v += nt) {
        const int dv = d[v];
        const int cv = cvec ? cvec[v] : 1;
        wgt += (dv != cv);
        if (a.d_out) a.d_out[(size_t)b * N + v] = (int8_t)dv;
    }
    for (int j = tid; j < M; j += nt) {
        const int deg = g.row_deg[j];
        const int32_t *rc = g.row_cols + (size_t)j * g.dcs;
        int p = 0;
        for (int k = 0; k < deg; ++k) p ^= d[rc[k]] < 0;
        synd |= p;
    }
    int sums[3] = {wgt, unc, synd};
    block_sum_n_t0<3>(sums, red);
    if (tid == 0) frame_account(a.counts, a.hist, a.frame_res, b, sums[0], sums[1], sums[2] > 0, total, total);
    __syncthreads();
}

template <typename F, int SRC>
__global__ __launch_bounds__(256) void k_rgdbf_lds(RgdbfArgs a, DevGraph g, RgdbfLayout L)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int red[16 * 4];
    __shared__ F wtab[kRgdbfWtab];
    rgdbf_fill_wtab<F>(a, wtab);
    rgdbf_codeword<F, SRC>(a, g, blockIdx.x, reinterpret_cast<F *>(smem), reinterpret_cast<F *>(smem + L.theta),
                           reinterpret_cast<int16_t *>(smem + L.dsum), reinterpret_cast<int8_t *>(smem + L.d),
                           reinterpret_cast<int8_t *>(smem + L.r), reinterpret_cast<int8_t *>(smem + L.s), red, wtab);
}

template <typename F, int SRC>
__global__ __launch_bounds__(1024) void k_rgdbf_global(RgdbfArgs a, DevGraph g, RgdbfLayout L, unsigned char *scratch)
{
    __shared__ int red[16 * 4];
    __shared__ F wtab[kRgdbfWtab];
    rgdbf_fill_wtab<F>(a, wtab);
    unsigned char *base = scratch + L.total * blockIdx.x;
    for (int b = blockIdx.x; b < a.batch; b += gridDim.x)
        rgdbf_codeword<F, SRC>(a, g, b, reinterpret_cast<F *>(base), reinterpret_cast<F *>(base + L.theta),
                               reinterpret_cast<int16_t *>(base + L.dsum), reinterpret_cast<int8_t *>(base + L.d),
                               reinterpret_cast<int8_t *>(base + L.r), reinterpret_cast<int8_t *>(base + L.s), red,
                               wtab);
}

// ---------------------------------------------------------------------
// rgdbf_rows: codes with N <= 4 * 1024, row degree <= 8 and column degree <= 12
// (those gdbf_rows takes). Ownership as in gdbf_rows: thread t owns the Philox group
// of bits 4t..4t+3 and rows t and t + blockDim; the graph sits in registers as packed
// 16-bit words; yq, theta, dsum, d and r of the thread's bits stay in registers; the
// workgroup is persistent and takes codewords by ticket (a failing frame costs up to
// maxphase * T iterations, most frames a handful). What differs is what a check
// leaves in LDS: one parity byte (1: s_j = -1), not the term w * s_j, because the
// weight belongs to the bit. A bit computes its w_i once per workgroup (double, then
// rounded to F) and adds w_i with its sign bit flipped by the parity byte; an edge
// beyond the lane's own degree reads a dummy byte (1) and takes the weight 0 by a select
// on the lane's degree, so it adds -0.0 (E + -0.0 == E for every E). LDS per codeword: the d < 0 flag bytes, the parity bytes and the
// double-buffered early-stop flag -- about N + M bytes.
// The parity bytes are indexed by the plain check number: the lanes of a bit slot
// read checks j0 + 4t (bits 4t + q of a quasi-cyclic block), which as bytes are the
// consecutive dwords j0/4 + t -- 32 lanes, 32 banks -- so gdbf_rows' pad word per 32
// checks (its F terms at stride 4 were 4-way conflicts) has nothing to remove here.
// The phase loop is inside the codeword: a restart is a register copy, one flag
// store and one barrier; the early-stop flag alternates on the perturbation row
// ph * T + it, which keeps alternating across a restart for odd and even T.
// ---------------------------------------------------------------------
// RgdbfRowsLayout / rgdbf_rows_layout: rgdbf_shared.h.
// Every instance is bounded to 4 waves per SIMD (128 VGPRs): at gdbf_rows' 6 the fp32
// 512-thread instances spilled 16 to 128 bytes per lane (r, the weights and the degrees
// are registers gdbf_rows does not hold).
template <typename F, int SRC, int DVM, int NT>
__global__ __launch_bounds__(NT, 4) void k_rgdbf_rows(RgdbfArgs a, DevGraph g, int np, int poff, int floff)
{
    constexpr int DC = 8, BPT = 4, RPT = 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int red[16 * 4 + 1];                    // block sums; [64]: the next codeword
    uint8_t *dl = smem;                                // 1 where d = -1
    uint8_t *pl = smem + poff;                         // 1 where s_j = -1
    volatile int *fl = reinterpret_cast<int *>(smem + floff);
    const int tid = threadIdx.x;
    const int N = g.N, M = g.M, T = a.T;
    const int dbit = np - 1;              // dummy bit index
    const int v0 = BPT * tid;             // the thread's first bit
    const int g4 = tid;                   // its Philox group
    // ---- the graph, into registers (once per workgroup) ----
    uint32_t rc[RPT][DC / 2];
    bool rvalid[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const int j = tid + r * NT;
        rvalid[r] = j < M;
        const int deg = rvalid[r] ? g.row_deg[j] : 0;
#pragma unroll
        for (int k = 0; k < DC; k += 2) {
            const uint32_t c0 = k < deg ? (uint32_t)g.row_cols[(size_t)j * g.dcs + k] : (uint32_t)dbit;
            const uint32_t c1 = k + 1 < deg ? (uint32_t)g.row_cols[(size_t)j * g.dcs + k + 1] : (uint32_t)dbit;
            rc[r][k / 2] = c0 | (c1 << 16);
        }
    }
    const bool own = v0 < N;
    uint32_t bc[BPT][DVM / 2];
    int wdeg[BPT];        // wave-uniform bound of each slot's degree
    uint32_t degs = 0;    // the lane's own degrees, 4 bits per slot
    F wq[BPT];            // w_i of the thread's bits
#pragma unroll
    for (int q = 0; q < BPT; ++q) {
        const int i = v0 + q;
        int e0 = 0, deg = 0;
        if (i < N) {
            e0 = g.col_ptr[i];
            deg = g.col_ptr[i + 1] - e0;
        }
#pragma unroll
        for (int k = 0; k < DVM; k += 2) {
            const uint32_t j0 = k < deg ? g.col_refs[e0 + k] >> 6 : (uint32_t)M;
            const uint32_t j1 = k + 1 < deg ? g.col_refs[e0 + k + 1] >> 6 : (uint32_t)M;
            bc[q][k / 2] = j0 | (j1 << 16);
        }
        degs |= (uint32_t)deg << (4 * q);
        wq[q] = rgdbf_weight<F>(a, deg);
        int m = deg;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o, 64));
        wdeg[q] = __builtin_amdgcn_readfirstlane(m);
    }
    if (tid == 0) {
        *reinterpret_cast<uint32_t *>(dl + np - 4) = 0u;   // dummy bits: d = +1
        pl[M] = 1;                                          // dummy check: a padding edge adds 0 * s = -0.0
    }
    const bool smooth = (a.flags & GDBF_SMOOTH) != 0, noise = (a.flags & GDBF_NOISE) != 0;
    const bool adapt = (a.flags & GDBF_ADAPT) != 0;
    const F lambda = (F)a.lambda, nsig = (F)a.noise_sigma;
    const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);

    // Codewords: blockIdx.x first, then tickets from a.ticket; thread 0 draws the next
    // ticket while the current codeword decodes.
    unsigned nxt = 0;
    if (tid == 0) nxt = gridDim.x + atomicAdd(a.ticket, 1u);
    for (int b = blockIdx.x; b < a.batch;) {
        const uint64_t cw = a.first_cw + (uint64_t)b;
        const int8_t *cvec = frame_codeword<SRC>(a, b, N);
        // ---- channel + front-end (:252-275) ----
        F yq[BPT], theta[BPT];
        int d[BPT], dsum[BPT];
        uint32_t rneg = 0;   // bit q: r = -1
        int unc = 0;
#pragma unroll
        for (int q = 0; q < BPT; ++q) yq[q] = F(0);
        if (own) {
            F yv[BPT];
            channel_group<F, SRC, true>(a, b, g4, N, cvec, nullptr, yv);
#pragma unroll
            for (int q = 0; q < BPT; ++q) {
                const int v = v0 + q;
                if (v < N) {
                    int r;
                    yq[q] = gdbf_front<F>(yv[q], a, r);
                    const int cv = cvec ? cvec[v] : 1;
                    unc += (r * cv < 0);
                    rneg |= (uint32_t)(r < 0) << q;
                }
            }
        }
        auto put_d = [&]() {
            if (own)
                *reinterpret_cast<uint32_t *>(dl + v0) = (uint32_t)(d[0] < 0) | ((uint32_t)(d[1] < 0) << 8) |
                                                         ((uint32_t)(d[2] < 0) << 16) | ((uint32_t)(d[3] < 0) << 24);
        };
        if (tid == 0) {
            fl[0] = 0;
            fl[1] = 0;
        }

        int it = 0, total = 0;
        bool sat = false;
        for (int ph = 0; ph < a.maxphase; ++ph) {
            // ---- restart from r (:282-288, :303-306) ----
#pragma unroll
            for (int q = 0; q < BPT; ++q) {
                d[q] = (rneg >> q) & 1u ? -1 : 1;
                theta[q] = (F)a.theta0;
                dsum[q] = 0;
            }
            put_d();
            __syncthreads();
            for (it = 0; it < T; ++it) {
                const int gi = ph * T + it;   // the perturbation row; its parity picks the stop flag
                // the packed 16-bit schedule words are opaque per iteration: otherwise the
                // compiler hoists the unpacked indices out of the loop and spills them
#pragma unroll
                for (int r = 0; r < RPT; ++r)
#pragma unroll
                    for (int k = 0; k < DC / 2; ++k) asm volatile("" : "+v"(rc[r][k]));
#pragma unroll
                for (int q = 0; q < BPT; ++q)
#pragma unroll
                    for (int k = 0; k < DVM / 2; ++k) asm volatile("" : "+v"(bc[q][k]));
                asm volatile("" : "+v"(degs));   // likewise the per-edge masked weights derived from it
                // ---- check nodes (:533-550) ----
                uint32_t g8[RPT][DC];
#pragma unroll
                for (int r = 0; r < RPT; ++r)
#pragma unroll
                    for (int k = 0; k < DC; ++k)
                        g8[r][k] = dl[LDPC_CHK((rc[r][k / 2] >> (16 * (k & 1))) & 0xffffu, (uint32_t)np, CHK_RGDBF_BIT)];
                int fail = 0;
#pragma unroll
                for (int r = 0; r < RPT; ++r) {
                    uint32_t p = 0;
#pragma unroll
                    for (int k = 0; k < DC; ++k) p ^= g8[r][k];
                    if (rvalid[r]) pl[LDPC_CHK(tid + r * NT, (uint32_t)M + 1u, CHK_RGDBF_PARITY)] = (uint8_t)p;
                    fail |= (int)p;
                }
                if (fail) fl[gi & 1] = 1;
                __syncthreads();
                sat = fl[gi & 1] == 0;   // :320-321, uniform over the workgroup
                if (sat) break;
                if (tid == 0) fl[(gi + 1) & 1] = 0;   // nobody reads or sets it before the next barrier
                // the perturbations, only in an iteration that passed the check (:333-348)
                F pv[BPT];
#pragma unroll
                for (int q = 0; q < BPT; ++q) pv[q] = F(0);
                if (noise && own) {
                    if (SRC == SRC_GIVEN) {
                        const F *pr = reinterpret_cast<const F *>(a.pert) +
                                      ((size_t)b * ((size_t)a.maxphase * T) + gi) * N;
#pragma unroll
                        for (int q = 0; q < BPT; ++q) pv[q] = (v0 + q < N) ? pr[v0 + q] : F(0);
                    } else {
                        uint32_t u[4];
                        philox4x32_10<true>((uint32_t)g4, (uint32_t)cw, (uint32_t)(cw >> 32),
                                            (a.stream_id & 0xFFFFFu) | ((uint32_t)(gi + 1) << 20), k0, k1, u);
                        float n[4];
                        box_muller_hw(u[0], u[1], n[0], n[1]);
                        box_muller_hw(u[2], u[3], n[2], n[3]);
#pragma unroll
                        for (int q = 0; q < BPT; ++q) pv[q] = nsig * (F)n[q];
                    }
                }
                // ---- bit nodes (:552-), mu = 1 ----
                const bool acc_smooth = smooth && it > T - a.windowsize;   // :364
#pragma unroll
                for (int q = 0; q < BPT; ++q) {
                    // all of the slot's parity reads first (one LDS round trip), up to the
                    // wave's largest degree; the adds keep nlist order, and an edge beyond
                    // this lane's degree adds -0.0
                    constexpr int K0 = DVM < 4 ? DVM : 4;
                    const int dq = (int)((degs >> (4 * q)) & 15u);
                    uint32_t sv[K0];
#pragma unroll
                    for (int k = 0; k < K0; ++k)
                        sv[k] = pl[LDPC_CHK((bc[q][k / 2] >> (16 * (k & 1))) & 0xffffu, (uint32_t)M + 1u, CHK_RGDBF_PARITY)];
                    F E = (F)d[q] * yq[q];
#pragma unroll
                    for (int k = 0; k < K0; ++k) E += rgdbf_term(k < dq ? wq[q] : F(0), sv[k]);
                    if (DVM > K0 && wdeg[q] > K0) {
                        uint32_t sw[DVM - K0 > 0 ? DVM - K0 : 1];
#pragma unroll
                        for (int k = K0; k < DVM; ++k)
                            sw[k - K0] = pl[LDPC_CHK((bc[q][k / 2] >> (16 * (k & 1))) & 0xffffu, (uint32_t)M + 1u, CHK_RGDBF_PARITY)];
#pragma unroll
                        for (int k = K0; k < DVM; ++k)
                            if (k < wdeg[q]) E += rgdbf_term(k < dq ? wq[q] : F(0), sw[k - K0]);
                    }
                    if (noise) E += pv[q];
                    const bool flip = E < theta[q];
                    const int dn = flip ? -d[q] : d[q];
                    if (adapt && !flip) theta[q] *= lambda;
                    if (acc_smooth) dsum[q] += dn;
                    d[q] = dn;
                }
#pragma unroll
                for (int q = 0; q < BPT; ++q)   // bits past N keep +1
                    if (v0 + q >= N) d[q] = 1;
                put_d();
                __syncthreads();
            }
            total += it;   // :394
            if (sat) break;   // :398-399
        }
        if (smooth && !sat) {   // :373-382, of the last phase
#pragma unroll
            for (int q = 0; q < BPT; ++q) d[q] = (v0 + q < N) ? (dsum[q] > 0 ? 1 : -1) : 1;
            put_d();
        }
        __syncthreads();

        // ---- error weight (:393), syndrome of the output, accounting ----
        int wgt = 0, synd = 0;
        if (own)
#pragma unroll
            for (int q = 0; q < BPT; ++q) {
                const int v = v0 + q;
                if (v < N) {
                    const int cv = cvec ? cvec[v] : 1;
                    wgt += (d[q] != cv);
                    if (a.d_out) a.d_out[(size_t)b * N + v] = (int8_t)d[q];
                }
            }
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
            uint32_t p = 0;
#pragma unroll
            for (int k = 0; k < DC; ++k) p ^= dl[LDPC_CHK((rc[r][k / 2] >> (16 * (k & 1))) & 0xffffu, (uint32_t)np, CHK_RGDBF_BIT)];
            synd |= (int)p;
        }
        int sums[3] = {wgt, unc, synd};
        block_sum_n_t0<3>(sums, red);
        if (tid == 0) {
            frame_account(a.counts, a.hist, a.frame_res, b, sums[0], sums[1], sums[2] > 0, total, total);
            red[64] = (int)nxt;
        }
        __syncthreads();
        b = red[64];   // rewritten only after the next codeword's barriers
        if (tid == 0 && b < a.batch) nxt = gridDim.x + atomicAdd(a.ticket, 1u);
    }
}

constexpr size_t kRgdbfMaxLds = 64 * 1024;

LDPC_CHECK_TU(rgdbf)

RgdbfChoice rgdbf_choose(const DevGraph &g, bool f64, int maxdv, int maxdc)
{
    RgdbfChoice ch;
    if (rgdbf_rows_fits(g.N, g.M, maxdv, maxdc) && opt(LDPC_OPT_GDBF_KERNEL) != 1) {
        ch.name = "rgdbf_rows";
        ch.threads = g.N <= 4 * 512 && g.M <= 2 * 512 ? 512 : 1024;
        ch.dvm = maxdv <= 4 ? 4 : 12;
        ch.lds_bytes = rgdbf_rows_layout(g.N, g.M).total;
        return ch;
    }
    const RgdbfLayout L = rgdbf_layout(g.N, g.M, f64 ? 8 : 4);
    if (L.total <= kRgdbfMaxLds) {
        ch.name = "rgdbf_lds";
        ch.lds_bytes = (int)L.total;
        ch.threads = 256;
    } else {
        ch.name = "rgdbf_global";
        ch.threads = 1024;
        ch.slot_bytes = L.total;
    }
    return ch;
}

template <typename F, int SRC, int DVM, int NT>
static hipError_t rgdbf_rows_launch_b(const DevGraph &g, const RgdbfArgs &a, int num_cus, hipStream_t s)
{
    if (!a.ticket) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(a.ticket, 0, sizeof(unsigned), s);
    if (e != hipSuccess) return e;
    const RgdbfRowsLayout L = rgdbf_rows_layout(g.N, g.M);
    auto fn = k_rgdbf_rows<F, SRC, DVM, NT>;
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, NT, L.total) != hipSuccess || per_cu < 1)
        per_cu = 1;
    int grid = per_cu * (num_cus > 0 ? num_cus : 1);
    if (grid > a.batch) grid = a.batch;
    hipLaunchKernelGGL(fn, dim3(grid), dim3(NT), L.total, s, a, g, L.np, L.poff, L.floff);
    return hipGetLastError();
}

template <typename F, int SRC>
static hipError_t rgdbf_launch_t(const DevGraph &g, const RgdbfArgs &a, const RgdbfChoice &ch, void *scratch,
                                 int slots, int num_cus, hipStream_t s)
{
    if (ch.dvm == 4)
        return ch.threads == 512 ? rgdbf_rows_launch_b<F, SRC, 4, 512>(g, a, num_cus, s)
                                 : rgdbf_rows_launch_b<F, SRC, 4, 1024>(g, a, num_cus, s);
    if (ch.dvm == 12)
        return ch.threads == 512 ? rgdbf_rows_launch_b<F, SRC, 12, 512>(g, a, num_cus, s)
                                 : rgdbf_rows_launch_b<F, SRC, 12, 1024>(g, a, num_cus, s);
    const RgdbfLayout L = rgdbf_layout(g.N, g.M, sizeof(F));
    if (ch.lds_bytes > 0) {
        hipLaunchKernelGGL((k_rgdbf_lds<F, SRC>), dim3(a.batch), dim3(ch.threads), ch.lds_bytes, s, a, g, L);
    } else {
        const int grid = slots < a.batch ? slots : a.batch;
        if (grid <= 0 || !scratch) return hipErrorInvalidValue;
        hipLaunchKernelGGL((k_rgdbf_global<F, SRC>), dim3(grid), dim3(ch.threads), 0, s, a, g, L,
                           (unsigned char *)scratch);
    }
    return hipGetLastError();
}

hipError_t rgdbf_launch(const DevGraph &g, const RgdbfArgs &a, bool f64, const RgdbfChoice &ch, void *scratch,
                        int slots, int num_cus, hipStream_t s)
{
    if (a.batch <= 0) return hipSuccess;
    if (f64)
        return a.src == SRC_GIVEN ? rgdbf_launch_t<double, SRC_GIVEN>(g, a, ch, scratch, slots, num_cus, s)
                                  : rgdbf_launch_t<double, SRC_PHILOX>(g, a, ch, scratch, slots, num_cus, s);
    return a.src == SRC_GIVEN ? rgdbf_launch_t<float, SRC_GIVEN>(g, a, ch, scratch, slots, num_cus, s)
                              : rgdbf_launch_t<float, SRC_PHILOX>(g, a, ch, scratch, slots, num_cus, s);
}

}  // namespace ldpc
