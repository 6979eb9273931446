// rstat.hip -- CDNA4 (gfx950) kernels of the every-attempt NGDBF decoders: the reference's
// redecodeStatistics (src/newstat.cpp) and replayGDBF (src/replayGDBF.cpp), both built with
// -D addNoise -D thresholdAdaptation -D weightSyndromes -D outputSmoothing -D saturateSamples.
//
// A frame is decoded `attempts` times from the same channel samples (newstat.cpp:305-429).
// Every attempt starts from the channel hard decision r with theta_i = theta and dsum = 0
// and is one phase of rgdbf.hip: up to T iterations of
//   check nodes  s_j = prod_k d_k over mlist[j]; the attempt stops when every s_j = +1
//   bit nodes    E_i = d_i*y_i + sum_j w_i*s_j (nlist order) + perturbation, w_i =
//                alpha*Ymax/dv_i; flip d_i when E_i < theta_i, else theta_i *= lambda
//   smoothing    dsum += d when it > T - windowsize; an attempt that ended unsatisfied
//                outputs sgn(dsum)
// Unlike rgdbf.hip's phases every attempt runs, whatever the earlier ones gave, so a work
// item is (frame, attempt), items are numbered frame-major, and every item is independent.
// The perturbation of iteration `it` of local attempt ai is pert[frame][ai][it][bit], or
// Philox4x32-10 at counter (bit / 4, lo32(f), hi32(f) + at, stream_id | (it + 1) << 20) with
// f the frame number and at = first_attempt + ai: what phase 0 of frame f + (at << 32) draws
// in rgdbf.hip, so attempt 0 is that decoder with maxphase 1. The channel is frame f's own;
// every item redraws it (one Philox call per four bits against T rows of them).
//
// Two shapes, the pair rgdbf.hip has:
//   rstat_rows   the codes rgdbf_rows takes (N <= 4096, row degree <= 8, column degree <= 12),
//                with its ownership: thread t owns the Philox group of bits 4t..4t+3 and rows t
//                and t + blockDim, the graph sits in registers as packed 16-bit words, yq,
//                theta, dsum, d and r of the thread's bits stay in registers, LDS holds the
//                d < 0 flag bytes, the parity bytes and the double-buffered early-stop flag.
//                The workgroup is persistent and takes items by ticket.
//   rstat_wg     a 256-thread workgroup per item, its state in LDS or, where that does not
//                fit, in a global slot of a persistent grid (the rgdbf_lds / rgdbf_global
//                pair). Takes every graph; the one that writes the per-iteration traces, and
//                the one option LDPC_OPT_GDBF_KERNEL = 1 forces.
// Not built: the frame-resident shape (a workgroup that holds one frame's yq, r, weights and
// the graph as 16-bit indices in LDS and runs several of its attempts side by side). Whether
// it pays on codes like 802.3an, where rstat_wg waits on graph reads from L2, is open
// (DESIGN 13d).
// The frame-level accounting (newstat.cpp:421-465: error weight, syndrome and decisions of
// the last attempt, iterations summed over the attempts, uncoded errors once) is a small
// kernel of its own behind the attempts.
// Compiled with -ffp-contract=off; E keeps the reference's operation order.
#include "rstat.h"
#include "rgdbf_shared.h"
#include "gdbf_front.h"
#include "frame.h"
#include "minsum_common.h"

#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>

namespace ldpc {

// The Philox stream word and high counter word of iteration `it` of attempt `at` of frame cw.
template <typename F>
__device__ __forceinline__ void rstat_noise(const RstatArgs &a, uint64_t cw, uint32_t at, int it, int g4, F nsig,
                                            F (&pv)[4])
{
    uint32_t u[4];
    philox4x32_10<true>((uint32_t)g4, (uint32_t)cw, (uint32_t)(cw >> 32) + at,
                        (a.stream_id & 0xFFFFFu) | ((uint32_t)(it + 1) << 20), (uint32_t)a.seed,
                        (uint32_t)(a.seed >> 32), u);
    float n[4];
    box_muller_hw(u[0], u[1], n[0], n[1]);
    box_muller_hw(u[2], u[3], n[2], n[3]);
#pragma unroll
    for (int q = 0; q < 4; ++q) pv[q] = nsig * (F)n[q];
}

// ---------------------------------------------------------------------
// rstat_wg: one workgroup per item.
// ---------------------------------------------------------------------
template <typename F, int SRC, bool TRACE>
__device__ __forceinline__ void rstat_wg_item(const RstatArgs &a, const DevGraph &g, int item, F *yq, F *theta,
                                              int16_t *dsum, int8_t *d, int8_t *r8, int8_t *s, int *red, const F *wtab)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    const int N = g.N, M = g.M, T = a.T;
    const int b = item / a.attempts, ai = item - b * a.attempts;
    const uint64_t cw = a.first_cw + (uint64_t)b;
    const uint32_t at = (uint32_t)(a.first_attempt + ai);
    const int8_t *cvec = frame_codeword<SRC>(a, b, N);
    const bool smooth = (a.flags & GDBF_SMOOTH) != 0;
    const F lambda = (F)a.lambda, nsig = (F)a.noise_sigma;
    const size_t row0 = ((size_t)b * a.attempts + ai) * (size_t)T;   // the attempt's first row
    // ---- channel + front-end (newstat.cpp:279-302), start from r (:310-316, :331-334) ----
    int unc = 0;
    for (int g4 = tid; g4 * 4 < N; g4 += nt) {
        F yv[4];
        channel_group<F, SRC, true>(a, b, g4, N, cvec, ai == 0 ? a.y_out : nullptr, yv);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int v = g4 * 4 + q;
            if (v < N) {
                int r;
                yq[v] = gdbf_front<F>(yv[q], a, r);
                const int cv = cvec ? cvec[v] : 1;
                unc += (r * cv < 0);
                r8[v] = (int8_t)r;
                d[v] = (int8_t)r;
                theta[v] = (F)a.theta0;
                dsum[v] = 0;
            }
        }
    }
    __syncthreads();
    int it = 0;
    bool sat = false;
    for (it = 0; it < T; ++it) {
        // ---- check nodes ----
        int fail = 0, nun = 0;
        for (int j = tid; j < M; j += nt) {
            const int deg = g.row_deg[j];
            const int32_t *rc = g.row_cols + (size_t)j * g.dcs;
            int p = 0;
            for (int k = 0; k < deg; ++k) p ^= d[LDPC_CHK(rc[k], (uint32_t)N, CHK_RSTAT_BIT)] < 0;
            s[j] = (int8_t)p;
            fail |= p;
            nun += p;
        }
        sat = !__syncthreads_or(fail);
        if (sat) break;   // newstat.cpp:348-349, uniform over the workgroup; this iteration has no row
        if (TRACE && a.s_trace)
            for (int j = tid; j < M; j += nt) a.s_trace[(row0 + it) * M + j] = s[j] ? -1 : 1;
        // ---- bit nodes ----
        const bool acc_smooth = smooth && it > T - a.windowsize;   // :392
        int nerr = 0;
        for (int g4 = tid; g4 * 4 < N; g4 += nt) {
            F pv[4] = {F(0), F(0), F(0), F(0)};
            if (a.flags & GDBF_NOISE) {
                if (SRC == SRC_GIVEN) {
                    const F *pr = reinterpret_cast<const F *>(a.pert) + (row0 + it) * N;
#pragma unroll
                    for (int q = 0; q < 4; ++q) pv[q] = (g4 * 4 + q < N) ? pr[g4 * 4 + q] : F(0);
                } else {
                    rstat_noise<F>(a, cw, at, it, g4, nsig, pv);
                    if (a.pert_out) {
                        F *po = reinterpret_cast<F *>(a.pert_out) + (row0 + it) * N;
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            if (g4 * 4 + q < N) po[g4 * 4 + q] = pv[q];
                    }
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
                for (int e = e0; e < e1; ++e)
                    E += rgdbf_term(w, (uint32_t)s[LDPC_CHK(g.col_refs[e] >> 6, (uint32_t)M, CHK_RSTAT_PARITY)]);
                if (a.flags & GDBF_NOISE) E += pv[q];
                const bool flip = E < theta[i];
                const int dn = flip ? -di : di;
                if (flip) d[i] = (int8_t)dn;
                if ((a.flags & GDBF_ADAPT) && !flip) theta[i] *= lambda;
                if (acc_smooth) dsum[i] = (int16_t)(dsum[i] + dn);
                if (TRACE) {
                    nerr += (dn != (cvec ? cvec[i] : 1));
                    if (a.d_trace) a.d_trace[(row0 + it) * N + i] = (int8_t)dn;
                }
            }
        }
        if (TRACE) {   // the row replayGDBF.cpp:370-373 prints, as counts; the sums' barriers order the step
            int tr[2] = {nerr, nun};
            block_sum_n_t0<2>(tr, red);
            if (tid == 0) {
                if (a.err_trace) a.err_trace[row0 + it] = tr[0];
                if (a.unsat_trace) a.unsat_trace[row0 + it] = tr[1];
            }
        } else {
            __syncthreads();
        }
    }
    if (smooth && !sat)   // newstat.cpp:401-410
        for (int v = tid; v < N; v += nt) d[v] = dsum[v] > 0 ? 1 : -1;
    __syncthreads();

    // ---- error weight and syndrome of the output (:421-423) ----
    const bool last = ai == a.attempts - 1;
    int wgt = 0, synd = 0;
    for (int v = tid; v < N; v += nt) {
        const int dv = d[v];
        const int cv = cvec ? cvec[v] : 1;
        wgt += (dv != cv);
        if (last && a.d_out) a.d_out[(size_t)b * N + v] = (int8_t)dv;
    }
    for (int j = tid; j < M; j += nt) {
        const int deg = g.row_deg[j];
        const int32_t *rc = g.row_cols + (size_t)j * g.dcs;
        int p = 0;
        for (int k = 0; k < deg; ++k) p ^= d[LDPC_CHK(rc[k], (uint32_t)N, CHK_RSTAT_BIT)] < 0;
        synd |= p;
    }
    int sums[3] = {wgt, unc, synd};
    block_sum_n_t0<3>(sums, red);
    if (tid == 0) {
        a.attempt_res[(size_t)b * a.attempts + ai] =
            make_int4(sums[0], it, sums[2] > 0, (int)(smooth && it > T - a.windowsize));   // :415-418
        if (last) a.frame_unc[b] = sums[1];
    }
    __syncthreads();
}

template <typename F, int SRC, bool TRACE>
__global__ __launch_bounds__(256) void k_rstat_wg(RstatArgs a, DevGraph g, RgdbfLayout L)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int red[16 * 4];
    __shared__ F wtab[kRgdbfWtab];
    rgdbf_fill_wtab<F>(a, wtab);
    rstat_wg_item<F, SRC, TRACE>(a, g, blockIdx.x, reinterpret_cast<F *>(smem), reinterpret_cast<F *>(smem + L.theta),
                                 reinterpret_cast<int16_t *>(smem + L.dsum), reinterpret_cast<int8_t *>(smem + L.d),
                                 reinterpret_cast<int8_t *>(smem + L.r), reinterpret_cast<int8_t *>(smem + L.s), red,
                                 wtab);
}

template <typename F, int SRC, bool TRACE>
__global__ __launch_bounds__(1024) void k_rstat_wg_global(RstatArgs a, DevGraph g, RgdbfLayout L, unsigned char *scratch,
                                                          int items)
{
    __shared__ int red[16 * 4];
    __shared__ F wtab[kRgdbfWtab];
    rgdbf_fill_wtab<F>(a, wtab);
    unsigned char *base = scratch + L.total * blockIdx.x;
    for (int item = blockIdx.x; item < items; item += gridDim.x)
        rstat_wg_item<F, SRC, TRACE>(a, g, item, reinterpret_cast<F *>(base), reinterpret_cast<F *>(base + L.theta),
                                     reinterpret_cast<int16_t *>(base + L.dsum), reinterpret_cast<int8_t *>(base + L.d),
                                     reinterpret_cast<int8_t *>(base + L.r), reinterpret_cast<int8_t *>(base + L.s), red,
                                     wtab);
}

// ---------------------------------------------------------------------
// rstat_rows: rgdbf_rows (rgdbf.hip, where the layout, the dummy bit and check, the packed
// register schedule and the 4-waves-per-SIMD bound are explained) with one phase per item
// and the item's own outputs. What a check leaves in LDS is one parity byte; a bit adds
// w_i with its sign bit flipped by that byte, and an edge beyond the lane's own degree reads
// the dummy byte with the weight 0, so it adds -0.0.
// ---------------------------------------------------------------------
template <typename F, int SRC, int DVM, int NT>
__global__ __launch_bounds__(NT, 4) void k_rstat_rows(RstatArgs a, DevGraph g, int np, int poff, int floff, int items)
{
    constexpr int DC = 8, BPT = 4, RPT = 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int red[16 * 4 + 1];                    // block sums; [64]: the next item
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

    // Items: blockIdx.x first, then tickets from a.ticket; thread 0 draws the next ticket
    // while the current item decodes.
    unsigned nxt = 0;
    if (tid == 0) nxt = gridDim.x + atomicAdd(a.ticket, 1u);
    for (int item = blockIdx.x; item < items;) {
        const int b = item / a.attempts, ai = item - b * a.attempts;
        const uint64_t cw = a.first_cw + (uint64_t)b;
        const uint32_t at = (uint32_t)(a.first_attempt + ai);
        const size_t row0 = ((size_t)b * a.attempts + ai) * (size_t)T;
        const int8_t *cvec = frame_codeword<SRC>(a, b, N);
        // ---- channel + front-end (newstat.cpp:279-302), start from r ----
        F yq[BPT], theta[BPT];
        int d[BPT], dsum[BPT];
        int unc = 0;
#pragma unroll
        for (int q = 0; q < BPT; ++q) {
            yq[q] = F(0);
            d[q] = 1;
            theta[q] = (F)a.theta0;
            dsum[q] = 0;
        }
        if (own) {
            F yv[BPT];
            channel_group<F, SRC, true>(a, b, g4, N, cvec, ai == 0 ? a.y_out : nullptr, yv);
#pragma unroll
            for (int q = 0; q < BPT; ++q) {
                const int v = v0 + q;
                if (v < N) {
                    int r;
                    yq[q] = gdbf_front<F>(yv[q], a, r);
                    const int cv = cvec ? cvec[v] : 1;
                    unc += (r * cv < 0);
                    d[q] = r;
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
        put_d();
        __syncthreads();

        int it = 0;
        bool sat = false;
        for (it = 0; it < T; ++it) {
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
            // ---- check nodes ----
            uint32_t g8[RPT][DC];
#pragma unroll
            for (int r = 0; r < RPT; ++r)
#pragma unroll
                for (int k = 0; k < DC; ++k)
                    g8[r][k] = dl[LDPC_CHK((rc[r][k / 2] >> (16 * (k & 1))) & 0xffffu, (uint32_t)np, CHK_RSTAT_BIT)];
            int fail = 0;
#pragma unroll
            for (int r = 0; r < RPT; ++r) {
                uint32_t p = 0;
#pragma unroll
                for (int k = 0; k < DC; ++k) p ^= g8[r][k];
                if (rvalid[r]) pl[LDPC_CHK(tid + r * NT, (uint32_t)M + 1u, CHK_RSTAT_PARITY)] = (uint8_t)p;
                fail |= (int)p;
            }
            if (fail) fl[it & 1] = 1;
            __syncthreads();
            sat = fl[it & 1] == 0;   // newstat.cpp:348-349, uniform over the workgroup
            if (sat) break;
            if (tid == 0) fl[(it + 1) & 1] = 0;   // nobody reads or sets it before the next barrier
            // the perturbations, only in an iteration that passed the check (:361-376)
            F pv[BPT];
#pragma unroll
            for (int q = 0; q < BPT; ++q) pv[q] = F(0);
            if (noise && own) {
                if (SRC == SRC_GIVEN) {
                    const F *pr = reinterpret_cast<const F *>(a.pert) + (row0 + it) * N;
#pragma unroll
                    for (int q = 0; q < BPT; ++q) pv[q] = (v0 + q < N) ? pr[v0 + q] : F(0);
                } else {
                    rstat_noise<F>(a, cw, at, it, g4, nsig, pv);
                    if (a.pert_out) {
                        F *po = reinterpret_cast<F *>(a.pert_out) + (row0 + it) * N;
#pragma unroll
                        for (int q = 0; q < BPT; ++q)
                            if (v0 + q < N) po[v0 + q] = pv[q];
                    }
                }
            }
            // ---- bit nodes, mu = 1 ----
            const bool acc_smooth = smooth && it > T - a.windowsize;   // :392
#pragma unroll
            for (int q = 0; q < BPT; ++q) {
                // all of the slot's parity reads first (one LDS round trip), up to the wave's
                // largest degree; the adds keep nlist order, and an edge beyond this lane's
                // degree adds -0.0
                constexpr int K0 = DVM < 4 ? DVM : 4;
                const int dq = (int)((degs >> (4 * q)) & 15u);
                uint32_t sv[K0];
#pragma unroll
                for (int k = 0; k < K0; ++k)
                    sv[k] = pl[LDPC_CHK((bc[q][k / 2] >> (16 * (k & 1))) & 0xffffu, (uint32_t)M + 1u, CHK_RSTAT_PARITY)];
                F E = (F)d[q] * yq[q];
#pragma unroll
                for (int k = 0; k < K0; ++k) E += rgdbf_term(k < dq ? wq[q] : F(0), sv[k]);
                if (DVM > K0 && wdeg[q] > K0) {
                    uint32_t sw[DVM - K0 > 0 ? DVM - K0 : 1];
#pragma unroll
                    for (int k = K0; k < DVM; ++k)
                        sw[k - K0] = pl[LDPC_CHK((bc[q][k / 2] >> (16 * (k & 1))) & 0xffffu, (uint32_t)M + 1u, CHK_RSTAT_PARITY)];
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
        if (smooth && !sat) {   // newstat.cpp:401-410
#pragma unroll
            for (int q = 0; q < BPT; ++q) d[q] = (v0 + q < N) ? (dsum[q] > 0 ? 1 : -1) : 1;
            put_d();
        }
        __syncthreads();

        // ---- error weight and syndrome of the output (:421-423) ----
        const bool last = ai == a.attempts - 1;
        int wgt = 0, synd = 0;
        if (own)
#pragma unroll
            for (int q = 0; q < BPT; ++q) {
                const int v = v0 + q;
                if (v < N) {
                    const int cv = cvec ? cvec[v] : 1;
                    wgt += (d[q] != cv);
                    if (last && a.d_out) a.d_out[(size_t)b * N + v] = (int8_t)d[q];
                }
            }
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
            uint32_t p = 0;
#pragma unroll
            for (int k = 0; k < DC; ++k) p ^= dl[LDPC_CHK((rc[r][k / 2] >> (16 * (k & 1))) & 0xffffu, (uint32_t)np, CHK_RSTAT_BIT)];
            synd |= (int)p;
        }
        int sums[3] = {wgt, unc, synd};
        block_sum_n_t0<3>(sums, red);
        if (tid == 0) {
            a.attempt_res[(size_t)b * a.attempts + ai] =
                make_int4(sums[0], it, sums[2] > 0, (int)(smooth && it > T - a.windowsize));   // :415-418
            if (last) a.frame_unc[b] = sums[1];
            red[64] = (int)nxt;
        }
        __syncthreads();
        item = red[64];   // rewritten only after the next item's barriers
        if (tid == 0 && item < items) nxt = gridDim.x + atomicAdd(a.ticket, 1u);
    }
}

// ---------------------------------------------------------------------
// Frame accounting behind the attempts (newstat.cpp:421-465): one thread per frame.
// ---------------------------------------------------------------------
__global__ void k_rstat_account(RstatArgs a)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.batch) return;
    const int4 *res = a.attempt_res + (size_t)b * a.attempts;
    int total = 0;
    for (int k = 0; k < a.attempts; ++k) total += res[k].y;
    const int4 lastr = res[a.attempts - 1];
    frame_account(a.counts, a.hist, a.frame_res, b, lastr.x, a.frame_unc[b], lastr.z, total, total);
}

// dynamic LDS of a workgroup: 64 KB less the kernels' static arrays (red, wtab)
constexpr size_t kRstatMaxLds = 64 * 1024 - 1024;

LDPC_CHECK_TU(rstat)

RstatChoice rstat_choose(const DevGraph &g, bool f64, bool trace, int maxdv, int maxdc)
{
    RstatChoice ch;
    if (!trace && rgdbf_rows_fits(g.N, g.M, maxdv, maxdc) && opt(LDPC_OPT_GDBF_KERNEL) != 1) {
        ch.name = "rstat_rows";
        ch.threads = g.N <= 4 * 512 && g.M <= 2 * 512 ? 512 : 1024;
        ch.dvm = maxdv <= 4 ? 4 : 12;
        ch.lds_bytes = rgdbf_rows_layout(g.N, g.M).total;
        return ch;
    }
    const RgdbfLayout L = rgdbf_layout(g.N, g.M, f64 ? 8 : 4);
    ch.name = "rstat_wg";
    if (L.total <= kRstatMaxLds) {
        ch.lds_bytes = (int)L.total;
        ch.threads = 256;
    } else {
        ch.threads = 1024;
        ch.slot_bytes = L.total;
    }
    return ch;
}

template <typename F, int SRC, int DVM, int NT>
static hipError_t rstat_rows_launch(const DevGraph &g, const RstatArgs &a, int num_cus, hipStream_t s)
{
    if (!a.ticket) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(a.ticket, 0, sizeof(unsigned), s);
    if (e != hipSuccess) return e;
    const RgdbfRowsLayout L = rgdbf_rows_layout(g.N, g.M);
    const int items = a.batch * a.attempts;
    auto fn = k_rstat_rows<F, SRC, DVM, NT>;
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, NT, L.total) != hipSuccess || per_cu < 1)
        per_cu = 1;
    int grid = per_cu * (num_cus > 0 ? num_cus : 1);
    if (grid > items) grid = items;
    hipLaunchKernelGGL(fn, dim3(grid), dim3(NT), L.total, s, a, g, L.np, L.poff, L.floff, items);
    return hipGetLastError();
}

template <typename F, int SRC, bool TRACE>
static hipError_t rstat_wg_launch(const DevGraph &g, const RstatArgs &a, const RstatChoice &ch, void *scratch, int slots,
                                  hipStream_t s)
{
    const RgdbfLayout L = rgdbf_layout(g.N, g.M, sizeof(F));
    const int items = a.batch * a.attempts;
    if (ch.lds_bytes > 0) {
        hipLaunchKernelGGL((k_rstat_wg<F, SRC, TRACE>), dim3(items), dim3(ch.threads), ch.lds_bytes, s, a, g, L);
    } else {
        const int grid = slots < items ? slots : items;
        if (grid <= 0 || !scratch) return hipErrorInvalidValue;
        hipLaunchKernelGGL((k_rstat_wg_global<F, SRC, TRACE>), dim3(grid), dim3(ch.threads), 0, s, a, g, L,
                           (unsigned char *)scratch, items);
    }
    return hipGetLastError();
}

template <typename F, int SRC>
static hipError_t rstat_launch_t(const DevGraph &g, const RstatArgs &a, const RstatChoice &ch, void *scratch, int slots,
                                 int num_cus, hipStream_t s)
{
    if (ch.dvm == 4)
        return ch.threads == 512 ? rstat_rows_launch<F, SRC, 4, 512>(g, a, num_cus, s)
                                 : rstat_rows_launch<F, SRC, 4, 1024>(g, a, num_cus, s);
    if (ch.dvm == 12)
        return ch.threads == 512 ? rstat_rows_launch<F, SRC, 12, 512>(g, a, num_cus, s)
                                 : rstat_rows_launch<F, SRC, 12, 1024>(g, a, num_cus, s);
    const bool trace = a.err_trace || a.unsat_trace || a.d_trace || a.s_trace;
    return trace ? rstat_wg_launch<F, SRC, true>(g, a, ch, scratch, slots, s)
                 : rstat_wg_launch<F, SRC, false>(g, a, ch, scratch, slots, s);
}

hipError_t rstat_launch(const DevGraph &g, const RstatArgs &a, bool f64, const RstatChoice &ch, void *scratch, int slots,
                        int num_cus, hipStream_t s)
{
    if (a.batch <= 0 || a.attempts <= 0) return hipSuccess;
    if (!a.attempt_res || !a.frame_unc) return hipErrorInvalidValue;
    hipError_t e;
    if (f64)
        e = a.src == SRC_GIVEN ? rstat_launch_t<double, SRC_GIVEN>(g, a, ch, scratch, slots, num_cus, s)
                               : rstat_launch_t<double, SRC_PHILOX>(g, a, ch, scratch, slots, num_cus, s);
    else
        e = a.src == SRC_GIVEN ? rstat_launch_t<float, SRC_GIVEN>(g, a, ch, scratch, slots, num_cus, s)
                               : rstat_launch_t<float, SRC_PHILOX>(g, a, ch, scratch, slots, num_cus, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_rstat_account, dim3((a.batch + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace ldpc
