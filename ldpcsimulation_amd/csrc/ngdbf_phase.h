// ngdbf_phase.h -- one phase of the NGDBF decoder of src/RNGDBF.cpp, the body that the
// re-decoding kernels (rgdbf.hip) and the every-attempt kernels (rstat.hip; src/newstat.cpp
// and src/replayGDBF.cpp have the same checkNodeUpdates / symNodeUpdates) are written over.
//
// A phase starts from the channel hard decision r with theta_i = theta and dsum = 0 and
// runs up to T parallel-flip iterations:
//   check nodes  s_j = prod_k d_k over mlist[j]; the phase stops when every s_j = +1
//   bit nodes    E_i = d_i*y_i + sum_j w_i*s_j (nlist order) [+ perturbation], with
//                w_i = alpha*Ymax/dv_i (1 without WEIGHT); flip d_i when E_i < theta_i,
//                else theta_i *= lambda
//   smoothing    dsum += d when it > T - windowsize; a phase that ended unsatisfied
//                outputs sgn(dsum)
// What a decoder adds is its outer loop (rgdbf: up to maxphase phases, stop after a
// satisfied one; rstat: one phase per (frame, attempt) item), where a perturbation row
// comes from (a functor the kernel hands to the phase) and what an item writes at its end.
// E keeps the reference's operation order (-ffp-contract=off); w_i*(+-1) is exactly +-w_i,
// so the kernels flip the sign bit of w_i instead of multiplying.
//
// Two shapes:
//   NgdbfWg    one workgroup per item, its state in LDS (ngdbf_wg_lds) or in a global slot
//              of a persistent grid (ngdbf_wg_global); takes every graph.
//   NgdbfRows  the register schedule, for the codes gdbf_rows takes (rgdbf_rows_fits). A
//              persistent workgroup that takes items by ticket; explained at the struct.
#pragma once
#include "gdbf.h"
#include "gdbf_front.h"
#include "frame.h"

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

// One row of Philox perturbations for the bits of group g4: Philox4x32-10 keyed by the seed
// at counter (g4, c1, c2, stream_id | (row + 1) << 20), Box-Muller, times noise_sigma. Row 0
// of (c1, c2) = the codeword number is what gdbf.hip draws in its first iteration.
template <typename F>
__device__ __forceinline__ void ngdbf_draw(const GdbfArgs &a, int g4, uint32_t c1, uint32_t c2, int row, F (&pv)[4])
{
    uint32_t u[4];
    philox4x32_10<true>((uint32_t)g4, c1, c2, (a.stream_id & 0xFFFFFu) | ((uint32_t)(row + 1) << 20),
                        (uint32_t)a.seed, (uint32_t)(a.seed >> 32), u);
    float n[4];
    box_muller_hw(u[0], u[1], n[0], n[1]);
    box_muller_hw(u[2], u[3], n[2], n[3]);
    const F nsig = (F)a.noise_sigma;
#pragma unroll
    for (int q = 0; q < 4; ++q) pv[q] = nsig * (F)n[q];
}

// ---------------------------------------------------------------------
// The workgroup shape.
// ---------------------------------------------------------------------
constexpr int kRgdbfWtab = 64;   // weights by degree kept in LDS; larger degrees divide in place

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

// The per-iteration rows replayGDBF prints, each [item][T] rows and any of them null; row0 is
// the item's first row. Only a TRACE = true phase reads them.
struct NgdbfTrace {
    int32_t *err = nullptr, *unsat = nullptr;
    int8_t *d = nullptr, *s = nullptr;   // [..][N] / [..][M], +-1
    size_t row0 = 0;
};

template <typename F>
struct NgdbfWg {
    F *yq, *theta;
    int16_t *dsum;
    int8_t *d, *r, *s;
    int *red;        // block sums
    const F *wtab;   // w by degree

    __device__ __forceinline__ NgdbfWg(unsigned char *base, const RgdbfLayout &L, int *red_, const F *wtab_)
        : yq(reinterpret_cast<F *>(base)), theta(reinterpret_cast<F *>(base + L.theta)),
          dsum(reinterpret_cast<int16_t *>(base + L.dsum)), d(reinterpret_cast<int8_t *>(base + L.d)),
          r(reinterpret_cast<int8_t *>(base + L.r)), s(reinterpret_cast<int8_t *>(base + L.s)), red(red_),
          wtab(wtab_)
    {
    }

    // Channel + front-end of frame b (RNGDBF.cpp:252-275): yq and r; the uncoded errors of
    // the thread's bits.
    template <int SRC, typename Args>
    __device__ __forceinline__ int front(const Args &a, int b, int N, const int8_t *cvec, void *y_out) const
    {
        int unc = 0;
        for (int g4 = threadIdx.x; g4 * 4 < N; g4 += blockDim.x) {
            F yv[4];
            channel_group<F, SRC, true>(a, b, g4, N, cvec, y_out, yv);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int v = g4 * 4 + q;
                if (v < N) {
                    int rv;
                    yq[v] = gdbf_front<F>(yv[q], a, rv);
                    unc += (rv * (cvec ? cvec[v] : 1) < 0);
                    r[v] = (int8_t)rv;
                }
            }
        }
        return unc;
    }

    // One phase: restart from r (:282-288, :303-306; each thread its own bits, those it wrote
    // in front()), then up to T iterations. draw(it, g4, pv) gives the perturbations of the
    // bits of group g4. Returns the iterations run; sat: the phase ended on a satisfied check
    // step (that iteration has no bit step and no trace row).
    template <bool TRACE, unsigned SITE_BIT, unsigned SITE_PAR, typename Draw>
    __device__ __forceinline__ int phase(const GdbfArgs &a, const DevGraph &g, const int8_t *cvec,
                                         const NgdbfTrace &tr, bool &sat, Draw &&draw) const
    {
        const int tid = threadIdx.x, nt = blockDim.x;
        const int N = g.N, M = g.M, T = a.T;
        const F lambda = (F)a.lambda;
        for (int g4 = tid; g4 * 4 < N; g4 += nt)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int v = g4 * 4 + q;
                if (v < N) {
                    d[v] = r[v];
                    theta[v] = (F)a.theta0;
                    dsum[v] = 0;
                }
            }
        __syncthreads();
        int it = 0;
        sat = false;
        for (it = 0; it < T; ++it) {
            // ---- check nodes (:533-550) ----
            int fail = 0, nun = 0;
            for (int j = tid; j < M; j += nt) {
                const int deg = g.row_deg[j];
                const int32_t *rc = g.row_cols + (size_t)j * g.dcs;
                int p = 0;
                for (int k = 0; k < deg; ++k) p ^= d[LDPC_CHK(rc[k], (uint32_t)N, SITE_BIT)] < 0;
                s[j] = (int8_t)p;
                fail |= p;
                if (TRACE) nun += p;
            }
            sat = !__syncthreads_or(fail);
            if (sat) break;   // :320-321, uniform over the workgroup
            if (TRACE && tr.s)
                for (int j = tid; j < M; j += nt) tr.s[(tr.row0 + it) * M + j] = s[j] ? -1 : 1;
            // ---- bit nodes (:552-) ----
            const bool acc_smooth = (a.flags & GDBF_SMOOTH) && it > T - a.windowsize;   // :364
            int nerr = 0;
            for (int g4 = tid; g4 * 4 < N; g4 += nt) {
                F pv[4] = {F(0), F(0), F(0), F(0)};
                if (a.flags & GDBF_NOISE) draw(it, g4, pv);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int i = g4 * 4 + q;
                    if (i >= N) break;
                    const int di = d[i];
                    F E = (F)di * yq[i];
                    const int e0 = g.col_ptr[i], e1 = g.col_ptr[i + 1];
                    const int deg = e1 - e0;
                    const F w = deg < kRgdbfWtab ? wtab[deg] : rgdbf_weight<F>(a, deg);
                    for (int e = e0; e < e1; ++e)   // w_i * s_j
                        E += rgdbf_term(w, (uint32_t)s[LDPC_CHK(g.col_refs[e] >> 6, (uint32_t)M, SITE_PAR)]);
                    if (a.flags & GDBF_NOISE) E += pv[q];
                    const bool flip = E < theta[i];
                    const int dn = flip ? -di : di;
                    if (flip) d[i] = (int8_t)dn;
                    if ((a.flags & GDBF_ADAPT) && !flip) theta[i] *= lambda;
                    if (acc_smooth) dsum[i] = (int16_t)(dsum[i] + dn);
                    if (TRACE) {
                        nerr += (dn != (cvec ? cvec[i] : 1));
                        if (tr.d) tr.d[(tr.row0 + it) * N + i] = (int8_t)dn;
                    }
                }
            }
            if (TRACE) {   // the row replayGDBF.cpp:370-373 prints, as counts; the sums' barriers order the step
                int sums[2] = {nerr, nun};
                block_sum_n_t0<2>(sums, red);
                if (tid == 0) {
                    if (tr.err) tr.err[tr.row0 + it] = sums[0];
                    if (tr.unsat) tr.unsat[tr.row0 + it] = sums[1];
                }
            } else {
                __syncthreads();
            }
        }
        return it;
    }

    // The end of an item: the smoothed output when its last phase ended unsatisfied (:373-382),
    // the error weight (:393; the decisions go to d_row when it is not null) and the syndrome
    // of the output. Thread 0 gets the block's sums = {error weight, unc, syndrome != 0}.
    template <unsigned SITE_BIT>
    __device__ __forceinline__ void finish(const GdbfArgs &a, const DevGraph &g, const int8_t *cvec, bool sat,
                                           int8_t *d_row, int unc, int (&sums)[3]) const
    {
        const int tid = threadIdx.x, nt = blockDim.x;
        const int N = g.N, M = g.M;
        if ((a.flags & GDBF_SMOOTH) && !sat)
            for (int v = tid; v < N; v += nt) d[v] = dsum[v] > 0 ? 1 : -1;
        __syncthreads();
        int wgt = 0, synd = 0;
        for (int v = tid; v < N; v += nt) {
            const int dv = d[v];
            wgt += (dv != (cvec ? cvec[v] : 1));
            if (d_row) d_row[v] = (int8_t)dv;
        }
        for (int j = tid; j < M; j += nt) {
            const int deg = g.row_deg[j];
            const int32_t *rc = g.row_cols + (size_t)j * g.dcs;
            int p = 0;
            for (int k = 0; k < deg; ++k) p ^= d[LDPC_CHK(rc[k], (uint32_t)N, SITE_BIT)] < 0;
            synd |= p;
        }
        sums[0] = wgt, sums[1] = unc, sums[2] = synd;
        block_sum_n_t0<3>(sums, red);
    }
};

// The two homes of a workgroup's state. item(i, wg) decodes item i and ends on a barrier.
// LDS: one workgroup per item, L.total bytes of dynamic LDS.
template <typename F, typename Item>
__device__ __forceinline__ void ngdbf_wg_lds(const GdbfArgs &a, const RgdbfLayout &L, Item &&item)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int red[16 * 4];
    __shared__ F wtab[kRgdbfWtab];
    for (int k = threadIdx.x; k < kRgdbfWtab; k += blockDim.x) wtab[k] = rgdbf_weight<F>(a, k);
    __syncthreads();
    item((int)blockIdx.x, NgdbfWg<F>(smem, L, red, wtab));
}
// Global: a persistent grid, workgroup k in slot k of `scratch` (L.total bytes each).
template <typename F, typename Item>
__device__ __forceinline__ void ngdbf_wg_global(const GdbfArgs &a, const RgdbfLayout &L, unsigned char *scratch,
                                                int items, Item &&item)
{
    __shared__ int red[16 * 4];
    __shared__ F wtab[kRgdbfWtab];
    for (int k = threadIdx.x; k < kRgdbfWtab; k += blockDim.x) wtab[k] = rgdbf_weight<F>(a, k);
    __syncthreads();
    const NgdbfWg<F> wg(scratch + L.total * blockIdx.x, L, red, wtab);
    for (int i = blockIdx.x; i < items; i += gridDim.x) item(i, wg);
}

// ---------------------------------------------------------------------
// The register-schedule shape: codes with N <= 4 * 1024, row degree <= 8 and column degree
// <= 12 (those gdbf_rows takes). Ownership as in gdbf_rows: thread t owns the Philox group
// of bits 4t..4t+3 and rows t and t + blockDim; the graph sits in registers as packed
// 16-bit words; yq, theta, dsum and d of the thread's bits stay in registers (the kernel's
// own arrays); the workgroup is persistent and takes items by ticket (early stop makes
// them unequal). What differs from gdbf_rows is what a check leaves in LDS: one parity
// byte (1: s_j = -1), not the term w * s_j, because the weight belongs to the bit. A bit
// computes its w_i once per workgroup (double, then rounded to F) and adds w_i with its
// sign bit flipped by the parity byte; an edge beyond the lane's own degree reads a dummy
// byte (1) and takes the weight 0 by a select on the lane's degree, so it adds -0.0
// (E + -0.0 == E for every E). LDS per workgroup: the d < 0 flag bytes, the parity bytes
// and the double-buffered early-stop flag -- about N + M bytes.
// The parity bytes are indexed by the plain check number: the lanes of a bit slot read
// checks j0 + 4t (bits 4t + q of a quasi-cyclic block), which as bytes are the consecutive
// dwords j0/4 + t -- 32 lanes, 32 banks -- so gdbf_rows' pad word per 32 checks (its F
// terms at stride 4 were 4-way conflicts) has nothing to remove here.
// The early-stop flag of iteration `it` is fl[(fbase + it) & 1]; a caller that runs phase
// after phase passes fbase = ph * T, which keeps alternating across a restart for odd and
// even T.
// The kernels over this are bounded to 4 waves per SIMD (128 VGPRs): at gdbf_rows' 6 the
// fp32 512-thread instances spilled 16 to 128 bytes per lane (the weights and the degrees
// are registers gdbf_rows does not hold).
// ---------------------------------------------------------------------
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

template <typename F, int DVM, int NT>
struct NgdbfRows {
    static constexpr int DC = 8, BPT = 4, RPT = 2;
    static constexpr int K0 = DVM < 4 ? DVM : 4;   // edges of a bit slot read in the first stage
    static constexpr int kRed = 16 * 4 + 1;   // ints of the kernel's `red`: block sums; [64]: the next item

    uint8_t *dl;            // 1 where d = -1
    uint8_t *pl;            // 1 where s_j = -1
    volatile int *fl;       // the double-buffered early-stop flag
    int *red;
    int tid, N, M, T, np;
    int v0;                 // the thread's first bit; its Philox group is tid
    bool own;
    uint32_t rc[RPT][DC / 2];
    bool rvalid[RPT];
    uint32_t bc[BPT][DVM / 2];
    int wdeg[BPT];          // wave-uniform bound of each slot's degree
    uint32_t degs;          // the lane's own degrees, 4 bits per slot
    F wq[BPT];              // w_i of the thread's bits
    bool smooth, noise, adapt;
    F lambda;
    int windowsize;

    // Once per workgroup: the graph into registers, the dummy bit and the dummy check.
    __device__ __forceinline__ NgdbfRows(const GdbfArgs &a, const DevGraph &g, unsigned char *smem, int *red_, int np_,
                                         int poff, int floff)
        : dl(smem), pl(smem + poff), fl(reinterpret_cast<int *>(smem + floff)), red(red_), tid(threadIdx.x), N(g.N),
          M(g.M), T(a.T), np(np_), v0(BPT * (int)threadIdx.x)
    {
        const int dbit = np - 1;   // dummy bit index
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
        own = v0 < N;
        degs = 0;
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
            wdeg[q] = DVM;
            // Only the second read stage asks for it. Computed and left unused (DVM 4), its
            // shuffles die late, after their lane addresses merged with the block sum's: five
            // VGPRs live across the item loop, an occupancy step of the fp32 instances.
            if constexpr (DVM > K0) {
                int m = deg;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o, 64));
                wdeg[q] = __builtin_amdgcn_readfirstlane(m);
            }
        }
        if (tid == 0) {
            *reinterpret_cast<uint32_t *>(dl + np - 4) = 0u;   // dummy bits: d = +1
            pl[M] = 1;                                          // dummy check: a padding edge adds 0 * s = -0.0
        }
        smooth = (a.flags & GDBF_SMOOTH) != 0, noise = (a.flags & GDBF_NOISE) != 0;
        adapt = (a.flags & GDBF_ADAPT) != 0;
        lambda = (F)a.lambda;
        windowsize = a.windowsize;
    }

    // Items: blockIdx.x first, then tickets from `ticket` (zero at the launch); thread 0 draws
    // the next ticket while the current item decodes. first_ticket() before the loop;
    // next_item() ends an item (after thread 0 wrote its results) and gives the next one.
    __device__ __forceinline__ unsigned first_ticket(unsigned *ticket) const
    {
        return tid == 0 ? gridDim.x + atomicAdd(ticket, 1u) : 0u;
    }
    __device__ __forceinline__ int next_item(unsigned *ticket, int items, unsigned &nxt) const
    {
        if (tid == 0) red[64] = (int)nxt;
        __syncthreads();
        const int item = red[64];   // rewritten only after the next item's barriers
        if (tid == 0 && item < items) nxt = gridDim.x + atomicAdd(ticket, 1u);
        return item;
    }

    // Channel + front-end of frame b (RNGDBF.cpp:252-275): yq of the thread's bits (0 past N)
    // and their hard decisions (bit q of rneg: r = -1), the uncoded errors among them; clears
    // the stop flags.
    template <int SRC, typename Args>
    __device__ __forceinline__ int front(const Args &a, int b, const int8_t *cvec, void *y_out, F (&yq)[BPT],
                                         uint32_t &rneg) const
    {
        int unc = 0;
        rneg = 0;
#pragma unroll
        for (int q = 0; q < BPT; ++q) yq[q] = F(0);
        if (own) {
            F yv[BPT];
            channel_group<F, SRC, true>(a, b, tid, N, cvec, y_out, yv);
#pragma unroll
            for (int q = 0; q < BPT; ++q) {
                const int v = v0 + q;
                if (v < N) {
                    int r;
                    yq[q] = gdbf_front<F>(yv[q], a, r);
                    unc += (r * (cvec ? cvec[v] : 1) < 0);
                    rneg |= (uint32_t)(r < 0) << q;
                }
            }
        }
        if (tid == 0) {
            fl[0] = 0;
            fl[1] = 0;
        }
        return unc;
    }

    __device__ __forceinline__ void put_d(const int (&d)[BPT]) const
    {
        if (own)
            *reinterpret_cast<uint32_t *>(dl + v0) = (uint32_t)(d[0] < 0) | ((uint32_t)(d[1] < 0) << 8) |
                                                     ((uint32_t)(d[2] < 0) << 16) | ((uint32_t)(d[3] < 0) << 24);
    }

    // One phase from the state (yq, theta, d, dsum) the caller has set: up to T iterations.
    // draw(it, pv) gives the perturbations of the thread's bits; it is called only in an
    // iteration that passed the check (:333-348) and only by a thread that owns bits.
    // Returns the iterations run; sat: the phase ended on a satisfied check step.
    template <unsigned SITE_BIT, unsigned SITE_PAR, typename Draw>
    __device__ __forceinline__ int phase(int fbase, const F (&yq)[BPT], F (&theta)[BPT], int (&d)[BPT],
                                         int (&dsum)[BPT], bool &sat, Draw &&draw)
    {
        put_d(d);
        __syncthreads();
        int it = 0;
        sat = false;
        for (it = 0; it < T; ++it) {
            const int fi = (fbase + it) & 1;   // this iteration's stop flag
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
                    g8[r][k] = dl[LDPC_CHK((rc[r][k / 2] >> (16 * (k & 1))) & 0xffffu, (uint32_t)np, SITE_BIT)];
            int fail = 0;
#pragma unroll
            for (int r = 0; r < RPT; ++r) {
                uint32_t p = 0;
#pragma unroll
                for (int k = 0; k < DC; ++k) p ^= g8[r][k];
                if (rvalid[r]) pl[LDPC_CHK(tid + r * NT, (uint32_t)M + 1u, SITE_PAR)] = (uint8_t)p;
                fail |= (int)p;
            }
            if (fail) fl[fi] = 1;
            __syncthreads();
            sat = fl[fi] == 0;   // :320-321, uniform over the workgroup
            if (sat) break;
            if (tid == 0) fl[fi ^ 1] = 0;   // nobody reads or sets it before the next barrier
            F pv[BPT];
#pragma unroll
            for (int q = 0; q < BPT; ++q) pv[q] = F(0);
            if (noise && own) draw(it, pv);
            // ---- bit nodes (:552-), mu = 1 ----
            const bool acc_smooth = smooth && it > T - windowsize;   // :364
#pragma unroll
            for (int q = 0; q < BPT; ++q) {
                // all of the slot's parity reads first (one LDS round trip), up to the
                // wave's largest degree; the adds keep nlist order, and an edge beyond
                // this lane's degree adds -0.0
                const int dq = (int)((degs >> (4 * q)) & 15u);
                uint32_t sv[K0];
#pragma unroll
                for (int k = 0; k < K0; ++k)
                    sv[k] = pl[LDPC_CHK((bc[q][k / 2] >> (16 * (k & 1))) & 0xffffu, (uint32_t)M + 1u, SITE_PAR)];
                F E = (F)d[q] * yq[q];
#pragma unroll
                for (int k = 0; k < K0; ++k) E += rgdbf_term(k < dq ? wq[q] : F(0), sv[k]);
                if (DVM > K0 && wdeg[q] > K0) {
                    uint32_t sw[DVM - K0 > 0 ? DVM - K0 : 1];
#pragma unroll
                    for (int k = K0; k < DVM; ++k)
                        sw[k - K0] = pl[LDPC_CHK((bc[q][k / 2] >> (16 * (k & 1))) & 0xffffu, (uint32_t)M + 1u, SITE_PAR)];
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
            put_d(d);
            __syncthreads();
        }
        return it;
    }

    // The end of an item: the smoothed output when its last phase ended unsatisfied (:373-382),
    // the error weight (:393; the decisions go to d_row when it is not null) and the syndrome
    // of the output. Thread 0 gets the block's sums = {error weight, unc, syndrome != 0}.
    template <unsigned SITE_BIT>
    __device__ __forceinline__ void finish(const int8_t *cvec, bool sat, int (&d)[BPT], const int (&dsum)[BPT],
                                           int8_t *d_row, int unc, int (&sums)[3]) const
    {
        if (smooth && !sat) {
#pragma unroll
            for (int q = 0; q < BPT; ++q) d[q] = (v0 + q < N) ? (dsum[q] > 0 ? 1 : -1) : 1;
            put_d(d);
        }
        __syncthreads();
        int wgt = 0, synd = 0;
        if (own)
#pragma unroll
            for (int q = 0; q < BPT; ++q) {
                const int v = v0 + q;
                if (v < N) {
                    wgt += (d[q] != (cvec ? cvec[v] : 1));
                    if (d_row) d_row[v] = (int8_t)d[q];
                }
            }
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
            uint32_t p = 0;
#pragma unroll
            for (int k = 0; k < DC; ++k)
                p ^= dl[LDPC_CHK((rc[r][k / 2] >> (16 * (k & 1))) & 0xffffu, (uint32_t)np, SITE_BIT)];
            synd |= (int)p;
        }
        sums[0] = wgt, sums[1] = unc, sums[2] = synd;
        block_sum_n_t0<3>(sums, red);
    }
};

}  // namespace ldpc
