// flood.hip -- flooding min-sum of codes whose state exceeds LDS: the persistent kernel
// (k_decode_flood) and the phase-per-launch kernels (k_flood_*), their plan and launch.
#include "minsum_kernels.h"
#include "frame.h"

namespace ldpc {

// =====================================================================
// Global-memory flooding kernel (codes whose state exceeds LDS, DVB-S2).
//
// One workgroup per codeword (persistent), the codeword's state in a global
// scratch slot, laid out by the FloodSchedule so every access is coalesced:
//   app[NP + 1], yq[NP]     bits in storage order (NP = ngroups*64; app[NP] = +inf)
//   c2v[e_pad + 64]         edge e of position p at gbase[p/64] + 64e + p%64
//   m12[M_pad], meta[M_pad] the packed check state, rows in chain order:
//                           (min1, min2) after /alpha or the offset, and
//                           argmin | output sign bits << 5
// Check phase: thread per row (slot-major schedule: lane i reads sp[k*M_pad+i]);
// the row's last messages are rebuilt from its packed state, the new ones are
// computed with the reference's comparisons (as cn_exact) and scattered into
// c2v. Bit phase: thread per position, sum = yq + c2v in nlist order.
// =====================================================================
template <typename F, int SRC, int DC>
__global__ __launch_bounds__(512, (sizeof(F) == 4 && DC <= 8) ? 8 : 4) void k_decode_flood(DecodeArgs a, DevGraph g, FloodSched fs, unsigned char *scratch,
                                                      size_t slot_bytes)
{
    using F2 = typename F2T<F>::T;
    __shared__ int red[32 + 16 * 8];
    __shared__ unsigned long long acc[6];   // the block's totals (thread 0)
    const int tid = threadIdx.x, nt = blockDim.x;
    const int N = g.N, NP = fs.ngroups * 64, MP = fs.M_pad;
    unsigned char *base = scratch + slot_bytes * blockIdx.x;
    F *app = reinterpret_cast<F *>(base);                       // [NP + 1]
    F *yq = app + (NP + 1);                                     // [NP]
    F *c2v = yq + NP;                                           // [e_pad + 64]
    F2 *m12 = reinterpret_cast<F2 *>(c2v + (fs.e_pad + 64 + 1) / 2 * 2);   // 16-B aligned for double2
    uint32_t *meta = reinterpret_cast<uint32_t *>(m12 + MP);
    const F alpha = (F)a.alpha, delta = (F)a.delta;

    if (tid == 0) {
        app[NP] = dinf<F>();   // sentinel position of padding slots
#pragma unroll
        for (int q = 0; q < 6; ++q) acc[q] = 0;
    }

    for (int b = blockIdx.x; b < a.batch; b += gridDim.x) {
        const int8_t *cvec = frame_codeword<SRC>(a, b, N);
        // ---- channel + front-end (:214-238) into storage order ----
        int unc = 0;
        channel_bits<F, SRC, false>(a, b, N, cvec, a.y_out, [&](int v, F yv) {
            const F q = front_end<F>(yv, a);
            const int p = fs.pos_of_bit[v];
            yq[p] = q;
            app[p] = q;
            const int cv = cvec ? cvec[v] : 1;
            unc += ((q > F(0) ? 1 : -1) * cv < 0);
        });
        for (int i = tid; i < MP; i += nt) {   // c2v_old = +0: v2c = yq on the first pass (:364-370)
            F2 z;
            z.x = F(0);
            z.y = F(0);
            m12[i] = z;
            meta[i] = 0;
        }
        __syncthreads();

        for (int it = 0; it < a.T; ++it) {
            // ---- check nodes (:410-450, :494-515) ----
            for (int i = tid; i < MP; i += nt) {
                const int deg = fs.rdeg[i];
                if (deg == 0) continue;
                int sp[DC];
#pragma unroll
                for (int k = 0; k < DC; ++k) sp[k] = k < deg ? fs.sp[(size_t)k * MP + i] : NP;
                F xa[DC];
#pragma unroll
                for (int k = 0; k < DC; ++k) xa[k] = app[sp[k]];
                const F2 old = m12[i];
                const uint32_t om = meta[i];
                const int oidx = (int)(om & 31u);
                F mn1 = dinf<F>(), mn2 = dinf<F>();
                int amin = 31;
                uint32_t sg = 0;
                F ax[DC];
#pragma unroll
                for (int k = 0; k < DC; ++k) {
                    if (k < deg) {
                        F cold = (k == oidx) ? old.y : old.x;
                        if ((om >> (5 + k)) & 1u) cold = -cold;
                        const F x = xa[k] - cold;                     // v2c (:469)
                        sg |= (uint32_t)(!(x >= F(0))) << k;          // sgn(v2c) < 0 (:518-523)
                        ax[k] = dabs(x);
                        if (ax[k] <= mn1) { mn2 = mn1; mn1 = ax[k]; amin = k; }   // :428-433
                        else if (ax[k] < mn2) { mn2 = ax[k]; }                    // :434-437
                    }
                }
                const uint32_t degmask = (1u << deg) - 1u;
                uint32_t eff = (__popc(sg) & 1) ? (sg ^ degmask) : sg;   // prod * sgn(v2c_k)
                F M1 = mn1, M2 = mn2;
                if (a.variant == V_NMS) {
                    M1 = nms_div<F>(mn1, alpha, a);               // :498
                    M2 = nms_div<F>(mn2, alpha, a);
                } else if (a.variant == V_OMS) {
                    const F t1 = mn1 - delta, t2 = mn2 - delta;   // :509
                    const bool p1 = t1 > F(0), p2 = t2 > F(0);
                    M1 = p1 ? t1 : F(0);
                    M2 = p2 ? t2 : F(0);
                    // sgn(c2v) of :511 maps -0.0 to +1; a zeroed message is +0 (:513)
                    const uint32_t abit = (amin < 31) ? (1u << amin) : 0u;
                    if (!p1 || mn1 == F(0)) eff &= abit;
                    if (!p2 || mn2 == F(0)) eff &= ~abit;
                }
                F2 nw;
                nw.x = M1;
                nw.y = M2;
                m12[i] = nw;
                meta[i] = (uint32_t)amin | (eff << 5);
#pragma unroll
                for (int k = 0; k < DC; ++k) {
                    if (k < deg) {
                        const F mag = (k == amin) ? M2 : M1;
                        c2v[fs.sq[(size_t)k * MP + i]] = ((eff >> k) & 1u) ? -mag : mag;
                    }
                }
            }
            __syncthreads();
            // ---- bit nodes: sum = yq + c2v in nlist order (:452-476) ----
            for (int p = tid; p < NP; p += nt) {
                const int d = fs.pdeg[p];
                if (d == 0) continue;
                const F *cp = c2v + fs.gbase[p >> 6] + (p & 63);
                F sum = yq[p];
                for (int e = 0; e < d; ++e) sum += cp[64 * e];
                app[p] = sum;
            }
            __syncthreads();
        }

        // ---- decisions, error weight (:270, :382-393), syndrome ----
        int w = 0, synd = 0;
        for (int v = tid; v < N; v += nt) {
            const int d = app[fs.pos_of_bit[v]] > F(0) ? 1 : -1;   // :471-474
            const int cv = cvec ? cvec[v] : 1;
            w += (d != cv);
            if (a.d_out) a.d_out[(size_t)b * N + v] = (int8_t)d;
        }
        for (int i = tid; i < MP; i += nt) {
            const int deg = fs.rdeg[i];
            int par = 0;
            for (int k = 0; k < deg; ++k) par ^= (app[fs.sp[(size_t)k * MP + i]] > F(0)) ? 0 : 1;
            synd |= par;
        }
        int sums[3] = {w, unc, synd};
        block_sum_n_t0<3>(sums, red + 32);
        if (tid == 0) frame_account_acc(acc, a.hist, a.frame_res, b, sums[0], sums[1], sums[2] > 0);
        __syncthreads();
    }
    if (tid == 0) frame_flush(a.counts, acc, a.T);
}

static size_t flood_slot_bytes(const DevGraph &g, const FloodSched &fs, bool f64)
{
    const size_t fsz = f64 ? 8 : 4, NP = (size_t)fs.ngroups * 64;
    const size_t nf = (NP + 1) + NP + ((size_t)fs.e_pad + 64 + 1) / 2 * 2;
    return (nf * fsz + (size_t)fs.M_pad * (2 * fsz + 4) + 255) & ~(size_t)255;
}

// =====================================================================
// Phase-per-launch flooding (codes beyond LDS; the default since round 2,
// LDPC_FLOOD_MODE=persistent selects k_decode_flood).
//
// The same per-codeword state slots, arithmetic and storage order as
// k_decode_flood, but the resident set is sized to stay inside the 256 MiB
// Infinity Cache (K codewords, K * slot_bytes ~ 150 MB) and every phase is
// its own launch over all K codewords: init (channel), T x {check, bit},
// finish (decisions, accounting). A launch boundary is the flooding
// barrier, so a codeword is no longer confined to one workgroup: one thread
// per row (check) or per bit position (bit) of every resident codeword, the
// whole GPU on each phase, with no spin-waits. Grid (blocks of the phase,
// K); slot r of the launch holds codeword b0 + r.
// =====================================================================
struct FloodSlot {
    template <typename F> struct View {
        F *app, *yq, *c2v;
        typename F2T<F>::T *m12;
        uint32_t *meta;
    };
    template <typename F>
    static __device__ __forceinline__ View<F> at(unsigned char *scratch, size_t slot_bytes, int r, const FloodSched &fs)
    {
        using F2 = typename F2T<F>::T;
        View<F> v;
        const int NP = fs.ngroups * 64;
        unsigned char *base = scratch + slot_bytes * (size_t)r;
        v.app = reinterpret_cast<F *>(base);
        v.yq = v.app + (NP + 1);
        v.c2v = v.yq + NP;
        v.m12 = reinterpret_cast<F2 *>(v.c2v + (fs.e_pad + 64 + 1) / 2 * 2);
        v.meta = reinterpret_cast<uint32_t *>(v.m12 + fs.M_pad);
        return v;
    }
};

template <typename F, int SRC>
__global__ __launch_bounds__(256) void k_flood_init(DecodeArgs a, DevGraph g, FloodSched fs, unsigned char *scratch,
                                                    size_t slot_bytes, int b0, int *unc_out)
{
    const int r = blockIdx.y, b = b0 + r;
    if (b >= a.batch) return;
    const auto S = FloodSlot::at<F>(scratch, slot_bytes, r, fs);
    const int N = g.N, NP = fs.ngroups * 64, MP = fs.M_pad;
    const int8_t *cvec = frame_codeword<SRC>(a, b, N);
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    int unc = 0;
    if (t * 4 < N) {   // ---- channel + front-end (:214-238) into storage order ----
        F yv[4];
        channel_group<F, SRC, false>(a, b, t, N, cvec, a.y_out, yv);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int v = t * 4 + q;
            if (v < N) {
                const F q2 = front_end<F>(yv[q], a);
                const int p = LDPC_CHK(fs.pos_of_bit[v], NP, CHK_FLOOD_APP);
                S.yq[p] = q2;
                S.app[p] = q2;
                const int cv = cvec ? cvec[v] : 1;
                unc += ((q2 > F(0) ? 1 : -1) * cv < 0);
            }
        }
    }
    for (int i = t; i < MP; i += gridDim.x * blockDim.x) {   // c2v_old = +0 (:364-370)
        typename F2T<F>::T z;
        z.x = F(0);
        z.y = F(0);
        S.m12[i] = z;
        S.meta[i] = 0;
    }
    if (t == 0) S.app[NP] = dinf<F>();   // sentinel position of padding slots
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) unc += __shfl_xor(unc, o, 64);
    if ((threadIdx.x & 63) == 0 && unc) atomicAdd(&unc_out[r], unc);
}

// Codewords per thread of the phase kernels: the row's (or bit position's)
// schedule is loaded once and used for CPW resident codewords (slots
// blockIdx.y + j * gridDim.y).
//
// The check node of k_decode_flood (:410-450, :494-515) on one resident slot:
// xa = the gathered app values, (old, om) = the row's packed state.
template <typename F, int DC, bool C2V>
__device__ __forceinline__ void flood_cn(const DecodeArgs &a, const FloodSlot::View<F> &S, int i, int deg,
                                         const int (&sq)[DC], const F (&xa)[DC], typename F2T<F>::T old, uint32_t om)
{
    using F2 = typename F2T<F>::T;
    const F alpha = (F)a.alpha, delta = (F)a.delta;
    const int oidx = (int)(om & 31u);
    F mn1 = dinf<F>(), mn2 = dinf<F>();
    int amin = 31;
    uint32_t sg = 0;
#pragma unroll
    for (int k = 0; k < DC; ++k) {
        if (k < deg) {
            F cold = (k == oidx) ? old.y : old.x;
            if ((om >> (5 + k)) & 1u) cold = -cold;
            const F x = xa[k] - cold;                     // v2c (:469)
            sg |= (uint32_t)(!(x >= F(0))) << k;          // sgn(v2c) < 0 (:518-523)
            const F ax = dabs(x);
            if (ax <= mn1) { mn2 = mn1; mn1 = ax; amin = k; }   // :428-433
            else if (ax < mn2) { mn2 = ax; }                    // :434-437
        }
    }
    const uint32_t degmask = (1u << deg) - 1u;
    uint32_t eff = (__popc(sg) & 1) ? (sg ^ degmask) : sg;   // prod * sgn(v2c_k)
    F M1 = mn1, M2 = mn2;
    if (a.variant == V_NMS) {
        M1 = nms_div<F>(mn1, alpha, a);               // :498
        M2 = nms_div<F>(mn2, alpha, a);
    } else if (a.variant == V_OMS) {
        const F t1 = mn1 - delta, t2 = mn2 - delta;   // :509
        const bool p1 = t1 > F(0), p2 = t2 > F(0);
        M1 = p1 ? t1 : F(0);
        M2 = p2 ? t2 : F(0);
        const uint32_t abit = (amin < 31) ? (1u << amin) : 0u;   // sgn(-0.0) = +1 (:511-513)
        if (!p1 || mn1 == F(0)) eff &= abit;
        if (!p2 || mn2 == F(0)) eff &= ~abit;
    }
    F2 nw;
    nw.x = M1;
    nw.y = M2;
    S.m12[i] = nw;
    S.meta[i] = (uint32_t)amin | (eff << 5);
    if constexpr (C2V) {
#pragma unroll
        for (int k = 0; k < DC; ++k) {
            if (k < deg) {
                const F mag = (k == amin) ? M2 : M1;
                S.c2v[sq[k]] = ((eff >> k) & 1u) ? -mag : mag;
            }
        }
    }
}

// The c2v message of position k of a row with packed state (m, meta): exactly
// the value flood_cn stores (magnitude M2 at the argmin, M1 elsewhere, signed
// by the row's sign bit k).
template <typename F>
__device__ __forceinline__ F flood_msg(typename F2T<F>::T m, uint32_t meta, uint32_t k)
{
    const F mag = (k == (meta & 31u)) ? m.y : m.x;
    return ((meta >> (5 + k)) & 1u) ? -mag : mag;
}

// SPS resident slots per step: their gathers are issued together (one memory
// round trip for SPS slots), the check nodes then run slot by slot.
template <typename F, int DC, int SPS, bool C2V>
__global__ __launch_bounds__(256) void k_flood_check(DecodeArgs a, FloodSched fs, unsigned char *scratch,
                                                     size_t slot_bytes, int nres)
{
    using F2 = typename F2T<F>::T;
    const int MP = fs.M_pad, NP = fs.ngroups * 64;
#if LDPC_FLOOD_XCD
    // XCD-aware: blocks b and b + 8 share an XCD (round-robin placement, speed
    // only); XCD x decodes the slots x, x + 8, ... one after the other, all
    // rows of a slot at once, so the ~3.5 gathers of each app value hit its L2.
    const int i = (blockIdx.x >> 3) * blockDim.x + threadIdx.x, r0 = blockIdx.x & 7, rs = 8;
#else
    const int i = blockIdx.x * blockDim.x + threadIdx.x, r0 = blockIdx.y, rs = gridDim.y;
#endif
    if (i >= MP) return;
    const int deg = fs.rdeg[i];
    if (deg == 0) return;
    int sp[DC], sq[DC];
#pragma unroll
    for (int k = 0; k < DC; ++k) {
        sp[k] = k < deg ? LDPC_CHK(fs.sp[(size_t)k * MP + i], NP + 1, CHK_FLOOD_APP) : NP;
        sq[k] = k < deg ? LDPC_CHK(fs.sq[(size_t)k * MP + i], fs.e_pad + 64, CHK_FLOOD_C2V) : 0;
    }
    for (int r = r0; r < nres; r += SPS * rs) {
        F xa[SPS][DC];
        F2 old[SPS];
        uint32_t om[SPS];
#pragma unroll
        for (int j = 0; j < SPS; ++j) {
            const int rr = r + j * rs < nres ? r + j * rs : r;   // past the end: a harmless re-read of slot r
            const auto S = FloodSlot::at<F>(scratch, slot_bytes, rr, fs);
#pragma unroll
            for (int k = 0; k < DC; ++k) xa[j][k] = S.app[sp[k]];
            old[j] = S.m12[i];
            om[j] = S.meta[i];
        }
#pragma unroll
        for (int j = 0; j < SPS; ++j)
            if (r + j * rs < nres)
                flood_cn<F, DC, C2V>(a, FloodSlot::at<F>(scratch, slot_bytes, r + j * rs, fs), i, deg, sq, xa[j],
                                     old[j], om[j]);
    }
}

// DV = a bound on the column degree: the d loads of a bit are issued together
// (one memory round trip per slot instead of d dependent ones; the adds stay in
// nlist order), and SPS slots are in flight per step. DV = 0: any degree, one
// load at a time.
template <typename F, int DV, int SPS>
__global__ __launch_bounds__(256) void k_flood_bit(FloodSched fs, unsigned char *scratch, size_t slot_bytes, int nres)
{
    const int NP = fs.ngroups * 64;
#if LDPC_FLOOD_XCD
    const int p = (blockIdx.x >> 3) * blockDim.x + threadIdx.x, r0 = blockIdx.x & 7, rs = 8;
#else
    const int p = blockIdx.x * blockDim.x + threadIdx.x, r0 = blockIdx.y, rs = gridDim.y;
#endif
    if (p >= NP) return;
    const int d = fs.pdeg[p];
    if (d == 0) return;
    const int off = fs.gbase[p >> 6] + (p & 63);
    [[maybe_unused]] const int ea = fs.e_pad + 64;
    if constexpr (DV == 0) {
        for (int r = r0; r < nres; r += rs) {
            const auto S = FloodSlot::at<F>(scratch, slot_bytes, r, fs);
            const F *cp = S.c2v + off;
            F sum = S.yq[p];
            for (int e = 0; e < d; ++e) sum += cp[LDPC_CHK(64 * e, ea - off, CHK_FLOOD_C2V)];   // nlist order (:452-476)
            S.app[p] = sum;
        }
    } else {
        for (int r = r0; r < nres; r += SPS * rs) {
            F v[SPS][DV], y[SPS];
#pragma unroll
            for (int j = 0; j < SPS; ++j) {
                const auto S = FloodSlot::at<F>(scratch, slot_bytes, r + j * rs < nres ? r + j * rs : r, fs);
                y[j] = S.yq[p];
#pragma unroll
                for (int e = 0; e < DV; ++e) v[j][e] = e < d ? S.c2v[LDPC_CHK(off + 64 * e, ea, CHK_FLOOD_C2V)] : F(0);
            }
#pragma unroll
            for (int j = 0; j < SPS; ++j) {
                F sum = y[j];
#pragma unroll
                for (int e = 0; e < DV; ++e)
                    if (e < d) sum += v[j][e];   // nlist order (:452-476)
                if (r + j * rs < nres) FloodSlot::at<F>(scratch, slot_bytes, r + j * rs, fs).app[p] = sum;
            }
        }
    }
}

// Bit phase without the c2v array (LDPC_FLOOD_MSG=packed, the default): each
// message is rebuilt from its row's packed state (m12, meta), gathered through
// the element -> (row, position) table eref. The check phase then writes only
// the 12 (fp32) / 20 (fp64) bytes of state per row instead of dc messages, and
// the bit phase reads each row's state once per L2 instead of a message per
// edge -- the same sums, in nlist order, of the same values.
template <typename F, int DV, int SPS>
__global__ __launch_bounds__(256) void k_flood_bit_packed(FloodSched fs, unsigned char *scratch, size_t slot_bytes,
                                                          int nres)
{
    using F2 = typename F2T<F>::T;
    const int NP = fs.ngroups * 64;
#if LDPC_FLOOD_XCD
    const int p = (blockIdx.x >> 3) * blockDim.x + threadIdx.x, r0 = blockIdx.x & 7, rs = 8;
#else
    const int p = blockIdx.x * blockDim.x + threadIdx.x, r0 = blockIdx.y, rs = gridDim.y;
#endif
    if (p >= NP) return;
    const int d = fs.pdeg[p];
    if (d == 0) return;
    const int off = fs.gbase[p >> 6] + (p & 63);
    uint32_t ref[DV];
#pragma unroll
    for (int e = 0; e < DV; ++e) {
        ref[e] = e < d ? fs.eref[LDPC_CHK(off + 64 * e, fs.e_pad + 64, CHK_FLOOD_C2V)] : 0u;
#ifdef LDPC_CHECK
        ref[e] = (LDPC_CHK(ref[e] >> 5, (uint32_t)fs.M_pad, CHK_FLOOD_ROW) << 5) | (ref[e] & 31u);
#endif
    }
    for (int r = r0; r < nres; r += SPS * rs) {
        F2 m[SPS][DV];
        uint32_t me[SPS][DV];
        F y[SPS];
#pragma unroll
        for (int j = 0; j < SPS; ++j) {
            const auto S = FloodSlot::at<F>(scratch, slot_bytes, r + j * rs < nres ? r + j * rs : r, fs);
            y[j] = S.yq[p];
#pragma unroll
            for (int e = 0; e < DV; ++e)
                if (e < d) {
                    m[j][e] = S.m12[ref[e] >> 5];
                    me[j][e] = S.meta[ref[e] >> 5];
                }
        }
#pragma unroll
        for (int j = 0; j < SPS; ++j) {
            F sum = y[j];
#pragma unroll
            for (int e = 0; e < DV; ++e)
                if (e < d) sum += flood_msg<F>(m[j][e], me[j][e], ref[e] & 31u);   // nlist order (:452-476)
            if (r + j * rs < nres) FloodSlot::at<F>(scratch, slot_bytes, r + j * rs, fs).app[p] = sum;
        }
    }
}

// Decisions, error weight (:270, :382-393) and syndrome of every resident
// codeword: one thread per bit / row, per-slot sums by atomics.
template <typename F>
__global__ __launch_bounds__(256) void k_flood_finish(DecodeArgs a, DevGraph g, FloodSched fs, unsigned char *scratch,
                                                      size_t slot_bytes, int b0, int nres, int *wsum, int *ssum)
{
    const int N = g.N, MP = fs.M_pad;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    for (int r = blockIdx.y; r < nres; r += gridDim.y) {
        const int b = b0 + r;
        const auto S = FloodSlot::at<F>(scratch, slot_bytes, r, fs);
        int w = 0, par = 0;
        if (t < N) {
            const int8_t *cvec = a.src == SRC_GIVEN ? frame_codeword<SRC_GIVEN>(a, b, N) : frame_codeword<SRC_PHILOX>(a, b, N);
            const int d = S.app[LDPC_CHK(fs.pos_of_bit[t], fs.ngroups * 64 + 1, CHK_FLOOD_APP)] > F(0) ? 1 : -1;   // :471-474
            w = d != (cvec ? cvec[t] : 1);
            if (a.d_out) a.d_out[(size_t)b * N + t] = (int8_t)d;
        }
        if (t < MP) {
            const int deg = fs.rdeg[t];
            for (int k = 0; k < deg; ++k)
                par ^= (S.app[LDPC_CHK(fs.sp[(size_t)k * MP + t], fs.ngroups * 64 + 1, CHK_FLOOD_APP)] > F(0)) ? 0 : 1;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            w += __shfl_xor(w, o, 64);
            par += __shfl_xor(par, o, 64);
        }
        if ((threadIdx.x & 63) == 0) {
            if (w) atomicAdd(&wsum[r], w);
            if (par) atomicAdd(&ssum[r], par);
        }
    }
}

// The frame accounting of the resident codewords (one thread per slot).
__global__ __launch_bounds__(256) void k_flood_account(DecodeArgs a, int b0, int nres, const int *unc,
                                                       const int *wsum, const int *ssum)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nres) return;
    frame_account(a.counts, a.hist, a.frame_res, b0 + r, wsum[r], unc[r], ssum[r] > 0, a.T, 0);
}

// Messages between the phases: the packed row state (default) or the c2v
// array (option LDPC_OPT_FLOOD_MSG = 1). The packed bit phase is built for column degrees
// up to 32 (k_flood_bit_packed<F, 8|16|32>); a code with a heavier column takes
// the c2v array, whose bit phase has an any-degree instance (DV = 0).
constexpr int kFloodPackedMaxDv = 32;
static bool flood_packed(const FloodSched &fs)
{
    if (fs.dv > kFloodPackedMaxDv) return false;
    return opt(LDPC_OPT_FLOOD_MSG) != 1;
}

// Resident slots per step of the check (LDPC_OPT_FLOOD_SPS_CHECK) and bit
// (LDPC_OPT_FLOOD_SPS_BIT) phase kernels.
static int flood_sps(bool check, const FloodSched &fs)
{
    if (const int v = opt(check ? LDPC_OPT_FLOOD_SPS_CHECK : LDPC_OPT_FLOOD_SPS_BIT)) return v;
    return check || flood_packed(fs) ? 1 : 2;   // packed bit phase: 1 (2 204 vs 2 124 Mbit/s fp32)
}

// Resident codewords of the phase-per-launch flooding: the state the phases
// touch fits the Infinity Cache with room to spare. `touched` = bytes per slot
// the phases read and write (the packed-message phases leave the c2v array of
// the slot alone). Measured on DVB-S2 R1/2 with packed messages (4096
// codewords, T=50): fp32 K = 96/112/128/144 -> 2277/2307/2331/2310 Mbit/s,
// fp64 K = 64/80/96/128 -> 1520/1508/1487/1401 -- best near 110 MB touched.
// LDPC_OPT_FLOOD_RESIDENT overrides.
constexpr size_t kFloodPhaseExtra = 65536;   // per-slot counters after the slots (3 ints per slot)
static int flood_phase_resident(size_t touched, int slots)
{
    long k = (long)((112ull << 20) / touched);
    if (const int v = opt(LDPC_OPT_FLOOD_RESIDENT)) k = v;
    if (k > 4096) k = 4096;
    if (k > slots) k = slots;   // the scratch the plan asks for
    return k < 1 ? 1 : (int)k;
}

// The phase launches of resident slots [lo, lo + n) of a chunk whose first codeword
// is b0: init, T x (check, bit), finish, accounting -- issued on stream s.
template <typename F, int SRC>
struct FloodHalf {
    const DevGraph *g;
    const FloodSched *fs;
    const DecodeArgs *a;
    unsigned char *scratch;
    size_t sb;
    int *unc, *wsum, *ssum;   // per-slot counters (index = slot)
    hipStream_t s;
    int lo, n;
    hipError_t begin(int b0) const
    {
        if (n <= 0) return hipSuccess;
        hipError_t e = hipMemsetAsync(unc + lo, 0, sizeof(int) * (size_t)n, s);
        if (e == hipSuccess) e = hipMemsetAsync(wsum + lo, 0, sizeof(int) * (size_t)n, s);
        if (e == hipSuccess) e = hipMemsetAsync(ssum + lo, 0, sizeof(int) * (size_t)n, s);
        if (e != hipSuccess) return e;
        const int ib = ((g->N + 3) / 4 + 255) / 256;
        hipLaunchKernelGGL((k_flood_init<F, SRC>), dim3(ib > 1 ? ib : 1, n), dim3(256), 0, s, *a, *g, *fs,
                           scratch + sb * (size_t)lo, sb, b0 + lo, unc + lo);
        return hipSuccess;
    }
    void check() const
    {
        if (n <= 0) return;
        const int NPc = fs->M_pad;
#if LDPC_FLOOD_XCD
        const dim3 cg(8 * ((NPc + 255) / 256));
#else
        const dim3 cg((NPc + 255) / 256, (n + LDPC_FLOOD_CPW - 1) / LDPC_FLOOD_CPW);
#endif
        unsigned char *sc = scratch + sb * (size_t)lo;
        const int sps = flood_sps(true, *fs);
        const bool packed = flood_packed(*fs);
#define CHK(DC, SPS)                                                                                     \
    do {                                                                                                 \
        if (packed) hipLaunchKernelGGL((k_flood_check<F, DC, SPS, false>), cg, dim3(256), 0, s, *a, *fs, sc, sb, n); \
        else hipLaunchKernelGGL((k_flood_check<F, DC, SPS, true>), cg, dim3(256), 0, s, *a, *fs, sc, sb, n);         \
    } while (0)
        if (fs->dc <= 8) {
            if (sps >= 4) CHK(8, 4);
            else if (sps == 2) CHK(8, 2);
            else CHK(8, 1);
        } else if (fs->dc <= 16) {
            if (sps >= 2) CHK(16, 2);
            else CHK(16, 1);
        } else {
            CHK(32, 1);
        }
#undef CHK
    }
    void bit() const
    {
        if (n <= 0) return;
        const int NP = fs->ngroups * 64;
#if LDPC_FLOOD_XCD
        const dim3 bg(8 * ((NP + 255) / 256));
#else
        const dim3 bg((NP + 255) / 256, (n + LDPC_FLOOD_CPW - 1) / LDPC_FLOOD_CPW);
#endif
        unsigned char *sc = scratch + sb * (size_t)lo;
        const int sps = flood_sps(false, *fs);
        if (flood_packed(*fs)) {
            if (fs->dv <= 8) {
                if (sps >= 2) hipLaunchKernelGGL((k_flood_bit_packed<F, 8, 2>), bg, dim3(256), 0, s, *fs, sc, sb, n);
                else hipLaunchKernelGGL((k_flood_bit_packed<F, 8, 1>), bg, dim3(256), 0, s, *fs, sc, sb, n);
            } else if (fs->dv <= 16) {
                hipLaunchKernelGGL((k_flood_bit_packed<F, 16, 1>), bg, dim3(256), 0, s, *fs, sc, sb, n);
            } else {
                hipLaunchKernelGGL((k_flood_bit_packed<F, 32, 1>), bg, dim3(256), 0, s, *fs, sc, sb, n);
            }
            return;
        }
        if (fs->dv <= 8) {
            if (sps >= 4) hipLaunchKernelGGL((k_flood_bit<F, 8, 4>), bg, dim3(256), 0, s, *fs, sc, sb, n);
            else hipLaunchKernelGGL((k_flood_bit<F, 8, 2>), bg, dim3(256), 0, s, *fs, sc, sb, n);
        } else if (fs->dv <= 16) {
            if (sps >= 4) hipLaunchKernelGGL((k_flood_bit<F, 16, 4>), bg, dim3(256), 0, s, *fs, sc, sb, n);
            else hipLaunchKernelGGL((k_flood_bit<F, 16, 2>), bg, dim3(256), 0, s, *fs, sc, sb, n);
        } else {
            hipLaunchKernelGGL((k_flood_bit<F, 0, 1>), bg, dim3(256), 0, s, *fs, sc, sb, n);
        }
    }
    void end(int b0) const
    {
        if (n <= 0) return;
        const int gy = (n + LDPC_FLOOD_CPW - 1) / LDPC_FLOOD_CPW;
        const int fx = ((g->N > fs->M_pad ? g->N : fs->M_pad) + 255) / 256;
        hipLaunchKernelGGL((k_flood_finish<F>), dim3(fx, gy), dim3(256), 0, s, *a, *g, *fs, scratch + sb * (size_t)lo,
                           sb, b0 + lo, n, wsum + lo, ssum + lo);
        hipLaunchKernelGGL(k_flood_account, dim3((n + 255) / 256), dim3(256), 0, s, *a, b0 + lo, n, unc + lo, wsum + lo,
                           ssum + lo);
    }
};

// The resident set in two halves on two streams (aux): one half's launch
// boundaries and its small init / finish / accounting launches overlap the other
// half's phase kernels. The single stream is 95 % busy already
// (profiles/r03_dvbs2_flood_gaps.json).
// LDPC_OPT_FLOOD_STREAMS = 2 (opt-in): measured +6 % while the bit kernel's loads were
// serialised, 7 % slower once they are batched (1 855 vs 2 000 Mbit/s).
static bool flood_two_streams() { return opt(LDPC_OPT_FLOOD_STREAMS) == 2; }

template <typename F, int SRC>
static hipError_t launch_flood_phase_t(const DevGraph &g, const FloodSched &fs, const DecodeArgs &a,
                                       const LaunchPlan &p, void *gs, hipStream_t s, const AuxStream *aux)
{
    const size_t sb = p.scratch_per_block;
    const int K = p.grid;
    unsigned char *scratch = (unsigned char *)gs;
    int *unc = reinterpret_cast<int *>(scratch + sb * (size_t)K);   // per-slot counters after the slots
    int *wsum = unc + K, *ssum = wsum + K;
    const bool two = aux && aux->s && flood_two_streams() && K >= 2;
    hipError_t e;
    if (two) {   // fork: the aux stream starts after everything queued on s
        if ((e = hipEventRecord(aux->fork, s)) != hipSuccess) return e;
        if ((e = hipStreamWaitEvent(aux->s, aux->fork, 0)) != hipSuccess) return e;
    }
    for (int b0 = 0; b0 < a.batch; b0 += K) {
        const int nres = a.batch - b0 < K ? a.batch - b0 : K;
        const int na = two ? (nres + 1) / 2 : nres;
        const FloodHalf<F, SRC> A{&g, &fs, &a, scratch, sb, unc, wsum, ssum, s, 0, na};
        const FloodHalf<F, SRC> B{&g, &fs, &a, scratch, sb, unc, wsum, ssum, two ? aux->s : s, na, nres - na};
        if ((e = A.begin(b0)) != hipSuccess) return e;
        if ((e = B.begin(b0)) != hipSuccess) return e;
        for (int it = 0; it < a.T; ++it) {
            A.check();
            B.check();
            A.bit();
            B.bit();
        }
        A.end(b0);
        B.end(b0);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (two) {   // join: s continues after the aux stream's last launch
        if ((e = hipEventRecord(aux->join, aux->s)) != hipSuccess) return e;
        if ((e = hipStreamWaitEvent(s, aux->join, 0)) != hipSuccess) return e;
    }
    return hipSuccess;
}

LDPC_CHECK_TU(flood)

// Flooding of codes beyond LDS: one launch per phase over an Infinity-Cache-
// resident set (default; 1.5x the persistent kernel on DVB-S2) or the
// persistent workgroup-per-codeword kernel (LDPC_OPT_FLOOD_MODE = 1).
bool plan_flood(const PlanInput &in, LaunchPlan &p)
{
    if (!in.fs || in.fs->M_pad <= 0 || in.fs->dc > kPackedMaxDc) return false;
    const FloodSched &fs = *in.fs;
    p = LaunchPlan{};
    p.name = "flood";
    p.threads = 512;
    const size_t sb = p.scratch_per_block = flood_slot_bytes(in.g, fs, in.f64);
    // reported, and the resident blocks of either mode's scratch (kernels.hip plan_lds)
    p.blocks_per_cu = occupancy(in.f64 ? (const void *)k_decode_flood<double, SRC_PHILOX, 8>
                                       : (const void *)k_decode_flood<float, SRC_PHILOX, 8>, p.threads, 0);
    int per_cu = p.blocks_per_cu;
    if (const int cap = opt(LDPC_OPT_FLOOD_BPC)) per_cu = std::min(per_cu, cap);   // experiments
    if (per_cu <= 0) per_cu = 1;
    const int slots = std::min(per_cu * in.num_cus, in.a.batch);
    p.scratch_bytes = sb * (size_t)slots + kFloodPhaseExtra;
    if (opt(LDPC_OPT_FLOOD_MODE) == 1) {
        p.kernel = Kernel::flood_persistent;
        p.grid = slots;
        p.fn = for_f_src(in.f64, in.a.src, [&](auto f, auto s) {
            using F = typename decltype(f)::type;
            constexpr int SRC = decltype(s)::value;
            return fs.dc <= 8 ? (const void *)k_decode_flood<F, SRC, 8>
                              : fs.dc <= 16 ? (const void *)k_decode_flood<F, SRC, 16> : (const void *)k_decode_flood<F, SRC, 32>;
        });
    } else {
        p.kernel = Kernel::flood_phase;
        const size_t c2v_bytes = (size_t)((fs.e_pad + 64 + 1) / 2 * 2) * (in.f64 ? 8 : 4);
        p.grid = flood_phase_resident(flood_packed(fs) ? sb - c2v_bytes : sb, slots);
    }
    return true;
}

hipError_t launch_flood(const LaunchPlan &p, const DevGraph &g, const FloodSched &fs, const DecodeArgs &a, bool f64,
                        void *gscratch, hipStream_t s, const AuxStream *aux)
{
    if (p.kernel == Kernel::flood_phase)
        return for_f_src(f64, a.src, [&](auto f, auto src) {
            return launch_flood_phase_t<typename decltype(f)::type, decltype(src)::value>(g, fs, a, p, gscratch, s, aux);
        });
    unsigned char *gs = (unsigned char *)gscratch;
    size_t sb = p.scratch_per_block;
    void *args[] = {(void *)&a, (void *)&g, (void *)&fs, &gs, &sb};
    return launch_fn(p, args, s);
}

}  // namespace ldpc
