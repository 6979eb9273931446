// rows_pp.hip -- the headline kernel: flooding min-sum (src/decodeMinSum.cpp
// :247-263, check node :410-450, normalisation :494-515, bit node :452-476)
// with check and bit work of two codeword slots overlapped in one workgroup.
// A slot holds one fp64 codeword (the reference's arithmetic) or an fp32 pair
// interleaved as float2 (the fp32 throughput path): the same 8-byte LDS words,
// schedule and roles either way.
//
// k_rows_fast (rows_fast.hip) decodes one codeword per 512-thread block; inside
// a block the check phase (VALU-heavy: the f64 tournament, division, selects)
// and the bit phase (LDS-latency-bound: c2v reads and dependent adds) alternate
// between barriers, so a CU's VALU and LDS pipe are each busy only about half
// the time. Here one 1024-thread block holds TWO
// codewords (slots 0 and 1, 2 x 74 KB of LDS for N=1944) and its waves are
// specialised:
//   waves 0-7  (the check role) own check rows t and t+512, as k_rows_fast's
//              threads do, with their schedule in registers;
//   waves 8-15 (the bit role) own the bit slots of k_rows_fast's thread t-512.
// Between two barriers the check role runs iteration i of one slot while the
// bit role runs the bit nodes of the other slot:
//   | check(0,0) | check(1,0)  | check(0,1)  | ... | check(1,T-1) |             |
//   |            | bit(0,0)    | bit(1,0)    | ... | bit(0,T-1)   | bit(1,T-1)  |
// so every interval carries one check phase and one bit phase, on different
// waves of the same SIMDs: 2T + 1 barrier intervals per pair instead of 4T.
// A slot's check(i+1) follows its bit(i), which follows its check(i), each an
// interval apart: the flooding schedule of each codeword is unchanged, and so
// is every value (same arithmetic as k_rows_fast: cn_fast64 of fast64.h, sums
// in nlist order), hence the decisions equal the reference's bit for bit.
//
// The c2v a row sent last iteration (the `- msg` of :469) is kept per slot in
// registers (prev: 2 slots x rows x 8 edges); re-reading it from the row's own
// c2v slots instead (8 more ds_read_b64 per row) measured slower (16.9 vs 14.7 ms).
//
// Premise failures (fast64.h for fp64, minsum_common.h cn_fast for fp32): the
// slot's flag is raised and its codeword(s) are re-decoded on the exact path
// (k_redo) after the launch; the other slot is unaffected. Rows past M (degree 0) gather app[N + 2] = +0, so
// their messages stay 0 (their scatters land in per-lane dummy slots that the
// padding edges of real rows also use; those read +inf - finite = +inf).
//
// k_rows_ppi (in-register bits, fp64 slots): a degree-2 bit whose two check rows are the two rows of
// one check thread (graph.h pp_pair_rows: the dual-diagonal parity bits of the 802.11n
// codes, one per check thread) has no bit slot and no c2v element. Its posterior
// (yq + c2v_first) + c2v_second -- the bit node's sum in nlist order -- is formed by that
// thread from its own prev registers and the staged yq (app[bit], which nobody overwrites)
// at the start of the row's interval, and takes the place of the gather at the last
// position of both rows' check nodes; the two scatters, the bit role's two reads and its
// app write are not issued. The thread also forms the bit's decision, error weight and
// share of both rows' syndrome from the final prev. Same values, same order of additions.
// The fp64 bit role's read depth (minsum_common.h vn_phase: edges in flight per step with >= 3
// / < 3 active slots). 2 / 4 was the optimum while the check role was longer;
// re-measured with the shortened check stream, 4 / 8 is faster on the bench instance;
// it holds for every fp64 instance of this file. A build that sets the older switches
// (-DLDPC_VN_U3 / -DLDPC_VN_U1, the A/B recipes of DESIGN §5b) sets the fp64 depths with them.
#ifndef LDPC_VN_U3_F64
#ifdef LDPC_VN_U3
#define LDPC_VN_U3_F64 LDPC_VN_U3
#else
#define LDPC_VN_U3_F64 4
#endif
#endif
#ifndef LDPC_VN_U1_F64
#ifdef LDPC_VN_U1
#define LDPC_VN_U1_F64 LDPC_VN_U1
#else
#define LDPC_VN_U1_F64 8
#endif
#endif
#include "kernels.h"
#include "device_common.h"
#include "minsum_common.h"
#include "fast64.h"

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <type_traits>

namespace ldpc {

namespace {

// Timing experiments only (wrong results; `make ppvariant`): LDPC_PP_EXP =
// 1 bit role idle (barriers only), 2 check role idle, 3 check node replaced by
// a subtraction, 4 no c2v scatters, 5 gathers at lane-contiguous addresses (no
// bank conflicts), 6 scatters at lane-contiguous addresses, 7 both 5 and 6.
// LDPC_PP_BITDELAY: s_sleep units (64 cycles) the bit waves wait at an interval's start.
// fp64 premise flag: 0 = each row's hi-word maximum (fast64.h ACC) tested by a
// wave-uniform branch right after the row (no register lives across the step);
// 1 = a per-slot sticky maximum tested once after the step's last iteration (two
// VGPRs across the interval loop: the kernel setup then spills 16 B more per lane).
#ifndef LDPC_PP_STICKY
#define LDPC_PP_STICKY 0
#endif
// Timing ablations of the per-step work (results wrong by design): 1 no channel
// generation, 2 no syndrome / decisions, 4 no block reduction.
// Bit mask of the precisions (1 fp32 pairs, 2 fp64) whose step tail is folded into the
// last intervals: the bit role takes a slot's decisions and error weights from the sums of
// that slot's last bit-node pass (the values it writes to app), and the check role forms
// slot 0's syndrome in the extra interval, where it is idle; only slot 1's syndrome stays
// after the last barrier. Otherwise all of it follows the last barrier. Measured: fp32
// 7.16-7.21 -> 7.10-7.12 ms; fp64 12.28-12.29 -> 12.31 (the decisions lengthen the
// check-bound interval of bit(0,T-1)), so fp64 keeps the tail after the barrier.
#ifndef LDPC_PP_TAILFUSE
#define LDPC_PP_TAILFUSE 1
#endif
#ifndef LDPC_PP_TAILEXP
#define LDPC_PP_TAILEXP 0
#endif
// 1: the step's channel is generated by all 16 waves (one Philox group per thread and
// codeword pair at N <= 2048); 0: by the 8 bit waves (two groups per thread).
#ifndef LDPC_PP_CHAN_ALL
#define LDPC_PP_CHAN_ALL 0
#endif
// 1: no B2 -- the channel stages yq + 0 and flags the premise itself; the bit waves read
// their yq back during the first interval (where they are idle), the sentinels app[N] = inf
// and app[N + 2] = +0 are written once per kernel; 0: the bit waves re-stage yq between B1
// and B2 (read, canonicalise, check, write back).
#ifndef LDPC_PP_NOB2
#define LDPC_PP_NOB2 1
#endif
// 1: a plain step's channel (pp_plain_step) is generated by all 16 waves, one Philox group
// per thread at N = 1944 fp64 (the check waves otherwise wait at B1); other steps by the bit
// waves. 0: always the bit waves. (LDPC_PP_CHAN_ALL puts the general loop on all waves.)
#ifndef LDPC_PP_CHAN_SPLIT
#define LDPC_PP_CHAN_SPLIT 0
#endif
#ifndef LDPC_PP_EXP
#define LDPC_PP_EXP 0
#endif
// Wrong-result timing switches build only into A/B libraries (the *variant targets define
// LDPC_AB_BUILD); a product build with one of them set is refused.
#if LDPC_PP_EXP != 0 && !defined(LDPC_AB_BUILD)
#error "LDPC_PP_EXP != 0 gives wrong results by design: make ppvariant only"
#endif
#if LDPC_PP_TAILEXP != 0 && !defined(LDPC_AB_BUILD)
#error "LDPC_PP_TAILEXP != 0 gives wrong results by design: make ppvariant only"
#endif
#ifndef LDPC_PP_BITDELAY
#define LDPC_PP_BITDELAY 0
#endif
// 0: no scheduling fence between a check wave's two rows (the compiler may interleave them)
#ifndef LDPC_PP_ROWFENCE
#define LDPC_PP_ROWFENCE 1
#endif

// Wave priority (s_setprio): 0 none, 1 check role above the bit role, 2 the reverse,
// 3 the younger half of each role (waves 4-7, 12-15) above the older half, 4 the younger
// check waves (4-7) above all others, 5 younger check > older check > bit waves.
#ifndef LDPC_PP_PRIO
#define LDPC_PP_PRIO 0
#endif
// 1: the check role issues both rows' LDS reads before computing row 0; 0: row 1's after it.
#ifndef LDPC_PP_PREFETCH
#define LDPC_PP_PREFETCH 1
#endif
// 1: the fp64 check node's scatters are pinned in per-edge order behind each message's
// selects (sched_group_barrier); 0: the machine scheduler places them (it tended to sink
// all of a row's stores behind all of its selects, a 3 % swing between builds).
#ifndef LDPC_PP_STORE_ORDER
#define LDPC_PP_STORE_ORDER 1
#endif
// 1: the scheduler is asked to issue all of an interval's gathers before the check-node
// arithmetic (sched_group_barrier); 0: left to the scheduler.
#ifndef LDPC_PP_GATHER_FIRST
#define LDPC_PP_GATHER_FIRST 0
#endif
// k_rows_ppi, where the staged sample of a check thread's in-register bit lives: 0 one
// ds_read_b64 of app[bit] per interval (nobody overwrites that word); 1 two registers per
// slot, read back after B1 as the bit waves read their yq (pp_role IR == 1 only). Measured
// 11.42-11.44 (1) against 11.52-11.54 ms (0) per bench launch.
#ifndef LDPC_PP_INREG_Y
#define LDPC_PP_INREG_Y 1
#endif
// fp64 check role, N > 0: row 1's front (its v2c subtractions, two-min tournament and sign
// parity: fast64.h CnFront64) is issued inside row 0's per-edge store chain, N operations
// behind each of row 0's edges in source order and in that edge's pinned VALU group
// (LDPC_PP_STORE_ORDER), so that they fill the compare -> select wait states; what is left of
// the front, and the rest of row 1, stays behind the row fence. 0: row 1 follows row 0 whole.
// Same operations on the same operands. Measured: DESIGN §5g.
#ifndef LDPC_PP_ILV
#define LDPC_PP_ILV 2
#endif
// LDPC_PP_ILV: row 0's first edges that take no operation of row 1 (their stores issue as early as without it)
#ifndef LDPC_PP_ILV_SKIP
#define LDPC_PP_ILV_SKIP 0
#endif
// 1: the check role's address arithmetic reads the slot's app / c2v base from an SGPR
// (fast64.h addr8 SB) and the fp64 reciprocal of alpha lives in an SGPR pair; 0: VGPR copies.
#ifndef LDPC_PP_SBASE
#define LDPC_PP_SBASE 0
#endif
// fp64 premise flag (LDPC_PP_STICKY 0), 1: row 0's hi-word maximum is carried into row 1's
// (fast64.h ACC takes the maximum) and tested once per interval, after row 1; both rows flag
// the same slot, so the same codewords are re-decoded. 0: one test per row.
#ifndef LDPC_PP_ONEPREM
#define LDPC_PP_ONEPREM 1
#endif
// k_rows_ppw (the 12-wave block: 8 check waves as in k_rows_ppi, 4 bit waves that each take the
// bit slots of two schedule threads; 168 VGPRs per wave instead of 128). It runs on the
// in-register schedule with 3 bit slots per schedule thread (the 4-slot one was not measured
// and stays on k_rows_ppi: 40 + 80 registers of read addresses and values) and on the fixed-stride LDS layout (pp_slots FIX): slot 1 of app / c2v lies a compile-time
// distance behind slot 0, so the slot is selected by the immediate offset of the ds_read_b64 /
// ds_write_b64 and one base serves both.
// LDPC_PP_W12_UNP 1: a check row's gather and scatter byte addresses (slot 0's) are formed once
// per launch and kept in registers; 0: from the packed 16-bit schedule per edge.
#ifndef LDPC_PP_W12_UNP
#define LDPC_PP_W12_UNP 1
#endif
// k_rows_ppw's bit role: reads of a lane's slot 0 (the largest group degree) / of
// its other slots that are issued ahead of the first add; edges past them take one round trip each.
#ifndef LDPC_PP_W12_K0
#define LDPC_PP_W12_K0 12
#endif
#ifndef LDPC_PP_W12_K1
#define LDPC_PP_W12_K1 4
#endif
#if LDPC_PP_SBASE && !defined(LDPC_CHECK)
#define PP_ADDR8(DC, w, k, base, n, site) addr8<DC, true>(w, k, base)
#else
#define PP_ADDR8(DC, w, k, base, n, site) LDPC_ADDR8(DC, w, k, base, n, site)
#endif

// Diagnostic builds (-DLDPC_STAMPS, `make ppvariant`): per wave, s_memtime cycles
// spent working and waiting at the interval barriers, to a.stamps[(block*16+wave)*2].
#ifdef LDPC_STAMPS
#define PP_STAMP_DECL unsigned long long st_work = 0, st_wait = 0, st_step[6] = {}, st_t0 = __builtin_amdgcn_s_memtime()
#define PP_BARRIER()                                                        \
    do {                                                                    \
        const unsigned long long te_ = __builtin_amdgcn_s_memtime();        \
        __syncthreads();                                                    \
        const unsigned long long tb_ = __builtin_amdgcn_s_memtime();        \
        st_work += te_ - st_t0;                                             \
        st_wait += tb_ - te_;                                               \
        st_t0 = tb_;                                                        \
    } while (0)
// Per step, to a.stamps[8192 + (block*16+wave)*6 + k]: k = 0 the tail (last interval
// barrier -> the next step's top: syndrome, decisions, the block accounting), 1 the channel
// (step top -> B1), 2 the wait at B1, 3 the yq staging (B1 -> B2), 4 the wait at B2, 5 the
// syndrome and decisions after the last interval barrier (k = 0 is then the block accounting).
#define PP_STAMP_ACC(k)                                                     \
    do {                                                                    \
        const unsigned long long t_ = __builtin_amdgcn_s_memtime();         \
        st_step[k] += t_ - st_t0;                                           \
        st_t0 = t_;                                                         \
    } while (0)
#define PP_STAMP_TOP() PP_STAMP_ACC(0)
#define PP_SYNC_STAMPED(k0)                                                 \
    do {                                                                    \
        PP_STAMP_ACC(k0);                                                   \
        __syncthreads();                                                    \
        PP_STAMP_ACC(k0 + 1);                                               \
    } while (0)
#define PP_STAMP_OUT()                                                                              \
    if (a.stamps && (threadIdx.x & 63) == 0 && blockIdx.x < 256) {                                  \
        a.stamps[(blockIdx.x * 16 + (threadIdx.x >> 6)) * 2] = st_work;                             \
        a.stamps[(blockIdx.x * 16 + (threadIdx.x >> 6)) * 2 + 1] = st_wait;                         \
        for (int k_ = 0; k_ < 6; ++k_)                                                              \
            a.stamps[8192 + (blockIdx.x * 16 + (threadIdx.x >> 6)) * 6 + k_] = st_step[k_];         \
    }
#else
#define PP_STAMP_DECL
#define PP_BARRIER() __syncthreads()
#define PP_STAMP_TOP()
#define PP_STAMP_ACC(k)
#define PP_SYNC_STAMPED(k0) __syncthreads()
#define PP_STAMP_OUT()
#endif

constexpr int kPPRole = 512;          // threads per role
constexpr int kPPWaves = 2 * kPPRole / 64;
constexpr int kPPMaxCw = 4;           // codewords per block step (2 slots x an fp32 pair)
// red[] ints: [0,2) slot flags, [32, 32 + 16 waves x 3 x 4 codewords) block sums, then acc (6 x u64)
constexpr int kPPRedSums = 32;
constexpr int kPPRedAcc = kPPRedSums + kPPWaves * 3 * kPPMaxCw;
constexpr int kPPRedInts = kPPRedAcc + 2 * 6 + 4;
static_assert(kPPRedAcc % 2 == 0 && kPPRedAcc + 2 * 6 <= kPPRedInts, "acc (6 x u64) outside red[]");

// f(integral_constant<int, I>) for I = B .. E-1: a row loop whose index is a
// compile-time constant (each row slot has its own compile-time degree)
template <int B, int E, typename Fn>
__device__ __forceinline__ void static_for(Fn &&f)
{
    if constexpr (B < E) {
        f(std::integral_constant<int, B>());
        static_for<B + 1, E>(f);
    }
}

template <typename F> struct PPCw { static constexpr int C = sizeof(F) == 8 ? 1 : 2; };   // codewords per slot

template <typename P>
struct PPSlots {
    P *app[2], *c2v[2];
    uint32_t app_base[2], c2v_base[2];   // LDS byte addresses
    int *red;
};

// 8-byte words per slot (app[N + 3] then c2v[EA]), even so that both slots' app arrays are
// 16-byte aligned (the channel's ds_write_b128 pairs)
__host__ __device__ constexpr int pp_slot_words(int N, int EA) { return (N + 3 + EA + 1) & ~1; }

// The fixed-stride layout (k_rows_ppw): app[0] at 0, app[1] at kPPAppStride; behind them per slot
// one word that holds +0 (what the bit role reads for an edge its bit-slot group does not have)
// and the slot's c2v array of at most kPPC2vStride bytes, slot 1's word and array kPPC2vDist
// bytes behind slot 0's (a ds instruction's offset field holds 16 bits); red[] behind c2v[1].
constexpr uint32_t kPPAppStride = 16384, kPPC2vStride = 65520, kPPC2vDist = kPPC2vStride + 8;

template <typename P, bool FIX = false>
__device__ __forceinline__ PPSlots<P> pp_slots(unsigned char *smem, int N, int EA)
{
    static_assert(sizeof(P) == 8, "one 8-byte LDS word per slot element");
    PPSlots<P> s;
    P *b = reinterpret_cast<P *>(smem);
    if constexpr (FIX) {
#pragma unroll
        for (int X = 0; X < 2; ++X) {
            s.app[X] = b + X * (kPPAppStride / 8);
            s.c2v[X] = b + (2 * kPPAppStride + 8 + X * kPPC2vDist) / 8;   // the +0 word is c2v[X][-1]
            s.app_base[X] = lds_addr_of(s.app[X]);
            s.c2v_base[X] = lds_addr_of(s.c2v[X]);
        }
        s.red = reinterpret_cast<int *>(s.c2v[1] + EA);
        return s;
    }
    const int SL = pp_slot_words(N, EA);
#pragma unroll
    for (int X = 0; X < 2; ++X) {
        s.app[X] = b + X * SL;
        s.c2v[X] = s.app[X] + (N + 3);
        s.app_base[X] = lds_addr_of(s.app[X]);
        s.c2v_base[X] = lds_addr_of(s.c2v[X]);
    }
    s.red = reinterpret_cast<int *>(b + 2 * SL);
    return s;
}

// The common step (the bench's): all 2C codewords in the batch, the all-zero codeword
// (c = +1), no front end, no sample output, N a multiple of 4. Wave-uniform (kernel
// arguments and the step index).
__device__ __forceinline__ bool pp_plain_step(const DecodeArgs &a, int N, int grp, int C)
{
    return !a.cw_table && !a.y_out && !a.quantize && !a.saturate && (N & 3) == 0 && (grp + 1) * 2 * C <= a.batch;
}

// The channel of a plain step in straight-line code: the values of pp_channel's general
// loop (LDPC_PP_NOB2: yq + 0 staged, the premise flagged in *bad); fp64 slots store each
// pair of samples with one ds_write_b128. Items t0, t0 + nt, ...; unc[q] += this thread's
// uncoded errors (the caller zeroes unc).
template <typename F>
__device__ __forceinline__ void pp_channel_plain(const DecodeArgs &a, const PPSlots<Pack<F, PPCw<F>::C>> &s, int N,
                                                 int grp, int (&unc)[2 * PPCw<F>::C], int t0, int nt, unsigned *bad)
{
    constexpr int C = PPCw<F>::C;
    const F kMax = sizeof(F) == 8 ? (F)kFast64Max : (F)1e30f;   // premise bound on |yq|
    const int ng4 = N / 4;
    const F sigma = (F)a.sigma;
    for (int t = t0; t < 2 * C * ng4; t += nt) {
        int q = 0;
#pragma unroll
        for (int k = 1; k < 2 * C; ++k) q += t >= k * ng4 ? 1 : 0;
        const int g4 = t - q * ng4, X = q >= C ? 1 : 0, c = q - X * C;
        const uint64_t cw = a.first_cw + (uint64_t)(grp * 2 * C + q);
        uint32_t u[4];
        philox4x32_10<true>((uint32_t)g4, (uint32_t)cw, (uint32_t)(cw >> 32), a.stream_id, (uint32_t)a.seed,
                            (uint32_t)(a.seed >> 32), u);
        F n[4];
        box_muller(u[0], u[1], n[0], n[1]);
        box_muller(u[2], u[3], n[2], n[3]);
        F qv[4];
        int e = 0;
        bool ok = true;
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            qv[q4] = (F(1) + sigma * n[q4]) + F(0);   // (F)cv * (1 + sigma n) with cv = +1, then yq + 0
            e += (qv[q4] > F(0) ? 1 : -1) < 0;
            ok &= dabs(qv[q4]) < kMax;
        }
        if (!ok) *bad |= 1u << X;
        if constexpr (C == 1) {
            struct alignas(16) D2 { F d[2]; };
            const uint32_t at = (X ? s.app_base[1] : s.app_base[0]) + 32u * (uint32_t)g4;
            lds_put<D2>(at, D2{{qv[0], qv[1]}});
            lds_put<D2>(at + 16u, D2{{qv[2], qv[3]}});
        } else {
            auto *ap = X ? s.app[1] : s.app[0];
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) ap[4 * g4 + q4].v[c] = qv[q4];
        }
#pragma unroll
        for (int qq = 0; qq < 2 * C; ++qq) unc[qq] += qq == q ? e : 0;
    }
}

// Channel of the block step's 2C codewords (:214-238) staged into app[X][v].v[c]
// (v < N; codeword grp*2C + X*C + c), by the bit role (threads t0, t0 + nt, ...),
// 4 bits (one Philox call) per thread and step; unc[X*C + c] = this thread's
// uncoded errors. A missing codeword (past the batch) is staged as +1 samples:
// never a premise break, never counted. The check role stays out of it: with the
// f64 Box-Muller inlined into its loop, the compiler hoisted the channel's loop
// invariants and spilled 14 doubles per thread around every interval loop (1.2 GB
// of scratch write-backs per bench launch).
// LDPC_PP_NOB2: the value staged is yq + 0 (app is never -0: the fast check nodes' premise)
// and *bad collects bit X for an input of slot X past the premise bound (|yq| >= kMax, inf,
// NaN), so the bit waves only read their yq back (no write-back, no B2; pp_role).
template <typename F, int SRC>
__device__ __forceinline__ void pp_channel(const DecodeArgs &a, const PPSlots<Pack<F, PPCw<F>::C>> &s, int N, int grp,
                                           int (&unc)[2 * PPCw<F>::C], int t0, int nt, unsigned *bad = nullptr)
{
    constexpr int C = PPCw<F>::C;
    const F kMax = sizeof(F) == 8 ? (F)kFast64Max : (F)1e30f;   // premise bound on |yq|
#pragma unroll
    for (int q = 0; q < 2 * C; ++q) unc[q] = 0;
    const int ng4 = (N + 3) / 4;
    if constexpr (SRC == SRC_PHILOX && LDPC_PP_NOB2) {
        if (pp_plain_step(a, N, grp, C)) {
            pp_channel_plain<F>(a, s, N, grp, unc, t0, nt, bad);
            return;
        }
    }
    for (int t = t0; t < 2 * C * ng4; t += nt) {
        int q = 0;   // codeword of the step (compares, not a division; selects, not a dynamic index)
#pragma unroll
        for (int k = 1; k < 2 * C; ++k) q += t >= k * ng4 ? 1 : 0;
        const int g4 = t - q * ng4, X = q >= C ? 1 : 0, c = q - X * C;
        const int b = grp * 2 * C + q;
        auto *ap = X ? s.app[1] : s.app[0];
        if (b >= a.batch) {
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4)
                if (4 * g4 + q4 < N) ap[4 * g4 + q4].v[c] = F(1);
            continue;
        }
        const uint64_t cw = a.first_cw + (uint64_t)b;
        F yv[4];
        const int8_t *cvec;
        if (SRC == SRC_GIVEN) {
            cvec = a.c ? a.c + (size_t)b * N : nullptr;
            const F *y = reinterpret_cast<const F *>(a.y) + (size_t)b * N;
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) yv[q4] = 4 * g4 + q4 < N ? y[4 * g4 + q4] : F(0);
        } else {
            cvec = a.cw_table ? a.cw_table + (size_t)(cw % (uint64_t)a.cw_rows) * N : nullptr;
            uint32_t u[4];
            philox4x32_10<true>((uint32_t)g4, (uint32_t)cw, (uint32_t)(cw >> 32), a.stream_id, (uint32_t)a.seed,
                          (uint32_t)(a.seed >> 32), u);
            F n[4];
            box_muller(u[0], u[1], n[0], n[1]);
            box_muller(u[2], u[3], n[2], n[3]);
            const F sigma = (F)a.sigma;
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const int v = 4 * g4 + q4;
                const int cv = (cvec && v < N) ? cvec[v] : 1;
                yv[q4] = (F)cv * (F(1) + sigma * n[q4]);
                if (a.y_out && v < N) reinterpret_cast<F *>(a.y_out)[(size_t)b * N + v] = yv[q4];
            }
        }
        int e = 0;
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const int v = 4 * g4 + q4;
            if (v < N) {
                const int cv = cvec ? cvec[v] : 1;
                F qv = front_end<F>(yv[q4], a);
                if (LDPC_PP_NOB2) {
                    qv = qv + F(0);
                    if (!(dabs(qv) < kMax)) *bad |= 1u << X;
                }
                ap[v].v[c] = qv;
                e += ((qv > F(0) ? 1 : -1) * cv < 0);
            }
        }
#pragma unroll
        for (int qq = 0; qq < 2 * C; ++qq) unc[qq] += qq == q ? e : 0;
    }
}

// A wave's sum of per-lane counts 0 .. 2^NB - 1, bit-sliced: NB ballots and popcounts on the
// scalar unit instead of a cross-lane shuffle tree.
template <int NB>
__device__ __forceinline__ int wave_sum(int x)
{
    int t = 0;
#pragma unroll
    for (int b = 0; b < NB; ++b) t += (1 << b) * __builtin_popcountll(__builtin_amdgcn_ballot_w64((x & (1 << b)) != 0));
    return t;
}

// Block sums of the step's (bit errors, uncoded errors, syndrome) per codeword and
// the per-codeword accounting (:270-288, :382-393) by thread 0; the codewords of a
// slot whose premise failed go to the re-decode list instead. Per lane the counts are
// small -- a bit-role lane holds CPT = 4 bit slots and one Philox group of each
// codeword (N <= 2048, rows_pp_supported), so its bit and uncoded errors are <= 4; a
// check-role lane holds the 0/1 syndrome of its rows (and, k_rows_ppi, the error of its one
// in-register bit) -- so each wave sums them by
// ballots (wave_sum; the syndrome is an OR) and lane 0 adds the wave's totals into
// red[kPPRedSums ...] with LDS atomics: one barrier, and only thread 0 reads the totals
// (it clears them for the next step).
// WCHK: the check role's lanes carry bit errors too (the in-register bits, <= 1 per lane and codeword).
// CHU: they carry uncoded errors too (their share of the channel). NB: bits of the sliced sums --
// 4 in k_rows_ppw, whose bit-role lanes hold up to 8 bit slots and, outside a plain step, two
// Philox groups of each codeword (counts <= 8).
template <int C, bool HB, bool WCHK = false, bool CHU = (LDPC_PP_CHAN_ALL || LDPC_PP_CHAN_SPLIT), int NB = 3>
__device__ __forceinline__ void pp_account(const DecodeArgs &a, int *red, int grp, int (&sums)[6 * C], unsigned *redo,
                                           unsigned long long *acc)
{
    int *tot = red + kPPRedSums;
    const bool lane0 = (threadIdx.x & 63) == 0;
    if (!(LDPC_PP_TAILEXP & 4)) {
#pragma unroll
        for (int q = 0; q < 2 * C; ++q) {
            if constexpr (HB) {
                const int w = wave_sum<NB>(sums[3 * q]), u = wave_sum<NB>(sums[3 * q + 1]);
                if (lane0 && w) atomicAdd(&tot[3 * q], w);
                if (lane0 && u) atomicAdd(&tot[3 * q + 1], u);
            } else {
                if (__builtin_amdgcn_ballot_w64(sums[3 * q + 2] != 0) && lane0) atomicAdd(&tot[3 * q + 2], 1);
                if constexpr (WCHK) {
                    const int w = wave_sum<NB>(sums[3 * q]);
                    if (lane0 && w) atomicAdd(&tot[3 * q], w);
                }
                if constexpr (CHU) {   // the check waves' share of the channel
                    const int u = wave_sum<NB>(sums[3 * q + 1]);
                    if (lane0 && u) atomicAdd(&tot[3 * q + 1], u);
                }
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int v = 0; v < 6 * C; ++v) {
            sums[v] = tot[v];
            tot[v] = 0;
        }
        const int fl[2] = {red[0], red[1]};
        red[0] = red[1] = 0;   // read once per step; raised again only after the next B1
#pragma unroll
        for (int q = 0; q < 2 * C; ++q) {
            const int b = grp * 2 * C + q;
            if (b >= a.batch) continue;
            if (fl[q / C]) {
                const unsigned at = atomicAdd(&redo[0], 1u);
                redo[1 + at] = (unsigned)b;
                continue;
            }
            const int w = sums[3 * q], uc = sums[3 * q + 1], sf = sums[3 * q + 2] > 0;
            acc[0] += (unsigned long long)w;
            acc[1] += (unsigned long long)(w > 0);
            acc[2] += (unsigned long long)uc;
            acc[3] += 1ull;
            acc[5] += (unsigned long long)sf;
            if (w > 0 && a.hist) atomicAdd(&a.hist[w - 1], 1ull);
            if (a.frame_res) a.frame_res[b] = make_int4(w, uc, sf, 0);
        }
    }
}

// The check node of one row: fp64 (fast64.h cn_fast64) or an fp32 pair (cn_fast,
// MS and NMS with the device-verified reciprocal; VAR picks).
// store(k, message) scatters the new message of edge k, called as each message is
// formed, in per-edge order (LDPC_PP_STORE_ORDER), so the scatters overlap the selects
// of the later edges (fp64: cn_fast64; fp32 pairs: cn_fast_pair).
// fp64: the premise is folded into the hi-word maximum *pacc (fast64.h ACC), tested by
// the caller (LDPC_PP_STICKY); the returned value is always true.
template <typename F, int DC, int VAR, bool FDIV, int C, int DCA, typename Store>
__device__ __forceinline__ bool pp_check_node(const Pack<F, C> (&xin)[DCA], Pack<F, C> (&pv)[DCA], F alpha, F rcp,
                                              F delta, Store store, uint32_t *pacc)
{
    if constexpr (sizeof(F) == 8) {
        return cn_fast64<DC, VAR, FDIV, DCA, Store, LDPC_PP_STORE_ORDER != 0, true>(xin, pv, alpha, rcp, delta, store,
                                                                                     pacc);
    } else {
        return cn_fast_pair<DC, DCA, Store, LDPC_PP_STORE_ORDER != 0>(xin, pv, VAR == V_NMS, alpha, rcp, store);
    }
}

// ---- one wave's work: R check rows of each slot, or (HB) CPT bit slots ----
// The split is per wave (an SGPR branch in the kernel): waves 0-7 hold rows t
// and t + 512 of the row schedule (R = 2), waves 8-15 the bit slots of schedule
// thread t - 512 (HB, R = 0). Row r runs a check node of compile-time degree
// DC0 (r = 0) or DC1 (r = 1): with the degree-aware slots (graph.h pp_row_slots)
// the younger check wave of each SIMD -- the SQ issues oldest-first, so it sets
// the interval -- holds only rows of degree <= 7 (DC0 = DC1 = 7) and the older
// one the degree-8 rows and the padding in its row 1 (DC1 = 8). A row of lower
// degree than its DC has padding edges: +inf gathers (no effect on min, sign or
// argmin) and scatters to the lane's dummy slot.
// IR (k_rows_ppi, the in-register schedule of graph.h build_pp_inreg_schedule): 0 the
// bit role, or every edge through LDS; 1 a check wave whose last positions (DC0 - 1 of row
// 0, DC1 - 1 of row 1) are in-register or padding edges in every lane: one gather of the
// staged yq (padding: +inf) and no scatter for them; 2 a check wave where some lanes hold
// real edges there: both gathers and scatters are issued (the paired lanes' scatters go to
// the dummy slot) and the in-register sum is selected per lane (rs.pair bit 0).
// W: waves of the block. 16: 8 check and 8 bit waves. 12 (k_rows_ppw): the same 8 check waves and
// 4 bit waves; bit wave w holds the bit slots of schedule threads 64 w + lane and 64 (w + 4) + lane
// (CPL = 2 CPT slots per lane, merged in non-increasing group degree), reads them in one round
// trip (LDPC_PP_W12_K0 / K1), and a plain step's channel is spread over all 768 threads.
template <typename F, int SRC, int DC0, int DC1, int CPT, int VAR, bool FDIV, int R, bool HB, int IR = 0, int W = 16>
__device__ __forceinline__ void pp_role(const DecodeArgs &a, const DevGraph &g, const RowSched &rs,
                                        const PPSlots<Pack<F, PPCw<F>::C>> &s, unsigned *redo,
                                        unsigned long long *acc)
{
    constexpr int C = PPCw<F>::C;
    using P = Pack<F, C>;
    constexpr int DCX = 8;                    // schedule stride (rs.dc)
    constexpr int RR = R > 0 ? R : 1;   // array extents
    static_assert(DC0 <= DCX && DC1 <= DCX && (R == 0) == HB, "pp_role shape");
    static_assert(W == 16 || W == 12, "pp_role block shape");
    constexpr bool W12 = W == 12;
    constexpr int NT = 64 * W, NBT = NT - kPPRole;   // threads of the block / of its bit role
    constexpr int CPL = HB ? CPT * (kPPRole / NBT) : CPT;   // bit slots per lane
    constexpr bool FIXL = W12;   // pp_slots FIX
    constexpr bool UNP = FIXL && LDPC_PP_W12_UNP && R > 0 && sizeof(F) == 8 && LDPC_PP_EXP == 0;
    constexpr bool SPLITCH = LDPC_PP_CHAN_SPLIT || W12;
    static_assert(!UNP || LDPC_PP_PREFETCH, "unpacked addresses: both rows' gathers ahead of row 0");
    // IR needs LDPC_PP_NOB2 (yq staged canonical by the channel) and LDPC_PP_PREFETCH (both rows'
    // gathers ahead of row 0); plan_rows_pp picks k_rows_ppi only in builds that have both
    static_assert(IR == 0 || R == 2, "in-register bits: two rows per check thread");
    constexpr int L0 = DC0 - 1, L1 = DC1 - 1;   // IR: the in-register edge's position in row 0 / row 1
    constexpr bool F64 = sizeof(F) == 8;
    const F kMax = F64 ? (F)kFast64Max : (F)1e30f;   // premise bound on |yq|
    const int tid = threadIdx.x, N = g.N, lane = tid & 63;
    [[maybe_unused]] const int EA = rs.e_pad + 64;   // c2v slots per codeword slot (LDPC_CHECK bounds)
    // check rows: schedule, and the c2v each sent last iteration, per slot
    // (entries past a row's DC are never touched, so they take no registers)
    [[maybe_unused]] int deg[RR];
    [[maybe_unused]] uint32_t colw[RR][DCX / 2], posw[RR][DCX / 2];
    [[maybe_unused]] P prev[2][RR][DCX];
    if constexpr (R > 0) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int j = tid + r * kPPRole;
            deg[r] = rs.cn_deg[j];
            const uint4 xc = reinterpret_cast<const uint4 *>(rs.cn_cols + (size_t)j * DCX)[0];
            const uint4 xp = reinterpret_cast<const uint4 *>(rs.cn_pos + (size_t)j * DCX)[0];
            colw[r][0] = xc.x; colw[r][1] = xc.y; colw[r][2] = xc.z; colw[r][3] = xc.w;
            posw[r][0] = xp.x; posw[r][1] = xp.y; posw[r][2] = xp.z; posw[r][3] = xp.w;
            if (deg[r] == 0)   // rows past M: gather the +0 entry, so their messages stay 0
#pragma unroll
                for (int q = 0; q < DCX / 2; ++q) colw[r][q] = (uint32_t)(N + 2) * 0x10001u;
        }
    }
    // IR: the lane has an in-register bit (IR == 1: or a padding edge, which behaves as one whose
    // sample is +inf); fr1: its row 1 comes first in the bit's nlist (never where DC0 == DC1)
    [[maybe_unused]] bool has = IR == 1, fr1 = false;
    if constexpr (IR != 0) {
        const uint32_t pf = rs.pair[LDPC_CHK(tid, kPPRole, CHK_PP_GATHER)];
        if (IR == 2) has = (pf & 1u) != 0;
        fr1 = DC0 != DC1 && (pf & 2u) != 0;
        // IR == 1: an empty row 0 keeps +0 edges, but the shared sample it gathers is a padding edge's +inf
        if (IR == 1 && deg[0] == 0)
            colw[0][L0 / 2] = (L0 & 1) ? (colw[0][L0 / 2] & 0xffffu) | ((uint32_t)N << 16)
                                       : (colw[0][L0 / 2] & 0xffff0000u) | (uint32_t)N;
    }
    // UNP: slot 0's LDS byte address of every gather (ga) and scatter (sa) of the rows, formed once
    // (the in-register edge of IR == 1 has neither); vin: the in-register bit (IR == 1: or N, a padding edge)
    [[maybe_unused]] uint32_t ga[RR][DCX], sa[RR][DCX], vin = 0;
    if constexpr (UNP) {
        static_for<0, R>([&](auto rc) {
            constexpr int r = decltype(rc)::value, DCr = r == 0 ? DC0 : DC1;
#pragma unroll
            for (int k = 0; k < DCr - (IR == 1 ? 1 : 0); ++k) {
                ga[r][k] = s.app_base[0] + 8u * (uint32_t)LDPC_CHK(u16_at<DCX>(colw[r], k), N + 3, CHK_PP_GATHER);
                sa[r][k] = s.c2v_base[0] + 8u * (uint32_t)LDPC_CHK(u16_at<DCX>(posw[r], k), EA, CHK_PP_SCATTER);
                // opaque: the compiler otherwise keeps 8 * entry and adds the array's base at every access
                asm("" : "+v"(ga[r][k]), "+v"(sa[r][k]));
            }
        });
        if constexpr (IR != 0) vin = (uint32_t)LDPC_CHK(u16_at<DCX>(colw[0], L0), N + 3, CHK_PP_GATHER);
    }
    [[maybe_unused]] auto inreg_col = [&]() -> int {
        if constexpr (UNP) return (int)vin;
        else return u16_at<DCX>(colw[0], L0);
    };
    // IR: (yq + c2v_first) + c2v_second of slot X's in-register bit, from the staged yq `y`
    // and the messages the two rows sent last (prev): the bit node's sum (:452-476)
    [[maybe_unused]] auto inreg_sum = [&](auto Xc, const P &y) -> P {
        constexpr int X = decltype(Xc)::value;
        P sum;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const F p0 = prev[X][0][L0].v[c], p1 = prev[X][RR - 1][L1].v[c];
            sum.v[c] = (y.v[c] + (fr1 ? p1 : p0)) + (fr1 ? p0 : p1);
        }
        return sum;
    };
    // bit slots of schedule thread bt
    const int bt = tid - kPPRole;
    static_assert(!UNP || IR != 1 || LDPC_PP_INREG_Y, "unpacked addresses: the in-register bit's sample in registers");
    [[maybe_unused]] int vgb[CPL], vgd[CPL];
    [[maybe_unused]] uint32_t vdst2[(CPL + 1) / 2] = {};
    [[maybe_unused]] uint32_t ra[CPL][LDPC_PP_W12_K0 > LDPC_PP_W12_K1 ? LDPC_PP_W12_K0 : LDPC_PP_W12_K1];   // W12: below
    if constexpr (HB) {
        // the schedule entry of lane slot i. W12: the slots of schedule threads bt and bt + NBT (the
        // bit-slot groups of two of the schedule's waves), merged by group degree -- wave-uniform, and
        // non-increasing along each thread's slots (graph.cpp build_row_schedule)
        int si[CPL];
        if constexpr (W12) {
            int pa = 0, pb = 0;
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                const int ia = bt * CPT + (pa < CPT ? pa : CPT - 1), ib = (bt + NBT) * CPT + (pb < CPT ? pb : CPT - 1);
                const int da = pa < CPT ? __builtin_amdgcn_readfirstlane((int)(rs.vn_info[ia] >> 24)) : -1;
                const int db = pb < CPT ? __builtin_amdgcn_readfirstlane((int)(rs.vn_info[ib] >> 24)) : -1;
                const bool ta = da >= db;
                si[i] = ta ? ia : ib;
                pa += ta ? 1 : 0;
                pb += ta ? 0 : 1;
            }
        } else {
#pragma unroll
            for (int i = 0; i < CPL; ++i) si[i] = bt * CPT + i;
        }
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int c = rs.vn_col[si[i]];
            vdst2[i / 2] |= (uint32_t)(c == 0xffff ? N + 1 : c) << (16 * (i & 1));
            const uint32_t info = rs.vn_info[si[i]];
            vgb[i] = __builtin_amdgcn_readfirstlane((int)(info & 0xffffu) - lane);
            vgd[i] = __builtin_amdgcn_readfirstlane((int)(info >> 24));
        }
        // padding slots of the bit-node layout hold +0 (adding +0 changes no sum); never written
        P z;
#pragma unroll
        for (int c = 0; c < C; ++c) z.v[c] = F(0);
        if constexpr (W12) {
            // slot 0's LDS byte address of edge k of lane slot i, or of the slot's +0 word (c2v[-1],
            // never written again) where the group has no edge k
            if (tid == kPPRole + 2) s.c2v[0][-1] = s.c2v[1][-1] = z;
            const int ln0 = lane;
#pragma unroll
            for (int i = 0; i < CPL; ++i)
#pragma unroll
                for (int k = 0; k < (i == 0 ? LDPC_PP_W12_K0 : LDPC_PP_W12_K1); ++k) {
                    const uint32_t e = (uint32_t)LDPC_CHK(k < vgd[i] ? vgb[i] + ln0 + k * 64 : 0, EA, CHK_PP_BIT_READ);
                    ra[i][k] = k < vgd[i] ? s.c2v_base[0] + 8u * e : s.c2v_base[0] - 8u;
                    asm("" : "+v"(ra[i][k]));   // opaque: kept as formed, not rebuilt from the group's base at every read
                }
        }
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int dg = (int)((rs.vn_info[si[i]] >> 16) & 0xffu);
            const int base = vgb[i] + lane, gd = vgd[i];
            for (int k = dg; k < gd; ++k) {
                const int e = LDPC_CHK(base + k * 64, EA, CHK_PP_BIT_READ);
                s.c2v[0][e] = s.c2v[1][e] = z;
            }
        }
    }
    auto vdst = [&](int i) -> int { return (int)((vdst2[i / 2] >> (16 * (i & 1))) & 0xffffu); };
    const F alpha = (F)a.alpha, delta = (F)a.delta;
    F rcp = F64 ? (F)(1.0 / a.alpha) : (F)a.alpha_rcp;
    if constexpr (F64 && LDPC_PP_SBASE && R > 0)   // the quotient of the f64 division sits in a VGPR pair: to SGPRs
        rcp = mkd((uint32_t)__builtin_amdgcn_readfirstlane((int)lo32(rcp)), (uint32_t)__builtin_amdgcn_readfirstlane((int)hi32(rcp)));
    const int nsteps = (a.batch + 2 * C - 1) / (2 * C);
    if constexpr (HB && LDPC_PP_NOB2) {   // sentinels (never overwritten): padding edges gather +inf, rows past M +0
        P inf, zero;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            inf.v[c] = dinf<F>();
            zero.v[c] = F(0);
        }
        if (tid == kPPRole) s.app[0][N] = s.app[1][N] = inf;
        if (tid == kPPRole + 1) s.app[0][N + 2] = s.app[1][N + 2] = zero;
    }
    PP_STAMP_DECL;
    for (int grp = blockIdx.x; grp < nsteps; grp += gridDim.x) {
        PP_STAMP_TOP();
        [[maybe_unused]] uint32_t pacc[2] = {0u, 0u};   // fp64, LDPC_PP_STICKY: per-slot premise maximum
        constexpr bool TF = (LDPC_PP_TAILFUSE & (F64 ? 2 : 1)) != 0;
        int unc[2 * C];
        [[maybe_unused]] int wdec[2 * C];   // LDPC_PP_TAILFUSE: bit errors per codeword (bit role)
        [[maybe_unused]] int synd0[C];      // LDPC_PP_TAILFUSE: slot 0's syndrome (check role)
#pragma unroll
        for (int q = 0; q < 2 * C; ++q) unc[q] = wdec[q] = 0;
        [[maybe_unused]] unsigned chan_bad = 0;   // LDPC_PP_NOB2: slots with an input past the premise
        if constexpr (LDPC_PP_CHAN_ALL && !HB) {   // the check waves take Philox groups too
            if (!(LDPC_PP_TAILEXP & 1)) pp_channel<F, SRC>(a, s, N, grp, unc, tid, NT, &chan_bad);
        }
        [[maybe_unused]] const bool split = SPLITCH && SRC == SRC_PHILOX && LDPC_PP_NOB2 &&
                                            !(LDPC_PP_TAILEXP & 1) && pp_plain_step(a, N, grp, C);
        if constexpr (SPLITCH && !HB) {   // the check waves' share of a plain step
            if (split) pp_channel_plain<F>(a, s, N, grp, unc, tid, NT, &chan_bad);
        }
        if constexpr (HB) {
            if (SPLITCH && split) {
                pp_channel_plain<F>(a, s, N, grp, unc, tid, NT, &chan_bad);
            } else if (!(LDPC_PP_TAILEXP & 1)) {
                pp_channel<F, SRC>(a, s, N, grp, unc, LDPC_PP_CHAN_ALL ? tid : bt, LDPC_PP_CHAN_ALL ? NT : NBT, &chan_bad);
            } else {   // timing only: a constant channel
                for (int q = 0; q < 2 * C; ++q) unc[q] = 0;
                for (int v = bt; v < N; v += NBT)
                    for (int c = 0; c < C; ++c) s.app[0][v].v[c] = s.app[1][v].v[c] = F(1);
            }
        }
        PP_SYNC_STAMPED(1);   // B1: channel staged
        [[maybe_unused]] P yq[2][CPL];
        if constexpr (R > 0) {
#pragma unroll
            for (int X = 0; X < 2; ++X)
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int k = 0; k < DCX; ++k)
#pragma unroll
                        for (int c = 0; c < C; ++c) prev[X][r][k].v[c] = F(0);
        }
        if constexpr ((SPLITCH || (LDPC_PP_CHAN_ALL && LDPC_PP_NOB2)) && !HB) {   // the check waves' share of the channel's flags
            if (__builtin_amdgcn_ballot_w64(chan_bad != 0)) {
                if (chan_bad & 1u) s.red[0] = 1;
                if (chan_bad & 2u) s.red[1] = 1;
            }
        }
        if constexpr (HB && LDPC_PP_NOB2) {
            // the flags of the previous step were read and cleared by thread 0 before B1
            if (__builtin_amdgcn_ballot_w64(chan_bad != 0)) {
                if (chan_bad & 1u) s.red[0] = 1;
                if (chan_bad & 2u) s.red[1] = 1;
            }
            // yq back from the staged channel (canonical there); padding slots read the +0
            // sentinel. No write-back: the first interval's check rows read app as staged, and
            // this slot's first bit pass (interval 2) writes app after a barrier.
#pragma unroll
            for (int X = 0; X < 2; ++X)
#pragma unroll
                for (int i = 0; i < CPL; ++i)
                    yq[X][i] = s.app[X][LDPC_CHK(vdst(i) < N ? vdst(i) : N + 2, N + 3, CHK_PP_APP_WRITE)];
        } else if constexpr (HB) {
#pragma unroll
            for (int X = 0; X < 2; ++X) {
                bool in_ok = true;
#pragma unroll
                for (int i = 0; i < CPL; ++i) {
                    const P st = s.app[X][LDPC_CHK(vdst(i) <= N ? vdst(i) : 0, N + 3, CHK_PP_APP_WRITE)];
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        // yq + 0 maps -0 to +0, so app is never -0 (the fast check nodes' premise)
                        yq[X][i].v[c] = st.v[c] + F(0);
                        in_ok &= dabs(yq[X][i].v[c]) < kMax;
                    }
                }
#pragma unroll
                for (int i = 0; i < CPL; ++i) s.app[X][LDPC_CHK(vdst(i), N + 3, CHK_PP_APP_WRITE)] = yq[X][i];   // v2c = yq on the first pass (:364-370)
                if (!in_ok) s.red[X] = 1;
            }
            P inf, zero;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                inf.v[c] = dinf<F>();
                zero.v[c] = F(0);
            }
            if (tid == kPPRole) s.app[0][N] = s.app[1][N] = inf;
            if (tid == kPPRole + 1) s.app[0][N + 2] = s.app[1][N + 2] = zero;
        }
        if constexpr (!LDPC_PP_NOB2) PP_SYNC_STAMPED(3);   // B2: yq in app

        // Decisions and error weight of slot Y's codewords from its final posteriors
        // (bit slots; :270, :382-393), into w[Y*C + c].
        auto decide = [&](int Y, const P *post, int *w) {
            // the common case (the bench's): the all-zero codeword, no decision output --
            // errors are the posteriors that are not > 0; a wave-uniform test
            const bool plain = (SRC == SRC_GIVEN ? !a.c : !a.cw_table) && !a.d_out;
            if (plain) {
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const int q = Y * C + c;
                    int e = 0;
#pragma unroll
                    for (int i = 0; i < CPL; ++i) e += (vdst(i) < N && !(post[i].v[c] > F(0))) ? 1 : 0;   // :471-474
                    w[q] = grp * 2 * C + q < a.batch ? e : 0;
                }
                return;
            }
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int q = Y * C + c, b = grp * 2 * C + q;
                if (b >= a.batch) continue;
                const int8_t *cvec =
                    SRC == SRC_GIVEN ? (a.c ? a.c + (size_t)b * N : nullptr)
                                     : (a.cw_table ? a.cw_table + (size_t)((a.first_cw + (uint64_t)b) % (uint64_t)a.cw_rows) * N
                                                   : nullptr);
                int e = 0;
#pragma unroll
                for (int i = 0; i < CPL; ++i) {
                    const int v = vdst(i);
                    if (v < N) {
                        const int d = post[i].v[c] > F(0) ? 1 : -1;   // :471-474
                        const int cv = cvec ? cvec[v] : 1;
                        e += (d != cv);
                        if (a.d_out) a.d_out[(size_t)b * N + v] = (int8_t)d;
                    }
                }
                w[q] = e;
            }
        };
        constexpr bool YREG = IR == 1 && LDPC_PP_INREG_Y;
        [[maybe_unused]] P yreg[2];   // LDPC_PP_INREG_Y: the in-register bit's staged sample per slot
        if constexpr (YREG) {
#pragma unroll
            for (int X = 0; X < 2; ++X) yreg[X] = s.app[X][LDPC_CHK(inreg_col(), N + 3, CHK_PP_GATHER)];
        }
        // IR: the in-register bit's final posterior per slot (inreg_final, once the slot's last check phase is done)
        [[maybe_unused]] P ipost[2];
        [[maybe_unused]] auto inreg_final = [&](auto Xc) {
            constexpr int X = decltype(Xc)::value;
            ipost[X] = inreg_sum(Xc, YREG ? yreg[X] : s.app[X][LDPC_CHK(inreg_col(), N + 3, CHK_PP_GATHER)]);
        };
        // Syndrome of slot X's codeword c (rows; padding edges read +inf: parity 0; rows past M skipped)
        auto syndrome = [&](int X, int c) -> int {
            int synd = 0;
            if constexpr (R > 0) {
                static_for<0, R>([&](auto rc) {
                    constexpr int r = decltype(rc)::value, DCr = r == 0 ? DC0 : DC1;
                    int par = 0;
#pragma unroll
                    for (int k = 0; k < DCr; ++k) {
                        if (IR == 1 && k == DCr - 1) continue;   // the in-register edge: below
                        int neg;
                        if constexpr (UNP) neg = (lds_at<P>(ga[r][k] + (X ? kPPAppStride : 0u)).v[c] > F(0)) ? 0 : 1;
                        else neg = (s.app[X][LDPC_CHK(u16_at<DCX>(colw[r], k), N + 3, CHK_PP_GATHER)].v[c] > F(0)) ? 0 : 1;
                        par ^= (IR == 2 && k == DCr - 1 && has) ? 0 : neg;
                    }
                    if constexpr (IR != 0) par ^= (has && !(ipost[X].v[c] > F(0))) ? 1 : 0;
                    synd |= deg[r] > 0 ? par : 0;
                });
            }
            return synd;
        };

        // One barrier interval: the rows of slot X (their reads first), the bit
        // nodes of slot 1 - X when `bits` (HB waves), then the rows' check nodes.
        auto interval = [&](auto Xc, bool rows, bool bits, bool last) {
            constexpr int X = decltype(Xc)::value, Y = 1 - X;
            [[maybe_unused]] P xin[RR][DCX];
            if constexpr (R > 0) {
                if (rows && LDPC_PP_EXP != 2) {
                    if constexpr (!UNP) {
#pragma unroll
                        for (int r = 0; r < R; ++r)
#pragma unroll
                            for (int q = 0; q < DCX / 2; ++q) asm volatile("" : "+v"(colw[r][q]), "+v"(posw[r][q]));
                    }
                    // FIXL: slot 0's base, the slot in the instruction's offset field
                    [[maybe_unused]] const uint32_t ab = s.app_base[FIXL ? 0 : X];
                    constexpr uint32_t aoff = FIXL ? X * kPPAppStride : 0u;
                    static_for<0, (LDPC_PP_PREFETCH ? R : 1)>([&](auto rc) {
                        constexpr int r = decltype(rc)::value, DCr = r == 0 ? DC0 : DC1;
#pragma unroll
                        for (int k = 0; k < DCr - (IR == 1 && (r == 1 || YREG) ? 1 : 0); ++k) {   // IR == 1: row 1's last edge is row 0's
                            if constexpr (UNP)
                                xin[r][k] = lds_at<P>(ga[r][k] + aoff);
                            else
                                xin[r][k] = lds_at<P>(((LDPC_PP_EXP == 5 || LDPC_PP_EXP == 7) ? ab + 8u * (uint32_t)(lane + 64 * (k + 8 * r))
                                                                                              : PP_ADDR8(DCX, colw[r], k, ab, N + 3, CHK_PP_GATHER)) + aoff);
                        }
                    });
                    if constexpr (LDPC_PP_GATHER_FIRST && LDPC_PP_PREFETCH) {
                        // every gather of the interval issued ahead of the check-node arithmetic
                        constexpr int NG = DC0 + (R > 1 ? DC1 : 0);
                        __builtin_amdgcn_sched_group_barrier(0x2, NG, 1);     // their addresses
                        __builtin_amdgcn_sched_group_barrier(0x100, NG, 1);   // the ds_read_b64s
                    }
                }
            }
            if constexpr (HB) {
                if (LDPC_PP_BITDELAY > 0) __builtin_amdgcn_s_sleep(LDPC_PP_BITDELAY);
                if (bits && LDPC_PP_EXP != 1) {   // bit nodes: sum = yq + c2v in nlist order (:452-476)
#pragma unroll
                    for (int q = 0; q < (CPL + 1) / 2; ++q) asm volatile("" : "+v"(vdst2[q]));
                    P sum[CPL];
#pragma unroll
                    for (int i = 0; i < CPL; ++i) sum[i] = yq[Y][i];
                    const int ln = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
                    if constexpr (W12) {
                        // Every read of the interval ahead of the first add: edges k < K0 of slot 0 and
                        // k < K1 of the other slots, from the addresses formed once per launch (ra: an
                        // edge past its group's degree reads the slot's +0 word, and adding +0 changes no
                        // sum), the slot in the offset field; then the adds, per slot in edge order (nlist
                        // order, as vn_phases). One basic block, one LDS round trip.
                        constexpr int K0 = LDPC_PP_W12_K0, K1 = LDPC_PP_W12_K1;
                        const P *cv = s.c2v[Y] + ln;
                        [[maybe_unused]] const int lim = LDPC_CHK_LIM(EA - ln);
                        P rd[CPL][K0 > K1 ? K0 : K1];
#pragma unroll
                        for (int i = 0; i < CPL; ++i)
#pragma unroll
                            for (int k = 0; k < (i == 0 ? K0 : K1); ++k) rd[i][k] = lds_at<P>(ra[i][k] + Y * kPPC2vDist);
#pragma unroll
                        for (int k = 0; k < (K0 > K1 ? K0 : K1); ++k)
#pragma unroll
                            for (int i = 0; i < CPL; ++i)
                                if (k < (i == 0 ? K0 : K1)) padd<false>(sum[i], rd[i][k]);
                        // group degrees past K0 / K1 (none in the bench code): one round trip per edge
#pragma unroll
                        for (int i = 0; i < CPL; ++i)
                            for (int k = (i == 0 ? K0 : K1); k < vgd[i]; ++k)
                                padd<false>(sum[i], cv[LDPC_CHK(vgb[i] + k * 64, lim, CHK_PP_BIT_READ)]);
                    } else {
                        int k = 0;
                        vn_phases<F, C, CPL, CPL>(s.c2v[Y] + ln, vgb, vgd, k, sum, LDPC_CHK_LIM(EA - ln), CHK_PP_BIT_READ);
                    }
#pragma unroll
                    for (int i = 0; i < CPL; ++i) s.app[Y][LDPC_CHK(vdst(i), N + 3, CHK_PP_APP_WRITE)] = sum[i];
                    if (TF && last) decide(Y, sum, wdec);   // slot Y's final pass
                }
            }
            if constexpr (R > 0) {
                if (rows && LDPC_PP_EXP != 2) {
                    [[maybe_unused]] const uint32_t ab = s.app_base[X], cb = s.c2v_base[FIXL ? 0 : X];
                    constexpr uint32_t coff = FIXL ? X * kPPC2vDist : 0u;
                    if constexpr (IR != 0) {   // the in-register bit's posterior in place of both rows' last gather
                        if constexpr (YREG) xin[0][L0] = yreg[X];
                        const P sum = inreg_sum(Xc, xin[0][L0]);
#pragma unroll
                        for (int c = 0; c < C; ++c) {
                            xin[0][L0].v[c] = has ? sum.v[c] : xin[0][L0].v[c];
                            xin[RR - 1][L1].v[c] = has ? sum.v[c] : xin[RR - 1][L1].v[c];
                        }
                    }
                    // LDPC_PP_ILV: row 1's front, issued in row 0's store chain (ILV steps per edge of row 0)
                    constexpr int ILV = (F64 && R == 2 && LDPC_PP_PREFETCH && LDPC_PP_STORE_ORDER && LDPC_PP_EXP == 0) ? LDPC_PP_ILV : 0;
                    using Front = std::conditional_t<(ILV > 0), CnFront64<DC1>, int>;
                    [[maybe_unused]] Front fr;
                    [[maybe_unused]] uint32_t pa1 = 0;   // LDPC_PP_ONEPREM: the interval's premise maximum
                    static_for<0, R>([&](auto rc) {
                        constexpr int r = decltype(rc)::value, DCr = r == 0 ? DC0 : DC1;
                        if (!LDPC_PP_PREFETCH && r > 0) {
#pragma unroll
                            for (int k = 0; k < DCr; ++k) xin[r][k] = lds_at<P>(LDPC_ADDR8(DCX, colw[r], k, ab, N + 3, CHK_PP_GATHER));
                        }
                        bool ok = true;
                        // the scatter of edge k into the bit-slot layout (experiments: none, or lane-contiguous)
                        auto store = [&](int k, const P &m) {
                            if (IR == 1 && k == DCr - 1) return;   // in-register (k is a constant once inlined)
                            if constexpr (UNP)
                                lds_put<P>(sa[r][k] + coff, m);
                            else if constexpr (LDPC_PP_EXP != 4)
                                lds_put<P>(((LDPC_PP_EXP == 6 || LDPC_PP_EXP == 7)
                                                ? cb + 8u * (uint32_t)(lane + 64 * ((k + 8 * r + 16 * (tid >> 6)) % 112))
                                                : PP_ADDR8(DCX, posw[r], k, cb, EA, CHK_PP_SCATTER)) + coff,
                                           m);
                        };
                        if constexpr (LDPC_PP_EXP == 3) {
#pragma unroll
                            for (int k = 0; k < DCr; ++k) {
#pragma unroll
                                for (int c = 0; c < C; ++c) prev[X][r][k].v[c] = xin[r][k].v[c] - prev[X][r][k].v[c];
                                store(k, prev[X][r][k]);
                            }
                        } else {
                            constexpr bool ONE = F64 && !LDPC_PP_STICKY && LDPC_PP_ONEPREM && R == 2;
                            [[maybe_unused]] uint32_t pa0 = 0;
                            uint32_t &pa = ONE ? pa1 : pa0;
                            if constexpr (ILV > 0) {
                                constexpr int NF = Front::N, SK = LDPC_PP_ILV_SKIP, CUT = ILV * (DC0 - SK) < NF ? ILV * (DC0 - SK) : NF;
                                if constexpr (r == 0) {
                                    // steps ILV (k - SK) .. + ILV - 1 of row 1's front behind row 0's edge k (k a constant once inlined)
                                    auto fill = [&](int k) {
                                        static_for<0, CUT>([&](auto ic) {
                                            constexpr int I = decltype(ic)::value;
                                            if (I / ILV + SK == k) fr.template step<I>(xin[1], prev[X][1]);
                                        });
                                    };
                                    ok = cn_fast64<DCr, VAR, FDIV, DCX, decltype(store), true, true, decltype(fill), ILV>(
                                        xin[r], prev[X][r], alpha, rcp, delta, store, LDPC_PP_STICKY ? &pacc[X] : &pa, fill);
                                } else {
                                    static_for<CUT, NF>([&](auto ic) { fr.template step<decltype(ic)::value>(xin[1], prev[X][1]); });
                                    ok = cn_fast64_back<DCr, VAR, FDIV, DCX, decltype(store), true, true>(
                                        fr.x, fr.mn1, fr.mn2, fr.par, prev[X][r], alpha, rcp, delta, store,
                                        LDPC_PP_STICKY ? &pacc[X] : &pa);
                                }
                            } else {
                                ok = pp_check_node<F, DCr, VAR, FDIV>(xin[r], prev[X][r], alpha, rcp, delta, store,
                                                                      LDPC_PP_STICKY ? &pacc[X] : &pa);
                            }
                            if constexpr (F64 && !LDPC_PP_STICKY && (!ONE || r == R - 1)) {
                                // rare: M2 >= 2^1000 (inf, NaN) or a tiny minimum in this row (ONE: in either row)
                                if (__builtin_amdgcn_ballot_w64(pa >= kFast64MaxHi)) {
                                    asm volatile(";");   // a side effect: stays a skipped branch
                                    if (pa >= kFast64MaxHi && LDPC_PP_EXP == 0) s.red[X] = 1;
                                }
                            }
                        }
                        if (!ok && deg[r] > 0 && LDPC_PP_EXP == 0) s.red[X] = 1;   // experiments: never re-decode
                        if (R > 1 && LDPC_PP_ROWFENCE) __builtin_amdgcn_sched_barrier(0);   // keep the rows' live ranges apart
                    });
                }
            }
        };
        for (int it = 0; it < a.T; ++it) {
            interval(std::integral_constant<int, 0>(), true, it > 0, false);
            PP_BARRIER();   // | check(0,it) | bit(1,it-1) |
            interval(std::integral_constant<int, 1>(), true, true, it == a.T - 1);
            PP_BARRIER();   // | check(1,it) | bit(0,it) |
        }
        if (a.T > 0) {
            interval(std::integral_constant<int, 0>(), false, true, true);
            if (TF && !(LDPC_PP_TAILEXP & 2)) {   // slot 0's posteriors are final
                if constexpr (IR != 0) inreg_final(std::integral_constant<int, 0>());
#pragma unroll
                for (int c = 0; c < C; ++c) synd0[c] = syndrome(0, c);
            }
            PP_BARRIER();   // | syndrome(0) | bit(1,T-1) |
        }
        if constexpr (F64 && R > 0 && LDPC_PP_STICKY) {   // the premise of every iteration of the step
            if (pacc[0] >= kFast64MaxHi && LDPC_PP_EXP == 0) s.red[0] = 1;
            if (pacc[1] >= kFast64MaxHi && LDPC_PP_EXP == 0) s.red[1] = 1;
        }

        if (LDPC_PP_TAILEXP & 2) {   // timing only: no syndrome, decisions or error weights
            int sums[6 * C] = {};
            pp_account<C, HB, IR != 0, SPLITCH || LDPC_PP_CHAN_ALL, W12 ? 4 : 3>(a, s.red, grp, sums, redo, acc);
            continue;
        }
        // syndrome and decisions / error weight of the step's codewords (what the last
        // intervals have not formed already, LDPC_PP_TAILFUSE; T = 0: all of it here)
        const bool fused = TF && a.T > 0;
        if constexpr (HB) {
            if (!fused) {
#pragma unroll
                for (int X = 0; X < 2; ++X) {
                    P post[CPL];
#pragma unroll
                    for (int i = 0; i < CPL; ++i) post[i] = s.app[X][LDPC_CHK(vdst(i) <= N ? vdst(i) : 0, N + 3, CHK_PP_APP_WRITE)];
                    decide(X, post, wdec);
                }
            }
        }
        if constexpr (IR != 0) {
            // the in-register bit: posterior, decision and error weight by its check thread (:270, :382-393)
            inreg_final(std::integral_constant<int, 0>());
            inreg_final(std::integral_constant<int, 1>());
            const int v = inreg_col();
            if (has && v < N) {   // IR == 1: a padding edge's index is N
#pragma unroll
                for (int q = 0; q < 2 * C; ++q) {
                    const int b = grp * 2 * C + q;
                    if (b >= a.batch) continue;
                    const int8_t *cvec =
                        SRC == SRC_GIVEN ? (a.c ? a.c + (size_t)b * N : nullptr)
                                         : (a.cw_table ? a.cw_table + (size_t)((a.first_cw + (uint64_t)b) % (uint64_t)a.cw_rows) * N
                                                       : nullptr);
                    const int d = ipost[q / C].v[q % C] > F(0) ? 1 : -1;   // :471-474
                    wdec[q] += d != (cvec ? cvec[v] : 1);
                    if (a.d_out) a.d_out[(size_t)b * N + v] = (int8_t)d;
                }
            }
        }
        int sums[6 * C];
#pragma unroll
        for (int X = 0; X < 2; ++X) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int q = X * C + c;
                sums[3 * q] = wdec[q];
                sums[3 * q + 1] = unc[q];
                sums[3 * q + 2] = (X == 0 && fused) ? synd0[c] : syndrome(X, c);
            }
        }
        PP_STAMP_ACC(5);
        pp_account<C, HB, IR != 0, SPLITCH || LDPC_PP_CHAN_ALL, W12 ? 4 : 3>(a, s.red, grp, sums, redo, acc);
    }
    PP_STAMP_OUT()
}

}  // namespace

LDPC_CHECK_TU(rows_pp)

// Experiments: s_nop instructions at the kernel entry shift the code that follows by 4 bytes
// each (the code-layout sensitivity of the loops, with and without -falign-loops).
#ifndef LDPC_PP_ENTRY_NOPS
#define LDPC_PP_ENTRY_NOPS 0
#endif

// SPLIT: the schedule has degree-aware row slots (rs.dc_low == 7, graph.h
// pp_row_slots): check waves 4-7 run two 7-edge rows, waves 0-3 a 7-edge and an
// 8-edge row. Otherwise every row runs the 8-edge check node.
// INREG (k_rows_ppi; SPLIT): rs is the in-register schedule, and each check wave runs the role
// rs.pair names for it (pp_role IR 1 or 2).
// W: the block's waves (pp_role): 16, or 12 (k_rows_ppw; INREG).
template <typename F, int SRC, int CPT, int VAR, bool FDIV, bool SPLIT, bool INREG, int W = 16>
__device__ __forceinline__ void pp_kernel(const DecodeArgs &a, const DevGraph &g, const RowSched &rs, unsigned *redo)
{
    static_assert(!INREG || SPLIT, "in-register bits come with the degree-aware row slots");
    static_assert(W == 16 || INREG, "the 12-wave block runs the in-register schedule");
    using P = Pack<F, PPCw<F>::C>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
#pragma unroll
    for (int i = 0; i < LDPC_PP_ENTRY_NOPS; ++i) asm volatile("s_nop 0");
    const PPSlots<P> s = pp_slots<P, W == 12>(smem, g.N, rs.e_pad + 64);
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(s.red + kPPRedAcc);   // thread 0's block totals
    if (threadIdx.x == 0) {
        s.red[0] = s.red[1] = 0;
#pragma unroll
        for (int q = 0; q < 6; ++q) acc[q] = 0;
#pragma unroll
        for (int v = 0; v < 3 * kPPMaxCw; ++v) s.red[kPPRedSums + v] = 0;   // pp_account's totals
    }
    // the split is wave-uniform (an SGPR branch), so every wave meets every barrier
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool low = wave < kPPRole / 64;
    if (LDPC_PP_PRIO == 1 && low) __builtin_amdgcn_s_setprio(1);
    if (LDPC_PP_PRIO == 2 && !low) __builtin_amdgcn_s_setprio(1);
    if (LDPC_PP_PRIO == 3 && ((threadIdx.x >> 8) & 1)) __builtin_amdgcn_s_setprio(1);
    if (LDPC_PP_PRIO == 4 && low && wave >= kPPRole / 128) __builtin_amdgcn_s_setprio(1);
    if (LDPC_PP_PRIO == 5 && low) {
        if (wave >= kPPRole / 128) __builtin_amdgcn_s_setprio(2);
        else __builtin_amdgcn_s_setprio(1);
    }
    if constexpr (INREG) {
        const bool pure = low && __builtin_amdgcn_readfirstlane((int)rs.pair[kPPRole + (low ? wave : 0)]) != 0;
        if (!low)
            pp_role<F, SRC, 8, 8, CPT, VAR, FDIV, 0, true, 0, W>(a, g, rs, s, redo, acc);
        else if (wave >= kPPRole / 128) {
            if (pure) pp_role<F, SRC, 7, 7, CPT, VAR, FDIV, 2, false, 1, W>(a, g, rs, s, redo, acc);
            else pp_role<F, SRC, 7, 7, CPT, VAR, FDIV, 2, false, 2, W>(a, g, rs, s, redo, acc);
        } else {
            if (pure) pp_role<F, SRC, 7, 8, CPT, VAR, FDIV, 2, false, 1, W>(a, g, rs, s, redo, acc);
            else pp_role<F, SRC, 7, 8, CPT, VAR, FDIV, 2, false, 2, W>(a, g, rs, s, redo, acc);
        }
    } else if (!low)
        pp_role<F, SRC, 8, 8, CPT, VAR, FDIV, 0, true>(a, g, rs, s, redo, acc);
    else if (!SPLIT)
        pp_role<F, SRC, 8, 8, CPT, VAR, FDIV, 2, false>(a, g, rs, s, redo, acc);
    else if (wave >= kPPRole / 128)
        pp_role<F, SRC, 7, 7, CPT, VAR, FDIV, 2, false>(a, g, rs, s, redo, acc);
    else
        pp_role<F, SRC, 7, 8, CPT, VAR, FDIV, 2, false>(a, g, rs, s, redo, acc);
    if (threadIdx.x == 0 && acc[3] > 0) {
        acc[4] = acc[3] * (unsigned long long)a.T;
#pragma unroll
        for (int q = 0; q < 6; ++q) atomicAdd(&a.counts[q], acc[q]);
    }
}

template <typename F, int SRC, int CPT, int VAR, bool FDIV, bool SPLIT>
__global__ __launch_bounds__(2 * kPPRole) void k_rows_pp(DecodeArgs a, DevGraph g, RowSched rs, unsigned *redo)
{
    pp_kernel<F, SRC, CPT, VAR, FDIV, SPLIT, false>(a, g, rs, redo);
}

// The degree-aware slots with the paired rows' degree-2 bits in registers (the header, graph.h
// pp_pair_rows): rs is the in-register schedule.
template <typename F, int SRC, int CPT, int VAR, bool FDIV>
__global__ __launch_bounds__(2 * kPPRole) void k_rows_ppi(DecodeArgs a, DevGraph g, RowSched rs, unsigned *redo)
{
    pp_kernel<F, SRC, CPT, VAR, FDIV, true, true>(a, g, rs, redo);
}

// The 12-wave block (the header of pp_role): the same in-register schedule, 8 check waves and 4 bit
// waves, the fixed-stride LDS layout (pp_slots FIX). fp64 slots only.
template <typename F, int SRC, int CPT, int VAR, bool FDIV>
__global__ __launch_bounds__(kPPRole + kPPRole / 2) void k_rows_ppw(DecodeArgs a, DevGraph g, RowSched rs, unsigned *redo)
{
    pp_kernel<F, SRC, CPT, VAR, FDIV, true, true, 12>(a, g, rs, redo);
}

static int rows_pp_lds_bytes(const DevGraph &g, const RowSched &rs)
{
    return (int)(2 * (size_t)pp_slot_words(g.N, rs.e_pad + 64) * 8 + kPPRedInts * sizeof(int));
}

static bool rows_pp_supported(const DevGraph &g, const RowSched &rs)
{
    // N <= 4 * kPPRole: a bit-role lane then holds <= 4 bits and one Philox group per
    // codeword, the bound pp_account's ballot-sliced wave sums rely on
    return rs.threads == kPPRole && rs.rpt == 2 && (rs.cpt == 4 || (rs.pair && rs.cpt == 3)) && rs.dc == 8 && (rs.dc_low == 0 || rs.dc_low == 7) &&
           g.N <= 4 * kPPRole && g.N + 3 <= 0xffff && rows_pp_lds_bytes(g, rs) <= 160 * 1024;
}

// Dynamic LDS of k_rows_ppw: the fixed-stride layout (pp_slots FIX) with red[] behind slot 1's c2v.
static size_t rows_ppw_lds_bytes(const RowSched &rs)
{
    return 2 * (size_t)kPPAppStride + 8 + kPPC2vDist + (size_t)(rs.e_pad + 64) * 8 + kPPRedInts * sizeof(int);
}

// k_rows_ppw decodes what k_rows_ppi does whenever the fixed-stride layout holds the code: both
// app arrays within their stride, a c2v array within the reach of a ds offset field, and all of
// it in the 160 KB of a workgroup.
bool pp_w12_layout(int N, int e_pad, int *lds_bytes)
{
    RowSched rs{};
    rs.e_pad = e_pad;
    const size_t bytes = rows_ppw_lds_bytes(rs);
    if (lds_bytes) *lds_bytes = (int)std::min<size_t>(bytes, 0x7fffffff);
    return N >= 0 && e_pad >= 0 && ((size_t)N + 3) * 8 <= kPPAppStride && ((size_t)e_pad + 64) * 8 <= kPPC2vStride &&
           bytes <= kMaxLds;
}

static bool rows_ppw_supported(const DevGraph &g, const RowSched &rs)
{
    return rs.cpt == 3 && pp_w12_layout(g.N, rs.e_pad, nullptr);
}

template <typename F, int SRC, int VAR, bool FDIV>
static const void *pp_fn_t(const RowSched &rs, bool w12)
{
    if constexpr (sizeof(F) == 8) {   // fp32 pairs measured slower with in-register bits: fp64 only
        if (rs.pair && w12) return (const void *)k_rows_ppw<F, SRC, 3, VAR, FDIV>;   // rows_ppw_supported: cpt 3
        if (rs.pair)
            return rs.cpt == 3 ? (const void *)k_rows_ppi<F, SRC, 3, VAR, FDIV> : (const void *)k_rows_ppi<F, SRC, 4, VAR, FDIV>;
    }
    return rs.dc_low == 7 ? (const void *)k_rows_pp<F, SRC, 4, VAR, FDIV, true>
                          : (const void *)k_rows_pp<F, SRC, 4, VAR, FDIV, false>;
}

static const void *pp_fn(const RowSched &rs, const DecodeArgs &a, bool f64, bool w12)
{
    const bool given = a.src == SRC_GIVEN;
#define LDPC_PP_SRC(FT, VARV, FD) \
    return given ? pp_fn_t<FT, SRC_GIVEN, VARV, FD>(rs, w12) : pp_fn_t<FT, SRC_PHILOX, VARV, FD>(rs, w12);
    if (!f64) {   // fp32 pairs: MS, or NMS with the verified reciprocal (rows_fast_f32_ok)
        if (a.variant == V_MS) { LDPC_PP_SRC(float, V_MS, false) }
        if (a.variant == V_NMS && a.nms_fast) { LDPC_PP_SRC(float, V_NMS, false) }
        return nullptr;
    }
    if (a.variant == V_MS) { LDPC_PP_SRC(double, V_MS, false) }
    if (a.variant == V_OMS) { LDPC_PP_SRC(double, V_OMS, false) }
    if (markstein_exact_alpha(a.alpha)) { LDPC_PP_SRC(double, V_NMS, true) }
    LDPC_PP_SRC(double, V_NMS, false)
#undef LDPC_PP_SRC
}

bool plan_rows_pp(const PlanInput &in, LaunchPlan &p)
{
    // The ping-pong kernel's schedule: the degree-aware row slots (graph.h
    // pp_row_slots) when the code admits them, else the row kernel's
    // (LDPC_OPT_PP_SLOTS = 1, tests / A/B: always the row kernel's slots).
    // fp64, LDPC_OPT_PP_SLOTS = 0 on a code with row pairs: k_rows_ppi on the in-register schedule
    // derived from the degree-aware one (the same LDS partition; the plan reports the latter);
    // 2: every bit in LDS on the degree-aware slots. The in-register schedule runs on the 12-wave
    // block (k_rows_ppw) where its LDS layout holds the code (rows_ppw_supported); 3: as 0 on the
    // 16-wave block (k_rows_ppi) always. The plan's lds_bytes stays the decoder state's (what the
    // 16-wave layout takes); the fixed-stride layout's gaps are pad_lds_bytes.
    const int slots = opt(LDPC_OPT_PP_SLOTS);
    const RowSched *rs = in.rs_pp && slots != 1 ? in.rs_pp : in.rs;
    if (!rows_pp_supported(in.g, *rs)) return false;
    const RowSched *ri = nullptr;
    if (in.f64 && LDPC_PP_NOB2 && LDPC_PP_PREFETCH && rs == in.rs_pp && in.rs_ppi && (slots == 0 || slots == 3) &&
        rs->dc_low == 7 && in.rs_ppi->pair && in.rs_ppi->e_pad == rs->e_pad && rows_pp_supported(in.g, *in.rs_ppi))
        ri = in.rs_ppi;
    p.kernel = Kernel::rows_pp;
    p.name = "rows_pp";
    p.redo = true;
    p.rs = rs;
    p.rs_inreg = ri;
    const bool w12 = ri && slots == 0 && rows_ppw_supported(in.g, *ri);
    p.fn = pp_fn(ri ? *ri : *rs, in.a, in.f64, w12);
    p.threads = w12 ? kPPRole + kPPRole / 2 : 2 * kPPRole;
    p.lds_bytes = rows_pp_lds_bytes(in.g, *rs);
    p.pad_lds_bytes = w12 ? (int)rows_ppw_lds_bytes(*ri) - p.lds_bytes : 0;
    p.blocks_per_cu = 1;   // one block per CU
    const int CW = 2 * (in.f64 ? PPCw<double>::C : PPCw<float>::C);
    p.grid = std::min(in.num_cus, (in.a.batch + CW - 1) / CW);
    return true;
}

hipError_t launch_rows_pp(const LaunchPlan &p, const DevGraph &g, const DecodeArgs &a, unsigned *redo, hipStream_t s)
{
    void *args[] = {(void *)&a, (void *)&g, (void *)(p.rs_inreg ? p.rs_inreg : p.rs), &redo};
    return launch_fn(p, args, s);
}

}  // namespace ldpc
