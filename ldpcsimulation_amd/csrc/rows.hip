// rows.hip -- the row-parallel min-sum kernel (k_decode_rows), its plan and launch.
// The fp32 row kernel (k_decode_rows) adds its pairs as one v_pk_add_f32: two plain
// v_add_f32 measured 10.0 vs 8.8 ms per bench launch there (the ping-pong kernel is the
// other way round: minsum_common.h padd, template parameter PK).
#include "minsum_kernels.h"

namespace ldpc {

// =====================================================================
// Row-parallel kernel (the throughput path).
//
// Block = `threads` threads (>= M, multiple of 64): thread t owns check row t
// for the whole persistent launch, with its row's bit indices and c2v slot
// positions held in registers (loaded once per launch from the RowSchedule
// built on the host), and CPT bit-node slots (columns sorted by degree).
// Each thread decodes C codewords at once (independent instruction streams).
// LDS per codeword: app[N] + c2v[e_pad], c2v in wave-slot-major order so the
// bit-node phase reads 64 consecutive words per wave instruction.
// Per iteration: check phase (gather app, rebuild the old c2v from the row
// state kept in registers, v2c = app - c2v_old, min/second-min/argmin/signs,
// normalise/offset, scatter the new c2v) | barrier | bit phase (sum yq + c2v
// in nlist order, write app) | barrier.
// =====================================================================


template <int DC, int C, int DCA = DC, bool PK = false>
__device__ __forceinline__ bool cn_fast(const Pack<double, C> (&)[DCA], Pack<double, C> (&)[DCA], bool, float, float)
{
    return false;   // never called: fp64 always takes the exact path
}

// Block shape per rows-per-thread: RPT=1 up to 1024 threads (4 waves/SIMD);
// RPT=2 512 threads and RPT=3 384 threads, sized for two blocks per CU
// (4 resp. 3 waves per SIMD: 128 resp. 168 VGPRs).
template <int RPT> struct RowsShape;
template <> struct RowsShape<1> { static constexpr int threads = 1024, waves_per_eu = 4; };
#ifndef LDPC_RPT2_WAVES
#define LDPC_RPT2_WAVES 4
#endif
template <> struct RowsShape<2> { static constexpr int threads = 512, waves_per_eu = LDPC_RPT2_WAVES; };
template <> struct RowsShape<3> { static constexpr int threads = 384, waves_per_eu = 3; };

template <typename F, int SRC, int C, int DC, int CPT, int RPT>
__global__ __launch_bounds__(RowsShape<RPT>::threads, RowsShape<RPT>::waves_per_eu) void k_decode_rows(
    DecodeArgs a, DevGraph g, RowSched rs)
{
    using MT = typename MetaOf<DC>::T;
    using P = Pack<F, C>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int N = g.N, EA = rs.e_pad + 64;         // + one dummy slot per lane for padding edges
    P *app = reinterpret_cast<P *>(smem);          // [N + 1]: bit N is the +INF sentinel of padding edges
    P *c2v = app + (N + 2);                        // [EA] (N+2 keeps 16-B alignment)
    int *red = reinterpret_cast<int *>(c2v + EA);

    // ---- the thread's rows (tid + r*nt) and bit slots, in registers for the whole launch ----
    int deg[RPT];
    MT degmask[RPT];
    uint32_t colw[RPT][DC / 2], posw[RPT][DC / 2];
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const int j = tid + r * nt;
        deg[r] = rs.cn_deg[j];
        degmask[r] = (deg[r] >= (int)(8 * sizeof(MT))) ? ~(MT)0 : (((MT)1 << deg[r]) - 1);
#pragma unroll
        for (int q = 0; q < DC / 8; ++q) {
            const uint4 xc = reinterpret_cast<const uint4 *>(rs.cn_cols + (size_t)j * DC)[q];
            const uint4 xp = reinterpret_cast<const uint4 *>(rs.cn_pos + (size_t)j * DC)[q];
            colw[r][4 * q + 0] = xc.x; colw[r][4 * q + 1] = xc.y; colw[r][4 * q + 2] = xc.z; colw[r][4 * q + 3] = xc.w;
            posw[r][4 * q + 0] = xp.x; posw[r][4 * q + 1] = xp.y; posw[r][4 * q + 2] = xp.z; posw[r][4 * q + 3] = xp.w;
        }
    }
    // bit slots: a thread's slots have non-increasing group degree (graph.cpp)
    // Slot i of lane l: c2v edge k at vgb[i] + l + 64k (vgb and the group degree
    // vgd are wave-uniform: SGPRs); the bit it sums into is vdst (two 16-bit
    // entries per register; the spare app entry N+1 for an empty slot).
    const int lane = tid & 63;
    int vgb[CPT], vgd[CPT];
    uint32_t vdst2[(CPT + 1) / 2] = {};
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
        const int c = rs.vn_col[tid * CPT + i];
        vdst2[i / 2] |= (uint32_t)(c == 0xffff ? N + 1 : c) << (16 * (i & 1));
        const uint32_t info = rs.vn_info[tid * CPT + i];
        vgb[i] = __builtin_amdgcn_readfirstlane((int)(info & 0xffffu) - lane);
        vgd[i] = __builtin_amdgcn_readfirstlane((int)(info >> 24));
    }
    auto vdst = [&](int i) -> int { return (int)((vdst2[i / 2] >> (16 * (i & 1))) & 0xffffu); };
    if (tid == 0) {
        P inf;
#pragma unroll
        for (int c = 0; c < C; ++c) inf.v[c] = dinf<F>();
        app[N] = inf;
#pragma unroll
        for (int q = 0; q < 3 * C; ++q) red[32 + q] = 0;   // block_sum_lds totals
        red[31] = 0;   // the premise flag: cleared again by thread 0 at the end of each group
    }
    // Padding slots of the bit-node layout hold +0 (adding +0 leaves every sum, and hence
    // every decision, unchanged); nothing writes them after this (the channel stages into
    // app, the check rows scatter into their own slots and the per-lane dummies).
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
        const int dg = (int)((rs.vn_info[tid * CPT + i] >> 16) & 0xffu);
        const int base = vgb[i] + lane, gd = vgd[i];
        P z;
#pragma unroll
        for (int c = 0; c < C; ++c) z.v[c] = F(0);
        for (int k = dg; k < gd; ++k) c2v[base + k * 64] = z;
    }
    __syncthreads();   // the flag's first clear before any channel raises it

    // The second-dispatched half of the workgroup at priority 1 for the whole
    // launch (MI355X_MICROARCH "Two waves per SIMD" item 4): +0.25 % in an
    // interleaved 3-round A/B (14 549 -> 14 594 Mbit/s), no change in results.
    if ((tid >> 6) >= (nt >> 7)) __builtin_amdgcn_s_setprio(1);
    const F alpha = (F)a.alpha, delta = (F)a.delta;
    const int ngrp = (a.batch + C - 1) / C;
    unsigned long long st_chan = 0, st_cn = 0, st_vn = 0, st_acct = 0;
    (void)st_chan; (void)st_cn; (void)st_vn; (void)st_acct;
    // the block's totals (thread 0), added to a.counts once at the end
    unsigned long long acc[6] = {0, 0, 0, 0, 0, 0};
    for (int grp = blockIdx.x; grp < ngrp; grp += gridDim.x) {
        STAMP(t_start);
        // ---- channel (:214-238), staged into app as yq + 0 (never -0: v2c = app - c2v then
        // differs at most in the sign of a zero, which sgn() and |.| ignore, and the decision
        // app > 0 is the same; the fast check node relies on it); an input outside the fast
        // premise (|yq| >= 1e30, inf, NaN) raises the flag, which thread 0 cleared at the end
        // of the previous group ----
        int unc[C];
        bool ch_ok = true;
        auto put = [&](int v, int c, F q) {
            q = q + F(0);
            ch_ok &= dabs(q) < F(1e30f);
            app[v].v[c] = q;
        };
        const int8_t *cvec[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            unc[c] = 0;
            cvec[c] = nullptr;
            const int b = grp * C + c;
            if (b >= a.batch) {   // missing partner of an odd batch: benign +1 samples, never counted
                for (int v = tid; v < N; v += nt) app[v].v[c] = F(1);
                continue;
            }
            const uint64_t cw = a.first_cw + (uint64_t)b;
            if (SRC == SRC_GIVEN) {
                if (a.c) cvec[c] = a.c + (size_t)b * N;
                const F *y = reinterpret_cast<const F *>(a.y) + (size_t)b * N;
                for (int v = tid; v < N; v += nt) {
                    const F q = front_end<F>(y[v], a);
                    put(v, c, q);
                    const int cv = cvec[c] ? cvec[c][v] : 1;
                    unc[c] += ((q > F(0) ? 1 : -1) * cv < 0);
                }
            } else {
                if (a.cw_table) cvec[c] = a.cw_table + (size_t)(cw % (uint64_t)a.cw_rows) * N;
                const F sigma = (F)a.sigma;
                const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
                if (!a.cw_table && !a.y_out && !a.quantize && !a.saturate && (N & 3) == 0) {
                    // the common case in straight-line code (the all-zero codeword, no front end,
                    // no sample output): the same values as the general loop below
                    for (int g4 = tid; g4 * 4 < N; g4 += nt) {
                        uint32_t u[4];
                        philox4x32_10<LDPC_ROWS_MAD64 != 0>((uint32_t)g4, (uint32_t)cw, (uint32_t)(cw >> 32), a.stream_id,
                                                            k0, k1, u);
                        F n[4];
                        box_muller(u[0], u[1], n[0], n[1]);
                        box_muller(u[2], u[3], n[2], n[3]);
#pragma unroll
                        for (int q4 = 0; q4 < 4; ++q4) {
                            const F qv = (F(1) + sigma * n[q4]) + F(0);   // (F)cv * (1 + sigma n), cv = +1; yq + 0
                            unc[c] += (qv > F(0) ? 1 : -1) < 0;
                            ch_ok &= dabs(qv) < F(1e30f);
                            app[4 * g4 + q4].v[c] = qv;
                        }
                    }
                    continue;
                }
                for (int g4 = tid; g4 * 4 < N; g4 += nt) {
                    uint32_t u[4];
                    philox4x32_10<LDPC_ROWS_MAD64 != 0>((uint32_t)g4, (uint32_t)cw, (uint32_t)(cw >> 32), a.stream_id, k0, k1, u);
                    F n[4];
                    box_muller(u[0], u[1], n[0], n[1]);
                    box_muller(u[2], u[3], n[2], n[3]);
#pragma unroll
                    for (int q4 = 0; q4 < 4; ++q4) {
                        const int v = g4 * 4 + q4;
                        if (v < N) {
                            const int cv = cvec[c] ? cvec[c][v] : 1;
                            const F yv = (F)cv * (F(1) + sigma * n[q4]);
                            if (a.y_out) reinterpret_cast<F *>(a.y_out)[(size_t)b * N + v] = yv;
                            const F q = front_end<F>(yv, a);
                            put(v, c, q);
                            unc[c] += ((q > F(0) ? 1 : -1) * cv < 0);
                        }
                    }
                }
            }
        }
        if (__builtin_amdgcn_ballot_w64(!ch_ok)) {   // rare: an input outside the fast premise
            asm volatile(";");
            if (!ch_ok) red[31] = 1;
        }
        __syncthreads();
        // yq of the thread's bit slots, read back as staged (v2c = yq on the first pass,
        // :364-370); a padding slot +0
        P yq[CPT];
#pragma unroll
        for (int i = 0; i < CPT; ++i) {
            yq[i] = app[vdst(i) < N ? vdst(i) : 0];
            if (vdst(i) >= N)
#pragma unroll
                for (int c = 0; c < C; ++c) yq[i].v[c] = F(0);
        }

        // c2v sent on each edge last iteration: +0 before the first. RPT <= 2 keeps
        // the check node's own copy in registers; larger RPT re-reads it from its
        // c2v slots (written only by this thread, read by the bit phase) to stay
        // within the register budget of two blocks per CU.
        // (Re-reading is only safe on the exact path: padding edges share per-lane
        // dummy slots, so their "old message" is whatever another row wrote there.)
        constexpr bool PREV_REG = RPT <= 2;
        P prev[PREV_REG ? RPT : 1][DC];
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
            if (PREV_REG) {
#pragma unroll
                for (int k = 0; k < DC; ++k)
#pragma unroll
                    for (int c = 0; c < C; ++c) prev[PREV_REG ? r : 0][k].v[c] = F(0);
            } else {
                P z;
#pragma unroll
                for (int c = 0; c < C; ++c) z.v[c] = F(0);
#pragma unroll
                for (int k = 0; k < DC; ++k) c2v[u16_at<DC>(posw[r], k)] = z;
            }
        }

        STAMP(t_iter0);
#ifdef LDPC_STAMPS
        st_chan += t_iter0 - t_start;
#endif
        // One iteration loop, instantiated twice: the fast check-node loop runs
        // while its premise holds (flag red[31] clear: every c2v entering the
        // iteration is below 1e30) and hands over to the exact loop, which
        // continues from the same state. Separate loops keep the two check-node
        // bodies out of each other's register allocation.
        auto iterate = [&](auto fast_tag, int it0) -> int {
            constexpr bool FAST = decltype(fast_tag)::value;
            int it = it0;
            // fast-path flag: read right after the check-node barrier of the previous
            // iteration (in flight during the bit-node phase), so no LDS round trip
            // opens the iteration; red[31] was cleared before the first iteration
            int flag = FAST ? red[31] : 0;   // set by an input outside the premise
            for (; it < a.T; ++it) {
                STAMP(t_cn0);
                if (FAST && __builtin_amdgcn_readfirstlane(flag) != 0) break;
                // ---- check nodes (:410-450, :494-515); row r+1's gathers are issued
                // before row r is computed ----
                P xin[2][DC];
                if (LDPC_ROWS_PRIOBAL) __builtin_amdgcn_s_setprio(3);
#pragma unroll
                for (int k = 0; k < DC; ++k) xin[0][k] = app[u16_at<DC>(colw[0], k)];   // padding edges read +INF
#pragma unroll
                for (int r = 0; r < RPT; ++r) {
                    if (LDPC_ROWS_PRIOBAL && r > 0) __builtin_amdgcn_s_setprio(2);
                    if (r + 1 < RPT) {
#pragma unroll
                        for (int k = 0; k < DC; ++k) xin[(r + 1) & 1][k] = app[u16_at<DC>(colw[r + 1 < RPT ? r + 1 : r], k)];
                    }
                    P (&pv)[DC] = prev[PREV_REG ? r : 0];
                    if (!PREV_REG) {
#pragma unroll
                        for (int k = 0; k < DC; ++k) pv[k] = c2v[u16_at<DC>(posw[r], k)];
                    }
                    if constexpr (FAST) {
                        const bool ok = cn_fast<DC, C, DC, true>(xin[r & 1], pv, a.variant == V_NMS, (float)alpha, a.alpha_rcp);
                        // Rows past M (degree 0) only write the never-read dummy slots.
                        if (!ok && deg[r] > 0) red[31] = 1;
                    } else {
#pragma unroll
                        for (int c = 0; c < C; ++c) cn_exact<F, C, DC>(xin[r & 1], c, pv, degmask[r], a, alpha, delta);
                    }
#pragma unroll
                    for (int k = 0; k < DC; ++k) c2v[u16_at<DC>(posw[r], k)] = pv[k];   // padding edges: the lane's dummy slot
#ifndef LDPC_NO_ROW_FENCE
                    // keep the rows' live ranges apart (register pressure: two blocks per CU)
                    if (RPT > 1) __builtin_amdgcn_sched_barrier(0);
#endif
                }
                if (LDPC_ROWS_PRIOBAL) __builtin_amdgcn_s_setprio(0);
                __syncthreads();
                if (FAST) flag = red[31];
                STAMP(t_vn0);
#ifdef LDPC_STAMPS
                st_cn += t_vn0 - t_cn0;
#endif
                // ---- bit nodes: sum = yq + c2v in nlist order (:452-476); edges past a
                // bit's own degree hold +0 ----
                {
                    P sum[CPT];
#pragma unroll
                    for (int i = 0; i < CPT; ++i) sum[i] = yq[i];
                    int k = 0;
                    vn_phases<F, C, CPT, CPT, true>(c2v + lane, vgb, vgd, k, sum);
#pragma unroll
                    for (int i = 0; i < CPT; ++i) app[vdst(i)] = sum[i];
                }
                __syncthreads();
#ifdef LDPC_STAMPS
                { STAMP(t_vn1); st_vn += t_vn1 - t_vn0; }
#endif
            }
            return it;
        };
        int it_done = 0;
        if constexpr (sizeof(F) == 4 && PREV_REG)
            if (a.variant == V_MS || (a.variant == V_NMS && a.nms_fast)) it_done = iterate(std::true_type{}, 0);
        if (it_done < a.T) iterate(std::false_type{}, it_done);
        STAMP(t_acct0);

        // ---- decisions, error weight, syndrome, accounting ----
        int sums[3 * C];   // per codeword: error weight, uncoded errors, syndrome failure
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int b = grp * C + c;
            int w = 0, synd = 0;
            if (b < a.batch) {
#pragma unroll
                for (int i = 0; i < CPT; ++i) {
                    const int v = vdst(i);
                    if (v < N) {
                        const int d = app[v].v[c] > F(0) ? 1 : -1;
                        const int cv = cvec[c] ? cvec[c][v] : 1;
                        w += (d != cv);
                        if (a.d_out) a.d_out[(size_t)b * N + v] = (int8_t)d;
                    }
                }
                // padding edges read the +inf sentinel: parity 0
#pragma unroll
                for (int r = 0; r < RPT; ++r) {
                    int par = 0;
#pragma unroll
                    for (int k = 0; k < DC; ++k) par ^= (app[u16_at<DC>(colw[r], k)].v[c] > F(0)) ? 0 : 1;
                    synd |= par;
                }
            }
            sums[3 * c] = w;
            sums[3 * c + 1] = unc[c];
            sums[3 * c + 2] = synd;
        }
        if (LDPC_ROWS_ACCT) block_sum_lds<3 * C>(sums, red + 32);   // re-zeroed by thread 0; the step's last barrier orders it
        else block_sum_n_t0<3 * C>(sums, red + 32);
        if (tid == 0) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int b = grp * C + c;
                if (b >= a.batch) continue;
                const int w = sums[3 * c], uc = sums[3 * c + 1], sf = sums[3 * c + 2] > 0;
                acc[0] += (unsigned long long)w;
                acc[1] += (unsigned long long)(w > 0);
                acc[2] += (unsigned long long)uc;
                acc[3] += 1ull;
                acc[5] += (unsigned long long)sf;
                if (w > 0 && a.hist) atomicAdd(&a.hist[w - 1], 1ull);
                if (a.frame_res) a.frame_res[b] = make_int4(w, uc, sf, 0);
            }
            red[31] = 0;   // the next group's premise flag (raised no earlier than its channel)
        }
        __syncthreads();
#ifdef LDPC_STAMPS
        { STAMP(t_end); st_acct += t_end - t_acct0; }
#endif
    }
    if (tid == 0 && acc[3] > 0) {
        acc[4] = acc[3] * (unsigned long long)a.T;
#pragma unroll
        for (int q = 0; q < 6; ++q) atomicAdd(&a.counts[q], acc[q]);
    }
#ifdef LDPC_STAMPS
    if (tid == 0 && a.stamps) {
        a.stamps[blockIdx.x * 4 + 0] = st_chan;
        a.stamps[blockIdx.x * 4 + 1] = st_cn;
        a.stamps[blockIdx.x * 4 + 2] = st_vn;
        a.stamps[blockIdx.x * 4 + 3] = st_acct;
    }
#endif
}
// Codewords per thread: 2 for the fp32 DC=8 kernel (no spills at 101 VGPRs),
// 1 where two would spill (fp64, wider rows).
static int rows_cw_per_block(bool f64, int dc)
{
#ifdef LDPC_C1
    (void)f64; (void)dc;
    return 1;
#else
    return (!f64 && dc == 8) ? 2 : 1;
#endif
}

static size_t rows_lds(const DevGraph &g, const RowSched &rs, bool f64, int C)
{
    const size_t fs = f64 ? 8 : 4;
    // + red: 32 ints (fast-path flag at [31]) and 16 waves x 8 sums
    return ((size_t)C * ((size_t)g.N + 2 + (size_t)rs.e_pad + 64) * fs + 4 * (32 + 16 * 8) + 15) & ~(size_t)15;
}
// The instantiation for a schedule's shape (C, DC, CPT, RPT); null: none is built.
template <typename F, int SRC>
static const void *rows_fn(const RowSched &rs)
{
#ifdef LDPC_C1
    constexpr int C8 = 1;
#else
    constexpr int C8 = sizeof(F) == 4 ? 2 : 1;
#endif
#define LDPC_ROWS_CASE(CV, DCV, CPTV, RPTV)                                   \
    if (rs.dc == DCV && rs.cpt == CPTV && rs.rpt == RPTV)                   \
        return (const void *)k_decode_rows<F, SRC, CV, DCV, CPTV, RPTV>;
    LDPC_ROWS_CASE(C8, 8, 2, 1)
    LDPC_ROWS_CASE(C8, 8, 4, 1)
    LDPC_ROWS_CASE(C8, 8, 4, 2)
    LDPC_ROWS_CASE(1, 16, 2, 1)
    LDPC_ROWS_CASE(1, 16, 4, 1)
    LDPC_ROWS_CASE(1, 16, 4, 2)
    LDPC_ROWS_CASE(1, 32, 2, 1)
    LDPC_ROWS_CASE(1, 32, 4, 1)
    LDPC_ROWS_CASE(1, 32, 4, 2)
#undef LDPC_ROWS_CASE
    return nullptr;
}

// Row graphs on the fast path: a kernel holding only the fast check node plus the
// exact re-decode (k_redo) of the codewords whose premise failed.
//   fp64: the ping-pong kernel (rows_pp.hip: two codewords per 1024-thread block,
//         check and bit waves overlapped) when the schedule fits it, else the
//         one-codeword-per-block k_rows_fast (LDPC_OPT_ROWS64 = 1 forces the latter);
//   fp32: pairs as float2 -- MS and NMS with the verified reciprocal (a after
//         nms_setup) -- on the ping-pong kernel (7.4 vs 8.8 ms per bench launch for
//         the row kernel), on the pair instance of k_rows_fast with
//         LDPC_OPT_ROWS32 = 1, on the row kernel (k_decode_rows, fast and
//         exact loops in one) with LDPC_OPT_ROWS32 = 2 and for everything else (OMS,
//         codes the ping-pong schedule does not fit).
// LDPC_OPT_ROWS64 = 2 keeps the row kernel for fp64 too.
static bool plan_fast_path(const PlanInput &in, LaunchPlan &p)
{
    const int r64 = opt(LDPC_OPT_ROWS64), r32 = opt(LDPC_OPT_ROWS32);
    if (in.f64 && r64 == 2) return false;
    if (redo_lds_bytes(in.g, in.f64) > 160 * 1024) return false;
    if (in.f64) return (r64 == 0 && plan_rows_pp(in, p)) || plan_rows_fast(in, p);
    if (!rows_fast_f32_ok(in.a)) return false;
    if (r32 == 1) return plan_rows_fast(in, p);
    if (r32 == 2) return false;
    return plan_rows_pp(in, p);
}

bool plan_rows(const PlanInput &in, LaunchPlan &p)
{
    if (!in.rs || in.rs->threads <= 0) return false;
    const RowSched &rs = *in.rs;
    const int C = rows_cw_per_block(in.f64, rs.dc);
    const size_t lds = rows_lds(in.g, rs, in.f64, C);
    if (lds > kMaxLds) return false;
    p = LaunchPlan{};
    p.kernel = Kernel::rows;
    p.name = "rows";
    p.threads = rs.threads;
    p.lds_bytes = (int)lds;
    p.cw_per_block = C;
    p.rs = in.rs;
    const bool fast = plan_fast_path(in, p);
    // reported: the row kernels of one (C) share the LDS / thread shape --
    // occupancy of a representative instantiation of the same block shape (kernels.hip
    // plan_lds; the fast row kernel reports the row kernel's, the ping-pong kernel its own 1)
    if (p.kernel != Kernel::rows_pp) {
        const void *rep = in.f64 ? (const void *)k_decode_rows<double, SRC_PHILOX, 1, 8, 4, 2>
                                 : (C == 2 ? (const void *)k_decode_rows<float, SRC_PHILOX, 2, 8, 4, 2>
                                           : (const void *)k_decode_rows<float, SRC_PHILOX, 1, 16, 4, 2>);
        p.blocks_per_cu = occupancy(rep, rs.threads, (int)lds);
    }
    if (fast) return true;
    p.fn = for_f_src(in.f64, in.a.src, [&](auto f, auto s) { return rows_fn<typename decltype(f)::type, decltype(s)::value>(rs); });
    if (!p.fn) return true;   // launch_rows refuses it
    // Persistent grid of the resident blocks: what the CU holds of the kernel that launches.
    int per_cu = std::max(1, occupancy(p.fn, p.threads, p.lds_bytes));
    if (const int cap = opt(LDPC_OPT_ROWS_BPC))   // diagnostic: fewer resident blocks
        if (cap < per_cu) per_cu = cap;
    p.grid = std::min(per_cu * in.num_cus, (in.a.batch + C - 1) / C);
    return true;
}

hipError_t launch_rows(const LaunchPlan &p, const DevGraph &g, const DecodeArgs &a, hipStream_t s)
{
    void *args[] = {(void *)&a, (void *)&g, (void *)p.rs};
    return launch_fn(p, args, s);
}

}  // namespace ldpc
