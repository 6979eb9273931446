// rows_es.hip -- the row-parallel min-sum kernel with early termination (k_rows_es), its
// plan and launch: ldpc_decoder_cfg.early_stop = 1 on a graph with a row schedule.
//
// The frame's result is D(s), what the fixed-T decoders return at T = s, for the smallest
// s in 0..T whose decisions are a codeword (s = T when none is): the syndrome is checked
// before every iteration and after the last one.
//
// Built on the row kernel (rows.hip k_decode_rows): the same RowSched, app and c2v in LDS,
// the thread's rows and bit slots in registers for the whole persistent launch, the exact
// check node (cn_exact) and vn_phases, one codeword per block. What differs:
//  * the check phase already gathers app for the thread's rows; the parity of !(x > 0)
//    over those gathers is the accounting's syndrome expression (padding edges read the
//    +INF sentinel: parity 0). A wave with an unsatisfied row raises the double-buffered
//    LDS flag fl[it & 1] before the barrier that follows the check phase anyway, and every
//    thread reads it after that barrier: no extra barrier, no extra LDS pass. With the
//    flag clear the codeword stops with iters = it completed bit phases; app still holds
//    D(it) (the check phase never writes it) and the c2v just scattered is discarded;
//  * early stop makes codewords unequal, so blocks take them by ticket as k_ddbmp_rows
//    does: blockIdx.x first, then gridDim.x + atomicAdd(ticket, 1); thread 0 draws the
//    next ticket while the current codeword decodes and broadcasts it at the accounting
//    barrier;
//  * no fast check node, no premise, no redo list.
#include "minsum_kernels.h"
#include "frame.h"

namespace ldpc {

// Block shapes of the row kernel (rows.hip RowsShape): RPT = 1 up to 1024 threads, RPT = 2
// 512 threads. fp32 sizes RPT = 2 for two blocks per CU (4 waves per SIMD, 128 VGPRs). fp64
// does not: at 128 VGPRs the (8, 4, 2) instance spills 244 bytes per lane, and with one block
// per CU (2 waves per SIMD: 192 VGPRs, no scratch) the N=1944 NMS launch of 65 536 frames
// takes 7.7 instead of 12.5 ms at 2.0 dB and 5.0 instead of 8.0 ms at 3.0 dB. (fp32 the
// other way round: 3.6 -> 6.1 ms at 2.0 dB with one block per CU.)
template <typename F, int RPT> struct EsShape;
template <typename F> struct EsShape<F, 1> {
    static constexpr int threads = 1024;
    static constexpr int waves_per_eu = 4;
};
template <typename F> struct EsShape<F, 2> {
    static constexpr int threads = 512;
    static constexpr int waves_per_eu = (sizeof(F) == 8) ? 2 : 4;
};

// red: [0..1] the stop flag fl, [2] the next codeword, [4..] block_sum_n_t0's 16 x 3 partials
constexpr int kEsRedInts = 4 + 16 * 3;

template <typename F, int SRC, int DC, int CPT, int RPT>
__global__ __launch_bounds__((EsShape<F, RPT>::threads), (EsShape<F, RPT>::waves_per_eu)) void k_rows_es(
    DecodeArgs a, DevGraph g, RowSched rs, unsigned *ticket)
{
    using MT = typename MetaOf<DC>::T;
    using P = Pack<F, 1>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int N = g.N, EA = rs.e_pad + 64;         // + one dummy slot per lane for padding edges
    P *app = reinterpret_cast<P *>(smem);          // [N + 2]: bit N is the +INF sentinel of padding edges, N + 1 spare
    P *c2v = app + (N + 2);                        // [EA]
    int *red = reinterpret_cast<int *>(c2v + EA);
    volatile int *fl = red;

    // ---- the thread's rows (tid + r*nt) and bit slots, in registers for the whole launch ----
    MT degmask[RPT];
    uint32_t colw[RPT][DC / 2], posw[RPT][DC / 2];
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const int j = tid + r * nt;
        const int deg = rs.cn_deg[j];
        degmask[r] = (deg >= (int)(8 * sizeof(MT))) ? ~(MT)0 : (((MT)1 << deg) - 1);
#pragma unroll
        for (int q = 0; q < DC / 8; ++q) {
            const uint4 xc = reinterpret_cast<const uint4 *>(rs.cn_cols + (size_t)j * DC)[q];
            const uint4 xp = reinterpret_cast<const uint4 *>(rs.cn_pos + (size_t)j * DC)[q];
            colw[r][4 * q + 0] = xc.x; colw[r][4 * q + 1] = xc.y; colw[r][4 * q + 2] = xc.z; colw[r][4 * q + 3] = xc.w;
            posw[r][4 * q + 0] = xp.x; posw[r][4 * q + 1] = xp.y; posw[r][4 * q + 2] = xp.z; posw[r][4 * q + 3] = xp.w;
        }
    }
    // Slot i of lane l: c2v edge k at vgb[i] + l + 64k (vgb and the group degree vgd are
    // wave-uniform); the bit it sums into is vdst (the spare app entry N + 1 for an empty slot).
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
    auto vdst = [&](int i) -> int {
        return LDPC_CHK((int)((vdst2[i / 2] >> (16 * (i & 1))) & 0xffffu), N + 2, CHK_ES_APP_WRITE);
    };
    auto col = [&](int r, int k) -> int { return LDPC_CHK(u16_at<DC>(colw[r], k), N + 2, CHK_ES_GATHER); };
    auto pos = [&](int r, int k) -> int { return LDPC_CHK(u16_at<DC>(posw[r], k), EA, CHK_ES_SCATTER); };
    if (tid == 0) app[N].v[0] = dinf<F>();
    // Padding slots of the bit-node layout hold +0 (adding +0 leaves every sum unchanged);
    // nothing writes them after this.
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
        const int dg = (int)((rs.vn_info[tid * CPT + i] >> 16) & 0xffu);
        const int base = vgb[i] + lane, gd = vgd[i];
        for (int k = dg; k < gd; ++k) c2v[LDPC_CHK(base + k * 64, EA, CHK_ES_BIT_READ)].v[0] = F(0);
    }

    const F alpha = (F)a.alpha, delta = (F)a.delta;
    const int T = a.T;
    // the block's totals (thread 0), added to a.counts once at the end
    unsigned long long acc[6] = {0, 0, 0, 0, 0, 0};
    // Codewords: blockIdx.x first, then tickets; thread 0 draws the next ticket while the
    // current codeword decodes.
    unsigned nxt = 0;
    if (tid == 0) nxt = gridDim.x + atomicAdd(ticket, 1u);
    for (int b = blockIdx.x; b < a.batch;) {
        // ---- channel (:214-238), staged into app as yq + 0 (as the row kernel stages it) ----
        const int8_t *cvec = frame_codeword<SRC>(a, b, N);
        int unc = 0;
        channel_bits<F, SRC, LDPC_ROWS_MAD64 != 0>(a, b, N, cvec, a.y_out, [&](int v, F yv) {
            const F q = front_end<F>(yv, a);
            app[v].v[0] = q + F(0);
            const int cv = cvec ? cvec[v] : 1;
            unc += ((q > F(0) ? 1 : -1) * cv < 0);
        });
        if (tid == 0) {
            fl[0] = 0;
            fl[1] = 0;
        }
        __syncthreads();
        // yq of the thread's bit slots, read back as staged; a padding slot +0
        P yq[CPT];
#pragma unroll
        for (int i = 0; i < CPT; ++i) {
            yq[i] = app[vdst(i) < N ? vdst(i) : 0];
            if (vdst(i) >= N) yq[i].v[0] = F(0);
        }
        // c2v sent on each edge last iteration: +0 before the first (:364-370)
        P prev[RPT][DC];
#pragma unroll
        for (int r = 0; r < RPT; ++r)
#pragma unroll
            for (int k = 0; k < DC; ++k) prev[r][k].v[0] = F(0);

        int it = 0;
        for (; it < T; ++it) {
            // ---- check nodes (:410-450, :494-515) and the syndrome of D(it): row r+1's
            // gathers are issued before row r is computed ----
            P xin[2][DC];
            int fail = 0;
            if (LDPC_ROWS_PRIOBAL) __builtin_amdgcn_s_setprio(3);
#pragma unroll
            for (int k = 0; k < DC; ++k) xin[0][k] = app[col(0, k)];   // padding edges read +INF
#pragma unroll
            for (int r = 0; r < RPT; ++r) {
                if (LDPC_ROWS_PRIOBAL && r > 0) __builtin_amdgcn_s_setprio(2);
                if (r + 1 < RPT) {
#pragma unroll
                    for (int k = 0; k < DC; ++k) xin[(r + 1) & 1][k] = app[col(r + 1 < RPT ? r + 1 : r, k)];
                }
                P (&xr)[DC] = xin[r & 1];
                P (&pv)[DC] = prev[r];
                int par = 0;
#pragma unroll
                for (int k = 0; k < DC; ++k) par ^= (xr[k].v[0] > F(0)) ? 0 : 1;
                fail |= par;
                cn_exact<F, 1, DC>(xr, 0, pv, degmask[r], a, alpha, delta);
#pragma unroll
                for (int k = 0; k < DC; ++k) c2v[pos(r, k)] = pv[k];   // padding edges: the lane's dummy slot
                // keep the rows' live ranges apart (register pressure)
                if (RPT > 1) __builtin_amdgcn_sched_barrier(0);
            }
            if (LDPC_ROWS_PRIOBAL) __builtin_amdgcn_s_setprio(0);
            if (__builtin_amdgcn_ballot_w64(fail != 0) != 0 && lane == 0) fl[it & 1] = 1;
            __syncthreads();
            if (fl[it & 1] == 0) break;           // uniform over the block: D(it) is a codeword
            if (tid == 0) fl[(it + 1) & 1] = 0;   // nobody reads or sets it before the next barrier
            // ---- bit nodes: sum = yq + c2v in nlist order (:452-476); edges past a bit's
            // own degree hold +0 ----
            {
                P sum[CPT];
#pragma unroll
                for (int i = 0; i < CPT; ++i) sum[i] = yq[i];
                int k = 0;
                vn_phases<F, 1, CPT, CPT, false>(c2v + lane, vgb, vgd, k, sum, LDPC_CHK_LIM(EA - lane), CHK_ES_BIT_READ);
#pragma unroll
                for (int i = 0; i < CPT; ++i) app[vdst(i)] = sum[i];
            }
            __syncthreads();
        }

        // ---- decisions, error weight, syndrome (after iteration T; 0 after a stop), accounting ----
        int w = 0, synd = 0;
#pragma unroll
        for (int i = 0; i < CPT; ++i) {
            const int v = vdst(i);
            if (v < N) {
                const int d = app[v].v[0] > F(0) ? 1 : -1;
                const int cv = cvec ? cvec[v] : 1;
                w += (d != cv);
                if (a.d_out) a.d_out[(size_t)b * N + v] = (int8_t)d;
            }
        }
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
            int par = 0;
#pragma unroll
            for (int k = 0; k < DC; ++k) par ^= (app[col(r, k)].v[0] > F(0)) ? 0 : 1;
            synd |= par;
        }
        int sums[3] = {w, unc, synd};
        block_sum_n_t0<3>(sums, red + 4);
        if (tid == 0) {
            const int sf = sums[2] > 0;
            acc[0] += (unsigned long long)sums[0];
            acc[1] += (unsigned long long)(sums[0] > 0);
            acc[2] += (unsigned long long)sums[1];
            acc[3] += 1ull;
            acc[4] += (unsigned long long)it;
            acc[5] += (unsigned long long)sf;
            if (sums[0] > 0 && a.hist) atomicAdd(&a.hist[sums[0] - 1], 1ull);
            if (a.frame_res) a.frame_res[b] = make_int4(sums[0], sums[1], sf, it);
            red[2] = (int)nxt;
        }
        __syncthreads();
        b = red[2];   // rewritten only after the next codeword's barriers
        if (tid == 0 && b < a.batch) nxt = gridDim.x + atomicAdd(ticket, 1u);
    }
    if (tid == 0 && acc[3] > 0) {
#pragma unroll
        for (int q = 0; q < 6; ++q) atomicAdd(&a.counts[q], acc[q]);
    }
}

LDPC_CHECK_TU(rows_es)

static size_t rows_es_lds(const DevGraph &g, const RowSched &rs, bool f64)
{
    const size_t fs = f64 ? 8 : 4;
    return (((size_t)g.N + 2 + (size_t)rs.e_pad + 64) * fs + 4 * kEsRedInts + 15) & ~(size_t)15;
}

// The instantiation for a schedule's shape (DC, CPT, RPT): the nine of rows.hip rows_fn; null: none is built.
template <typename F, int SRC>
static const void *rows_es_fn(const RowSched &rs)
{
#define LDPC_ES_CASE(DCV, CPTV, RPTV)                                       \
    if (rs.dc == DCV && rs.cpt == CPTV && rs.rpt == RPTV)                   \
        return (const void *)k_rows_es<F, SRC, DCV, CPTV, RPTV>;
    LDPC_ES_CASE(8, 2, 1)
    LDPC_ES_CASE(8, 4, 1)
    LDPC_ES_CASE(8, 4, 2)
    LDPC_ES_CASE(16, 2, 1)
    LDPC_ES_CASE(16, 4, 1)
    LDPC_ES_CASE(16, 4, 2)
    LDPC_ES_CASE(32, 2, 1)
    LDPC_ES_CASE(32, 4, 1)
    LDPC_ES_CASE(32, 4, 2)
#undef LDPC_ES_CASE
    return nullptr;
}

bool plan_rows_es(const PlanInput &in, LaunchPlan &p)
{
    if (!in.rs || in.rs->threads <= 0) return false;
    const RowSched &rs = *in.rs;
    const size_t lds = rows_es_lds(in.g, rs, in.f64);
    if (lds > kMaxLds) return false;
    const auto fn = [&](auto f, auto s) { return rows_es_fn<typename decltype(f)::type, decltype(s)::value>(rs); };
    const void *rep = for_f_src(in.f64, SRC_PHILOX, fn);   // reported figures: see kernels.hip plan_lds
    if (!rep) return false;
    p = LaunchPlan{};
    p.kernel = Kernel::rows_es;
    p.name = "rows_es";
    p.fn = for_f_src(in.f64, in.a.src, fn);
    p.threads = rs.threads;
    p.lds_bytes = (int)lds;
    p.cw_per_block = 1;
    p.rs = in.rs;
    p.blocks_per_cu = occupancy(rep, rs.threads, (int)lds);
    // Persistent grid of the resident blocks: what the CU holds of the kernel that launches.
    int per_cu = std::max(1, occupancy(p.fn, p.threads, p.lds_bytes));
    if (const int cap = opt(LDPC_OPT_ROWS_BPC))
        if (cap < per_cu) per_cu = cap;
    p.grid = std::min(per_cu * (in.num_cus > 0 ? in.num_cus : 1), in.a.batch);
    return true;
}

hipError_t launch_rows_es(const LaunchPlan &p, const DevGraph &g, const DecodeArgs &a, unsigned *ticket, hipStream_t s)
{
    if (a.batch <= 0) return hipSuccess;
    if (!ticket) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(ticket, 0, sizeof(unsigned), s);
    if (e != hipSuccess) return e;
    void *args[] = {(void *)&a, (void *)&g, (void *)p.rs, &ticket};
    return launch_fn(p, args, s);
}

}  // namespace ldpc
