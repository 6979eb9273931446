// ddbmp.hip -- CDNA4 (gfx950) kernels of the DD-BMP decoder: differential decoding
// with binary message passing (variant LDPC_DDBMP).
//
// Restates src/decodeDDBMP.cpp. Every message is one bit; the only floating-point
// state is one "memory" per edge, touched only by its own bit node:
//   front-end    yq = front_end(y) (quantize :434-443), r = yq > 0 ? +1 : -1, d = r (:174-185)
//   init         mem[i][k] = yq[i]; s2c[i][k] = sgn(mem[i][k]) always, so it is not stored (:301-310)
//   check nodes  par_j = prod_k s2c over row j; c2s[j][k] = par_j * s2c of that edge (:350-372)
//   bit nodes    sum = yq[i] + c2s_0 + c2s_1 + ... in nlist order; then, in the same order,
//                mem[i][k] += (sum - c2s_k); d[i] = sgn(yq[i]) + sum_k sgn(mem[i][k]) > 0 (:396-423)
//   stop         when every row's product of d is +1, before `it` is incremented (:203-204),
//                so a frame that stops inside iteration index `it` counts `it` iterations
// with sgn(x) = x >= 0 ? +1 : -1 (:426-431; a comparison, not the sign bit).
//
// What travels between threads is one flag byte per edge, kept in the slot of its check
// row (row j's edges at [j * stride, j * stride + deg)): bit 0 is set when sgn(mem) = -1,
// bit 1 when the edge's bit decides d = -1. The xor of a row's bytes is then both the row
// parity par_j (bit 0) and the stop rule's product of d (bit 1) in one pass, and the stop
// check of iteration `it` rides on the check phase of iteration `it + 1`; the check phase
// after the last iteration is the syndrome of the returned decisions. A bit reads the
// parity byte of each of its checks and forms c2s = par_j * sgn(own memory) itself.
// Edges beyond a bit's degree are skipped by predication: they add nothing, not +-0.
//
// Compiled with -ffp-contract=off: the additions keep the reference's order and
// rounding, so fp64 reproduces it bit for bit; fp32 is the same algorithm in float.
#include "ddbmp.h"
#include "frame.h"
#include "minsum_common.h"

#include <hip/hip_runtime.h>
#include <algorithm>

namespace ldpc {

template <typename F> __device__ __forceinline__ int dneg(F x) { return !(x >= F(0)); }   // sgn(x) == -1

// ---------------------------------------------------------------------
// Generic: one workgroup per codeword, every valid graph. State: mem[E] in column (nlist)
// order, yq[N], the edge flags ef[M * dcs] in row order, par[M], d[N]; in LDS or in a
// global slot per resident workgroup.
// ---------------------------------------------------------------------
template <typename F, int SRC>
__device__ __forceinline__ void ddbmp_codeword(const DecodeArgs &a, const DevGraph &g, int b, F *mem, F *yq,
                                               uint8_t *ef, uint8_t *par, int8_t *d, int *red, volatile int *fl)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    const int N = g.N, M = g.M, T = a.T;
    [[maybe_unused]] const uint32_t nef = (uint32_t)M * (uint32_t)g.dcs;   // LDPC_CHK bound
    const int8_t *cvec = frame_codeword<SRC>(a, b, N);
    // ---- channel + front-end (:174-185), initialisation (:301-310) ----
    int unc = 0;
    channel_bits<F, SRC, true>(a, b, N, cvec, a.y_out, [&](int v, F yv) {
        const F q = front_end<F>(yv, a);
        const int r = q > F(0) ? 1 : -1;
        const int cv = cvec ? cvec[v] : 1;
        unc += (r * cv < 0);
        yq[v] = q;
        d[v] = (int8_t)r;
        const uint8_t flags = (uint8_t)(dneg(q) | ((r < 0) << 1));
        const int e1 = g.col_ptr[v + 1];
        for (int e = g.col_ptr[v]; e < e1; ++e) {
            const uint32_t ref = g.col_refs[e];
            mem[e] = q;
            ef[LDPC_CHK((ref >> 6) * (uint32_t)g.dcs + (ref & 63u), nef, CHK_DDBMP_EDGE)] = flags;
        }
    });
    if (tid == 0) {
        fl[0] = 0;
        fl[1] = 0;
    }
    __syncthreads();

    int it = 0, cnt = 0, synd = 0;
    for (;;) {
        // ---- check nodes of iteration `it` (:350-372) and, in bit 1 of the same bytes, the
        // stop rule of iteration `it - 1` (:375-393; at it = 0 the syndrome of d = r) ----
        int fail = 0;
        for (int j = tid; j < M; j += nt) {
            const int deg = g.row_deg[j];
            const uint8_t *rf = ef + (size_t)j * g.dcs;
            unsigned x = 0;
            for (int k = 0; k < deg; ++k) x ^= rf[k];
            par[j] = (uint8_t)(x & 1u);
            fail |= (int)((x >> 1) & 1u);
        }
        if (fail) fl[it & 1] = 1;
        __syncthreads();
        const int f = fl[it & 1];   // uniform over the workgroup
        if (it > 0 && !f) {         // :203-204: stopped inside iteration index it - 1
            cnt = it - 1;
            synd = 0;
            break;
        }
        if (it == T) {
            cnt = T;
            synd = f != 0;
            break;
        }
        if (tid == 0) fl[(it + 1) & 1] = 0;   // nobody reads or sets it before the next barrier
        // ---- bit nodes (:396-423) ----
        for (int v = tid; v < N; v += nt) {
            const int e0 = g.col_ptr[v], e1 = g.col_ptr[v + 1];
            const F q = yq[v];
            F sum = q;
            for (int e = e0; e < e1; ++e) {
                const int cn = par[LDPC_CHK(g.col_refs[e] >> 6, (uint32_t)M, CHK_DDBMP_CHECK)] ^ dneg(mem[e]);
                sum += cn ? F(-1) : F(1);
            }
            int ds = dneg(q) ? -1 : 1;
            for (int e = e0; e < e1; ++e) {
                const F m0 = mem[e];
                const int cn = par[LDPC_CHK(g.col_refs[e] >> 6, (uint32_t)M, CHK_DDBMP_CHECK)] ^ dneg(m0);
                const F m = m0 + (sum - (cn ? F(-1) : F(1)));
                mem[e] = m;
                ds += dneg(m) ? -1 : 1;
            }
            const int dn = ds > 0 ? 0 : 1;
            d[v] = (int8_t)(dn ? -1 : 1);
            for (int e = e0; e < e1; ++e) {
                const uint32_t ref = g.col_refs[e];
                ef[LDPC_CHK((ref >> 6) * (uint32_t)g.dcs + (ref & 63u), nef, CHK_DDBMP_EDGE)] =
                    (uint8_t)(dneg(mem[e]) | (dn << 1));
            }
        }
        __syncthreads();
        ++it;
    }

    // ---- error weight (:212, :322-333), accounting ----
    int wgt = 0;
    for (int v = tid; v < N; v += nt) {
        const int dv = d[v];
        const int cv = cvec ? cvec[v] : 1;
        wgt += (dv != cv);
        if (a.d_out) a.d_out[(size_t)b * N + v] = (int8_t)dv;
    }
    int sums[2] = {wgt, unc};
    block_sum_n_t0<2>(sums, red);
    if (tid == 0)   // totalIterations += it (:230)
        frame_account(a.counts, a.hist, a.frame_res, b, sums[0], sums[1], synd, cnt, cnt);
    __syncthreads();
}

// Byte offsets of one codeword's state: mem[E] | yq[N] | ef[M * dcs] | par[M] | d[N].
struct DdbmpLayout {
    size_t yq, ef, par, d, total;
};
static DdbmpLayout ddbmp_layout(int N, int M, int E, int dcs, size_t fsz)
{
    DdbmpLayout L;
    auto al = [](size_t x) { return (x + 15) & ~(size_t)15; };
    L.yq = al(fsz * (size_t)E);
    L.ef = L.yq + al(fsz * (size_t)N);
    L.par = L.ef + al((size_t)M * (size_t)dcs);
    L.d = L.par + al((size_t)M);
    L.total = L.d + al((size_t)N);
    return L;
}

template <typename F, int SRC>
__global__ __launch_bounds__(256) void k_ddbmp_lds(DecodeArgs a, DevGraph g, DdbmpLayout L)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int red[16 * 2];
    __shared__ int fl[2];
    ddbmp_codeword<F, SRC>(a, g, blockIdx.x, reinterpret_cast<F *>(smem), reinterpret_cast<F *>(smem + L.yq),
                           smem + L.ef, smem + L.par, reinterpret_cast<int8_t *>(smem + L.d), red, fl);
}

template <typename F, int SRC>
__global__ __launch_bounds__(1024) void k_ddbmp_global(DecodeArgs a, DevGraph g, DdbmpLayout L, unsigned char *scratch,
                                                       size_t slot_bytes)
{
    __shared__ int red[16 * 2];
    __shared__ int fl[2];
    unsigned char *base = scratch + slot_bytes * blockIdx.x;
    for (int b = blockIdx.x; b < a.batch; b += gridDim.x)
        ddbmp_codeword<F, SRC>(a, g, b, reinterpret_cast<F *>(base), reinterpret_cast<F *>(base + L.yq), base + L.ef,
                               base + L.par, reinterpret_cast<int8_t *>(base + L.d), red, fl);
}

// ---------------------------------------------------------------------
// ddbmp_rows: codes with N <= 4 * NT bits, M <= 2 * NT rows, row degree <= 8 and column
// degree <= DVM. Same arithmetic, in the same order, as ddbmp_codeword; what differs is
// where the state lives:
//  * thread t owns the Philox group of bits 4t..4t+3 and rows t and t + NT;
//  * the memories, yq and d of the thread's bits stay in registers (4 * DVM values of F),
//    and so does the flag slot of every edge (16 bits each, two per register), loaded once
//    per workgroup; a check's parity byte is at slot >> 3;
//  * LDS holds the flag bytes, 8 per row (a row's check phase is one 8-byte read and an
//    xor fold; the bytes past its degree stay 0), the parity byte of every row and the
//    double-buffered stop flag, so an iteration costs two barriers;
//  * the parity reads of a bit slot are issued together, the first four always and the
//    rest behind one branch on the wave's largest degree; each lane's own degree
//    predicates the arithmetic, so edges it does not have change nothing;
//  * the workgroup is persistent and takes codewords by ticket (early stop makes them unequal).
// ---------------------------------------------------------------------
struct DdbmpRowsLayout {
    int paroff, floff, total;
};
static DdbmpRowsLayout ddbmp_rows_layout(int nt)
{
    DdbmpRowsLayout L;
    L.paroff = 2 * nt * 8;            // flag bytes: 8 per row, 2 * nt rows
    L.floff = L.paroff + 2 * nt;      // parity bytes
    L.total = L.floff + 16;           // fl[2] (+ pad)
    return L;
}

template <typename F, int SRC, int DVM, int NT>
__global__ __launch_bounds__(NT) void k_ddbmp_rows(DecodeArgs a, DevGraph g, unsigned *ticket, int paroff, int floff)
{
    constexpr int DC = 8, BPT = 4, RPT = 2;
    constexpr int K0 = DVM < 4 ? DVM : 4;
    [[maybe_unused]] constexpr uint32_t NEF = (uint32_t)RPT * NT * DC, NPAR = (uint32_t)RPT * NT;   // LDPC_CHK bounds
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int red[16 * 2 + 1];                    // block sums; [32]: the next codeword
    uint8_t *ef = smem;                                // edge flags, row j's at [8j, 8j + 8)
    uint8_t *par = smem + paroff;                      // row parities
    volatile int *fl = reinterpret_cast<int *>(smem + floff);
    const int tid = threadIdx.x;
    const int N = g.N, T = a.T;
    const int v0 = BPT * tid;             // the thread's first bit
    const bool own = v0 < N;
    // ---- the bit side of the graph, into registers (once per workgroup) ----
    uint32_t es[BPT][DVM / 2];   // flag slot of edge k of bit q: 8 * check + position in its row
    int deg[BPT], wdeg[BPT];     // the bit's degree; the wave's largest (uniform)
#pragma unroll
    for (int q = 0; q < BPT; ++q) {
        const int i = v0 + q;
        int e0 = 0;
        deg[q] = 0;
        if (i < N) {
            e0 = g.col_ptr[i];
            deg[q] = g.col_ptr[i + 1] - e0;
        }
#pragma unroll
        for (int k = 0; k < DVM; k += 2) {
            uint32_t s0 = 0, s1 = 0;
            if (k < deg[q]) {
                const uint32_t ref = g.col_refs[e0 + k];
                s0 = (ref >> 6) * DC + (ref & 63u);
            }
            if (k + 1 < deg[q]) {
                const uint32_t ref = g.col_refs[e0 + k + 1];
                s1 = (ref >> 6) * DC + (ref & 63u);
            }
            es[q][k / 2] = s0 | (s1 << 16);
        }
        int m = deg[q];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o, 64));
        wdeg[q] = __builtin_amdgcn_readfirstlane(m);
    }
    reinterpret_cast<uint4 *>(ef)[tid] = make_uint4(0u, 0u, 0u, 0u);   // 16 bytes each: all 2 * NT rows
    __syncthreads();
    auto slot = [&](int q, int k) -> uint32_t { return (es[q][k / 2] >> (16 * (k & 1))) & 0xffffu; };
    // the flag bytes of bit q: nm bit k = sgn(mem[q][k]) is -1; dn = d is -1
    auto put = [&](int q, uint32_t nm, int dn) {
#pragma unroll
        for (int k = 0; k < K0; ++k)
            if (k < deg[q]) ef[LDPC_CHK(slot(q, k), NEF, CHK_DDBMP_EDGE)] = (uint8_t)(((nm >> k) & 1u) | (uint32_t)(dn << 1));
        if (DVM > K0 && wdeg[q] > K0) {
#pragma unroll
            for (int k = K0; k < DVM; ++k)
                if (k < deg[q]) ef[LDPC_CHK(slot(q, k), NEF, CHK_DDBMP_EDGE)] = (uint8_t)(((nm >> k) & 1u) | (uint32_t)(dn << 1));
        }
    };

    // Codewords: blockIdx.x first, then tickets; thread 0 draws the next ticket while the
    // current codeword decodes.
    unsigned nxt = 0;
    if (tid == 0) nxt = gridDim.x + atomicAdd(ticket, 1u);
    for (int b = blockIdx.x; b < a.batch;) {
        const int8_t *cvec = frame_codeword<SRC>(a, b, N);
        // ---- channel + front-end (:174-185), initialisation (:301-310), as ddbmp_codeword ----
        F yq[BPT], mem[BPT][DVM];
        int d[BPT];
        int unc = 0;
#pragma unroll
        for (int q = 0; q < BPT; ++q) {
            yq[q] = F(0);
            d[q] = 1;
        }
        if (own) {
            F yv[BPT];
            channel_group<F, SRC, true>(a, b, tid, N, cvec, a.y_out, yv);
#pragma unroll
            for (int q = 0; q < BPT; ++q) {
                const int v = v0 + q;
                if (v < N) {
                    yq[q] = front_end<F>(yv[q], a);
                    d[q] = yq[q] > F(0) ? 1 : -1;
                    const int cv = cvec ? cvec[v] : 1;
                    unc += (d[q] * cv < 0);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < BPT; ++q) {
#pragma unroll
            for (int k = 0; k < DVM; ++k) mem[q][k] = yq[q];
            put(q, dneg(yq[q]) ? 0xffffu : 0u, d[q] < 0);
        }
        if (tid == 0) {
            fl[0] = 0;
            fl[1] = 0;
        }
        __syncthreads();

        int it = 0, cnt = 0, synd = 0;
        for (;;) {
            // the packed 16-bit slots are opaque per iteration: otherwise the compiler
            // hoists the unpacked indices out of the loop and spills them
#pragma unroll
            for (int q = 0; q < BPT; ++q)
#pragma unroll
                for (int k = 0; k < DVM / 2; ++k) asm volatile("" : "+v"(es[q][k]));
            // ---- check nodes of iteration `it` (:350-372); bit 1: the stop rule of it - 1 ----
            int fail = 0;
#pragma unroll
            for (int r = 0; r < RPT; ++r) {
                const uint32_t j = (uint32_t)tid + r * NT;
                const uint2 w = *reinterpret_cast<const uint2 *>(ef + j * DC);
                uint32_t x = w.x ^ w.y;
                x ^= x >> 16;
                x ^= x >> 8;
                par[j] = (uint8_t)(x & 1u);
                fail |= (int)((x >> 1) & 1u);
            }
            if (fail) fl[it & 1] = 1;
            __syncthreads();
            const int f = fl[it & 1];   // uniform over the workgroup
            if (it > 0 && !f) {         // :203-204: stopped inside iteration index it - 1
                cnt = it - 1;
                synd = 0;
                break;
            }
            if (it == T) {
                cnt = T;
                synd = f != 0;
                break;
            }
            if (tid == 0) fl[(it + 1) & 1] = 0;   // nobody reads or sets it before the next barrier
            // ---- bit nodes (:396-423) ----
#pragma unroll
            for (int q = 0; q < BPT; ++q) {
                const bool more = DVM > K0 && wdeg[q] > K0;
                // the parities of the slot's checks, read together; cm bit k: c2s_k is -1
                uint32_t cm = 0;
#pragma unroll
                for (int k = 0; k < K0; ++k)
                    cm |= (uint32_t)par[LDPC_CHK(slot(q, k) >> 3, NPAR, CHK_DDBMP_CHECK)] << k;
                if (more) {
#pragma unroll
                    for (int k = K0; k < DVM; ++k)
                        cm |= (uint32_t)par[LDPC_CHK(slot(q, k) >> 3, NPAR, CHK_DDBMP_CHECK)] << k;
                }
#pragma unroll
                for (int k = 0; k < DVM; ++k) cm ^= (uint32_t)dneg(mem[q][k]) << k;
                // sum = yq + c2s in nlist order (:400-408)
                F sum = yq[q];
#pragma unroll
                for (int k = 0; k < K0; ++k) {
                    const F s = sum + (((cm >> k) & 1u) ? F(-1) : F(1));
                    sum = k < deg[q] ? s : sum;
                }
                if (more) {
#pragma unroll
                    for (int k = K0; k < DVM; ++k) {
                        const F s = sum + (((cm >> k) & 1u) ? F(-1) : F(1));
                        sum = k < deg[q] ? s : sum;
                    }
                }
                // mem += sum - c2s, the new signs, d (:409-421)
                uint32_t nm = 0;
                int ds = dneg(yq[q]) ? -1 : 1;
                auto upd = [&](int k) {
                    const F m = mem[q][k] + (sum - (((cm >> k) & 1u) ? F(-1) : F(1)));
                    const bool has = k < deg[q];
                    mem[q][k] = has ? m : mem[q][k];
                    const int ng = dneg(m);
                    nm |= (uint32_t)(has && ng) << k;
                    ds += has ? (ng ? -1 : 1) : 0;
                };
#pragma unroll
                for (int k = 0; k < K0; ++k) upd(k);
                if (more) {
#pragma unroll
                    for (int k = K0; k < DVM; ++k) upd(k);
                }
                d[q] = ds > 0 ? 1 : -1;
                put(q, nm, d[q] < 0);
            }
            __syncthreads();
            ++it;
        }

        // ---- error weight (:212, :322-333), accounting ----
        int wgt = 0;
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
        int sums[2] = {wgt, unc};
        block_sum_n_t0<2>(sums, red);
        if (tid == 0) {
            frame_account(a.counts, a.hist, a.frame_res, b, sums[0], sums[1], synd, cnt, cnt);
            red[32] = (int)nxt;
        }
        __syncthreads();
        b = red[32];   // rewritten only after the next codeword's barriers
        if (tid == 0 && b < a.batch) nxt = gridDim.x + atomicAdd(ticket, 1u);
    }
}

LDPC_CHECK_TU(ddbmp)

static bool ddbmp_rows_fits(const DevGraph &g, int maxdv)
{
    if (opt(LDPC_OPT_DDBMP_KERNEL) == 1) return false;
    if (g.N < 1 || g.N > 4 * 1024 || g.M > 2 * 1024 || g.dcs > 8 || maxdv > 12) return false;
    // the 12-edge instance holds 48 memories per thread: 512-thread workgroups only
    return maxdv <= 4 || (g.N <= 4 * 512 && g.M <= 2 * 512);
}

template <typename F, int SRC> static const void *ddbmp_fn(Kernel k, int threads, int dvm)
{
    if (k == Kernel::ddbmp_lds) return (const void *)k_ddbmp_lds<F, SRC>;
    if (k == Kernel::ddbmp_global) return (const void *)k_ddbmp_global<F, SRC>;
    if (dvm == 12) return (const void *)k_ddbmp_rows<F, SRC, 12, 512>;
    return threads == 512 ? (const void *)k_ddbmp_rows<F, SRC, 4, 512> : (const void *)k_ddbmp_rows<F, SRC, 4, 1024>;
}

void plan_ddbmp(const PlanInput &in, LaunchPlan &p)
{
    const DevGraph &g = in.g;
    p = LaunchPlan{};
    const int dvm = in.maxdv <= 4 ? 4 : 12;
    if (ddbmp_rows_fits(g, in.maxdv)) {
        p.kernel = Kernel::ddbmp_rows;
        p.name = "ddbmp_rows";
        p.threads = g.N <= 4 * 512 && g.M <= 2 * 512 ? 512 : 1024;
        p.lds_bytes = ddbmp_rows_layout(p.threads).total;
    } else {
        const DdbmpLayout L = ddbmp_layout(g.N, g.M, in.E, g.dcs, in.f64 ? 8 : 4);
        if (L.total + 256 <= kMaxLds) {   // + the static block-sum and flag words
            p.kernel = Kernel::ddbmp_lds;
            p.name = "ddbmp_lds";
            p.threads = 256;
            p.lds_bytes = (int)L.total;
        } else {
            p.kernel = Kernel::ddbmp_global;
            p.name = "ddbmp_global";
            p.threads = 1024;
            p.scratch_per_block = (L.total + 255) & ~(size_t)255;
        }
    }
    p.fn = for_f_src(in.f64, in.a.src, [&](auto f, auto s) {
        return ddbmp_fn<typename decltype(f)::type, decltype(s)::value>(p.kernel, p.threads, dvm);
    });
    if (p.kernel == Kernel::ddbmp_rows) {   // persistent: what the CU holds
        p.blocks_per_cu = std::max(1, occupancy(p.fn, p.threads, p.lds_bytes));
        p.grid = std::min(p.blocks_per_cu * (in.num_cus > 0 ? in.num_cus : 1), in.a.batch);
    } else if (p.kernel == Kernel::ddbmp_lds) {
        p.grid = in.a.batch;
    } else {
        p.grid = std::min(in.a.batch, 2 * in.num_cus);
        p.scratch_bytes = p.scratch_per_block * (size_t)p.grid;
    }
}

hipError_t launch_ddbmp(const LaunchPlan &p, const DevGraph &g, const DecodeArgs &a, bool f64, int E, void *gscratch,
                        unsigned *ticket, hipStream_t s)
{
    if (a.batch <= 0) return hipSuccess;
    if (p.kernel == Kernel::ddbmp_rows) {
        if (!ticket) return hipErrorInvalidValue;
        const hipError_t e = hipMemsetAsync(ticket, 0, sizeof(unsigned), s);
        if (e != hipSuccess) return e;
        DdbmpRowsLayout L = ddbmp_rows_layout(p.threads);
        void *args[] = {(void *)&a, (void *)&g, &ticket, &L.paroff, &L.floff};
        return launch_fn(p, args, s);
    }
    DdbmpLayout L = ddbmp_layout(g.N, g.M, E, g.dcs, f64 ? 8 : 4);
    unsigned char *gs = (unsigned char *)gscratch;
    size_t sb = p.scratch_per_block;
    if (p.kernel == Kernel::ddbmp_global && !gs) return hipErrorInvalidValue;
    void *args[] = {(void *)&a, (void *)&g, &L, &gs, &sb};   // ddbmp_lds takes the first three
    return launch_fn(p, args, s);
}

}  // namespace ldpc
