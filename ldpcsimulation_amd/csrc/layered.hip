// layered.hip -- layered (row-serial) min-sum: k_decode_layered_lds / _global, plan and launch.
#include "minsum_kernels.h"
#include "frame.h"

namespace ldpc {

// =====================================================================
// Layered (row-serial) min-sum -- SURVEY §8(f) row 2, BASELINE config 3.
// The reference only floods (src/decodeMinSum.cpp:247-263); this is the
// row-serial schedule of the same check-node rule (:410-450, :494-515),
// restated in oracle/ldpc_oracle.c (orc_decode_layered_*):
//   x_k = app[b_k] - c2v_old_k;  c2v_k = rule(x);  app[b_k] = x_k + c2v_k
// row by row in the layered order. Rows that share no bit commute exactly, so
// each layer (LayerSched: bit-disjoint sets of whole row chains; DVB-S2
// N=64800: 17 layers of 275-3 044 rows) is updated by all its rows at once,
// one thread per row, with a workgroup barrier between layers. One workgroup
// per codeword (persistent over the batch). State:
//   app[NP + 1]            posteriors in layered position order (app[NP] = +inf pad)
//   m12[M_pad], meta[M_pad] the packed check state as in k_decode_flood (meta:
//                          argmin | signs << 5, 16 bits for rows of degree <= 8)
// -- in LDS when it fits (k_decode_layered_lds) or in a per-workgroup global
// slot (k_decode_layered_global: DVB-S2's 583 KB), where in fp64 positions [0, P) --
// the highest-degree bits, LayerSchedule::pos_of_bit -- stay in LDS (LayApp).
// No yq and no E-sized message array: a row's old messages are rebuilt from
// its packed state.
// =====================================================================
// Raw buffer access (32-bit byte offsets from a descriptor). The global half
// of a split posterior array goes through these: a distinct instruction, so
// the compiler cannot fold "LDS or global" into one flat load.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(void *p, uint32_t bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(p, 0, (int)bytes, 0x00020000);
}
template <typename F>
__device__ __forceinline__ F buf_ld(__amdgpu_buffer_rsrc_t r, uint32_t off);
template <>
__device__ __forceinline__ float buf_ld<float>(__amdgpu_buffer_rsrc_t r, uint32_t off)
{
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, (int)off, 0, 0));
}
template <>
__device__ __forceinline__ double buf_ld<double>(__amdgpu_buffer_rsrc_t r, uint32_t off)
{
    typedef unsigned u2 __attribute__((ext_vector_type(2)));
    const u2 v = __builtin_amdgcn_raw_buffer_load_b64(r, (int)off, 0, 0);
    return __hiloint2double((int)v.y, (int)v.x);
}
__device__ __forceinline__ void buf_st(__amdgpu_buffer_rsrc_t r, uint32_t off, float x)
{
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(x), r, (int)off, 0, 0);
}
__device__ __forceinline__ void buf_st(__amdgpu_buffer_rsrc_t r, uint32_t off, double x)
{
    typedef unsigned u2 __attribute__((ext_vector_type(2)));
    u2 v;
    v.x = (unsigned)__double2loint(x);
    v.y = (unsigned)__double2hiint(x);
    __builtin_amdgcn_raw_buffer_store_b64(v, r, (int)off, 0, 0);
}

// SPLIT: branch-free -- every access issues both the LDS and the buffer
// instruction; the side that does not hold p gets LDS slot P (a dummy) or an
// offset past the descriptor's range (the buffer unit drops it: no traffic).
template <typename F, bool SPLIT>
struct LayApp {
    F *lo;                       // positions [0, P): LDS (all of them unless SPLIT); SPLIT: lo[P] = dummy
    __amdgpu_buffer_rsrc_t hi;   // positions [P, NP]: the global slot, at p - P (SPLIT only)
    int P;
    static constexpr uint32_t kOut = 0x80000000u;   // beyond any slot
    __device__ __forceinline__ F ld(int p) const
    {
        if (!SPLIT) return lo[p];
        const bool in = p < P;
        const F a = lo[in ? p : P];
        const F b = buf_ld<F>(hi, in ? kOut : (uint32_t)(p - P) * (uint32_t)sizeof(F));
        return in ? a : b;
    }
    __device__ __forceinline__ void st(int p, F x) const
    {
        if (!SPLIT) {
            lo[p] = x;
            return;
        }
        const bool in = p < P;
        lo[in ? p : P] = x;
        buf_st(hi, in ? kOut : (uint32_t)(p - P) * (uint32_t)sizeof(F), x);
    }
};

template <typename F, int SRC, bool SPLIT>
__device__ __forceinline__ int channel_to_storage(const DecodeArgs &a, const DevGraph &g, const LayerSched &ls,
                                                  int b, const int8_t *cvec, const LayApp<F, SPLIT> &app,
                                                  [[maybe_unused]] int np1)
{
    int unc = 0;
    channel_bits<F, SRC, false, true>(a, b, g.N, cvec, a.y_out, [&](int v, F yv) {
        const F q = front_end<F>(yv, a);
        app.st(LDPC_CHK(ls.pos_of_bit[v], np1, CHK_FLOOD_APP), q);
        const int cv = cvec ? cvec[v] : 1;
        unc += ((q > F(0) ? 1 : -1) * cv < 0);
    });
    return unc;
}

// One check row of the layered schedule: xs[k] = app of its bits on entry,
// the updated posteriors x_k + c2v_k on exit; returns the new packed meta
// (argmin | sign bits << 5) and the new minima in nw. The check-node rule is
// the reference's (checkNodeUpdates :410-450, applyNormalization :494-499,
// applyOffset :503-515), as in k_decode_flood.
template <typename F, int DC>
__device__ __forceinline__ uint32_t layered_row(const DecodeArgs &a, int deg, typename F2T<F>::T old, uint32_t om,
                                                F (&xs)[DC], F alpha, F delta, typename F2T<F>::T &nw)
{
    const int oidx = (int)(om & 31u);
    F mn1 = dinf<F>(), mn2 = dinf<F>();
    int amin = 31;
    uint32_t sg = 0;
#pragma unroll
    for (int k = 0; k < DC; ++k) {
        if (k < deg) {
            F cold = (k == oidx) ? old.y : old.x;
            if ((om >> (5 + k)) & 1u) cold = -cold;
            xs[k] = xs[k] - cold;                           // v2c (:469)
            sg |= (uint32_t)(!(xs[k] >= F(0))) << k;        // sgn(v2c) < 0 (:518-523)
            const F ax = dabs(xs[k]);
            if (ax <= mn1) { mn2 = mn1; mn1 = ax; amin = k; }   // :428-433
            else if (ax < mn2) { mn2 = ax; }                    // :434-437
        }
    }
    const uint32_t degmask = (1u << deg) - 1u;
    uint32_t eff = (__popc(sg) & 1) ? (sg ^ degmask) : sg;   // prod * sgn(v2c_k)
    F M1 = mn1, M2 = mn2;
    if (a.variant == V_NMS) {
        M1 = nms_div<F>(mn1, alpha, a);                   // :498
        M2 = nms_div<F>(mn2, alpha, a);
    } else if (a.variant == V_OMS) {
        const F t1 = mn1 - delta, t2 = mn2 - delta;       // :509
        const bool p1 = t1 > F(0), p2 = t2 > F(0);
        M1 = p1 ? t1 : F(0);
        M2 = p2 ? t2 : F(0);
        // sgn(c2v) of :511 maps -0.0 to +1; a zeroed message is +0 (:513)
        const uint32_t abit = (amin < 31) ? (1u << amin) : 0u;
        if (!p1 || mn1 == F(0)) eff &= abit;
        if (!p2 || mn2 == F(0)) eff &= ~abit;
    }
    nw.x = M1;
    nw.y = M2;
#pragma unroll
    for (int k = 0; k < DC; ++k) {
        if (k < deg) {
            const F mag = (k == amin) ? M2 : M1;
            xs[k] = xs[k] + (((eff >> k) & 1u) ? -mag : mag);
        }
    }
    return (uint32_t)amin | (eff << 5);
}

// Layered check state: argmin (5 bits) | signs << 5 -- 16 bits for the DC = 8 instantiation
// (fs.dc <= 8, launch_layered_dc), 32 above (2 B less state per row: DVB-S2
// 65 KB per codeword, more resident codewords inside the Infinity Cache).
template <int DC> using LayMeta = typename std::conditional<(DC <= 8), uint16_t, uint32_t>::type;
__host__ __device__ inline size_t layered_meta_bytes(const FloodSched &fs) { return fs.dc <= 8 ? 2 : 4; }

// Diagnostic builds (-DLDPC_STAMPS, `make variant`; scripts/lay_stamp_run.sh): per wave,
// s_memtime cycles of the layered kernel's phases, each closed by a wait on its memory
// operations (0 schedule loads, 1 posterior gathers + check state, 2 check rule, 6 scatter
// issue, 3 scatter drain, 4 layer barrier, 5 channel, init, decisions and accounting;
// 7 counts the passes), to a.stamps[(block*16+wave)*8 + k].
struct LayStamps {
#ifdef LDPC_STAMPS
    unsigned long long t0 = __builtin_amdgcn_s_memtime(), acc[8] = {};
    __device__ __forceinline__ void mark(int k, bool drain = false)
    {
        if (drain) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        const unsigned long long t = __builtin_amdgcn_s_memtime();
        acc[k] += t - t0;
        t0 = t;
    }
    __device__ __forceinline__ void pass() { acc[7] += 1; }
    __device__ __forceinline__ void out(const DecodeArgs &a) const
    {
        if (a.stamps && (threadIdx.x & 63) == 0 && blockIdx.x < 256)
            for (int k = 0; k < 8; ++k) a.stamps[(blockIdx.x * 16 + (threadIdx.x >> 6)) * 8 + k] = acc[k];
    }
#else
    __device__ __forceinline__ void mark(int, bool = false) {}
    __device__ __forceinline__ void pass() {}
    __device__ __forceinline__ void out(const DecodeArgs &) const {}
#endif
};

template <typename F, int SRC, int DC, int R, bool SPLIT>
__device__ __forceinline__ void decode_layered_cw(const DecodeArgs &a, const DevGraph &g, const FloodSched &fs,
                                                  const LayerSched &ls, int b, const LayApp<F, SPLIT> &app,
                                                  typename F2T<F>::T *m12, LayMeta<DC> *meta, int *red,
                                                  unsigned long long *acc, LayStamps &st)
{
    using F2 = typename F2T<F>::T;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int N = g.N, NP = fs.ngroups * 64, MP = ls.M_pad;
    const F alpha = (F)a.alpha, delta = (F)a.delta;
    const int8_t *cvec = frame_codeword<SRC>(a, b, N);
    // ---- channel + front-end (:214-238): app = yq in storage order ----
    const int unc = channel_to_storage<F, SRC, SPLIT>(a, g, ls, b, cvec, app, NP + 1);
    for (int i = tid; i < MP; i += nt) {   // c2v_old = +0 (:364-370)
        F2 z;
        z.x = F(0);
        z.y = F(0);
        m12[i] = z;
        meta[i] = 0;
    }
    __syncthreads();
    st.mark(5);

    for (int it = 0; it < a.T; ++it) {
        for (int L = 0; L < ls.nlayers; ++L) {
            const int r1 = ls.lptr[L + 1];
            // R rows per thread per pass: every gather of the pass is issued
            // before the first row is computed (one memory round trip per pass)
            for (int i0 = ls.lptr[L] + tid; i0 < r1; i0 += nt * R) {
                int deg[R], sp[R][DC];
                F xs[R][DC];
                F2 old[R];
                uint32_t om[R];
#pragma unroll
                for (int r = 0; r < R; ++r) deg[r] = (i0 + r * nt < r1) ? ls.rdeg[i0 + r * nt] : 0;
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int k = 0; k < DC; ++k)
                        sp[r][k] = k < deg[r] ? LDPC_CHK(ls.sp[(size_t)k * MP + i0 + r * nt], NP + 1, CHK_FLOOD_APP) : NP;
                st.pass();
                st.mark(0, true);
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int k = 0; k < DC; ++k) xs[r][k] = app.ld(sp[r][k]);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (deg[r]) {
                        old[r] = m12[i0 + r * nt];
                        om[r] = meta[i0 + r * nt];
                    }
                }
                st.mark(1, true);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (deg[r]) {
                        F2 nw;
                        const uint32_t nm = layered_row<F, DC>(a, deg[r], old[r], om[r], xs[r], alpha, delta, nw);
                        st.mark(2);
                        m12[i0 + r * nt] = nw;
                        meta[i0 + r * nt] = (LayMeta<DC>)nm;
#pragma unroll
                        for (int k = 0; k < DC; ++k)
                            if (k < deg[r]) app.st(sp[r][k], xs[r][k]);   // posterior update
                    }
                }
                st.mark(6);
                st.mark(3, true);
            }
            __syncthreads();
            st.mark(4);
        }
    }

    // ---- decisions, error weight (:270, :382-393), syndrome ----
    int w = 0, synd = 0;
    for (int v = tid; v < N; v += nt) {
        const int d = app.ld(LDPC_CHK(ls.pos_of_bit[v], NP + 1, CHK_FLOOD_APP)) > F(0) ? 1 : -1;   // :471-474
        const int cv = cvec ? cvec[v] : 1;
        w += (d != cv);
        if (a.d_out) a.d_out[(size_t)b * N + v] = (int8_t)d;
    }
    for (int i = tid; i < MP; i += nt) {
        const int deg = ls.rdeg[i];
        int par = 0;
        for (int k = 0; k < deg; ++k) par ^= (app.ld(LDPC_CHK(ls.sp[(size_t)k * MP + i], NP + 1, CHK_FLOOD_APP)) > F(0)) ? 0 : 1;
        synd |= par;
    }
    int sums[3] = {w, unc, synd};
    block_sum_n_t0<3>(sums, red);
    if (tid == 0) frame_account_acc(acc, a.hist, a.frame_res, b, sums[0], sums[1], sums[2] > 0);
    __syncthreads();
    st.mark(5);
}

// LDS offsets of the layered state: app[NP + 1] | pad | m12[M_pad] | meta[M_pad].
__host__ __device__ inline size_t layered_m12_off(const FloodSched &fs, size_t fsz)
{
    return (((size_t)fs.ngroups * 64 + 1) * fsz + 15) & ~(size_t)15;
}
__host__ __device__ inline size_t layered_state_bytes(const FloodSched &fs, const LayerSched &ls, size_t fsz)
{
    return (layered_m12_off(fs, fsz) + (size_t)ls.M_pad * (2 * fsz + layered_meta_bytes(fs)) + 255) & ~(size_t)255;
}

template <typename F, int SRC, int DC, int R>
__global__ __launch_bounds__(512) void k_decode_layered_lds(DecodeArgs a, DevGraph g, FloodSched fs, LayerSched ls)
{
    using F2 = typename F2T<F>::T;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int red[16 * 4];
    __shared__ unsigned long long acc[6];
    F *app = reinterpret_cast<F *>(smem);
    F2 *m12 = reinterpret_cast<F2 *>(smem + layered_m12_off(fs, sizeof(F)));
    LayMeta<DC> *meta = reinterpret_cast<LayMeta<DC> *>(m12 + ls.M_pad);
    if (threadIdx.x == 0) {
        app[fs.ngroups * 64] = dinf<F>();
#pragma unroll
        for (int q = 0; q < 6; ++q) acc[q] = 0;
    }
    const LayApp<F, false> la{app, buf_rsrc(app, 0), 0};
    LayStamps st;
    for (int b = blockIdx.x; b < a.batch; b += gridDim.x)
        decode_layered_cw<F, SRC, DC, R, false>(a, g, fs, ls, b, la, m12, meta, red, acc, st);
    st.out(a);
    if (threadIdx.x == 0) frame_flush(a.counts, acc, a.T);
}
// State in a global slot; SPLIT (fp64): except the posteriors of layered
// positions [0, P) (dynamic LDS, (P + 1) * sizeof(F) bytes) -- DVB-S2 keeps
// 19 455 of its 64 800 bits there, every degree-8 bit and a third of the
// degree-3 ones, 54 % of the edge gathers and scatters.
template <typename F, int SRC, int DC, int R, bool SPLIT, int NT = 512>
__global__ __launch_bounds__(NT) void k_decode_layered_global(DecodeArgs a, DevGraph g, FloodSched fs, LayerSched ls,
                                                              unsigned char *scratch, size_t slot_bytes, int P)
{
    using F2 = typename F2T<F>::T;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int red[16 * 4];
    __shared__ unsigned long long acc[6];
    unsigned char *base = scratch + slot_bytes * blockIdx.x;
    F *app = reinterpret_cast<F *>(base);
    F2 *m12 = reinterpret_cast<F2 *>(base + layered_m12_off(fs, sizeof(F)));
    LayMeta<DC> *meta = reinterpret_cast<LayMeta<DC> *>(m12 + ls.M_pad);
    const LayApp<F, SPLIT> la{SPLIT ? reinterpret_cast<F *>(smem) : app,
                              buf_rsrc(app, (uint32_t)layered_m12_off(fs, sizeof(F))), P};
    if (threadIdx.x == 0) {
        la.st(fs.ngroups * 64, dinf<F>());
#pragma unroll
        for (int q = 0; q < 6; ++q) acc[q] = 0;
    }
    LayStamps st;
    for (int b = blockIdx.x; b < a.batch; b += gridDim.x)
        decode_layered_cw<F, SRC, DC, R, SPLIT>(a, g, fs, ls, b, la, m12, meta, red, acc, st);
    st.out(a);
    if (threadIdx.x == 0) frame_flush(a.counts, acc, a.T);
}

LDPC_CHECK_TU(layered)

// ---------------------------------------------------------------- layered
// Layered positions (of np) the global kernel keeps in LDS: as many as fit
// beside the static LDS (LDPC_OPT_LAYERED_LDS_POS = P + 1 caps it at P; 1 = all in the slot).
static int layered_lds_positions(int np, size_t fsz)
{
    long P = (long)((kMaxLds - 4096) / fsz) - 1;
    if (const int v = opt(LDPC_OPT_LAYERED_LDS_POS)) P = std::min(P, (long)(v - 1));
    return (int)std::min(P, (long)np);
}

// Rows per thread per pass: the global kernel batches R rows' gathers
// (latency of the L2/Infinity Cache), the LDS kernel does one row at a time.
// fp64: 2 (DVB-S2 1 530 vs 1 470 Mbit/s at 1 and 1 425 at 3); LDPC_OPT_LAYERED_ROWS64 = 1 for A/B.
static int layered_r64() { return opt(LDPC_OPT_LAYERED_ROWS64) == 1 ? 1 : 2; }
// Threads of the global layered kernel: 1024 (4 waves per SIMD at <= 128 VGPRs,
// R = 2 rows per thread per pass in fp32, 1 in fp64) -- DVB-S2 T=50: fp32 59.4 ->
// 42.7 ms, fp64 87.4 -> 74.2 ms per 2,048 codewords against 512 threads (2 waves
// per SIMD at ~256 VGPRs, R = 4 / 2: the same rows in flight per pass, half the
// waves to hide the L2 / Infinity Cache latency); LDPC_OPT_LAYERED_THREADS = 512
// keeps the latter.
static int layered_nt() { return opt(LDPC_OPT_LAYERED_THREADS) == 512 ? 512 : 1024; }
static int layered_rows_per_pass(bool global, bool f64)
{
    if (!global) return 1;
    if (layered_nt() == 1024) return f64 ? 1 : 2;
    return f64 ? layered_r64() : 4;
}

static int layered_threads(const LayerSched &ls, int R, int cap)
{
    int t = ((ls.max_layer + R - 1) / R + 63) / 64 * 64;
    return t < 64 ? 64 : (t > cap ? cap : t);
}

// Resident-state budget of the global layered kernel (bytes its resident codewords touch):
// within MI355X's 256 MiB Infinity Cache with room for the schedule and the rest of the
// working set (measured knee: 208.5 MiB fine, 216 MiB 1.2x slower; plan_layered).
static constexpr size_t kLayeredResidentBudget = (size_t)208 << 20;

// Bytes of its global slot one resident codeword of the global layered kernel touches:
// the posteriors outside LDS (fp64: positions [P, NP]; fp32: all) and the packed check
// state (min1/min2 + meta per row). DVB-S2 N=64800: 1.01 MB fp64, 0.65 MB fp32.
static size_t layered_resident_bytes(const FloodSched &fs, const LayerSched &ls, bool f64, int P)
{
    const long np1 = (long)fs.ngroups * 64 + 1;
    const size_t fsz = f64 ? 8 : 4;
    return (size_t)(np1 - P) * fsz + (size_t)ls.M_pad * (2 * fsz + layered_meta_bytes(fs));
}

// reported, and the bound of the global kernel's resident blocks (kernels.hip plan_lds; the
// LDS share is the largest P any code gets, not this code's)
static int layered_blocks_per_cu(bool f64, int threads)
{
    const void *fn = threads > 512
                         ? (f64 ? (const void *)k_decode_layered_global<double, SRC_PHILOX, 8, 1, true, 1024>
                                : (const void *)k_decode_layered_global<float, SRC_PHILOX, 8, 2, false, 1024>)
                         : (f64 ? (const void *)k_decode_layered_global<double, SRC_PHILOX, 8, 2, true>
                                : (const void *)k_decode_layered_global<float, SRC_PHILOX, 8, 4, false>);
    return occupancy(fn, threads, f64 ? (layered_lds_positions(1 << 30, 8) + 1) * 8 : 0);
}

template <typename F, int SRC, int DC>
static const void *layered_fn(bool lds, int threads)
{
    if (lds) return (const void *)k_decode_layered_lds<F, SRC, DC, 1>;
    // fp64 (R = 2, fewer rows in flight per pass: latency-bound): the posteriors of
    // the highest-degree bits in LDS (DVB-S2 1 130 -> 1 470 Mbit/s at R = 1); fp32
    // (R = 4): all in the slot -- the split's dual accesses cost it more (2 230 -> 2 010)
    constexpr bool SPLIT = sizeof(F) == 8;
    const int r = layered_rows_per_pass(true, sizeof(F) == 8);
    decltype(&k_decode_layered_global<F, SRC, DC, 1, SPLIT>) fn;
    if (threads > 512) {   // LDPC_LAYERED_THREADS=1024
        if constexpr (sizeof(F) == 4) fn = k_decode_layered_global<F, SRC, DC, 2, SPLIT, 1024>;
        else fn = k_decode_layered_global<F, SRC, DC, 1, SPLIT, 1024>;
    } else if constexpr (sizeof(F) == 4) {
        fn = k_decode_layered_global<F, SRC, DC, 4, SPLIT>;
    } else {
        fn = r == 2 ? k_decode_layered_global<F, SRC, DC, 2, SPLIT> : k_decode_layered_global<F, SRC, DC, 1, SPLIT>;
    }
    return (const void *)fn;
}

void plan_layered(const PlanInput &in, LaunchPlan &p)
{
    const FloodSched &fs = *in.fs;
    const LayerSched &ls = *in.ls;
    const bool f64 = in.f64;
    p = LaunchPlan{};
    const size_t st = layered_state_bytes(fs, ls, f64 ? 8 : 4);
    const bool lds = st <= kMaxLds - 2048 && opt(LDPC_OPT_KERNEL) != 3;   // 3: "global" forced (tests)
    if (lds) {
        p.kernel = Kernel::layered_lds;
        p.name = "layered_lds";
        p.lds_bytes = (int)st;
        p.threads = layered_threads(ls, layered_rows_per_pass(false, f64), 512);
    } else {
        p.kernel = Kernel::layered_global;
        p.name = "layered_global";
        p.scratch_per_block = st;
        p.threads = layered_threads(ls, layered_rows_per_pass(true, f64), layered_nt());
        if (f64) {   // SPLIT (layered_fn)
            p.layered_pos = layered_lds_positions(fs.ngroups * 64 + 1, 8);
            p.cache_lds_bytes = (p.layered_pos + 1) * 8;   // + LayApp's dummy slot
        }
    }
    p.fn = for_f_src(f64, in.a.src, [&](auto f, auto s) -> const void * {
        using F = typename decltype(f)::type;
        constexpr int SRC = decltype(s)::value;
        if (fs.dc <= 8) return layered_fn<F, SRC, 8>(lds, p.threads);
        if (fs.dc <= 16) return layered_fn<F, SRC, 16>(lds, p.threads);
        if (fs.dc <= kPackedMaxDc) return layered_fn<F, SRC, kPackedMaxDc>(lds, p.threads);
        return nullptr;
    });
    if (lds) {
        if (!p.fn) return;   // launch_layered refuses it
        const int per_cu = std::max(1, occupancy(p.fn, p.threads, p.lds_bytes));
        p.grid = std::min(per_cu * in.num_cus, in.a.batch);
        return;
    }
    // At most one codeword per CU, and no more resident
    // codewords than the Infinity Cache holds (kLayeredResidentBudget: DVB-S2 fp64,
    // 1.01 MB touched per codeword, runs 6.4 ms per codeword round at 184-216
    // resident codewords and 7.6 / 8.7 / 9.3 ms at 224 / 240 / 256 -- the state
    // spills to HBM; 2 per CU measured 1.5x slower); LDPC_OPT_LAYERED_BPC
    // overrides both (experiments).
    p.blocks_per_cu = layered_blocks_per_cu(f64, p.threads);
    const int bpc = opt(LDPC_OPT_LAYERED_BPC);
    int per_cu = std::min(p.blocks_per_cu, bpc > 0 ? bpc : 1);
    if (per_cu <= 0) per_cu = 1;
    int gblocks = per_cu * in.num_cus;
    if (bpc <= 0) {
        const size_t fp = layered_resident_bytes(fs, ls, f64, p.layered_pos);
        gblocks = (int)std::min<size_t>((size_t)gblocks, std::max<size_t>(1, kLayeredResidentBudget / fp));
    }
    if (gblocks > in.a.batch) gblocks = in.a.batch;
    // the same number of codeword rounds on fewer resident codewords
    const int rounds = (in.a.batch + gblocks - 1) / gblocks;
    p.grid = (in.a.batch + rounds - 1) / rounds;
    p.scratch_bytes = p.scratch_per_block * (size_t)p.grid;
}

hipError_t launch_layered(const LaunchPlan &p, const DevGraph &g, const FloodSched &fs, const LayerSched &ls,
                          const DecodeArgs &a, void *gscratch, hipStream_t s)
{
    if (ls.nlayers <= 0 || !ls.lptr) return hipErrorInvalidValue;
    unsigned char *gs = (unsigned char *)gscratch;
    size_t sb = p.scratch_per_block;
    int P = p.layered_pos;
    void *args[] = {(void *)&a, (void *)&g, (void *)&fs, (void *)&ls, &gs, &sb, &P};   // layered_lds takes the first four
    return launch_fn(p, args, s);
}

}  // namespace ldpc
