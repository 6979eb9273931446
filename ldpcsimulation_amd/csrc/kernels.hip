// kernels.hip -- CDNA4 (gfx950) kernels of the flooding min-sum decoder.
//
// One workgroup (4 waves) decodes one codeword for all T iterations with its
// whole message state on chip:
//   app[N]   posterior sums  sum = yq + sum_k c2v  (symNodeUpdates :456-463)
//   yq[N]    channel samples after the front-end (:214-229)
//   rows[M]  compressed check state {m1, m2, meta}: the two smallest |v2c|
//            after normalisation/offset, argmin position and the sign of
//            every c2v on the row (checkNodeUpdates :410-450 +
//            applyNormalization :494-499 / applyOffset :503-515).
// Every c2v message is a pure function of its row state, so the flooding
// schedule needs no E-sized message arrays: the check phase rebuilds the old
// c2v from the row state it owns and forms v2c = app - c2v_old, which is
// bit-identical to the reference's v2c = sum - c2v (:469) because both are
// the same IEEE subtraction of the same operands. The bit phase re-sums
// yq + c2v in the reference's nlist order, so app (and the hard decision
// d = sum > 0 ? +1 : -1, :471-474) is bit-identical too, in fp64 to the
// reference and in fp32 to the fp32 restatement.
//
// The translation unit is compiled with -ffp-contract=off (see Makefile):
// no FMA may fuse the channel's 1 + sigma*n or the quantiser.
#include "minsum_kernels.h"
#include "frame.h"

namespace ldpc {

// ---------------------------------------------------------------------
// One codeword, all T iterations. rows/app/yq may live in LDS or in a
// per-workgroup global scratch slot; red is LDS.
// ES (DecodeArgs.early_stop; instantiations of their own, so that the fixed-T kernels keep
// their code): the syndrome of the decisions is also taken before every iteration, and the
// codeword stops with D(it), `it` iterations counted and reported, at the first one that
// is zero (rows_es.hip states the rule).
// ---------------------------------------------------------------------
template <typename F, int SRC, bool ES>
__device__ __forceinline__ void decode_codeword(const DecodeArgs &a, const DevGraph &g, int b,
                                                RowState<F> *rows, F *app, F *yq, int *red)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    const int N = g.N, M = g.M;

    // ---- channel + front-end (:214-238) ----
    const int8_t *cvec = frame_codeword<SRC>(a, b, N);
    int unc = 0;
    channel_bits<F, SRC, false>(a, b, N, cvec, a.y_out, [&](int v, F yv) {
        const F q = front_end<F>(yv, a);
        yq[v] = q;
        app[v] = q;
        const int cv = cvec ? cvec[v] : 1;
        unc += ((q > F(0) ? 1 : -1) * cv < 0);
    });
    for (int j = tid; j < M; j += nt) {
        RowState<F> z;
        z.m1 = F(0); z.m2 = F(0); z.meta = 0;
        rows[j] = z;   // c2v_old = +0: v2c = yq on the first pass (:364-370)
    }
    __syncthreads();

    const F alpha = (F)a.alpha, delta = (F)a.delta;
    // H * d of the decisions app holds (complete: a barrier precedes every call)
    auto syndrome = [&]() -> int {
        int synd = 0;
        for (int j = tid; j < M; j += nt) {
            const int deg = g.row_deg[j];
            const int32_t *rc = g.row_cols + (size_t)j * g.dcs;
            int par = 0;
            for (int k = 0; k < deg; ++k) par ^= (app[rc[k]] > F(0)) ? 0 : 1;
            synd |= par;
        }
        return synd;
    };
    int it = 0;
    for (; it < a.T; ++it) {
        if (ES && !__syncthreads_or(syndrome())) break;   // uniform: D(it) is a codeword
        // ---- check nodes ----
        for (int j = tid; j < M; j += nt) {
            RowState<F> st = rows[j];
            const int deg = g.row_deg[j];
            const int32_t *rc = g.row_cols + (size_t)j * g.dcs;
            const int oidx = (int)(st.meta & 63u);
            const uint64_t osg = st.meta >> 6;
            F mn1 = dinf<F>(), mn2 = dinf<F>();
            int amin = 63;
            uint64_t sg = 0;
            for (int k = 0; k < deg; ++k) {
                F cold = (k == oidx) ? st.m2 : st.m1;
                if ((osg >> k) & 1u) cold = -cold;
                const F x = app[rc[k]] - cold;               // v2c (:469)
                sg |= (uint64_t)(!(x >= F(0))) << k;          // sgn(v2c) < 0
                const F ax = dabs(x);
                if (ax <= mn1) { mn2 = mn1; mn1 = ax; amin = k; }   // :428-433
                else if (ax < mn2) { mn2 = ax; }                    // :434-437
            }
            const uint64_t degmask = (deg >= 64) ? ~0ull : ((1ull << deg) - 1ull);
            uint64_t eff = (__popcll(sg) & 1) ? (sg ^ degmask) : sg;   // prod * sgn(v2c_k)
            F M1 = mn1, M2 = mn2;
            if (a.variant == V_NMS) {
                M1 = mn1 / alpha;                              // :498 (IEEE division)
                M2 = mn2 / alpha;
            } else if (a.variant == V_OMS) {
                const F t1 = mn1 - delta, t2 = mn2 - delta;    // :509
                const bool p1 = t1 > F(0), p2 = t2 > F(0);
                M1 = p1 ? t1 : F(0);
                M2 = p2 ? t2 : F(0);
                // sgn(c2v) of :511 maps -0.0 to +1; a zeroed message is +0 (:513)
                const uint64_t abit = (amin < 64) ? (1ull << amin) : 0ull;
                if (!p1 || mn1 == F(0)) eff &= abit;
                if (!p2 || mn2 == F(0)) eff &= ~abit;
            }
            st.m1 = M1;
            st.m2 = M2;
            st.meta = (uint64_t)amin | (eff << 6);
            rows[j] = st;
        }
        __syncthreads();
        // ---- bit nodes: sum = yq + c2v in nlist order (:456-463) ----
        for (int v = tid; v < N; v += nt) {
            F sum = yq[v];
            const int e1 = g.col_ptr[v + 1];
            for (int e = g.col_ptr[v]; e < e1; ++e) {
                const uint32_t ref = g.col_refs[e];
                const int k = (int)(ref & 63u);
                const RowState<F> st = rows[ref >> 6];
                const F mag = (k == (int)(st.meta & 63u)) ? st.m2 : st.m1;
                sum += ((st.meta >> (6 + k)) & 1u) ? -mag : mag;
            }
            app[v] = sum;
        }
        __syncthreads();
    }

    // ---- decisions, error weight (:270, :382-393), syndrome ----
    int w = 0;
    for (int v = tid; v < N; v += nt) {
        const int d = app[v] > F(0) ? 1 : -1;                 // :471-474
        const int cv = cvec ? cvec[v] : 1;
        w += (d != cv);
        if (a.d_out) a.d_out[(size_t)b * N + v] = (int8_t)d;
    }
    int sums[3] = {w, unc, syndrome()};
    block_sum_n_t0<3>(sums, red);
    if (tid == 0)   // the block totals exist in thread 0 only
        frame_account(a.counts, a.hist, a.frame_res, b, sums[0], sums[1], sums[2] > 0, ES ? it : a.T, ES ? it : 0);
    __syncthreads();
}

// State in LDS: one codeword per workgroup, grid = batch.
template <typename F, int SRC, bool ES>
__global__ __launch_bounds__(256) void k_decode_lds(DecodeArgs a, DevGraph g)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    RowState<F> *rows = reinterpret_cast<RowState<F> *>(smem);
    F *app = reinterpret_cast<F *>(smem + sizeof(RowState<F>) * (size_t)g.M);
    F *yq = app + g.N;
    int *red = reinterpret_cast<int *>(yq + g.N);
    decode_codeword<F, SRC, ES>(a, g, blockIdx.x, rows, app, yq, red);
}

// Re-decode list of the fast row kernel (rows_fast.hip): redo[0] codewords
// whose fast-path premise failed, batch indices in redo[1..]; each is decoded
// from scratch on this exact path (state in LDS), persistent grid. With an
// empty list every block exits at once. The fast kernels are not planned with early_stop:
// this one never stops early.
template <typename F, int SRC>
__global__ __launch_bounds__(256) void k_redo(DecodeArgs a, DevGraph g, const unsigned *redo)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    RowState<F> *rows = reinterpret_cast<RowState<F> *>(smem);
    F *app = reinterpret_cast<F *>(smem + sizeof(RowState<F>) * (size_t)g.M);
    F *yq = app + g.N;
    int *red = reinterpret_cast<int *>(yq + g.N);
    const unsigned n = redo[0];
    for (unsigned i = blockIdx.x; i < n; i += gridDim.x) decode_codeword<F, SRC, false>(a, g, (int)redo[1 + i], rows, app, yq, red);
}

// State in a global scratch slot per workgroup (codes whose state exceeds
// LDS, e.g. DVB-S2 N=64800): persistent grid, codewords strided.
template <typename F, int SRC, bool ES>
__global__ __launch_bounds__(256) void k_decode_global(DecodeArgs a, DevGraph g, unsigned char *scratch,
                                                       size_t slot_bytes)
{
    __shared__ int red[16];
    unsigned char *base = scratch + slot_bytes * blockIdx.x;
    RowState<F> *rows = reinterpret_cast<RowState<F> *>(base);
    F *app = reinterpret_cast<F *>(base + sizeof(RowState<F>) * (size_t)g.M);
    F *yq = app + g.N;
    for (int b = blockIdx.x; b < a.batch; b += gridDim.x)
        decode_codeword<F, SRC, ES>(a, g, b, rows, app, yq, red);
}


// Exhaustive check of the reciprocal division (see kernels.h).
__global__ __launch_bounds__(256) void k_verify_div(float alpha, float rcp, unsigned long long *bad)
{
    const uint32_t total = 0x7f800000u;   // all finite non-negative floats
    unsigned long long nbad = 0;
    for (uint32_t u = blockIdx.x * blockDim.x + threadIdx.x; u < total; u += gridDim.x * blockDim.x) {
        const float x = __uint_as_float(u);
        const float q = x * rcp;
        const float f = __builtin_fmaf(__builtin_fmaf(-q, alpha, x), rcp, q);
        const float d = x / alpha;
        nbad += (__float_as_uint(f) != __float_as_uint(d));
    }
    for (int o = 32; o > 0; o >>= 1) nbad += __shfl_xor(nbad, o, 64);
    if ((threadIdx.x & 63) == 0 && nbad) atomicAdd(bad, nbad);
}


hipError_t verify_div_by_reciprocal(float alpha, float rcp, unsigned long long *bad, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(bad, 0, sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_verify_div, dim3(8192), dim3(256), 0, s, alpha, rcp, bad);
    return hipGetLastError();
}

static size_t state_bytes(const DevGraph &g, bool f64)
{
    const size_t rs = f64 ? sizeof(RowState<double>) : sizeof(RowState<float>);
    const size_t fs = f64 ? 8 : 4;
    return rs * (size_t)g.M + 2 * fs * (size_t)g.N;
}

constexpr int kThreads = 256;

int occupancy(const void *fn, int threads, int lds_bytes)
{
    int nb = 0;
    if (lds_bytes > 0) (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, threads, lds_bytes) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return nb;
}

hipError_t launch_fn(const LaunchPlan &p, void **args, hipStream_t s)
{
    const int lds = p.lds_bytes + p.cache_lds_bytes + p.pad_lds_bytes;
    if (!p.fn || p.grid <= 0) return hipErrorInvalidValue;
    if (lds > 0) {
        const hipError_t e = hipFuncSetAttribute(p.fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return e;
    }
    return hipLaunchKernel(p.fn, dim3(p.grid), dim3(p.threads), args, (size_t)lds, s);
}

// The blocks-per-CU figures the plans report ask the SRC_PHILOX instance of each kernel
// (and, for the families with a degree axis, one representative degree): the info calls
// have no sample source, and the figure sizes the scratch kernels' grids, so it must not
// move with the source of a launch.
bool plan_lds(const PlanInput &in, LaunchPlan &p)
{
    const size_t lds = (state_bytes(in.g, in.f64) + 64 + 15) & ~(size_t)15;
    if (lds > kMaxLds) return false;
    const bool es = in.a.early_stop != 0;
    const auto fn = [es](auto f, auto s) {
        using F = typename decltype(f)::type;
        constexpr int SRC = decltype(s)::value;
        return es ? (const void *)k_decode_lds<F, SRC, true> : (const void *)k_decode_lds<F, SRC, false>;
    };
    p = LaunchPlan{};
    p.kernel = Kernel::lds;
    p.name = "lds";
    p.fn = for_f_src(in.f64, in.a.src, fn);
    p.threads = kThreads;
    p.lds_bytes = (int)lds;
    p.blocks_per_cu = occupancy(for_f_src(in.f64, SRC_PHILOX, fn), p.threads, p.lds_bytes);
    p.grid = in.a.batch;
    return true;
}

void plan_global(const PlanInput &in, LaunchPlan &p)
{
    const bool es = in.a.early_stop != 0;
    const auto fn = [es](auto f, auto s) {
        using F = typename decltype(f)::type;
        constexpr int SRC = decltype(s)::value;
        return es ? (const void *)k_decode_global<F, SRC, true> : (const void *)k_decode_global<F, SRC, false>;
    };
    p = LaunchPlan{};
    p.kernel = Kernel::global;
    p.name = "global";
    p.fn = for_f_src(in.f64, in.a.src, fn);
    p.threads = kThreads;
    p.scratch_per_block = (state_bytes(in.g, in.f64) + 255) & ~(size_t)255;
    p.blocks_per_cu = occupancy(for_f_src(in.f64, SRC_PHILOX, fn), p.threads, 0);
    int per_cu = p.blocks_per_cu;
    if (const int cap = opt(LDPC_OPT_FLOOD_BPC)) per_cu = std::min(per_cu, cap);   // experiments (as the flood kernel)
    if (per_cu <= 0) per_cu = 1;
    p.grid = std::min(per_cu * in.num_cus, in.a.batch);
    p.scratch_bytes = p.scratch_per_block * (size_t)p.grid;
}

hipError_t launch_generic(const LaunchPlan &p, const DevGraph &g, const DecodeArgs &a, void *gscratch, hipStream_t s)
{
    unsigned char *gs = (unsigned char *)gscratch;
    size_t spb = p.scratch_per_block;
    void *args[] = {(void *)&a, (void *)&g, &gs, &spb};   // k_decode_lds takes the first two
    return launch_fn(p, args, s);
}

size_t redo_lds_bytes(const DevGraph &g, bool f64) { return (state_bytes(g, f64) + 64 + 15) & ~(size_t)15; }

hipError_t launch_redo(const DevGraph &g, const DecodeArgs &a, bool f64, const unsigned *redo, hipStream_t s,
                       int num_cus)
{
    const size_t lds = redo_lds_bytes(g, f64);
    return for_f_src(f64, a.src, [&](auto f, auto src) -> hipError_t {
        auto fn = k_redo<typename decltype(f)::type, decltype(src)::value>;
        hipError_t e = hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(fn, dim3(num_cus), dim3(kThreads), lds, s, a, g, redo);
        return hipGetLastError();
    });
}

}  // namespace ldpc
