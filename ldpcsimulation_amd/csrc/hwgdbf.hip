// hwgdbf.hip -- CDNA4 (gfx950) kernels of the fixed-point NGDBF hardware model
// (src/NGDBFhw.cpp of the reference; line numbers below are that file's).
//
// Front end, in the cfg's precision F (:218-252, :611-677): a channel sample is saturated
// to +-Ymax, gives the hard decision r, and y / (2w) is quantised to the odd integer
// Y = +-(2m + 1), m = floor(|y / (2w)| NL / (2 lmax)), a sign-magnitude NQ-bit code.
// The qlen noise draws q go through (q - theta0) / (2w) - 1, clipped to +-lmax, and the
// same quantiser to Q[k]. From there everything is integer. A frame runs maxphase phases,
// every one from r (:280-373):
//   check nodes  s_j = parity of d over mlist[j]; the phase stops when every s_j = 0
//   bit nodes    E_i = (1 - 2 d_i) Y_i + Smult (satisfied checks of bit i) + Q[i + qpointer];
//                d_i flips when E_i <= theta; all bits read the same syndrome
//   pointer      qpointer++ per iteration, 0 when it reaches qlen - N; it runs on from
//                phase to phase (and, in the CLI, from frame to frame through qptr0)
// The frame reports the least error weight and the least iteration count over its phases,
// the last phase's decisions and whether that phase ended unsatisfied; every phase runs
// (the reference does not stop after a satisfied one).
//
// One kernel body, two shapes (template WAVE):
//   hwgdbf_wg    a 256-thread workgroup per codeword, two workgroup barriers per iteration
//   hwgdbf_wave  the wave-per-codeword skeleton (wave_cw.h): a lane owns bits
//                lane, lane + 64, ... and checks likewise
// Both are persistent and take codewords by ticket: a failing frame costs maxphase * T
// iterations, most frames a handful. hwgdbf_layout.h has the state of a codeword in LDS.
// The graph (template STAGE): where it fits beside the codewords every workgroup copies it
// into LDS once as 16-bit indices -- the checks' bits slot-major (edge k of check j at
// k * M + j, so the lanes of a wave read consecutive halfwords whatever the row degree) and
// the bits' checks in column order -- and the iterations read no global memory but col_ptr
// and row_deg. Without it the 2 E indices an iteration reads come from the device copy of
// the graph (DevGraph) through the caches.
#include "hwgdbf.h"
#include "gdbf_front.h"
#include "frame.h"
#include "wave_cw.h"

#include <hip/hip_runtime.h>

namespace ldpc {

// pack(quantize(v), sgn(v)) then unpack (:640-677): the magnitude keeps NQ - 1 bits.
template <typename F>
__device__ __forceinline__ int hw_quant(F v, F nl, F two_lmax, int nq)
{
    const int m = (int)gfloor(gabs(v) * nl / two_lmax);
    const int mag = ((m & ((1 << (nq - 1)) - 1)) << 1) | 1;
    const bool neg = !(v > F(0)) || ((m >> (nq - 1)) & 1);   // pack()'s sign bit is also bit NQ - 1 of |m|
    return neg ? -mag : mag;
}

template <bool WAVE> __device__ __forceinline__ void grp_sync()
{
    if (WAVE)
        wave_sync();
    else
        __syncthreads();
}
template <bool WAVE> __device__ __forceinline__ bool grp_or(int x)
{
    if (WAVE) {
        wave_sync();
        return wave_any(x);
    }
    return __syncthreads_or(x) != 0;
}
// Sum over the codeword's threads, valid in its first thread (WAVE: in every lane).
template <bool WAVE> __device__ __forceinline__ int grp_sum(int x, int *red)
{
    if (WAVE) return wave_sum(x);
    int v[1] = {x};
    block_sum_n_t0<1>(v, red);
    return v[0];
}

template <typename F, int SRC, bool WAVE, bool STAGE>
__global__ __launch_bounds__(WAVE ? 1024 : 256) void k_hwgdbf(HwgdbfArgs a, DevGraph g, HwgdbfLayout L)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int red[16 + 1];   // hwgdbf_wg: block sums; [16]: the next codeword
    const int lane = WAVE ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
    const int gs = WAVE ? 64 : (int)blockDim.x;
    const int upb = WAVE ? (int)(blockDim.x >> 6) : 1;   // codewords in flight per workgroup
    const uint16_t *gr = reinterpret_cast<const uint16_t *>(smem);             // [dcs][M] bits of the checks
    const uint16_t *gc = reinterpret_cast<const uint16_t *>(smem + L.gcoff);   // [E] checks of the bits
    if (STAGE) {   // once per workgroup, before its waves part ways
        uint16_t *wr = reinterpret_cast<uint16_t *>(smem), *wc = reinterpret_cast<uint16_t *>(smem + L.gcoff);
        for (int j = threadIdx.x; j < g.M; j += blockDim.x)
            for (int k = 0; k < g.dcs; ++k) wr[(size_t)k * g.M + j] = (uint16_t)g.row_cols[(size_t)j * g.dcs + k];
        for (int e = threadIdx.x; e < L.E; e += blockDim.x) wc[e] = (uint16_t)(g.col_refs[e] >> 6);
        __syncthreads();
    }
    unsigned char *base = smem + (STAGE ? L.cwoff : 0) + (WAVE ? (size_t)(threadIdx.x >> 6) * L.total : 0);
    int8_t *Y = reinterpret_cast<int8_t *>(base);
    int8_t *Q = reinterpret_cast<int8_t *>(base + L.qoff);
    uint8_t *D = base + L.doff;
    uint8_t *S = base + L.soff;
    const int N = g.N, M = g.M, T = a.T, qlen = a.qlen, nq = a.nq;
    const int wrap = qlen - N;   // >= 1 (the host refuses qlen <= N)
    const F ymax = (F)a.ymax, two_w = (F)a.two_w, lmax = (F)a.lmax, nl = (F)((1 << nq) - 1);
    const F two_lmax = F(2) * lmax, theta0 = (F)a.theta0, nsig = (F)a.noise_sigma;
    const int smult = a.smult, theta = a.theta;
    const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);

    CwTickets tk(a.ticket, a.batch, upb, lane == 0);
    for (int b = tk.first(WAVE ? (int)(threadIdx.x >> 6) : 0); b < a.batch;) {
        const uint64_t cw = a.first_cw + (uint64_t)b;
        const int8_t *cvec = frame_codeword<SRC>(a, b, N);
        // ---- channel + front end (:218-237) ----
        int unc = 0;
        for (int g4 = lane; g4 * 4 < N; g4 += gs) {
            F yv[4];
            channel_group<F, SRC, true>(a, b, g4, N, cvec, a.y_out, yv);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int v = g4 * 4 + q;
                if (v < N) {
                    F y = yv[q];
                    if (gabs(y) > ymax) y *= ymax / gabs(y);
                    const int rbit = y > F(0) ? 0 : 1;   // d = (1 - r) / 2
                    const int cbit = cvec ? cvec[v] < 0 : 0;
                    unc += rbit != cbit;
                    Y[v] = (int8_t)hw_quant<F>(y / two_w, nl, two_lmax, nq);
                    D[v] = (uint8_t)(rbit << 1);
                }
            }
        }
        // ---- the noise shift register (:239-252) ----
        for (int k4 = lane; k4 * 4 < qlen; k4 += gs) {
            F qv[4];
            if (SRC == SRC_GIVEN) {
                const F *qr = reinterpret_cast<const F *>(a.q) + (size_t)b * qlen;
#pragma unroll
                for (int q = 0; q < 4; ++q) qv[q] = (k4 * 4 + q < qlen) ? qr[k4 * 4 + q] : F(0);
            } else {
                uint32_t u[4];
                philox4x32_10<true>((uint32_t)k4, (uint32_t)cw, (uint32_t)(cw >> 32),
                                    (a.stream_id & 0xFFFFFu) | (1u << 20), k0, k1, u);
                float n[4];
                box_muller_hw(u[0], u[1], n[0], n[1]);
                box_muller_hw(u[2], u[3], n[2], n[3]);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    qv[q] = nsig * (F)n[q];
                    if (a.q_out && k4 * 4 + q < qlen)
                        reinterpret_cast<F *>(a.q_out)[(size_t)b * qlen + k4 * 4 + q] = qv[q];
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k = k4 * 4 + q;
                if (k < qlen) {
                    F qm = (qv[q] - theta0) / two_w - F(1);
                    if (qm > lmax)
                        qm = lmax;
                    else if (qm < -lmax)
                        qm = -lmax;
                    Q[k] = (int8_t)hw_quant<F>(qm, nl, two_lmax, nq);
                }
            }
        }
        int qp = 0;
        if (SRC == SRC_GIVEN && a.qptr0) {
            const int p0 = a.qptr0[b];
            qp = (unsigned)p0 < (unsigned)wrap ? p0 : 0;   // the host has checked it
        }

        grp_sync<WAVE>();   // the front end wrote D by groups of 4 bits, the restart reads it by bit

        int it = 0, total = 0, least_it = T, least_err = N;
        bool sat = false;
        for (int ph = 0; ph < a.maxphase; ++ph) {
            // ---- restart from the channel decision (:283-286); each thread its own bits ----
            for (int v = lane; v < N; v += gs) {
                const uint32_t dd = D[v];
                D[v] = (uint8_t)((dd & 2u) | (dd >> 1));
            }
            grp_sync<WAVE>();
            for (it = 0; it < T; ++it) {
                // ---- check nodes (:546-563) ----
                int fail = 0;
                for (int j = lane; j < M; j += gs) {
                    const int deg = g.row_deg[j];
                    const int32_t *rc = g.row_cols + (size_t)j * g.dcs;
                    uint32_t p = 0;
                    for (int k = 0; k < deg; ++k) {
                        const uint32_t i = STAGE ? (uint32_t)gr[(size_t)k * M + j] : (uint32_t)rc[k];
                        p ^= D[LDPC_CHK(i, (uint32_t)N, CHK_HWGDBF_BIT)];
                    }
                    p &= 1u;
                    S[j] = (uint8_t)p;
                    fail |= (int)p;
                }
                sat = !grp_or<WAVE>(fail);
                if (sat) break;   // :298-299, uniform over the codeword's threads
                // ---- bit nodes (:565-593) ----
                for (int v = lane; v < N; v += gs) {
                    const int e0 = g.col_ptr[v], e1 = g.col_ptr[v + 1];
                    int uns = 0;
                    for (int e = e0; e < e1; ++e) {
                        const uint32_t j = STAGE ? (uint32_t)gc[e] : g.col_refs[e] >> 6;
                        uns += S[LDPC_CHK(j, (uint32_t)M, CHK_HWGDBF_CHECK)];
                    }
                    const uint32_t dd = D[v];
                    const int yv = Y[v];
                    const int E = ((dd & 1u) ? -yv : yv) + (e1 - e0 - uns) * smult +
                                  Q[LDPC_CHK(v + qp, (uint32_t)qlen, CHK_HWGDBF_NOISE)];
                    if (E <= theta) D[v] = (uint8_t)(dd ^ 1u);
                }
                grp_sync<WAVE>();
                if (++qp >= wrap) qp = 0;   // :356-358
            }
            // ---- the phase's result (:366-372) ----
            int errs = 0;
            for (int v = lane; v < N; v += gs) errs += (int)(D[v] & 1u) != (cvec ? cvec[v] < 0 : 0);
            errs = grp_sum<WAVE>(errs, red);
            least_err = min(least_err, errs);
            least_it = min(least_it, it);
            total += it;
        }
        if (a.d_out)
            for (int v = lane; v < N; v += gs) a.d_out[(size_t)b * N + v] = (D[v] & 1u) ? -1 : 1;
        unc = grp_sum<WAVE>(unc, red);
        if (lane == 0) {
            frame_account(a.counts, a.hist, a.frame_res, b, least_err, unc, !sat, least_it, least_it);
            if (a.iters_run) a.iters_run[b] = total;
        }
        if (WAVE) {
            b = tk.next();
        } else {   // hwgdbf_wg: the first thread hands its ticket to the workgroup
            if (lane == 0) red[16] = (int)tk.nxt;
            __syncthreads();
            b = tk.redraw(red[16]);   // rewritten only after the next codeword's barriers
        }
    }
}

LDPC_CHECK_TU(hwgdbf)

#if defined(LDPC_HWGDBF_FORCE_WAVE) && !defined(LDPC_AB_BUILD)
#error "LDPC_HWGDBF_FORCE_WAVE changes the kernel choice the tests pin: variant builds only"
#endif

HwgdbfChoice hwgdbf_choose(const DevGraph &g, int E, int qlen)
{
#ifdef LDPC_HWGDBF_FORCE_WAVE   // A/B builds (make hwgdbfvariant): the wavefront shape wherever it is not forced off
    const bool wg_competes = false;
#else
    const bool wg_competes = true;
#endif
    return hwgdbf_plan({g.N, g.M, g.dcs, E}, qlen, opt(LDPC_OPT_GDBF_KERNEL) == 1, wg_competes);
}

hipError_t hwgdbf_launch(const DevGraph &g, const HwgdbfArgs &a, bool f64, const HwgdbfChoice &ch, int E, int num_cus,
                         hipStream_t s)
{
    return wave_cw_launch(
        a, f64, ch, num_cus, s,
        [&](auto f, auto src) {
            using F = typename decltype(f)::type;
            constexpr int SRC = decltype(src)::value;
            if (ch.staged) return ch.wave ? k_hwgdbf<F, SRC, true, true> : k_hwgdbf<F, SRC, false, true>;
            return ch.wave ? k_hwgdbf<F, SRC, true, false> : k_hwgdbf<F, SRC, false, false>;
        },
        g, hwgdbf_layout({g.N, g.M, g.dcs, E}, a.qlen));
}

}  // namespace ldpc
