// rgdbf.hip -- CDNA4 (gfx950) kernels of the re-decoding NGDBF decoder
// (src/RNGDBF.cpp built as decodeRSMNGDBF: -D redecode -D addNoise
// -D thresholdAdaptation -D weightSyndromes -D outputSmoothing -D saturateSamples).
//
// A frame is decoded in up to `maxphase` phases (:277-400), each the phase of
// ngdbf_phase.h (check step, bit step, smoothing; shared with rstat.hip).
// The phase loop ends after a satisfied phase; the frame's output and error weight
// are the last phase's, its iteration count the sum over its phases (:394). A failed
// phase runs exactly T iterations, so the host derives the phase count from it.
// The perturbation of iteration `it` of phase `ph` is row ph*T + it: given by the
// caller as pert[frame][ph*T + it][bit], or Philox4x32-10 at stream word
// stream_id | (ph*T + it + 1) << 20 -- phase 0 draws what gdbf.hip draws.
// Compiled with -ffp-contract=off.
#include "rgdbf.h"
#include "ngdbf_phase.h"
#include "gdbf_launch.h"
#include "minsum_common.h"

#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>

namespace ldpc {

// Here: the phase loop, where a perturbation row comes from, and the frame's accounting.

// ---------------------------------------------------------------------
// Generic kernels: one workgroup per codeword, its state in LDS (rgdbf_lds) or in
// a global slot (rgdbf_global), as gdbf_lds / gdbf_global.
// ---------------------------------------------------------------------
template <typename F, int SRC>
__device__ __forceinline__ void rgdbf_codeword(const RgdbfArgs &a, const DevGraph &g, int b, const NgdbfWg<F> &wg)
{
    const int N = g.N, T = a.T;
    const uint64_t cw = a.first_cw + (uint64_t)b;
    const int8_t *cvec = frame_codeword<SRC>(a, b, N);
    const int unc = wg.template front<SRC>(a, b, N, cvec, nullptr);
    int total = 0;
    bool sat = false;
    for (int ph = 0; ph < a.maxphase; ++ph) {
        total += wg.template phase<false, CHK_RGDBF_BIT, CHK_RGDBF_PARITY>(   // :394
            a, g, cvec, NgdbfTrace{}, sat, [&](int it, int g4, F(&pv)[4]) {
                const int gi = ph * T + it;   // the perturbation row
                if (SRC == SRC_GIVEN) {
                    const F *pr = reinterpret_cast<const F *>(a.pert) + ((size_t)b * ((size_t)a.maxphase * T) + gi) * N;
#pragma unroll
                    for (int q = 0; q < 4; ++q) pv[q] = (g4 * 4 + q < N) ? pr[g4 * 4 + q] : F(0);
                } else {
                    ngdbf_draw<F>(a, g4, (uint32_t)cw, (uint32_t)(cw >> 32), gi, pv);
                }
            });
        if (sat) break;   // :398-399
    }
    int sums[3];
    wg.template finish<CHK_RGDBF_BIT>(a, g, cvec, sat, a.d_out ? a.d_out + (size_t)b * N : nullptr, unc, sums);
    if (threadIdx.x == 0)
        frame_account(a.counts, a.hist, a.frame_res, b, sums[0], sums[1], sums[2] > 0, total, total);
    __syncthreads();
}

template <typename F, int SRC>
__global__ __launch_bounds__(256) void k_rgdbf_lds(RgdbfArgs a, DevGraph g, RgdbfLayout L)
{
    ngdbf_wg_lds<F>(a, L, [&](int b, const NgdbfWg<F> &wg) { rgdbf_codeword<F, SRC>(a, g, b, wg); });
}

template <typename F, int SRC>
__global__ __launch_bounds__(1024) void k_rgdbf_global(RgdbfArgs a, DevGraph g, RgdbfLayout L, unsigned char *scratch)
{
    ngdbf_wg_global<F>(a, L, scratch, a.batch, [&](int b, const NgdbfWg<F> &wg) { rgdbf_codeword<F, SRC>(a, g, b, wg); });
}

// ---------------------------------------------------------------------
// rgdbf_rows: the register schedule (NgdbfRows, ngdbf_phase.h) with the phase loop inside
// the codeword: a restart is a register copy, one flag-byte store and one barrier, and the
// early-stop flag alternates on the perturbation row ph * T + it. A failing frame costs up
// to maxphase * T iterations, most frames a handful: codewords go out by ticket.
// ---------------------------------------------------------------------
template <typename F, int SRC, int DVM, int NT>
__global__ __launch_bounds__(NT, 4) void k_rgdbf_rows(RgdbfArgs a, DevGraph g, int np, int poff, int floff)
{
    using Rows = NgdbfRows<F, DVM, NT>;
    constexpr int BPT = Rows::BPT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int red[Rows::kRed];
    Rows R(a, g, smem, red, np, poff, floff);
    const int N = g.N, T = a.T;
    unsigned nxt = R.first_ticket(a.ticket);
    for (int b = blockIdx.x; b < a.batch; b = R.next_item(a.ticket, a.batch, nxt)) {
        const uint64_t cw = a.first_cw + (uint64_t)b;
        const int8_t *cvec = frame_codeword<SRC>(a, b, N);
        F yq[BPT], theta[BPT];
        int d[BPT], dsum[BPT];
        uint32_t rneg;   // bit q: r = -1
        const int unc = R.template front<SRC>(a, b, cvec, nullptr, yq, rneg);
        int total = 0;
        bool sat = false;
        for (int ph = 0; ph < a.maxphase; ++ph) {
            // ---- restart from r (:282-288, :303-306) ----
#pragma unroll
            for (int q = 0; q < BPT; ++q) {
                d[q] = (rneg >> q) & 1u ? -1 : 1;
                theta[q] = (F)a.theta0;
                dsum[q] = 0;
            }
            total += R.template phase<CHK_RGDBF_BIT, CHK_RGDBF_PARITY>(   // :394
                ph * T, yq, theta, d, dsum, sat, [&](int it, F(&pv)[BPT]) {
                    const int gi = ph * T + it;   // the perturbation row
                    if (SRC == SRC_GIVEN) {
                        const F *pr = reinterpret_cast<const F *>(a.pert) + ((size_t)b * ((size_t)a.maxphase * T) + gi) * N;
#pragma unroll
                        for (int q = 0; q < BPT; ++q) pv[q] = (R.v0 + q < N) ? pr[R.v0 + q] : F(0);
                    } else {
                        ngdbf_draw<F>(a, R.tid, (uint32_t)cw, (uint32_t)(cw >> 32), gi, pv);
                    }
                });
            if (sat) break;   // :398-399
        }
        int sums[3];
        R.template finish<CHK_RGDBF_BIT>(cvec, sat, d, dsum, a.d_out ? a.d_out + (size_t)b * N : nullptr, unc, sums);
        if (R.tid == 0) frame_account(a.counts, a.hist, a.frame_res, b, sums[0], sums[1], sums[2] > 0, total, total);
    }
}

constexpr size_t kRgdbfMaxLds = 64 * 1024;

LDPC_CHECK_TU(rgdbf)

RgdbfChoice rgdbf_choose(const DevGraph &g, bool f64, int maxdv, int maxdc)
{
    RgdbfChoice ch;
    if (rgdbf_rows_fits(g.N, g.M, maxdv, maxdc) && opt(LDPC_OPT_GDBF_KERNEL) != 1) {
        ch.name = "rgdbf_rows";
        ch.threads = g.N <= 4 * 512 && g.M <= 2 * 512 ? 512 : 1024;
        ch.dvm = maxdv <= 4 ? 4 : 12;
        ch.lds_bytes = rgdbf_rows_layout(g.N, g.M).total;
        return ch;
    }
    const RgdbfLayout L = rgdbf_layout(g.N, g.M, f64 ? 8 : 4);
    if (L.total <= kRgdbfMaxLds) {
        ch.name = "rgdbf_lds";
        ch.lds_bytes = (int)L.total;
        ch.threads = 256;
    } else {
        ch.name = "rgdbf_global";
        ch.threads = 1024;
        ch.slot_bytes = L.total;
    }
    return ch;
}

hipError_t rgdbf_launch(const DevGraph &g, const RgdbfArgs &a, bool f64, const RgdbfChoice &ch, void *scratch,
                        int slots, int num_cus, hipStream_t s)
{
    if (a.batch <= 0) return hipSuccess;
    return gdbf_dispatch(f64, a.src, [&](auto f, auto src) {
        using F = decltype(f);
        constexpr int SRC = decltype(src)::value;
        if (ch.dvm) {
            const RgdbfRowsLayout L = rgdbf_rows_layout(g.N, g.M);
            return gdbf_rows_dispatch(ch, [&](auto dvm, auto nt) {
                return gdbf_rows_grid_launch(k_rgdbf_rows<F, SRC, decltype(dvm)::value, decltype(nt)::value>,
                                             decltype(nt)::value, L.total, a.ticket, true, a.batch, num_cus, s, a, g,
                                             L.np, L.poff, L.floff);
            });
        }
        const RgdbfLayout L = rgdbf_layout(g.N, g.M, sizeof(F));
        if (ch.lds_bytes > 0) {
            hipLaunchKernelGGL((k_rgdbf_lds<F, SRC>), dim3(a.batch), dim3(ch.threads), ch.lds_bytes, s, a, g, L);
        } else {
            const int grid = slots < a.batch ? slots : a.batch;
            if (grid <= 0 || !scratch) return hipErrorInvalidValue;
            hipLaunchKernelGGL((k_rgdbf_global<F, SRC>), dim3(grid), dim3(ch.threads), 0, s, a, g, L,
                               (unsigned char *)scratch);
        }
        return hipGetLastError();
    });
}

}  // namespace ldpc
