// rstat.hip -- CDNA4 (gfx950) kernels of the every-attempt NGDBF decoders: the reference's
// redecodeStatistics (src/newstat.cpp) and replayGDBF (src/replayGDBF.cpp), both built with
// -D addNoise -D thresholdAdaptation -D weightSyndromes -D outputSmoothing -D saturateSamples.
//
// A frame is decoded `attempts` times from the same channel samples (newstat.cpp:305-429).
// Every attempt is one phase of ngdbf_phase.h (the body rgdbf.hip's phases have): from the
// channel hard decision r with theta_i = theta and dsum = 0, up to T iterations.
// Unlike rgdbf.hip's phases every attempt runs, whatever the earlier ones gave, so a work
// item is (frame, attempt), items are numbered frame-major, and every item is independent.
// The perturbation of iteration `it` of local attempt ai is pert[frame][ai][it][bit], or
// Philox4x32-10 at counter (bit / 4, lo32(f), hi32(f) + at, stream_id | (it + 1) << 20) with
// f the frame number and at = first_attempt + ai: what phase 0 of frame f + (at << 32) draws
// in rgdbf.hip, so attempt 0 is that decoder with maxphase 1. The channel is frame f's own;
// every item redraws it (one Philox call per four bits against T rows of them).
//
// Two shapes, the pair rgdbf.hip has:
//   rstat_rows   the codes rgdbf_rows takes (N <= 4096, row degree <= 8, column degree <= 12):
//                the register schedule (NgdbfRows), persistent, items by ticket.
//   rstat_wg     a 256-thread workgroup per item, its state in LDS or, where that does not
//                fit, in a global slot of a persistent grid (the rgdbf_lds / rgdbf_global
//                pair). Takes every graph; the one that writes the per-iteration traces, and
//                the one option LDPC_OPT_GDBF_KERNEL = 1 forces.
// Not built: the frame-resident shape (a workgroup that holds one frame's yq, r, weights and
// the graph as 16-bit indices in LDS and runs several of its attempts side by side). Whether
// it pays on codes like 802.3an, where rstat_wg waits on graph reads from L2, is open
// (DESIGN 13d).
// The frame-level accounting (newstat.cpp:421-465: error weight, syndrome and decisions of
// the last attempt, iterations summed over the attempts, uncoded errors once) is a small
// kernel of its own behind the attempts.
// Compiled with -ffp-contract=off; E keeps the reference's operation order.
#include "rstat.h"
#include "ngdbf_phase.h"
#include "gdbf_launch.h"
#include "minsum_common.h"

#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>

namespace ldpc {

// What one (frame, attempt) item is: the frame b and local attempt ai of item number `item`,
// the Philox high counter word of its perturbations, its first row in pert / pert_out / the
// traces, and what it writes at its end.
struct RstatItem {
    int b, ai;
    uint32_t c1, c2;   // Philox counter words 1 and 2: lo32(f), hi32(f) + at
    size_t row0;
    bool last;         // the frame's last attempt: the one d_out and frame_unc are written with

    __device__ __forceinline__ RstatItem(const RstatArgs &a, int item) : b(item / a.attempts), ai(item - b * a.attempts)
    {
        const uint64_t cw = a.first_cw + (uint64_t)b;
        c1 = (uint32_t)cw;
        c2 = (uint32_t)(cw >> 32) + (uint32_t)(a.first_attempt + ai);
        row0 = ((size_t)b * a.attempts + ai) * (size_t)a.T;
        last = ai == a.attempts - 1;
    }
    __device__ __forceinline__ void *y_out(const RstatArgs &a) const { return ai == 0 ? a.y_out : nullptr; }
    __device__ __forceinline__ int8_t *d_row(const RstatArgs &a, int N) const
    {
        return last && a.d_out ? a.d_out + (size_t)b * N : nullptr;
    }
    // Row `it` of the item's perturbations for the bits v0..v0+3 of Philox group g4 (:361-376).
    template <typename F, int SRC>
    __device__ __forceinline__ void draw(const RstatArgs &a, int N, int it, int g4, int v0, F (&pv)[4]) const
    {
        if (SRC == SRC_GIVEN) {
            const F *pr = reinterpret_cast<const F *>(a.pert) + (row0 + it) * N;
#pragma unroll
            for (int q = 0; q < 4; ++q) pv[q] = (v0 + q < N) ? pr[v0 + q] : F(0);
        } else {
            ngdbf_draw<F>(a, g4, c1, c2, it, pv);
            if (a.pert_out) {
                F *po = reinterpret_cast<F *>(a.pert_out) + (row0 + it) * N;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (v0 + q < N) po[v0 + q] = pv[q];
            }
        }
    }
    // Thread 0, with the block's sums of finish(): the attempt's record (:415-418).
    __device__ __forceinline__ void account(const RstatArgs &a, const int (&sums)[3], int it) const
    {
        a.attempt_res[(size_t)b * a.attempts + ai] =
            make_int4(sums[0], it, sums[2] > 0, (int)((a.flags & GDBF_SMOOTH) && it > a.T - a.windowsize));
        if (last) a.frame_unc[b] = sums[1];
    }
};

// ---------------------------------------------------------------------
// rstat_wg: one workgroup per item (NgdbfWg, ngdbf_phase.h), with the trace rows.
// ---------------------------------------------------------------------
template <typename F, int SRC, bool TRACE>
__device__ __forceinline__ void rstat_wg_item(const RstatArgs &a, const DevGraph &g, int item, const NgdbfWg<F> &wg)
{
    const int N = g.N;
    const RstatItem I(a, item);
    const int8_t *cvec = frame_codeword<SRC>(a, I.b, N);
    const int unc = wg.template front<SRC>(a, I.b, N, cvec, I.y_out(a));
    NgdbfTrace tr;
    if (TRACE) tr = NgdbfTrace{a.err_trace, a.unsat_trace, a.d_trace, a.s_trace, I.row0};
    bool sat;
    const int it = wg.template phase<TRACE, CHK_RSTAT_BIT, CHK_RSTAT_PARITY>(
        a, g, cvec, tr, sat, [&](int it, int g4, F(&pv)[4]) { I.template draw<F, SRC>(a, N, it, g4, g4 * 4, pv); });
    int sums[3];
    wg.template finish<CHK_RSTAT_BIT>(a, g, cvec, sat, I.d_row(a, N), unc, sums);
    if (threadIdx.x == 0) I.account(a, sums, it);
    __syncthreads();
}

template <typename F, int SRC, bool TRACE>
__global__ __launch_bounds__(256) void k_rstat_wg(RstatArgs a, DevGraph g, RgdbfLayout L)
{
    ngdbf_wg_lds<F>(a, L, [&](int item, const NgdbfWg<F> &wg) { rstat_wg_item<F, SRC, TRACE>(a, g, item, wg); });
}

template <typename F, int SRC, bool TRACE>
__global__ __launch_bounds__(1024) void k_rstat_wg_global(RstatArgs a, DevGraph g, RgdbfLayout L, unsigned char *scratch,
                                                          int items)
{
    ngdbf_wg_global<F>(a, L, scratch, items,
                       [&](int item, const NgdbfWg<F> &wg) { rstat_wg_item<F, SRC, TRACE>(a, g, item, wg); });
}

// ---------------------------------------------------------------------
// rstat_rows: the register schedule (NgdbfRows, ngdbf_phase.h) with one phase per item.
// ---------------------------------------------------------------------
template <typename F, int SRC, int DVM, int NT>
__global__ __launch_bounds__(NT, 4) void k_rstat_rows(RstatArgs a, DevGraph g, int np, int poff, int floff, int items)
{
    using Rows = NgdbfRows<F, DVM, NT>;
    constexpr int BPT = Rows::BPT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int red[Rows::kRed];
    Rows R(a, g, smem, red, np, poff, floff);
    const int N = g.N;
    unsigned nxt = R.first_ticket(a.ticket);
    for (int item = blockIdx.x; item < items; item = R.next_item(a.ticket, items, nxt)) {
        const RstatItem I(a, item);
        const int8_t *cvec = frame_codeword<SRC>(a, I.b, N);
        // ---- channel + front-end (newstat.cpp:279-302), start from r (:310-316, :331-334) ----
        F yq[BPT], theta[BPT];
        int d[BPT], dsum[BPT];
        uint32_t rneg;
        const int unc = R.template front<SRC>(a, I.b, cvec, I.y_out(a), yq, rneg);
#pragma unroll
        for (int q = 0; q < BPT; ++q) {
            d[q] = (rneg >> q) & 1u ? -1 : 1;
            theta[q] = (F)a.theta0;
            dsum[q] = 0;
        }
        bool sat;
        const int it = R.template phase<CHK_RSTAT_BIT, CHK_RSTAT_PARITY>(
            0, yq, theta, d, dsum, sat, [&](int it, F(&pv)[BPT]) { I.template draw<F, SRC>(a, N, it, R.tid, R.v0, pv); });
        int sums[3];
        R.template finish<CHK_RSTAT_BIT>(cvec, sat, d, dsum, I.d_row(a, N), unc, sums);
        if (R.tid == 0) I.account(a, sums, it);
    }
}

// ---------------------------------------------------------------------
// Frame accounting behind the attempts (newstat.cpp:421-465): one thread per frame.
// ---------------------------------------------------------------------
__global__ void k_rstat_account(RstatArgs a)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.batch) return;
    const int4 *res = a.attempt_res + (size_t)b * a.attempts;
    int total = 0;
    for (int k = 0; k < a.attempts; ++k) total += res[k].y;
    const int4 lastr = res[a.attempts - 1];
    frame_account(a.counts, a.hist, a.frame_res, b, lastr.x, a.frame_unc[b], lastr.z, total, total);
}

// dynamic LDS of a workgroup: 64 KB less the kernels' static arrays (red, wtab)
constexpr size_t kRstatMaxLds = 64 * 1024 - 1024;

LDPC_CHECK_TU(rstat)

RstatChoice rstat_choose(const DevGraph &g, bool f64, bool trace, int maxdv, int maxdc)
{
    RstatChoice ch;
    if (!trace && rgdbf_rows_fits(g.N, g.M, maxdv, maxdc) && opt(LDPC_OPT_GDBF_KERNEL) != 1) {
        ch.name = "rstat_rows";
        ch.threads = g.N <= 4 * 512 && g.M <= 2 * 512 ? 512 : 1024;
        ch.dvm = maxdv <= 4 ? 4 : 12;
        ch.lds_bytes = rgdbf_rows_layout(g.N, g.M).total;
        return ch;
    }
    const RgdbfLayout L = rgdbf_layout(g.N, g.M, f64 ? 8 : 4);
    ch.name = "rstat_wg";
    if (L.total <= kRstatMaxLds) {
        ch.lds_bytes = (int)L.total;
        ch.threads = 256;
    } else {
        ch.threads = 1024;
        ch.slot_bytes = L.total;
    }
    return ch;
}

template <typename F, int SRC, bool TRACE>
static hipError_t rstat_wg_launch(const DevGraph &g, const RstatArgs &a, const RstatChoice &ch, void *scratch, int slots,
                                  hipStream_t s)
{
    const RgdbfLayout L = rgdbf_layout(g.N, g.M, sizeof(F));
    const int items = a.batch * a.attempts;
    if (ch.lds_bytes > 0) {
        hipLaunchKernelGGL((k_rstat_wg<F, SRC, TRACE>), dim3(items), dim3(ch.threads), ch.lds_bytes, s, a, g, L);
    } else {
        const int grid = slots < items ? slots : items;
        if (grid <= 0 || !scratch) return hipErrorInvalidValue;
        hipLaunchKernelGGL((k_rstat_wg_global<F, SRC, TRACE>), dim3(grid), dim3(ch.threads), 0, s, a, g, L,
                           (unsigned char *)scratch, items);
    }
    return hipGetLastError();
}

hipError_t rstat_launch(const DevGraph &g, const RstatArgs &a, bool f64, const RstatChoice &ch, void *scratch, int slots,
                        int num_cus, hipStream_t s)
{
    if (a.batch <= 0 || a.attempts <= 0) return hipSuccess;
    if (!a.attempt_res || !a.frame_unc) return hipErrorInvalidValue;
    const hipError_t e = gdbf_dispatch(f64, a.src, [&](auto f, auto src) {
        using F = decltype(f);
        constexpr int SRC = decltype(src)::value;
        if (ch.dvm) {
            const RgdbfRowsLayout L = rgdbf_rows_layout(g.N, g.M);
            const int items = a.batch * a.attempts;
            return gdbf_rows_dispatch(ch, [&](auto dvm, auto nt) {
                return gdbf_rows_grid_launch(k_rstat_rows<F, SRC, decltype(dvm)::value, decltype(nt)::value>,
                                             decltype(nt)::value, L.total, a.ticket, true, items, num_cus, s, a, g, L.np,
                                             L.poff, L.floff, items);
            });
        }
        const bool trace = a.err_trace || a.unsat_trace || a.d_trace || a.s_trace;
        return trace ? rstat_wg_launch<F, SRC, true>(g, a, ch, scratch, slots, s)
                     : rstat_wg_launch<F, SRC, false>(g, a, ch, scratch, slots, s);
    });
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_rstat_account, dim3((a.batch + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace ldpc
