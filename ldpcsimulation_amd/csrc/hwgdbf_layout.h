// hwgdbf_layout.h -- LDS layout and launch shape of the NGDBFhw kernels (hwgdbf.hip), on the
// host (no HIP include: wave_cw_plan.h). State of a codeword, bytes:
//   Y[N] (int8) | Q[qlen] (int8) | D[N] (bit 0: d, bit 1: the channel decision) | S[M] parity
// and, staged before the codewords, the graph as 16-bit indices: the checks' bits slot-major,
// then the bits' checks in column order.
#pragma once
#include "wave_cw_plan.h"

namespace ldpc {

struct HwgdbfLayout {
    int qoff, doff, soff, total;   // of one codeword
    int E, gcoff, cwoff;           // STAGE: edges, byte offset of the bits' checks, of the first codeword
};
inline HwgdbfLayout hwgdbf_layout(const WaveCwSizes &z, int qlen)
{
    HwgdbfLayout L;
    const long long q = lds_al16(z.N), d = q + lds_al16(qlen), s = d + lds_al16(z.N), t = s + lds_al16(z.M);
    L.qoff = lds_cap(q);
    L.doff = lds_cap(d);
    L.soff = lds_cap(s);
    L.total = lds_cap(t);
    L.E = z.E;
    const long long gc = lds_al16(2ll * z.M * z.dcs), cw = gc + lds_al16(2ll * z.E);
    L.gcoff = lds_cap(gc);
    L.cwoff = lds_cap(cw);
    return L;
}

struct HwgdbfChoice : WaveCwChoice {   // name: "hwgdbf_wave" | "hwgdbf_wg"
    bool wave = false;                 // a wavefront per codeword
};

constexpr int kHwgdbfMaxLds = 64 * 1024;   // the codewords of a workgroup; one codeword's state must fit

// The shape that keeps more waves on a CU, up to the instances' register bound (5 waves per
// SIMD for the wavefront shape's 84-92 VGPRs, 6 for the workgroup shape's 62-77); a tie goes to
// the wavefront shape, and among its workgroup sizes to the smaller: both shapes are
// latency-bound, and the measured A/B follows the count. force_wg: option
// LDPC_OPT_GDBF_KERNEL = 1; wg_competes = false: the LDPC_HWGDBF_FORCE_WAVE A/B builds.
inline HwgdbfChoice hwgdbf_plan(const WaveCwSizes &z, int qlen, bool force_wg, bool wg_competes = true)
{
    HwgdbfChoice ch;
    const HwgdbfLayout L = hwgdbf_layout(z, qlen);
    ch.cw_bytes = L.total;
    if (L.total > kHwgdbfMaxLds) return ch;   // name stays empty: the caller reports the bound
    // the 16-bit graph beside the codewords, when the indices fit 16 bits and it leaves room for a codeword
    ch.staged = z.N <= 65535 && z.M <= 65535 && (size_t)L.cwoff + (size_t)L.total + 128 <= kWaveCwLds;
    const int gb = ch.staged ? L.cwoff : 0;
    const WaveCwPlan pw = wave_cw_plan(gb, L.total, 20, false);
    const int wg_w = wg_competes ? wave_cw_waves(gb, L.total, 1, 4, 24) : 0;
    if (force_wg || wg_w > pw.waves) {
        ch.name = "hwgdbf_wg";
        ch.cw_per_block = 1;
        ch.threads = 256;
    } else {
        ch.name = "hwgdbf_wave";
        ch.wave = true;
        ch.cw_per_block = pw.cw_per_block < 1 ? 1 : pw.cw_per_block;
        ch.threads = 64 * ch.cw_per_block;
    }
    ch.lds_bytes = gb + L.total * ch.cw_per_block;
    return ch;
}

}  // namespace ldpc
