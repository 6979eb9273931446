// fxlms_layout.h -- LDS layout and launch shape of the layered fixed-point min-sum kernel
// (fxlms.hip), on the host (no HIP include: wave_cw_plan.h). State of a codeword:
//   app[N] (int8 when app_bits <= 8, else int16) | S0[M] | S1[M] (row degree > 26 only) | MG[M]
// and, staged before the codewords, the schedule: the rows' bits as 16-bit indices slot-major,
// then the rows' degrees. Below them, the shape of the workgroup-per-codeword kernel (fxlms_wg.hip).
#pragma once
#include "fxms_layout.h"

namespace ldpc {

struct FxlmsLayout {
    int slots;                       // dcs * M schedule entries
    int s0off, s1off, mgoff, total;  // of one codeword, bytes
    int hi;                          // row degree > 26: S1 exists
    int gdoff, cwoff;                // STAGE: byte offset of the degrees, of the first codeword
};
inline FxlmsLayout fxlms_layout(const WaveCwSizes &z, bool wide)
{
    FxlmsLayout L;
    const long long slots = (long long)z.M * z.dcs;
    L.hi = z.dcs > 26;
    const long long s0 = lds_al16((long long)z.N * (wide ? 2 : 1)), s1 = s0 + lds_al16(4ll * z.M),
                    mg = s1 + (L.hi ? lds_al16(4ll * z.M) : 0), t = mg + lds_al16((long long)z.M * (wide ? 4 : 2));
    L.slots = lds_cap(slots);
    L.s0off = lds_cap(s0);
    L.s1off = lds_cap(s1);
    L.mgoff = lds_cap(mg);
    L.total = lds_cap(t);
    const long long gd = lds_al16(2 * slots), cw = gd + lds_al16(z.M);
    L.gdoff = lds_cap(gd);
    L.cwoff = lds_cap(cw);
    return L;
}

// name: "fxlms_i8" | "fxlms_i16" (fxlms.hip) or "fxlms_wg_i8" | "fxlms_wg_i16" (fxlms_wg.hip);
// wide: int16 APPs, 15-bit magnitudes (app_bits > 8)
struct FxlmsChoice : FxmsChoice {
    bool wg = false;      // a workgroup per codeword (fxlms_wg.hip): lds_bytes holds the APPs, and
    int slot_bytes = 0;   // the packed row state sits in a global slot of this size per workgroup
};

constexpr int kFxlmsMaxLds = 64 * 1024;   // one codeword's state must fit (the fxms bound)

// Up to 32 waves per CU; a tie goes to the larger workgroup. The schedule goes into LDS when
// its indices fit 16 bits and the copy costs at most a quarter of the waves a CU would hold
// without it (the kernel hides LDS and instruction latency with resident waves only).
inline FxlmsChoice fxlms_plan(const WaveCwSizes &z, int app_bits)
{
    FxlmsChoice ch;
    ch.wide = app_bits > 8;
    const FxlmsLayout L = fxlms_layout(z, ch.wide);
    ch.cw_bytes = L.total;
    if (L.total > kFxlmsMaxLds) return ch;   // name stays empty: the caller reports the bound
    const WaveCwPlan pu = wave_cw_plan(0, L.total, 32, true);
    const WaveCwPlan ps = z.N <= 65535 && L.cwoff < (int)kWaveCwLds ? wave_cw_plan(L.cwoff, L.total, 32, true) : WaveCwPlan{};
    ch.staged = ps.waves > 0 && 4 * ps.waves >= 3 * pu.waves;
    const int gb = ch.staged ? L.cwoff : 0;
    ch.name = ch.wide ? "fxlms_i16" : "fxlms_i8";
    ch.cw_per_block = ch.staged ? ps.cw_per_block : pu.cw_per_block;
    ch.threads = 64 * ch.cw_per_block;
    ch.lds_bytes = gb + L.total * ch.cw_per_block;
    return ch;
}

// ---- A workgroup per codeword (fxlms_wg.hip): LDS holds kFxlmsWgRed bytes of
// reduction and ticket words and behind them app[N]; the packed row state S0[M] | S1[M] (row
// degree > 26 only) | MG[M], indexed by layered position, sits in a global slot per workgroup.
constexpr int kFxlmsWgRed = 256;   // 32 words of block sums, 16 of wave flags, the next codeword
constexpr long long kFxlmsWgSlotAlign = 256;

struct FxlmsWgLayout {
    int s1off, mgoff, slot_bytes;   // of a workgroup's global slot, bytes (S0 at 0)
    int hi;                         // row degree > 26: S1 exists
};
inline FxlmsWgLayout fxlms_wg_layout(const WaveCwSizes &z, bool wide)
{
    auto al = [](long long x) { return (x + kFxlmsWgSlotAlign - 1) & ~(kFxlmsWgSlotAlign - 1); };
    FxlmsWgLayout L;
    L.hi = z.dcs > 26;
    const long long s1 = al(4ll * z.M), mg = s1 + (L.hi ? al(4ll * z.M) : 0), t = mg + al((long long)z.M * (wide ? 4 : 2));
    L.s1off = lds_cap(s1);
    L.mgoff = lds_cap(mg);
    L.slot_bytes = lds_cap(t);
    return L;
}

// The name is empty where kFxlmsWgRed + N APPs exceed the LDS of a workgroup (cw_bytes has the
// sum). LDS decides how many codewords a CU holds; each gets its share of the 16 waves a CU
// runs of this kernel (1024 threads over the workgroups LDS admits), 64 threads at least.
inline FxlmsChoice fxlms_wg_plan(const WaveCwSizes &z, int app_bits)
{
    FxlmsChoice ch;
    ch.wg = true;
    ch.wide = app_bits > 8;
    const long long need = kFxlmsWgRed + (long long)z.N * (ch.wide ? 2 : 1);
    ch.cw_bytes = lds_cap(need);
    if (need > (long long)kWaveCwLds) return ch;   // name stays empty: the caller reports the bound
    ch.name = ch.wide ? "fxlms_wg_i16" : "fxlms_wg_i8";
    ch.lds_bytes = (int)lds_al16(need);
    ch.cw_per_block = 1;
    const int t = (1024 / (int)(kWaveCwLds / (size_t)ch.lds_bytes)) & ~63;   // the kernel has no static LDS
    ch.threads = t < 64 ? 64 : t;
    ch.slot_bytes = fxlms_wg_layout(z, ch.wide).slot_bytes;
    return ch;
}

}  // namespace ldpc
