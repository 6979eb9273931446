// fxms_layout.h -- LDS layout and launch shape of the fixed-point min-sum kernel (fxms.hip), on
// the host (no HIP include: wave_cw_plan.h). State of a codeword:
//   msg[dcs * M] (int8 when msg_bits <= 8, else int16) | Y[N] (int8) | D[N] (the decisions)
// and, staged before the codewords, the graph as 16-bit indices: the checks' bits slot-major,
// then the slot of every column edge.
#pragma once
#include "wave_cw_plan.h"

namespace ldpc {

struct FxmsLayout {
    int slots;                 // dcs * M message slots
    int yoff, doff, total;     // of one codeword, bytes
    int E, gcoff, cwoff;       // STAGE: edges, byte offset of the column edges' slots, of the first codeword
};
inline FxmsLayout fxms_layout(const WaveCwSizes &z, bool wide)
{
    FxmsLayout L;
    const long long slots = (long long)z.M * z.dcs;
    const long long y = lds_al16(slots * (wide ? 2 : 1)), d = y + lds_al16(z.N), t = d + lds_al16(z.N);
    L.slots = lds_cap(slots);
    L.yoff = lds_cap(y);
    L.doff = lds_cap(d);
    L.total = lds_cap(t);
    L.E = z.E;
    const long long gc = lds_al16(2 * slots), cw = gc + lds_al16(2ll * z.E);
    L.gcoff = lds_cap(gc);
    L.cwoff = lds_cap(cw);
    return L;
}

struct FxmsChoice : WaveCwChoice {   // name: "fxms_i8" | "fxms_i16"
    bool wide = false;               // int16 messages (msg_bits > 8)
};

constexpr int kFxmsMaxLds = 64 * 1024;   // one codeword's state must fit (the hwgdbf bound)

// Up to 28 waves per CU (7 per SIMD at the kernel's 64 VGPRs); a tie goes to the larger workgroup.
inline FxmsChoice fxms_plan(const WaveCwSizes &z, int msg_bits)
{
    FxmsChoice ch;
    ch.wide = msg_bits > 8;
    const FxmsLayout L = fxms_layout(z, ch.wide);
    ch.cw_bytes = L.total;
    if (L.total > kFxmsMaxLds) return ch;   // name stays empty: the caller reports the bound
    // the 16-bit graph beside the codewords, when the indices fit 16 bits and it leaves room for a codeword
    ch.staged = z.N <= 65535 && (long long)z.M * z.dcs <= 65536 && (size_t)L.cwoff + (size_t)L.total + 128 <= kWaveCwLds;
    const int gb = ch.staged ? L.cwoff : 0;
    ch.name = ch.wide ? "fxms_i16" : "fxms_i8";
    ch.cw_per_block = wave_cw_plan(gb, L.total, 28, true).cw_per_block;
    if (ch.cw_per_block < 1) ch.cw_per_block = 1;
    ch.threads = 64 * ch.cw_per_block;
    ch.lds_bytes = gb + L.total * ch.cw_per_block;
    return ch;
}

}  // namespace ldpc
