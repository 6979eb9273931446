// wave_cw_plan.h -- the launch shape of a decoder whose wavefronts each own a codeword (hwgdbf,
// fxms, fxlms), planned on the host: plain C++ with no HIP include, so that
// tests/native/wave_cw_host.cpp compiles it and the families' *_layout.h with g++.
#pragma once
#include <cstddef>

namespace ldpc {

constexpr size_t kWaveCwLds = 160 * 1024;   // LDS one workgroup may use (kMaxLds of kernels.h; wave_cw.h asserts it)

// Byte offsets of the LDS layouts: 16-byte aligned, and an int that saturates (a size past
// 2 GB is refused by its 64 KB bound, not wrapped).
inline long long lds_al16(long long x) { return (x + 15) & ~15ll; }
inline int lds_cap(long long x) { return x > 0x7fffffffll ? 0x7fffffff : (int)x; }

struct WaveCwSizes {
    int N, M, dcs, E;   // the graph's bits, checks, row stride (max(maxdc, 1)) and edges
};

// What a family's *_choose returns; each adds the bool that names its kernel instance.
struct WaveCwChoice {
    const char *name = "";   // empty: one codeword's state does not fit
    int lds_bytes = 0;       // dynamic LDS of a workgroup
    int cw_bytes = 0;        // state bytes of one codeword
    int threads = 0, cw_per_block = 0;
    bool staged = false;     // the graph sits in LDS beside the codewords (lds_bytes includes it)
};

// Waves a CU holds: workgroups by LDS (each carries the staged graph and 128 bytes of slack)
// times the waves of one, up to the instances' register bound `cap`; 0 where one does not fit.
inline int wave_cw_waves(size_t graph_bytes, size_t cw_bytes, int cw_per_block, int waves_per_block, int cap)
{
    const size_t wg = graph_bytes + cw_bytes * cw_per_block + 128;
    if (wg > kWaveCwLds) return 0;
    const int waves = (int)(kWaveCwLds / wg) * waves_per_block;
    return waves < cap ? waves : cap;
}

struct WaveCwPlan {
    int waves = 0, cw_per_block = 0;   // 0, 0: not even one codeword fits beside the graph
};
// Codewords (waves) per workgroup, 1..16, that keep most waves on a CU. A tie goes to the
// larger workgroup, which stages the graph fewer times, or to the smaller one.
inline WaveCwPlan wave_cw_plan(size_t graph_bytes, size_t cw_bytes, int cap, bool tie_to_larger)
{
    WaveCwPlan p;
    for (int c = 1; c <= 16; ++c) {
        const int w = wave_cw_waves(graph_bytes, cw_bytes, c, c, cap);
        if (w == 0) break;
        if (tie_to_larger ? w >= p.waves : w > p.waves) p = {w, c};
    }
    return p;
}

}  // namespace ldpc
