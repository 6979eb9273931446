// nb_layout.h -- constants and message-layout arithmetic of the GF(q) EMS kernels
// shared by the device code (nb.hip) and the host-only graph code (nb_graph.cpp),
// which is also built without HIP for the host sanitizer (Makefile `asan`).
#pragma once
#include <cstddef>

#if defined(__HIPCC__) || defined(__HIP__)
#define LDPC_NB_HD __host__ __device__
#else
#define LDPC_NB_HD
#endif

namespace ldpc {

constexpr int kNbQ = 16;          // the field of BASELINE config 5; the kernels are also built for GF(4) and GF(8)
constexpr int kNbMaxDc = 8;       // row degree bound (DC template 4 / 8)
constexpr size_t kNbMaxLds = 160 * 1024;

// field sizes k_ems is instantiated for (nb.hip nb_launch)
LDPC_NB_HD inline bool nb_q_supported(int q) { return q == 4 || q == 8 || q == 16; }

// Position-major message slot count (maxdc * M) rounded up to a power of two
// (at least 4): the chunk stride of the message layout of nb.hip, where the byte
// offset of entry p of slot s is (s << 4) ^ nb_lambda(p) -- XOR-linear in p.
LDPC_NB_HD inline int nb_ep(int maxdc, int M)
{
    int e = 4;
    while (e < maxdc * M) e <<= 1;
    return e;
}
LDPC_NB_HD inline int nb_ep_log2(int ep)
{
    int k = 0;
    while ((1 << k) < ep) ++k;
    return k;
}
// Byte offset of entry p (0..q-1) relative to its slot's s << 4, chunk stride 2^k slots:
// chunk p >> 2 at (p >> 2) << (k + 4), the slot XOR-ed with the chunk index (bits 4-5),
// the entry within its 16-byte chunk at (p & 3) << 2. A slot has q / 4 chunks -- one
// for GF(4), two for GF(8), four for GF(16) -- so the same function serves every q
// (p < q keeps the chunk index below q / 4) and a codeword's messages take nb_ep * q * 4 bytes.
LDPC_NB_HD inline int nb_lambda(int p, int k) { return (p << 2) ^ ((p >> 2) << (k + 4)); }

// LDS of one workgroup and the kernel that follows from it (nb.hip k_ems, nb_choose).
// State, written per codeword: [lam N*m f32] [dec N u8] [synd ceil(M/4) u32] [red 72 i32].
// Schedule, read only:         [cn_d M u8] [vn N u32] [vslot E u16] [vh E u8].
// ems_lds keeps messages, state and schedule in LDS; ems_global moves the messages to
// a global slot per workgroup; ems_global_sched also leaves the schedule in its device
// copy and is chosen only where state + schedule exceed LDS.
LDPC_NB_HD inline size_t nb_align16(size_t x) { return (x + 15) & ~(size_t)15; }
LDPC_NB_HD inline size_t nb_state_bytes(int N, int M, int m)
{
    return nb_align16((size_t)N * m * 4) + nb_align16((size_t)N) + nb_align16((size_t)(M + 3) / 4 * 4) +
           (16 * 3 + 16 + 4 + 4) * 4;
}
LDPC_NB_HD inline size_t nb_sched_bytes(int N, int M, int E)
{
    return nb_align16((size_t)M) + nb_align16((size_t)N * 4) + nb_align16((size_t)E * 2) + nb_align16((size_t)E);
}
enum NbKind { NB_NONE = 0, NB_LDS, NB_GLOBAL, NB_GLOBAL_SCHED };
struct NbPlan {
    int kind = NB_NONE;
    size_t lds_bytes = 0, slot_bytes = 0;
};
LDPC_NB_HD inline NbPlan nb_plan(int N, int M, int E, int q, int m, int maxdc)
{
    NbPlan p;
    const size_t state = nb_state_bytes(N, M, m), aux = state + nb_sched_bytes(N, M, E);
    const size_t msgb = nb_align16((size_t)nb_ep(maxdc, M) * q * 4);
    // The 16-bit schedule entries are the slot indices (< maxdc * M: vslot) and the
    // symbols (< N); the chunk stride Ep (maxdc * M rounded up to a power of two, up to
    // 65 536) only enters int offsets.
    if (maxdc > kNbMaxDc || state > kNbMaxLds || (long)maxdc * M > 65535 || N > 65535) return p;
    p.kind = aux + msgb <= kNbMaxLds ? NB_LDS : aux <= kNbMaxLds ? NB_GLOBAL : NB_GLOBAL_SCHED;
    p.lds_bytes = p.kind == NB_LDS ? aux + msgb : p.kind == NB_GLOBAL ? aux : state;
    p.slot_bytes = p.kind == NB_LDS ? 0 : msgb;
    return p;
}

}  // namespace ldpc
