// kernels.h -- internal launch interface between api.cpp and the min-sum kernel files
// (kernels.hip, rows.hip, rows_es.hip, rows_fast.hip, rows_pp.hip, flood.hip, layered.hip).
#pragma once
#include "options.h"
#include <hip/hip_runtime.h>
#include <cstdint>

namespace ldpc {

struct DevGraph {
    int N, M, dcs;                  // dcs = row stride of row_cols (max(maxdc,1))
    const int32_t *row_cols;        // [M * dcs]
    const uint8_t *row_deg;         // [M]
    const int32_t *col_ptr;         // [N + 1]
    const uint32_t *col_refs;       // [E]  (check << 6) | position
};

enum { SRC_GIVEN = 0, SRC_PHILOX = 1 };
enum { VARIANT_BP = 3, VARIANT_DDBMP = 4 };   // ldpc_variant LDPC_BP, LDPC_DDBMP

struct DecodeArgs {
    int batch, T, variant, quantize, saturate;
    int early_stop;                 // MS / NMS / OMS / BP: stop at the first t in 0..T whose decisions are a codeword
    double ymax, nq, alpha, delta;
    double n0, max_llr;             // BP front-end: yq = 4*y/n0 clipped to +-max_llr
    // fp32 NMS: q = x*r, q += fma(-q, alpha, x)*r equals x/alpha for every
    // finite float x (verified on the device by verify_div_by_reciprocal)
    int nms_fast;
    float alpha_rcp;
    int src;
    const void *y;                  // SRC_GIVEN: [batch][N] float|double (device)
    const int8_t *c;                // SRC_GIVEN: [batch][N] bipolar, or null (+1)
    const int8_t *cw_table;         // SRC_PHILOX: [cw_rows][N] bipolar, or null
    int cw_rows;
    uint64_t seed, first_cw;
    uint32_t stream_id;
    double sigma;
    int8_t *d_out;                  // [batch][N] or null
    void *y_out;                    // SRC_PHILOX: channel samples [batch][N] F (pre front-end) or null
    int4 *frame_res;                // [batch] {bit_err, uncoded, syndrome_fail, iterations (DD-BMP, early_stop; else 0)} or null
    unsigned long long *counts;     // [6] accumulated
    unsigned long long *hist;       // [N] accumulated (weight w -> hist[w-1])
    unsigned long long *stamps;     // diagnostic builds (-DLDPC_STAMPS): [grid][4] cycle sums, else null
};

// Device copy of graph.h's RowSchedule (row-parallel kernel).
struct RowSched {
    int threads, cpt, dc, e_pad, rpt;
    int dc_low;                     // > 0: degree-aware row slots (graph.h pp_row_slots)
    const uint16_t *cn_cols;       // [threads * rpt * dc]  (row j = thread j % threads, r = j / threads)
    const uint16_t *cn_pos;         // [threads * rpt * dc]
    const uint8_t *cn_deg;          // [threads * rpt]
    const uint16_t *vn_col;         // [threads * cpt]
    const uint32_t *vn_info;        // [threads * cpt]
    // the in-register schedule only (graph.h build_pp_inreg_schedule; null / 0 elsewhere)
    const uint8_t *pair;            // [threads + threads / 64] per thread: bit 0 paired, bit 1 row 1 first; per wave: 1 = no LDS at the last positions
    int e_used;                     // padded bit-slot edges of its layout (e_pad is the split schedule's: same LDS partition)
    int n_inreg;                    // in-register bits
    int lds_edge_slots;             // check-edge slots that pass through LDS per codeword-iteration
};

// Device copy of graph.h's FloodSchedule (global-memory flooding kernel).
struct FloodSched {
    int M_pad, dc, ngroups, e_pad;
    int dv;                         // max column degree
    const int32_t *sp, *sq;         // [dc * M_pad] slot-major bit position / c2v element
    const uint8_t *rdeg;            // [M_pad]
    const int32_t *pos_of_bit;      // [N]
    const int32_t *bit_at;          // [ngroups * 64]
    const uint8_t *pdeg;            // [ngroups * 64]
    const int32_t *gbase;           // [ngroups]
    const uint32_t *eref;           // [e_pad + 64] per c2v element: (row << 5) | position in the row
};

// Device copy of graph.h's LayerSchedule.
struct LayerSched {
    int nlayers = 0, max_layer = 0, M_pad = 0;
    const int32_t *lptr = nullptr;  // [nlayers + 1] layered row positions of each layer
    const int32_t *sp = nullptr;    // [dc * M_pad] slot-major layered positions (graph.h LayerSchedule)
    const uint8_t *rdeg = nullptr;  // [M_pad]
    const int32_t *pos_of_bit = nullptr;   // [N] layered position of each bit
};

// What a plan can launch: one value per kernel family member.
enum class Kernel {
    rows, rows_fast, rows_pp,           // row graphs (rows.hip, rows_fast.hip, rows_pp.hip)
    rows_es,                            // row graphs with early termination (rows_es.hip)
    lds, global,                        // one workgroup per codeword (kernels.hip)
    flood_persistent, flood_phase,      // codes beyond LDS (flood.hip); both report "flood"
    layered_lds, layered_global,        // layered schedule (layered.hip)
    bp_rows, bp_lds, bp_global,         // belief propagation (bp.hip)
    ddbmp_rows, ddbmp_lds, ddbmp_global // DD-BMP (ddbmp.hip)
};

// Everything one decode launch of the binary context needs, decided once (api.cpp
// build_plan composes the families' plan_*): run_kernel sizes the scratch and launches
// from it, ldpc_ctx_kernel_info / ldpc_ctx_row_sched_info report it.
struct LaunchPlan {
    Kernel kernel = Kernel::global;
    const char *name = "";          // as reported: "rows", "rows_fast", "rows_pp", "rows_es", "lds", "flood", "global", ...
    const void *fn = nullptr;       // the instantiation that launches (null: flood_phase, a launch per phase)
    int threads = 0;
    int lds_bytes = 0;              // dynamic LDS per block that holds decoder state, as reported
    int layered_pos = 0;            // layered_global: P, the posteriors of the global slot cached in LDS,
    int cache_lds_bytes = 0;        //   and their dynamic LDS (P + the dummy slot, fp64 only); not reported
    int pad_lds_bytes = 0;          // rows_pp on the 12-wave block: the gaps of its fixed-stride LDS layout; not reported
    int cw_per_block = 1;           // row kernels: codewords decoded together per thread (as reported)
    int blocks_per_cu = 0;          // as reported; sizes the grid of the kernels that work in global scratch
    int grid = 0;                   // blocks of the launch; flood_phase: resident slots K
    size_t scratch_per_block = 0;   // global scratch slot of one block / resident codeword
    size_t scratch_bytes = 0;       // scratch the launch needs in all
    const RowSched *rs = nullptr;   // the row schedule the plan describes (the context's rs or rs_pp)
    const RowSched *rs_inreg = nullptr;   // rows_pp: the in-register schedule the kernel reads instead (k_rows_ppi)
    bool redo = false;              // fast row kernels: a redo list goes in and launch_redo follows
};

// What the planners read. Options come through opt() (the caller's OptScope).
struct PlanInput {
    const DevGraph &g;
    int E;
    const RowSched *rs, *rs_pp;     // null where the graph admits none
    const FloodSched *fs;           // null: none
    const LayerSched *ls;           // null: none
    int num_cus;
    const DecodeArgs &a;            // after nms_setup; a.batch sizes the grid
    bool f64;
    int maxdv = 0;                  // the code's largest column degree (plan_ddbmp)
    const RowSched *rs_ppi = nullptr;   // the ping-pong kernel's in-register schedule (null: the code has no row pair)
};

// The (precision, sample source) template axes every kernel has: fn(type_tag<F>{}, src_tag<SRC>{}).
template <typename T> struct type_tag { using type = T; };
template <int V> struct src_tag { static constexpr int value = V; };
template <class Fn>
auto for_f_src(bool f64, int src, Fn &&fn)
{
    if (f64)
        return src == SRC_GIVEN ? fn(type_tag<double>{}, src_tag<SRC_GIVEN>{}) : fn(type_tag<double>{}, src_tag<SRC_PHILOX>{});
    return src == SRC_GIVEN ? fn(type_tag<float>{}, src_tag<SRC_GIVEN>{}) : fn(type_tag<float>{}, src_tag<SRC_PHILOX>{});
}

constexpr size_t kMaxLds = 160 * 1024;   // LDS one workgroup may use

// Blocks of `fn` a CU holds at this shape (the dynamic LDS limit raised first); 0 on error.
int occupancy(const void *fn, int threads, int lds_bytes);
// One launch of plan.fn over plan.grid blocks with the plan's threads and dynamic LDS.
hipError_t launch_fn(const LaunchPlan &p, void **args, hipStream_t s);

// Each plan_* fills `p` and returns true when its kernel decodes the input; the order in
// which api.cpp build_plan asks them is the preference order.
//
// kernels.hip: state in LDS ("lds") or in a global slot per block ("global", always possible).
bool plan_lds(const PlanInput &in, LaunchPlan &p);
void plan_global(const PlanInput &in, LaunchPlan &p);
hipError_t launch_generic(const LaunchPlan &p, const DevGraph &g, const DecodeArgs &a, void *gscratch, hipStream_t s);
// rows.hip: the row kernel, or one of the fast row kernels where they apply (rows_fast.hip,
// rows_pp.hip: plan_rows_fast / plan_rows_pp amend the row kernel's plan).
bool plan_rows(const PlanInput &in, LaunchPlan &p);
hipError_t launch_rows(const LaunchPlan &p, const DevGraph &g, const DecodeArgs &a, hipStream_t s);
// rows_es.hip: the row kernel with early termination (DecodeArgs.early_stop), codewords by
// ticket (a zeroed word of the context; the launch clears it).
bool plan_rows_es(const PlanInput &in, LaunchPlan &p);
hipError_t launch_rows_es(const LaunchPlan &p, const DevGraph &g, const DecodeArgs &a, unsigned *ticket, hipStream_t s);
// flood.hip: codes whose state exceeds LDS (row degree <= kPackedMaxDc), persistent or one
// launch per phase over an Infinity-Cache-resident set of plan.grid codewords.
// aux (may be null): a second stream with fork/join events; the resident set is
// then split in two halves, one per stream, so one half's launch boundaries
// overlap the other half's kernels.
struct AuxStream {
    hipStream_t s = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
};
bool plan_flood(const PlanInput &in, LaunchPlan &p);
hipError_t launch_flood(const LaunchPlan &p, const DevGraph &g, const FloodSched &fs, const DecodeArgs &a, bool f64,
                        void *gscratch, hipStream_t s, const AuxStream *aux);
// layered.hip (k_decode_layered_*): state in LDS when it fits ("layered_lds"), else in a
// global slot per block ("layered_global"). Requires the flood schedule (row order,
// storage order) and row degree <= kPackedMaxDc.
void plan_layered(const PlanInput &in, LaunchPlan &p);
hipError_t launch_layered(const LaunchPlan &p, const DevGraph &g, const FloodSched &fs, const LayerSched &ls,
                          const DecodeArgs &a, void *gscratch, hipStream_t s);
// Packed check state of the flood and layered kernels: a 5-bit argmin and one
// sign bit per edge in a 32-bit meta word.
constexpr int kPackedMaxDc = 26;

// Exhaustive device check that dividing by alpha through its correctly rounded
// reciprocal plus one FMA correction step reproduces IEEE x/alpha for all
// 2^31 - 2^23 finite non-negative floats x (the only operands the check-node
// normalisation divides: |v2c| minima). *mismatches receives the count.
hipError_t verify_div_by_reciprocal(float alpha, float rcp, unsigned long long *mismatches_dev, hipStream_t s);

// Fast-path row kernel (rows_fast.hip): fp64 (one codeword per block) and fp32
// (a pair, dc <= 8), same LDS layout and schedule as the "rows" kernel
// (lds_bytes of its plan), check node compiled per variant; codeword
// groups whose premise fails are appended to redo (redo[0] = count, must be 0
// at launch; redo[1..] batch indices, capacity batch), and launch_redo
// (kernels.hip) decodes them on the exact path. fp32 takes it only for MS and
// for NMS with the verified reciprocal (rows_fast_f32_ok, after nms_setup).
// plan_rows_fast: p is the row kernel's plan; true and amended when the fast kernel decodes it.
bool plan_rows_fast(const PlanInput &in, LaunchPlan &p);
bool rows_fast_f32_ok(const DecodeArgs &a);
hipError_t launch_rows_fast(const LaunchPlan &p, const DevGraph &g, const DecodeArgs &a, unsigned *redo, hipStream_t s);
// alpha for which the fast fp64 NMS division x*r + one fma correction is exact
bool markstein_exact_alpha(double alpha);
size_t redo_lds_bytes(const DevGraph &g, bool f64);
hipError_t launch_redo(const DevGraph &g, const DecodeArgs &a, bool f64, const unsigned *redo, hipStream_t s,
                       int num_cus);

// Ping-pong row kernel (rows_pp.hip): two slots per 1024-thread block -- an
// fp64 codeword or an fp32 pair (float2) each -- check waves and bit waves
// overlapped (schedule: 512 threads, 2 rows and 4 bit slots each, dc 8, the
// degree-aware row slots when rs.dc_low == 7); redo as above (fp32: MS and NMS
// with the verified reciprocal, rows_fast_f32_ok). plan_rows_pp: as plan_rows_fast.
// With PlanInput.rs_ppi (fp64, LDPC_OPT_PP_SLOTS 0) the launch is k_rows_ppi: the degree-2
// bits that join a check thread's two rows stay in that thread's registers (graph.h
// pp_pair_rows); the plan still describes the split schedule it is derived from. Where the
// code fits the fixed-stride LDS layout that launch is k_rows_ppw: a 768-thread block, the same
// 8 check waves and 4 bit waves (LDPC_OPT_PP_SLOTS 3: k_rows_ppi always).
bool plan_rows_pp(const PlanInput &in, LaunchPlan &p);
// Whether k_rows_ppw's fixed-stride LDS layout holds a code of N bits whose split schedule has
// e_pad padded edge slots; *lds_bytes (may be null): the dynamic LDS that layout takes.
bool pp_w12_layout(int N, int e_pad, int *lds_bytes);
// Bit slots per thread of the in-register schedule: 3 where the bits left fit 3 x 512 slots
// in at most 24 groups (the bench code: 1458 bits, 23 groups), else 4 as in the schedule it
// derives from. LDPC_PP_INREG_CPT = 4 (A/B builds): always 4.
#ifndef LDPC_PP_INREG_CPT
#define LDPC_PP_INREG_CPT 3
#endif
hipError_t launch_rows_pp(const LaunchPlan &p, const DevGraph &g, const DecodeArgs &a, unsigned *redo, hipStream_t s);

// Row-kernel template bounds (host picks the smallest that fits).
constexpr int kRowsMaxThreads = 1024;
constexpr int kRowsCpt[] = {2, 4, 8};
// rows per thread -> block threads cap
constexpr int kRowsMaxThreadsForRpt[] = {0, 1024, 512, 384};
constexpr int kRowsDc[] = {8, 16, 32};

}  // namespace ldpc
