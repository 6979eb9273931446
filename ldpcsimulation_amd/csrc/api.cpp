// api.cpp -- C ABI of libldpc_hip.so (include/ldpc_hip.h).
//
// Owns the binary context's device state (graph and schedule uploads, staging
// buffers) on top of the runtime it shares with nb_api.cpp (host_rt.h: errors,
// staging, CtxCore) and maps the reference's per-frame loop onto batched kernel
// launches. No C++ exception crosses the ABI; every HIP failure becomes
// LDPC_ERR_DEVICE with a message in ldpc_last_error().
#include "ldpc_hip.h"
#include "gdbf.h"
#include "rgdbf.h"
#include "rstat.h"
#include "hwgdbf.h"
#include "fxms.h"
#include "fxlms.h"
#include "bp.h"
#include "ddbmp.h"
#include "nb.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "graph.h"
#include "kernels.h"
#include "host_rt.h"

using namespace ldpc;   // host_rt.h: set_err, HIP_TRY, DevBuf, CtxCore, Blob and the call skeleton

static thread_local std::string g_last_error;

#ifdef LDPC_CHECK
namespace ldpc {
static const char *check_site_name(unsigned s)
{
    static const char *const names[CHK_SITES] = {
        "?", "rows_pp gather (app entry)", "rows_pp scatter (c2v slot)", "rows_pp bit read (c2v slot)",
        "rows_pp app write", "rows_fast gather (app entry)", "rows_fast scatter (c2v slot)",
        "rows_fast bit read (c2v slot)", "rows_fast app write", "flood/layered bit position",
        "flood c2v / eref slot", "flood packed-state row", "gdbf_rows bit", "gdbf_rows check term slot",
        "EMS message slot", "bp_rows bit", "bp_rows message slot", "ddbmp edge flag slot", "ddbmp check parity",
        "rgdbf_rows bit flag", "rgdbf_rows check parity", "hwgdbf decision byte", "hwgdbf check parity",
        "hwgdbf noise sample", "rstat decision byte", "rstat check parity", "rows_es gather (app entry)",
        "rows_es scatter (c2v slot)", "rows_es bit read (c2v slot)", "rows_es app write", "fxms message slot",
        "fxms decision byte", "fxlms schedule entry", "fxlms APP", "fxlms row state",
        "fxlms_wg schedule entry", "fxlms_wg APP", "fxlms_wg row state", "fxlms_wg global slot"};
    return s < CHK_SITES ? names[s] : "?";
}
long check_collect(hipStream_t s, char *msg, size_t msg_len)
{
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) return -(long)e;
    hipError_t (*const take[])(CheckRec *) = {check_take_rows_pp, check_take_rows_fast, check_take_flood, check_take_layered,
                                              check_take_gdbf, check_take_nb, check_take_bp, check_take_ddbmp,
                                              check_take_rgdbf, check_take_hwgdbf, check_take_rstat, check_take_rows_es,
                                              check_take_fxms, check_take_fxlms, check_take_fxlms_wg};
    long total = 0;
    for (auto fn : take) {
        CheckRec r{};
        if ((e = fn(&r)) != hipSuccess) return -(long)e;
        if (r.count && !total)
            std::snprintf(msg, msg_len, "LDPC_CHECK: %s index %u >= bound %u (block %u, thread %u)",
                          check_site_name(r.site), r.idx, r.bound, r.block, r.thread);
        total += r.count;
    }
    return total;
}
}  // namespace ldpc
#endif

struct ldpc_ctx : CtxCore {
    const ldpc_graph *g = nullptr;
    ldpc::DevGraph dg{};
    DevBuf graph, hist, y_stage, c_stage, d_stage, fw_stage, cw_table, gscratch, p_stage;
    DevBuf rs_att_stage, rs_unc, rs_tr_stage[4];          // every-attempt decoders: attempt results, uncoded errors, traces
    DevBuf hw_ptr_stage, hw_it_stage;                     // NGDBFhw: start pointers in, iterations run out
    DevBuf fx_code_stage;                                 // fixed-point min-sum: the integer codes out
    bool has_fxl = false;                                 // layered fixed-point min-sum: the layered row order, built by its first launch
    ldpc::FxlmsSched fxl{};
    DevBuf fxl_sched;
    int fxl_wg_grid = 0;                                  // fxlms_wg: the workgroups of the launch being made (its slots are in gscratch)
    int cw_rows = 0;
    ldpc::AuxStream aux;          // second stream of the flooding phase launches (kernels.h)
    bool has_rs = false;
    ldpc::RowSched rs{};
    DevBuf sched;
    bool has_rs_pp = false;                               // the ping-pong kernel's degree-aware row slots
    ldpc::RowSched rs_pp{};
    DevBuf sched_pp;
    bool has_rs_ppi = false;                              // its in-register schedule (the code has row pairs)
    ldpc::RowSched rs_ppi{};
    DevBuf sched_ppi;
    bool has_fs = false;
    ldpc::FloodSched fs{};
    DevBuf fsched;                                        // flood kernel schedule (codes beyond LDS)
    bool has_ls = false;
    ldpc::LayerSched ls{};                                // layered schedule (row order = fs order)
    DevBuf lsched;
    DevBuf divcheck;                                      // mismatch counter of verify_div_by_reciprocal
    DevBuf redo;                                          // re-decode list of the fast row kernel
    bool last_fast = false;                               // last min-sum launch used the fast row kernel
    std::vector<std::pair<float, bool>> div_ok;           // alpha -> reciprocal division exact
};

namespace ldpc {
int set_last_error(int code, const std::string &msg)
{
    g_last_error = msg;
    return code;
}

static const Options kNoOptions{};
static thread_local const Options *t_opts = nullptr;
const Options &cur_opts() { return t_opts ? *t_opts : kNoOptions; }
OptScope::OptScope(const Options &o) : prev_(t_opts) { t_opts = &o; }
OptScope::~OptScope() { t_opts = prev_; }

bool option_value_ok(int option, int v)
{
    switch (option) {
    case LDPC_OPT_ROWS64:
    case LDPC_OPT_ROWS32: return v >= 0 && v <= 2;
    case LDPC_OPT_PP_SLOTS: return v >= 0 && v <= 3;
    case LDPC_OPT_FLOOD_MODE:
    case LDPC_OPT_FLOOD_MSG:
    case LDPC_OPT_BP_KERNEL:
    case LDPC_OPT_GDBF_KERNEL:
    case LDPC_OPT_DDBMP_KERNEL:
    case LDPC_OPT_EMS_SWIZZLE: return v == 0 || v == 1;
    case LDPC_OPT_KERNEL: return v >= 0 && v <= 3;
    case LDPC_OPT_FLOOD_SPS_CHECK:
    case LDPC_OPT_FLOOD_SPS_BIT: return v >= 0 && v <= 4;
    case LDPC_OPT_FLOOD_RESIDENT: return v >= 0 && v <= 4096;
    case LDPC_OPT_FLOOD_STREAMS: return v >= 0 && v <= 2;
    case LDPC_OPT_FLOOD_BPC:
    case LDPC_OPT_LAYERED_BPC:
    case LDPC_OPT_ROWS_BPC:
    case LDPC_OPT_FAST_BPC: return v >= 0 && v <= 64;
    case LDPC_OPT_LAYERED_LDS_POS: return v >= 0 && v <= 65536;
    case LDPC_OPT_LAYERED_ROWS64: return v >= 0 && v <= 2;
    case LDPC_OPT_LAYERED_THREADS:
    case LDPC_OPT_EMS_THREADS: return v == 0 || v == 512 || v == 1024;
    default: return false;
    }
}
}  // namespace ldpc

// Device copies of the graph and of the host schedules (graph.cpp): each is one blob of
// 256-byte aligned sections (blob.h) and a struct of pointers into it.
template <class T> static const T *section(const DevBuf &buf, size_t off) { return (const T *)((const unsigned char *)buf.p + off); }

static hipError_t upload_graph(const ldpc_graph &g, DevBuf &buf, ldpc::DevGraph &dg)
{
    Blob b(256);
    const size_t o_rc = b.add(g.row_cols), o_rd = b.add(g.row_deg), o_cp = b.add(g.col_ptr),
                 o_cr = b.add(g.col_refs.data(), sizeof(uint32_t) * g.col_refs.size(), sizeof(uint32_t) * ((size_t)g.E + 1));
    const hipError_t e = upload(b, buf);
    if (e != hipSuccess) return e;
    dg = {g.N, g.M, g.maxdc > 0 ? g.maxdc : 1, section<int32_t>(buf, o_rc), section<uint8_t>(buf, o_rd),
          section<int32_t>(buf, o_cp), section<uint32_t>(buf, o_cr)};
    return hipSuccess;
}

// pair_flags (graph.h build_pp_inreg_schedule): the in-register schedule's, else null.
static hipError_t upload_row_sched(const ldpc::RowSchedule &hs, DevBuf &buf, ldpc::RowSched &rs,
                                   const std::vector<uint8_t> *pair_flags = nullptr)
{
    Blob b(256);
    const size_t o_cc = b.add(hs.cn_cols), o_cp = b.add(hs.cn_pos), o_cd = b.add(hs.cn_deg), o_vc = b.add(hs.vn_col),
                 o_vi = b.add(hs.vn_info), o_pf = pair_flags ? b.add(*pair_flags) : 0;
    const hipError_t e = upload(b, buf);
    if (e != hipSuccess) return e;
    rs = {hs.threads, hs.cpt, hs.dc, hs.e_pad, hs.rpt, hs.dc_low, section<uint16_t>(buf, o_cc),
          section<uint16_t>(buf, o_cp), section<uint8_t>(buf, o_cd), section<uint16_t>(buf, o_vc),
          section<uint32_t>(buf, o_vi), pair_flags ? section<uint8_t>(buf, o_pf) : nullptr, hs.e_pad, 0, 0};
    return hipSuccess;
}

static hipError_t upload_flood_sched(const ldpc_graph &g, const ldpc::FloodSchedule &fh, DevBuf &buf, ldpc::FloodSched &fs)
{
    // element -> (row, position) of the c2v layout: the packed-message bit phase
    // (flood.hip k_flood_bit_packed) rebuilds a message from its row's state
    std::vector<uint32_t> eref((size_t)fh.e_pad + 64, 0);
    for (int i = 0; i < fh.M_pad; ++i)
        for (int k = 0; k < fh.rdeg[i]; ++k)
            eref[fh.sq[(size_t)k * fh.M_pad + i]] = ((uint32_t)i << 5) | (uint32_t)k;
    Blob b(256);
    const size_t o_sp = b.add(fh.sp), o_sq = b.add(fh.sq), o_rd = b.add(fh.rdeg), o_pb = b.add(fh.pos_of_bit),
                 o_ba = b.add(fh.bit_at), o_pd = b.add(fh.pdeg), o_gb = b.add(fh.gbase), o_er = b.add(eref);
    const hipError_t e = upload(b, buf);
    if (e != hipSuccess) return e;
    fs = {fh.M_pad, fh.dc, fh.ngroups, fh.e_pad, g.maxdv, section<int32_t>(buf, o_sp), section<int32_t>(buf, o_sq),
          section<uint8_t>(buf, o_rd), section<int32_t>(buf, o_pb), section<int32_t>(buf, o_ba),
          section<uint8_t>(buf, o_pd), section<int32_t>(buf, o_gb), section<uint32_t>(buf, o_er)};
    return hipSuccess;
}

static hipError_t upload_layer_sched(const ldpc::LayerSchedule &lh, DevBuf &buf, ldpc::LayerSched &ls)
{
    Blob b(256);
    const size_t o_lp = b.add(lh.lptr), o_sp = b.add(lh.sp), o_rd = b.add(lh.rdeg), o_pb = b.add(lh.pos_of_bit);
    const hipError_t e = upload(b, buf);
    if (e != hipSuccess) return e;
    ls = {(int)lh.lptr.size() - 1, 0, lh.M_pad, section<int32_t>(buf, o_lp), section<int32_t>(buf, o_sp),
          section<uint8_t>(buf, o_rd), section<int32_t>(buf, o_pb)};
    for (int L = 0; L < ls.nlayers; ++L) ls.max_layer = std::max(ls.max_layer, lh.lptr[L + 1] - lh.lptr[L]);
    return hipSuccess;
}

// The layered row order as fxlms.hip reads it: row n is the check at layered position n.
static hipError_t upload_fxlms_sched(const ldpc_graph &g, const ldpc::LayerSchedule &lh, DevBuf &buf, ldpc::FxlmsSched &sc)
{
    const int M = g.M, dcs = g.maxdc > 0 ? g.maxdc : 1;
    std::vector<int32_t> cols((size_t)dcs * M, 0);
    std::vector<uint8_t> deg(M, 0);
    for (int n = 0; n < M; ++n) {
        const int j = lh.row_order[n], d = g.row_deg[j];
        deg[n] = (uint8_t)d;
        for (int k = 0; k < dcs; ++k)   // edges past the row repeat its last bit
            cols[(size_t)k * M + n] = d ? g.row_cols[(size_t)j * dcs + std::min(k, d - 1)] : 0;
    }
    Blob b(256);
    const size_t o_lp = b.add(lh.lptr), o_c = b.add(cols), o_d = b.add(deg);
    const hipError_t e = upload(b, buf);
    if (e != hipSuccess) return e;
    sc = {g.N, M, dcs, (int)lh.lptr.size() - 1, section<int32_t>(buf, o_lp), section<int32_t>(buf, o_c),
          section<uint8_t>(buf, o_d)};
    return hipSuccess;
}

// ----------------------------------------------------------------- the binary families' shared steps
static const char kFramesDev[] = "frames_dev must be a device pointer";

// The given samples of a decode call, in the order they are copied: y, the family's second
// input of `extra_elems` samples (pert / q; null: none) and the codewords sent.
template <class Args>
static int stage_given(SyncCall &s, ldpc_ctx *c, Args &a, bool f64, const void *y, const void *extra, size_t extra_elems,
                       const void **extra_dev, const int8_t *cw)
{
    const size_t fsz = f64 ? 8 : 4, nb = (size_t)a.batch * c->g->N;
    a.src = ldpc::SRC_GIVEN;
    RC_TRY(s.in(y, nb * fsz, c->y_stage, a.y));
    if (extra) RC_TRY(s.in(extra, extra_elems * fsz, c->p_stage, *extra_dev));
    return s.in(cw, nb, c->c_stage, a.c);
}

// After the checks: the synchronous form of a launch whose only output is the frame records.
template <class Run>
static int sim_batch_frames(ldpc_ctx *c, int batch, ldpc_frame_result *frames, ldpc_counts *accum, Run run)
{
    RC_TRY(c->enter());
    SyncCall s(*c);
    RC_TRY(s.snapshot());
    ldpc_frame_result *w;
    RC_TRY(s.out(frames, c->fw_stage, sizeof(ldpc_frame_result) * (size_t)batch, w));
    RC_TRY(run(w));
    return s.finish(accum);
}

// The decisions and the frame records, host or device.
template <class Args>
static int bind_decisions(SyncCall &s, ldpc_ctx *c, Args &a, int8_t *d_out, ldpc_frame_result *frames)
{
    RC_TRY(s.out(d_out, c->d_stage, (size_t)a.batch * c->g->N, a.d_out));
    return s.out(frames, c->fw_stage, sizeof(ldpc_frame_result) * (size_t)a.batch, a.frame_res);
}

// What ldpc_rgdbf_cfg and ldpc_rstat_cfg have in common: the flags, the per-bit syndrome
// weight and no quantiser.
template <class Args, class Cfg> static void redecode_fill(Args &a, ldpc_ctx *c, const Cfg *cfg, int batch)
{
    std::memset((void *)&a, 0, sizeof a);
    a.batch = batch;
    a.T = cfg->T;
    a.flags = cfg->flags;
    a.windowsize = cfg->windowsize;
    a.theta0 = cfg->theta;
    a.lambda = cfg->lambda;
    // RNGDBF.cpp:566 and newstat.cpp symNodeUpdates, alpha*Ymax/dv left to right: the kernels divide
    a.w = cfg->alpha * cfg->ymax;
    a.ymax = cfg->ymax;
    a.qmax = 1.0;
    fill_accounting(a, *c);
}

// The rules of the fields ldpc_fxms_cfg and ldpc_fxlms_cfg share; own() holds the cfg's own
// rule that comes after the precision's (fxms: reserved).
template <class Cfg, class Own> static int fx_check_cfg(const Cfg *cfg, Own own)
{
    if (!cfg) return set_err(LDPC_ERR_INVALID, "cfg is null");
    if (cfg->variant != LDPC_MS && cfg->variant != LDPC_NMS && cfg->variant != LDPC_OMS)
        return set_err(cfg->variant == LDPC_BP || cfg->variant == LDPC_DDBMP ? LDPC_ERR_UNSUPPORTED : LDPC_ERR_INVALID,
                       "variant %d: fixed-point min-sum is MS, NMS or OMS", cfg->variant);
    if (cfg->precision != LDPC_F32 && cfg->precision != LDPC_F64)
        return set_err(LDPC_ERR_INVALID, "bad precision %d", cfg->precision);
    RC_TRY(own());
    if (cfg->T < 0) return set_err(LDPC_ERR_INVALID, "T must be >= 0");
    if (cfg->qbits < 2 || cfg->qbits > 7) return set_err(LDPC_ERR_INVALID, "qbits must be in 2..7");
    if (cfg->msg_bits < 2 || cfg->msg_bits > 16) return set_err(LDPC_ERR_INVALID, "msg_bits must be in 2..16");
    if (cfg->variant == LDPC_NMS) {
        if (cfg->nms_shift < 0 || cfg->nms_shift > 7) return set_err(LDPC_ERR_INVALID, "nms_shift must be in 0..7");
        if (cfg->nms_num < 1 || cfg->nms_num > (1 << cfg->nms_shift))
            return set_err(LDPC_ERR_INVALID, "nms_num must be in 1..2^nms_shift = %d", 1 << cfg->nms_shift);
    }
    if (cfg->variant == LDPC_OMS && cfg->beta < 0) return set_err(LDPC_ERR_INVALID, "beta must be >= 0");
    if (cfg->early_stop != 0 && cfg->early_stop != 1) return set_err(LDPC_ERR_INVALID, "early_stop must be 0 or 1");
    if (!(cfg->ymax > 0) || !std::isfinite(cfg->ymax)) return set_err(LDPC_ERR_INVALID, "ymax must be > 0");
    return LDPC_OK;
}

// The launch arguments both fixed-point min-sum cfgs set.
template <class Args, class Cfg> static void fx_fill(Args &a, ldpc_ctx *c, const Cfg *cfg, int batch)
{
    std::memset((void *)&a, 0, sizeof a);
    a.batch = batch;
    a.T = cfg->T;
    a.variant = cfg->variant;   // LDPC_MS / NMS / OMS are V_MS / V_NMS / V_OMS
    a.nq1 = (1 << cfg->qbits) - 1;
    a.vmax = (1 << (cfg->msg_bits - 1)) - 1;
    a.nms_num = cfg->nms_num;
    a.nms_shift = cfg->nms_shift;
    a.beta = cfg->beta;
    a.early_stop = cfg->early_stop;
    a.ymax = cfg->ymax;
    fill_accounting(a, *c);
}

extern "C" {

int ldpc_abi_version(void) { return LDPC_ABI_VERSION; }
int ldpc_f64_nms_fast_division(double alpha) { return ldpc::markstein_exact_alpha(alpha) ? 1 : 0; }
const char *ldpc_last_error(void) { return g_last_error.c_str(); }

// ----------------------------------------------------------------- graph
int ldpc_graph_create(int N, int M, const int *num_nlist, const int *const *nlist, const int *num_mlist,
                      const int *const *mlist, ldpc_graph **out)
{
    if (!out) return set_err(LDPC_ERR_INVALID, "out is null");
    *out = nullptr;
    ldpc_graph *g = new (std::nothrow) ldpc_graph();
    if (!g) return set_err(LDPC_ERR_NOMEM, "graph allocation failed");
    std::string err;
    try {
        err = ldpc::build_graph(N, M, num_nlist, nlist, num_mlist, mlist, *g);
    } catch (const std::bad_alloc &) {
        delete g;
        return set_err(LDPC_ERR_NOMEM, "graph build out of memory");
    }
    if (!err.empty()) {
        delete g;
        return set_err(LDPC_ERR_GRAPH, "%s", err.c_str());
    }
    *out = g;
    return LDPC_OK;
}

int ldpc_graph_load_alist(const char *path, ldpc_graph **out)
{
    if (!out || !path) return set_err(LDPC_ERR_INVALID, "null argument");
    *out = nullptr;
    ldpc_graph *g = new (std::nothrow) ldpc_graph();
    if (!g) return set_err(LDPC_ERR_NOMEM, "graph allocation failed");
    std::string err;
    try {
        err = ldpc::load_alist(path, *g);
    } catch (const std::bad_alloc &) {
        delete g;
        return set_err(LDPC_ERR_NOMEM, "alist load out of memory");
    }
    if (!err.empty()) {
        delete g;
        const bool io = err.rfind("cannot open", 0) == 0;
        return set_err(io ? LDPC_ERR_IO : LDPC_ERR_GRAPH, "%s", err.c_str());
    }
    *out = g;
    return LDPC_OK;
}

int ldpc_graph_info(const ldpc_graph *g, int *N, int *M, int *E, int *maxdv, int *maxdc)
{
    if (!g) return set_err(LDPC_ERR_INVALID, "graph is null");
    if (N) *N = g->N;
    if (M) *M = g->M;
    if (E) *E = g->E;
    if (maxdv) *maxdv = g->maxdv;
    if (maxdc) *maxdc = g->maxdc;
    return LDPC_OK;
}

void ldpc_graph_destroy(ldpc_graph *g) { delete g; }

int ldpc_graph_layers(const ldpc_graph *g, int32_t *row_order, int32_t *layer_ptr, int *nlayers)
{
    if (!g || !nlayers) return set_err(LDPC_ERR_INVALID, "null argument");
    ldpc::FloodSchedule fh;
    ldpc::LayerSchedule lh;
    std::string err;
    try {
        err = ldpc::build_flood_schedule(*g, fh, ldpc::kMaxRowDegree);   // the order alone: every row degree
        if (err.empty()) err = ldpc::build_layers(*g, fh, lh);
    } catch (const std::bad_alloc &) {
        return set_err(LDPC_ERR_NOMEM, "layer schedule out of memory");
    }
    if (!err.empty()) return set_err(LDPC_ERR_GRAPH, "%s", err.c_str());
    *nlayers = (int)lh.lptr.size() - 1;
    if (row_order)
        for (int i = 0; i < g->M; ++i) row_order[i] = lh.row_order[i];
    if (layer_ptr)
        for (size_t L = 0; L < lh.lptr.size(); ++L) layer_ptr[L] = lh.lptr[L];
    return LDPC_OK;
}

// ----------------------------------------------------------------- context
int ldpc_bp_math_probe(int device, const double *x, int n, double *tanh_out, double *log_out)
{
    if (!x || n < 0) return set_err(LDPC_ERR_INVALID, "x is null or n < 0");
    if (n == 0) return LDPC_OK;
    HIP_TRY(hipSetDevice(device));
    const size_t bytes = sizeof(double) * (size_t)n;
    double *dx = nullptr, *dt = nullptr, *dl = nullptr;
    hipError_t e = hipMalloc(&dx, 3 * bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return set_err(LDPC_ERR_NOMEM, "hipMalloc(%zu): %s", 3 * bytes, hipGetErrorString(e));
    }
    dt = dx + n;
    dl = dt + n;
    e = hipMemcpy(dx, x, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = ldpc::bp_math_probe(dx, tanh_out ? dt : nullptr, log_out ? dl : nullptr, n, nullptr);
    if (e == hipSuccess && tanh_out) e = hipMemcpy(tanh_out, dt, bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess && log_out) e = hipMemcpy(log_out, dl, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(dx);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return set_err(LDPC_ERR_DEVICE, "bp math probe: %s", hipGetErrorString(e));
    }
    return LDPC_OK;
}

int ldpc_check_selftest(int device)
{
#ifdef LDPC_CHECK
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(ldpc::check_selftest_launch(nullptr));
    LDPC_CHECK_AFTER_LAUNCH(nullptr);
    return set_err(LDPC_ERR_DEVICE, "LDPC_CHECK self-test: the violation was not recorded");
#else
    (void)device;
    return set_err(LDPC_ERR_UNSUPPORTED, "this library has no device index checks (build `make checked`)");
#endif
}

int ldpc_device_count(int *n)
{
    if (!n) return set_err(LDPC_ERR_INVALID, "n is null");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        *n = 0;
        return set_err(LDPC_ERR_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *n = c;
    return LDPC_OK;
}

static void ctx_free(ldpc_ctx *c)
{
    if (!c) return;
    c->destroy({&c->graph, &c->hist, &c->y_stage, &c->c_stage, &c->d_stage, &c->fw_stage, &c->cw_table, &c->gscratch,
                &c->sched, &c->sched_pp, &c->sched_ppi, &c->divcheck, &c->fsched, &c->lsched, &c->p_stage, &c->redo,
                &c->hw_ptr_stage, &c->hw_it_stage, &c->fx_code_stage, &c->fxl_sched, &c->rs_att_stage, &c->rs_unc, &c->rs_tr_stage[0], &c->rs_tr_stage[1],
                &c->rs_tr_stage[2], &c->rs_tr_stage[3]});
    if (c->aux.fork) (void)hipEventDestroy(c->aux.fork);
    if (c->aux.join) (void)hipEventDestroy(c->aux.join);
    if (c->aux.s) (void)hipStreamDestroy(c->aux.s);
    delete c;
}

// Everything ldpc_ctx_create puts on the device; on failure the caller frees the context.
static int ctx_init(ldpc_ctx *c, int device, const ldpc_graph *g, int max_batch)
{
    c->g = g;
    RC_TRY(c->init(device, max_batch));
    HIP_TRY(hipStreamCreateWithFlags(&c->aux.s, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&c->aux.fork, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&c->aux.join, hipEventDisableTiming));
    HIP_TRY(upload_graph(*g, c->graph, c->dg));

    // Row-parallel schedule (the throughput kernel) when the graph fits it.
    // Rows per thread: 1 up to 512 rows (512-thread blocks), 2 up to 1024 rows
    // (512 threads, two blocks per CU: their barriers overlap; measured 1.13x
    // over one 1024-thread block with 1 row per thread on the N=1944 code).
    const int rpt = g->M <= 512 ? 1 : 2;
    int threads = ((((g->M + rpt - 1) / rpt) + 63) / 64) * 64;
    if (threads < 64) threads = 64;
    int dc = 0, cpt = 0;
    for (int d : ldpc::kRowsDc)
        if (!dc && g->maxdc <= d) dc = d;
    static const int cpt_for_rpt[][3] = {{0, 0, 0}, {2, 4, 0}, {4, 0, 0}};
    for (int q : cpt_for_rpt[rpt])
        if (q && !cpt && (long)(threads / 64) * q >= (g->N + 63) / 64) cpt = q;
    ldpc::RowSchedule hs;
    if (threads <= ldpc::kRowsMaxThreadsForRpt[rpt] && dc && cpt &&
        ldpc::build_row_schedule(*g, threads, cpt, dc, rpt, hs).empty()) {
        HIP_TRY(upload_row_sched(hs, c->sched, c->rs));
        c->has_rs = true;
        // the ping-pong kernel's copy: degree-7 rows on the younger check waves (graph.h pp_row_slots)
        const std::vector<int> slots = ldpc::pp_row_slots(*g, threads, 7);
        ldpc::RowSchedule hp;
        if (rpt == 2 && dc == 8 && cpt == 4 && !slots.empty() &&
            ldpc::build_row_schedule(*g, threads, cpt, dc, rpt, hp, &slots).empty()) {
            hp.dc_low = 7;
            HIP_TRY(upload_row_sched(hp, c->sched_pp, c->rs_pp));
            c->has_rs_pp = true;
            // and its in-register variant where a check thread can hold both rows of a degree-2 bit
            ldpc::PPPairing pr;
            ldpc::RowSchedule hi;
            std::vector<uint8_t> flags;
            if (ldpc::pp_pair_rows(*g, threads, 7, dc, pr) &&
                ((LDPC_PP_INREG_CPT == 3 && ldpc::build_pp_inreg_schedule(*g, threads, 3, dc, 7, pr, hi, flags).empty()) ||
                 ldpc::build_pp_inreg_schedule(*g, threads, cpt, dc, 7, pr, hi, flags).empty()) &&
                hi.e_pad <= hp.e_pad) {
                const int e_used = hi.e_pad;
                hi.e_pad = hp.e_pad;   // the split schedule's LDS partition; the smaller c2v area lies inside it
                HIP_TRY(upload_row_sched(hi, c->sched_ppi, c->rs_ppi, &flags));
                c->rs_ppi.e_used = e_used;
                c->rs_ppi.n_inreg = pr.pairs;
                int pure = 0;
                for (int w = 0; w < threads / 64; ++w) pure += flags[(size_t)threads + w];
                // a wave without LDS at its last positions issues two edge slots less per lane
                c->rs_ppi.lds_edge_slots = (threads + threads / 2) * 7 + (threads / 2) * dc - pure * 64 * 2;
                c->has_rs_ppi = true;
            }
        }
    }
    // Flood schedule (global-memory kernel for codes whose state exceeds LDS; also
    // selectable with LDPC_OPT_KERNEL for tests), and the layered schedule built on it.
    ldpc::FloodSchedule fh;
    if (ldpc::build_flood_schedule(*g, fh).empty()) {
        HIP_TRY(upload_flood_sched(*g, fh, c->fsched, c->fs));
        c->has_fs = true;
        ldpc::LayerSchedule lh;
        if (fh.dc <= ldpc::kPackedMaxDc && ldpc::build_layers(*g, fh, lh).empty()) {
            HIP_TRY(upload_layer_sched(lh, c->lsched, c->ls));
            c->has_ls = true;
        }
    }
    HIP_TRY(c->hist.ensure(sizeof(unsigned long long) * (size_t)g->N));
    HIP_TRY(hipMemset(c->hist.p, 0, c->hist.n));
    return LDPC_OK;
}

int ldpc_ctx_create(int device, const ldpc_graph *g, int max_batch, ldpc_ctx **out)
{
    if (!out || !g) return set_err(LDPC_ERR_INVALID, "null argument");
    *out = nullptr;
    if (max_batch <= 0) return set_err(LDPC_ERR_INVALID, "max_batch must be > 0");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return set_err(LDPC_ERR_INVALID, "device %d of %d", device, ndev);
    ldpc_ctx *c = new (std::nothrow) ldpc_ctx();
    if (!c) return set_err(LDPC_ERR_NOMEM, "ctx allocation failed");
    const int rc = ctx_init(c, device, g, max_batch);
    if (rc) {
        ctx_free(c);
        return rc;
    }
    *out = c;
    return LDPC_OK;
}

int ldpc_ctx_set_stream(ldpc_ctx *c, void *s) { return c ? c->set_stream(s) : set_err(LDPC_ERR_INVALID, "ctx is null"); }

int ldpc_ctx_synchronize(ldpc_ctx *c)
{
    if (!c) return set_err(LDPC_ERR_INVALID, "ctx is null");
    RC_TRY(c->enter());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return LDPC_OK;
}

void ldpc_ctx_destroy(ldpc_ctx *c) { ctx_free(c); }

int ldpc_ctx_set_option(ldpc_ctx *c, int option, int value)
{
    return c ? c->set_option(option, value, false) : set_err(LDPC_ERR_INVALID, "ctx is null");
}

int ldpc_ctx_get_option(const ldpc_ctx *c, int option, int *value)
{
    if (!c || !value) return set_err(LDPC_ERR_INVALID, "null argument");
    if (option <= 0 || option >= LDPC_OPT_COUNT) return set_err(LDPC_ERR_INVALID, "unknown option %d", option);
    *value = c->opts.v[option];
    return LDPC_OK;
}

// ----------------------------------------------------------------- helpers
static int check_cfg(const ldpc_ctx *c, const ldpc_decoder_cfg *cfg)
{
    if (!cfg) return set_err(LDPC_ERR_INVALID, "cfg is null");
    if (cfg->variant < LDPC_MS || cfg->variant > LDPC_DDBMP) return set_err(LDPC_ERR_INVALID, "bad variant %d", cfg->variant);
    if (cfg->variant == LDPC_BP) {
        if (cfg->schedule != LDPC_FLOODING) return set_err(LDPC_ERR_UNSUPPORTED, "BP is flooding only");
        if (c->g->maxdc > ldpc::kBpMaxDc)
            return set_err(LDPC_ERR_UNSUPPORTED, "BP supports row degree <= %d", ldpc::kBpMaxDc);
        if (cfg->max_llr < 0) return set_err(LDPC_ERR_INVALID, "max_llr must be >= 0");
    }
    if (cfg->variant == LDPC_DDBMP && cfg->schedule == LDPC_LAYERED)
        return set_err(LDPC_ERR_UNSUPPORTED, "DD-BMP is flooding only");
    if (cfg->precision != LDPC_F32 && cfg->precision != LDPC_F64)
        return set_err(LDPC_ERR_INVALID, "bad precision %d", cfg->precision);
    if (cfg->T < 0) return set_err(LDPC_ERR_INVALID, "T must be >= 0");
    if ((cfg->quantize || cfg->saturate) && !(cfg->ymax > 0))
        return set_err(LDPC_ERR_INVALID, "quantize/saturate need ymax > 0");
    if (cfg->quantize && (cfg->qbits < 1 || cfg->qbits > 30)) return set_err(LDPC_ERR_INVALID, "qbits out of range");
    if (cfg->schedule != LDPC_FLOODING && cfg->schedule != LDPC_LAYERED)
        return set_err(LDPC_ERR_INVALID, "bad schedule %d", cfg->schedule);
    if (cfg->schedule == LDPC_LAYERED && !c->has_ls)
        return set_err(LDPC_ERR_UNSUPPORTED, "layered schedule unavailable for this graph (row degree > %d)",
                       ldpc::kPackedMaxDc);
    if (cfg->early_stop && cfg->variant != LDPC_DDBMP) {   // DD-BMP always stops: the field is not read
        if (cfg->early_stop != 1) return set_err(LDPC_ERR_INVALID, "early_stop must be 0 or 1");
        if (cfg->schedule == LDPC_LAYERED)
            return set_err(LDPC_ERR_UNSUPPORTED, "early_stop is not supported with the layered schedule");
        if (cfg->variant != LDPC_BP && c->opts.v[LDPC_OPT_KERNEL] == 2)
            return set_err(LDPC_ERR_UNSUPPORTED, "early_stop is not supported by the flood kernels (LDPC_OPT_KERNEL = 2)");
    }
    return LDPC_OK;
}

static void fill_common(ldpc::DecodeArgs &a, ldpc_ctx *c, const ldpc_decoder_cfg *cfg, int batch)
{
    std::memset(&a, 0, sizeof a);
    a.batch = batch;
    a.T = cfg->T;
    a.variant = cfg->variant;
    a.quantize = cfg->quantize;
    a.saturate = cfg->saturate;
    a.early_stop = cfg->variant != LDPC_DDBMP && cfg->early_stop;
    a.ymax = cfg->ymax;
    a.nq = std::pow(2.0, (double)cfg->qbits);   // Nq = pow(2.0, Q) (:121)
    a.alpha = cfg->alpha;
    a.delta = cfg->delta;
    a.n0 = cfg->n0;
    a.max_llr = cfg->max_llr > 0 ? cfg->max_llr : 20.0;   // MAXLLR = 20 (decodeBP.cpp:58)
    a.counts = (unsigned long long *)c->counts.p;
    a.hist = (unsigned long long *)c->hist.p;
}

static_assert(sizeof(ldpc_frame_result) == sizeof(int4), "frame result layout");

// fp32 NMS: use the reciprocal division only after the device has checked it
// against IEEE x/alpha for every finite non-negative float (cached per alpha).
static int nms_setup(ldpc_ctx *c, const ldpc_decoder_cfg *cfg, ldpc::DecodeArgs &a)
{
    a.nms_fast = 0;
    a.alpha_rcp = 0.f;
    if (cfg->variant != LDPC_NMS || cfg->precision != LDPC_F32) return LDPC_OK;
    const float alpha = (float)cfg->alpha;
    if (!(alpha > 0.f) || !std::isfinite(alpha)) return LDPC_OK;
    const float rcp = 1.0f / alpha;
    bool ok = false, known = false;
    for (const auto &e : c->div_ok)
        if (e.first == alpha) { ok = e.second; known = true; }
    if (!known) {
        HIP_TRY(c->divcheck.ensure(sizeof(unsigned long long)));
        HIP_TRY(ldpc::verify_div_by_reciprocal(alpha, rcp, (unsigned long long *)c->divcheck.p, c->stream));
        unsigned long long bad = 1;
        HIP_TRY(hipMemcpyAsync(&bad, c->divcheck.p, sizeof bad, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        ok = bad == 0;
        c->div_ok.emplace_back(alpha, ok);
    }
    if (ok) {
        a.nms_fast = 1;
        a.alpha_rcp = rcp;
    }
    return LDPC_OK;
}

// The launch plan of a decode (kernels.h): which kernel, its shape, grid and scratch. The
// families' planners are asked in the order of preference (each says whether its kernel
// decodes the input); LDPC_OPT_KERNEL (tests) forces one of the generic kernels.
static ldpc::LaunchPlan build_plan(const ldpc_ctx *c, const ldpc::DecodeArgs &a, bool f64, int schedule)
{
    enum { AUTO = 0, LDS = 1, FLOOD = 2, GLOBAL = 3 };   // values of LDPC_OPT_KERNEL
    const ldpc::OptScope os(c->opts);
    const ldpc::PlanInput in{c->dg, c->g->E, c->has_rs ? &c->rs : nullptr, c->has_rs_pp ? &c->rs_pp : nullptr,
                             c->has_fs ? &c->fs : nullptr, c->has_ls ? &c->ls : nullptr, c->num_cus, a, f64, c->g->maxdv,
                             c->has_rs_ppi ? &c->rs_ppi : nullptr};
    const int force = c->opts.v[LDPC_OPT_KERNEL];
    ldpc::LaunchPlan p;
    if (a.variant == ldpc::VARIANT_BP) {
        ldpc::plan_bp(in, p);
    } else if (a.variant == ldpc::VARIANT_DDBMP) {
        ldpc::plan_ddbmp(in, p);
    } else if (schedule == LDPC_LAYERED) {
        ldpc::plan_layered(in, p);   // check_cfg: the context has the layered schedule
    } else if (a.early_stop) {
        // rows_es -> lds -> global: the fast row kernels, flood and layered never stop early (check_cfg
        // refuses force == FLOOD)
        const bool planned = (force == AUTO && ldpc::plan_rows_es(in, p)) ||
                             ((force == AUTO || force == LDS) && ldpc::plan_lds(in, p));
        if (!planned) ldpc::plan_global(in, p);
    } else {
        const bool planned = (force == FLOOD && ldpc::plan_flood(in, p)) || (force == AUTO && ldpc::plan_rows(in, p)) ||
                             ((force == AUTO || force == LDS) && ldpc::plan_lds(in, p)) ||
                             (force != GLOBAL && ldpc::plan_flood(in, p));
        if (!planned) ldpc::plan_global(in, p);
    }
    return p;
}

static int run_kernel(ldpc_ctx *c, ldpc::DecodeArgs a, bool f64, int schedule)
{
    using ldpc::Kernel;
    const ldpc::OptScope os(c->opts);
    const ldpc::LaunchPlan p = build_plan(c, a, f64, schedule);
    if (p.scratch_bytes) HIP_TRY(c->gscratch.ensure(p.scratch_bytes));
    if (p.redo) HIP_TRY(c->redo.ensure(sizeof(unsigned) * ((size_t)c->max_batch + 1)));
#ifdef LDPC_STAMPS
    // diagnostic builds: per-block phase cycle sums appended to $LDPC_STAMPS
    static DevBuf stamp_buf;
    const char *stamp_path = std::getenv("LDPC_STAMPS");
    if (stamp_path) {
        HIP_TRY(stamp_buf.ensure(8192 * 4 * sizeof(unsigned long long)));
        HIP_TRY(hipMemsetAsync(stamp_buf.p, 0, stamp_buf.n, c->stream));
        a.stamps = (unsigned long long *)stamp_buf.p;
    }
#endif
    RC_TRY(c->begin_launch());
    c->last_fast = p.redo;
    if (p.redo) HIP_TRY(hipMemsetAsync(c->redo.p, 0, sizeof(unsigned), c->stream));
    switch (p.kernel) {
    case Kernel::rows: HIP_TRY(ldpc::launch_rows(p, c->dg, a, c->stream)); break;
    case Kernel::rows_fast: HIP_TRY(ldpc::launch_rows_fast(p, c->dg, a, (unsigned *)c->redo.p, c->stream)); break;
    case Kernel::rows_pp: HIP_TRY(ldpc::launch_rows_pp(p, c->dg, a, (unsigned *)c->redo.p, c->stream)); break;
    case Kernel::rows_es: HIP_TRY(ldpc::launch_rows_es(p, c->dg, a, c->ticket(), c->stream)); break;
    case Kernel::lds:
    case Kernel::global: HIP_TRY(ldpc::launch_generic(p, c->dg, a, c->gscratch.p, c->stream)); break;
    case Kernel::flood_persistent:
    case Kernel::flood_phase:
        HIP_TRY(ldpc::launch_flood(p, c->dg, c->fs, a, f64, c->gscratch.p, c->stream, &c->aux));
        break;
    case Kernel::layered_lds:
    case Kernel::layered_global:
        HIP_TRY(ldpc::launch_layered(p, c->dg, c->fs, c->ls, a, c->gscratch.p, c->stream));
        break;
    case Kernel::bp_rows:
    case Kernel::bp_lds:
    case Kernel::bp_global:
        HIP_TRY(ldpc::launch_bp(p, c->dg, a, f64, c->g->E, c->gscratch.p, c->ticket(), c->stream));
        break;
    case Kernel::ddbmp_rows:
    case Kernel::ddbmp_lds:
    case Kernel::ddbmp_global:
        HIP_TRY(ldpc::launch_ddbmp(p, c->dg, a, f64, c->g->E, c->gscratch.p, c->ticket(), c->stream));
        break;
    }
    // the exact re-decode of any codeword whose fast-path premise failed
    if (p.redo) HIP_TRY(ldpc::launch_redo(c->dg, a, f64, (const unsigned *)c->redo.p, c->stream, c->num_cus));
    RC_TRY(c->end_launch());
#ifdef LDPC_STAMPS
    if (stamp_path) {
        std::vector<unsigned long long> h(8192 * 4);
        HIP_TRY(hipMemcpyAsync(h.data(), stamp_buf.p, stamp_buf.n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (FILE *f = std::fopen(stamp_path, "ab")) {
            std::fwrite(h.data(), sizeof(unsigned long long), h.size(), f);
            std::fclose(f);
        }
    }
#endif
    return LDPC_OK;
}

// ----------------------------------------------------------------- decode
int ldpc_decode_batch(ldpc_ctx *c, const void *y, int batch, const ldpc_decoder_cfg *cfg, const int8_t *cw,
                      int8_t *d_out, ldpc_frame_result *frame_weights, ldpc_counts *counts)
{
    if (!c || !y) return set_err(LDPC_ERR_INVALID, "null argument");
    RC_TRY(check_cfg(c, cfg));
    RC_TRY(check_batch(*c, batch));
    if (cfg->variant == LDPC_BP && !(cfg->n0 > 0)) return set_err(LDPC_ERR_INVALID, "BP needs cfg->n0 > 0");
    RC_TRY(c->enter());
    const bool f64 = cfg->precision == LDPC_F64;
    ldpc::DecodeArgs a;
    fill_common(a, c, cfg, batch);
    RC_TRY(nms_setup(c, cfg, a));
    SyncCall s(*c);
    RC_TRY(stage_given(s, c, a, f64, y, nullptr, 0, nullptr, cw));
    RC_TRY(bind_decisions(s, c, a, d_out, frame_weights));
    RC_TRY(s.snapshot());
    RC_TRY(run_kernel(c, a, f64, cfg->schedule));
    return s.finish(counts);
}

// ----------------------------------------------------------------- Monte-Carlo
int ldpc_sim_set_codewords(ldpc_ctx *c, const uint8_t *bits, int rows)
{
    if (!c) return set_err(LDPC_ERR_INVALID, "ctx is null");
    if (rows < 0 || (rows > 0 && !bits)) return set_err(LDPC_ERR_INVALID, "bad codeword table");
    RC_TRY(c->enter());
    c->cw_rows = 0;
    if (rows == 0) return LDPC_OK;
    const size_t n = (size_t)rows * c->g->N;
    std::vector<int8_t> bip(n);
    for (size_t i = 0; i < n; ++i) {
        if (bits[i] > 1) return set_err(LDPC_ERR_INVALID, "codeword bit %zu is %d (want 0/1)", i, bits[i]);
        bip[i] = bits[i] ? -1 : +1;   // '1' -> c = -1, '0' -> c = +1 (:204-207)
    }
    HIP_TRY(c->cw_table.ensure(n));
    HIP_TRY(hipMemcpy(c->cw_table.p, bip.data(), n, hipMemcpyHostToDevice));
    c->cw_rows = rows;
    return LDPC_OK;
}

// After the checks and enter(); y_out_dev / d_out_dev: device pointers or null.
static int sim_run(ldpc_ctx *c, const SimCall &q, const ldpc_decoder_cfg *cfg, ldpc_frame_result *frames_dev,
                   void *y_out_dev, int8_t *d_out_dev)
{
    ldpc::DecodeArgs a;
    fill_common(a, c, cfg, q.batch);
    RC_TRY(nms_setup(c, cfg, a));
    const SimPoint pt = fill_sim(a, *c, q);      // :146-147
    fill_cw_table(a, *c);
    if (cfg->variant == LDPC_BP) a.n0 = pt.N0;   // 4*y/N0 (decodeBP.cpp:104,188)
    a.frame_res = (int4 *)frames_dev;
    a.y_out = y_out_dev;
    a.d_out = d_out_dev;
    return run_kernel(c, a, cfg->precision == LDPC_F64, cfg->schedule);
}

int ldpc_sim_launch(ldpc_ctx *c, double ebn0_db, double R, const ldpc_decoder_cfg *cfg, uint64_t seed,
                    uint32_t stream_id, uint64_t first_cw, int batch, ldpc_frame_result *frames_dev)
{
    const SimCall q{ebn0_db, R, seed, stream_id, first_cw, batch};
    RC_TRY(check_sim(c, [&] { return check_cfg(c, cfg); }, q, false));
    RC_TRY(require_device(frames_dev, kFramesDev));
    RC_TRY(c->enter());
    return sim_run(c, q, cfg, frames_dev, nullptr, nullptr);
}

int ldpc_ctx_read_counts(ldpc_ctx *c, ldpc_counts *out, int reset)
{
    if (!c) return set_err(LDPC_ERR_INVALID, "ctx is null");
    RC_TRY(c->enter());
    return c->read_counts(out, reset);
}

int ldpc_ctx_read_histogram(ldpc_ctx *c, int64_t *out, int reset)
{
    if (!c || !out) return set_err(LDPC_ERR_INVALID, "null argument");
    RC_TRY(c->enter());
    HIP_TRY(hipMemcpyAsync(out, c->hist.p, c->hist.n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (reset) HIP_TRY(hipMemsetAsync(c->hist.p, 0, c->hist.n, c->stream));
    return LDPC_OK;
}

// Synchronous sim with optional host-or-device outputs (staged when host).
int ldpc_sim_trace(ldpc_ctx *c, double ebn0_db, double R, const ldpc_decoder_cfg *cfg, uint64_t seed,
                   uint32_t stream_id, uint64_t first_cw, int batch, void *y_out, int8_t *d_out,
                   ldpc_frame_result *frames, ldpc_counts *accum)
{
    const SimCall q{ebn0_db, R, seed, stream_id, first_cw, batch};
    RC_TRY(check_sim(c, [&] { return check_cfg(c, cfg); }, q, false));
    RC_TRY(c->enter());
    const size_t nb = (size_t)batch * c->g->N;
    SyncCall s(*c);
    RC_TRY(s.snapshot());
    ldpc_frame_result *w;
    void *y;
    int8_t *d;
    RC_TRY(s.out(frames, c->fw_stage, sizeof(ldpc_frame_result) * (size_t)batch, w));
    RC_TRY(s.out(y_out, c->y_stage, nb * (cfg->precision == LDPC_F64 ? 8 : 4), y));
    RC_TRY(s.out(d_out, c->d_stage, nb, d));
    RC_TRY(sim_run(c, q, cfg, w, y, d));
    return s.finish(accum);
}

int ldpc_sim_batch(ldpc_ctx *c, double ebn0_db, double R, const ldpc_decoder_cfg *cfg, uint64_t seed,
                   uint32_t stream_id, uint64_t first_cw, int batch, ldpc_frame_result *frames, ldpc_counts *accum)
{
    return ldpc_sim_trace(c, ebn0_db, R, cfg, seed, stream_id, first_cw, batch, nullptr, nullptr, frames, accum);
}

int ldpc_ctx_last_kernel_ms(ldpc_ctx *c, float *ms)
{
    return c ? c->last_kernel_ms(ms) : set_err(LDPC_ERR_INVALID, "null argument");
}

// The plan of cfg as the info calls report it (a one-codeword batch, no sample source).
static int info_plan(ldpc_ctx *c, const ldpc_decoder_cfg *cfg, ldpc::LaunchPlan &p)
{
    if (!c || !cfg) return set_err(LDPC_ERR_INVALID, "null argument");
    RC_TRY(check_cfg(c, cfg));
    RC_TRY(c->enter());
    ldpc::DecodeArgs a;
    fill_common(a, c, cfg, 1);
    RC_TRY(nms_setup(c, cfg, a));   // fp32 NMS: whether the verified reciprocal (and so the fast kernels) applies
    p = build_plan(c, a, cfg->precision == LDPC_F64, cfg->schedule);
    return LDPC_OK;
}

int ldpc_ctx_row_sched_info(ldpc_ctx *c, const ldpc_decoder_cfg *cfg, int32_t *info)
{
    if (!info) return set_err(LDPC_ERR_INVALID, "null argument");
    ldpc::LaunchPlan p;
    RC_TRY(info_plan(c, cfg, p));
    if (!p.rs) return set_err(LDPC_ERR_UNSUPPORTED, "the row kernel does not decode this cfg (kernel %s)", p.name);
    const ldpc::RowSched &rs = *p.rs;
    info[0] = rs.threads;
    info[1] = rs.rpt;
    info[2] = rs.cpt;
    info[3] = rs.dc;
    info[4] = rs.e_pad;
    info[5] = p.cw_per_block;
    info[6] = p.lds_bytes;
    info[7] = p.blocks_per_cu;
    info[8] = rs.dc_low;
    // check edge slots issued per codeword-iteration; with degree-aware slots (rows_pp.hip k_rows_pp
    // SPLIT) every row-0 slot and the row-1 slots of threads >= threads/2 run a dc_low-edge check
    // node, the other row-1 slots a dc-edge one
    info[9] = rs.dc_low ? (rs.threads + rs.threads / 2) * rs.dc_low + (rs.threads / 2) * rs.dc
                        : rs.threads * rs.rpt * rs.dc;
    return LDPC_OK;
}

int ldpc_ctx_pp_inreg_info(ldpc_ctx *c, const ldpc_decoder_cfg *cfg, int32_t *info)
{
    if (!info) return set_err(LDPC_ERR_INVALID, "null argument");
    ldpc::LaunchPlan p;
    RC_TRY(info_plan(c, cfg, p));
    if (p.kernel != ldpc::Kernel::rows_pp || !p.rs)
        return set_err(LDPC_ERR_UNSUPPORTED, "the ping-pong kernel does not decode this cfg (kernel %s)", p.name);
    int32_t rsi[10];
    RC_TRY(ldpc_ctx_row_sched_info(c, cfg, rsi));
    const ldpc::RowSched *ri = p.rs_inreg;
    info[0] = ri ? ri->n_inreg : 0;
    info[1] = ri ? ri->lds_edge_slots : rsi[9];
    info[2] = ri ? ri->e_used : p.rs->e_pad;
    info[3] = ri ? ri->cpt : p.rs->cpt;
    return LDPC_OK;
}

int ldpc_pp_block_layout(int n_bits, int e_pad, int32_t *info)
{
    if (!info) return set_err(LDPC_ERR_INVALID, "null argument");
    int bytes = 0;
    info[0] = ldpc::pp_w12_layout(n_bits, e_pad, &bytes) ? 1 : 0;
    info[1] = bytes;
    return LDPC_OK;
}

int ldpc_ctx_pp_block_info(ldpc_ctx *c, const ldpc_decoder_cfg *cfg, int32_t *info)
{
    if (!info) return set_err(LDPC_ERR_INVALID, "null argument");
    ldpc::LaunchPlan p;
    RC_TRY(info_plan(c, cfg, p));
    if (p.kernel != ldpc::Kernel::rows_pp || !p.rs)
        return set_err(LDPC_ERR_UNSUPPORTED, "the ping-pong kernel does not decode this cfg (kernel %s)", p.name);
    info[0] = p.threads;
    info[1] = p.lds_bytes + p.cache_lds_bytes + p.pad_lds_bytes;
    return LDPC_OK;
}

int ldpc_ctx_pp_row_slots(ldpc_ctx *c, const ldpc_decoder_cfg *cfg, uint16_t *cols, uint8_t *deg, int cap, int *nslots)
{
    if (!cols || !deg || !nslots || cap < 0) return set_err(LDPC_ERR_INVALID, "null argument");
    ldpc::LaunchPlan p;
    RC_TRY(info_plan(c, cfg, p));
    if (p.kernel != ldpc::Kernel::rows_pp || !p.rs)
        return set_err(LDPC_ERR_UNSUPPORTED, "the ping-pong kernel does not decode this cfg (kernel %s)", p.name);
    const ldpc::RowSched *rs = p.rs_inreg ? p.rs_inreg : p.rs;   // the schedule launch_rows_pp passes to the kernel
    *nslots = rs->threads * rs->rpt;
    if (cap < *nslots) return set_err(LDPC_ERR_INVALID, "%d row slots, room for %d", *nslots, cap);
    RC_TRY(c->enter());
    HIP_TRY(hipMemcpyAsync(cols, rs->cn_cols, sizeof(uint16_t) * (size_t)*nslots * rs->dc, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(deg, rs->cn_deg, sizeof(uint8_t) * (size_t)*nslots, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return LDPC_OK;
}

int ldpc_ctx_redo_count(ldpc_ctx *c, int64_t *n)
{
    if (!c || !n) return set_err(LDPC_ERR_INVALID, "null argument");
    *n = 0;
    if (!c->last_fast || !c->redo.p) return LDPC_OK;
    RC_TRY(c->enter());
    unsigned h = 0;
    HIP_TRY(hipMemcpyAsync(&h, c->redo.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *n = (int64_t)h;
    return LDPC_OK;
}

int ldpc_ctx_redo_list(ldpc_ctx *c, uint32_t *list, int64_t cap, int64_t *n)
{
    if (!c || !n || cap < 0 || (cap > 0 && !list)) return set_err(LDPC_ERR_INVALID, "null argument");
    RC_TRY(ldpc_ctx_redo_count(c, n));
    const int64_t m = std::min(*n, cap);
    if (m > 0) {
        HIP_TRY(hipMemcpyAsync(list, (const unsigned *)c->redo.p + 1, sizeof(unsigned) * (size_t)m, hipMemcpyDeviceToHost,
                               c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return LDPC_OK;
}

int ldpc_ctx_kernel_info(ldpc_ctx *c, const ldpc_decoder_cfg *cfg, char *name, int name_len, int *lds_bytes,
                         int *bpc)
{
    ldpc::LaunchPlan p;
    RC_TRY(info_plan(c, cfg, p));
    if (bpc) *bpc = p.blocks_per_cu;
    return report_choice(p, name, name_len, lds_bytes);
}


// ----------------------------------------------------------------- GDBF / NGDBF
static int gdbf_check_cfg(const ldpc_gdbf_cfg *cfg)
{
    if (!cfg) return set_err(LDPC_ERR_INVALID, "cfg is null");
    if (cfg->precision != LDPC_F32 && cfg->precision != LDPC_F64)
        return set_err(LDPC_ERR_INVALID, "bad precision %d", cfg->precision);
    if (cfg->T < 0 || cfg->T > 4094) return set_err(LDPC_ERR_INVALID, "T must be in 0..4094");
    if (cfg->flags & ~511) return set_err(LDPC_ERR_INVALID, "unknown GDBF flags 0x%x", cfg->flags);
    if ((cfg->flags & LDPC_GDBF_ADAPT) && (cfg->flags & (LDPC_GDBF_SEQUENTIAL | LDPC_GDBF_MODESWITCH)))
        return set_err(LDPC_ERR_UNSUPPORTED, "threshold adaptation with single-bit flips is not supported");
    if ((cfg->flags & LDPC_GDBF_QPROB) && (cfg->flags & LDPC_GDBF_NOISE))
        return set_err(LDPC_ERR_UNSUPPORTED, "QPROB with NOISE is not supported");
    if ((cfg->flags & LDPC_GDBF_MODESWITCH) && cfg->tswitch < 0) return set_err(LDPC_ERR_INVALID, "tswitch < 0");
    if ((cfg->flags & (LDPC_GDBF_SATURATE | LDPC_GDBF_QUANTIZE)) && !(cfg->ymax > 0))
        return set_err(LDPC_ERR_INVALID, "saturate/quantize need ymax > 0");
    if ((cfg->flags & LDPC_GDBF_QUANTIZE) && (cfg->nq < 1 || cfg->nq > 30))
        return set_err(LDPC_ERR_INVALID, "nq out of range");
    if ((cfg->flags & LDPC_GDBF_SMOOTH) && (cfg->windowsize < 0 || cfg->windowsize > 32767))
        return set_err(LDPC_ERR_INVALID, "windowsize out of range");
    return LDPC_OK;
}

static void gdbf_fill(ldpc::GdbfArgs &a, ldpc_ctx *c, const ldpc_gdbf_cfg *cfg, int batch)
{
    std::memset(&a, 0, sizeof a);
    a.batch = batch;
    a.T = cfg->T;
    a.flags = cfg->flags;
    a.windowsize = cfg->windowsize;
    a.theta0 = cfg->theta;
    a.lambda = cfg->lambda;
    a.w = (cfg->flags & LDPC_GDBF_WEIGHT) ? cfg->alpha : 1.0;   // :541-551
    a.ymax = cfg->ymax;
    a.qmax = std::pow(2, (cfg->nq - 1));                       // :490
    a.tswitch = cfg->tswitch;
    a.qsigma = cfg->qsigma;
    fill_accounting(a, *c);
}

static int gdbf_run(ldpc_ctx *c, const ldpc::GdbfArgs &a, bool f64)
{
    const ldpc::OptScope os(c->opts);
    const ldpc::GdbfChoice ch = ldpc::gdbf_choose(c->dg, f64, a.flags, c->g->maxdv, c->g->maxdc);
    return run_with_slots(*c, c->gscratch, ch, a.batch, 2 * c->num_cus, [&](void *scratch, int slots) {
        return ldpc::gdbf_launch(c->dg, a, f64, ch, scratch, slots, c->num_cus, c->stream);
    });
}

int ldpc_gdbf_decode_batch(ldpc_ctx *c, const void *y, const void *pert, int batch, const ldpc_gdbf_cfg *cfg,
                           const int8_t *cw, int8_t *d_out, ldpc_frame_result *frames, ldpc_counts *counts)
{
    if (!c || !y) return set_err(LDPC_ERR_INVALID, "null argument");
    RC_TRY(gdbf_check_cfg(cfg));
    RC_TRY(check_batch(*c, batch));
    const bool with_pert = cfg->flags & (LDPC_GDBF_NOISE | LDPC_GDBF_QPROB);
    if (with_pert && !pert) return set_err(LDPC_ERR_INVALID, "NOISE / QPROB need pert");
    if ((cfg->flags & LDPC_GDBF_QPROB) && !(cfg->qsigma > 0)) return set_err(LDPC_ERR_INVALID, "QPROB needs qsigma > 0");
    RC_TRY(c->enter());
    const bool f64 = cfg->precision == LDPC_F64;
    ldpc::GdbfArgs a;
    gdbf_fill(a, c, cfg, batch);
    SyncCall s(*c);
    RC_TRY(stage_given(s, c, a, f64, y, with_pert ? pert : nullptr, (size_t)batch * c->g->N * (size_t)cfg->T, &a.pert, cw));
    RC_TRY(bind_decisions(s, c, a, d_out, frames));
    RC_TRY(s.snapshot());
    RC_TRY(gdbf_run(c, a, f64));
    return s.finish(counts);
}

// After the checks and enter().
static int gdbf_sim_run(ldpc_ctx *c, const SimCall &q, const ldpc_gdbf_cfg *cfg, ldpc_frame_result *frames_dev)
{
    ldpc::GdbfArgs a;
    gdbf_fill(a, c, cfg, q.batch);
    fill_sim(a, *c, q);                                       // :175-176
    fill_cw_table(a, *c);
    a.frame_res = (int4 *)frames_dev;
    a.noise_sigma = a.sigma * cfg->noise_scale;               // :296
    a.qsigma = a.noise_sigma;                                  // symNodeUpdates' sigma (:353, :563)
    return gdbf_run(c, a, cfg->precision == LDPC_F64);
}

int ldpc_gdbf_sim_launch(ldpc_ctx *c, double ebn0_db, double R, const ldpc_gdbf_cfg *cfg, uint64_t seed,
                         uint32_t stream_id, uint64_t first_cw, int batch, ldpc_frame_result *frames_dev)
{
    const SimCall q{ebn0_db, R, seed, stream_id, first_cw, batch};
    RC_TRY(check_sim(c, [&] { return gdbf_check_cfg(cfg); }, q, true));
    RC_TRY(require_device(frames_dev, kFramesDev));
    RC_TRY(c->enter());
    return gdbf_sim_run(c, q, cfg, frames_dev);
}

int ldpc_gdbf_sim_batch(ldpc_ctx *c, double ebn0_db, double R, const ldpc_gdbf_cfg *cfg, uint64_t seed,
                        uint32_t stream_id, uint64_t first_cw, int batch, ldpc_frame_result *frames,
                        ldpc_counts *accum)
{
    const SimCall q{ebn0_db, R, seed, stream_id, first_cw, batch};
    RC_TRY(check_sim(c, [&] { return gdbf_check_cfg(cfg); }, q, true));
    return sim_batch_frames(c, batch, frames, accum, [&](ldpc_frame_result *w) { return gdbf_sim_run(c, q, cfg, w); });
}

int ldpc_gdbf_kernel_info(ldpc_ctx *c, const ldpc_gdbf_cfg *cfg, char *name, int name_len, int *lds_bytes)
{
    RC_TRY(gdbf_check_cfg(cfg));
    if (!c) return set_err(LDPC_ERR_INVALID, "ctx is null");
    const ldpc::OptScope os(c->opts);
    return report_choice(ldpc::gdbf_choose(c->dg, cfg->precision == LDPC_F64, cfg->flags, c->g->maxdv, c->g->maxdc), name,
                         name_len, lds_bytes);
}

// ----------------------------------------------------------------- re-decoding NGDBF
static int rgdbf_check_cfg(const ldpc_rgdbf_cfg *cfg)
{
    if (!cfg) return set_err(LDPC_ERR_INVALID, "cfg is null");
    if (cfg->precision != LDPC_F32 && cfg->precision != LDPC_F64)
        return set_err(LDPC_ERR_INVALID, "bad precision %d", cfg->precision);
    if (cfg->flags & ~511) return set_err(LDPC_ERR_INVALID, "unknown GDBF flags 0x%x", cfg->flags);
    if (cfg->flags & ~ldpc::kRgdbfFlags)
        return set_err(LDPC_ERR_UNSUPPORTED, "the re-decoding decoder takes NOISE|ADAPT|WEIGHT|SMOOTH|SATURATE only");
    // the reference reads an uninitialised `satisfied` at T 0
    if (cfg->T < 1) return set_err(LDPC_ERR_INVALID, "T must be >= 1");
    if (cfg->maxphase < 1) return set_err(LDPC_ERR_INVALID, "maxphase must be >= 1");
    if ((int64_t)cfg->maxphase * cfg->T > 4094)   // the 12-bit iteration field of the Philox stream word
        return set_err(LDPC_ERR_INVALID, "maxphase * T must be <= 4094");
    if ((cfg->flags & (LDPC_GDBF_SATURATE | LDPC_GDBF_WEIGHT)) && !(cfg->ymax > 0))
        return set_err(LDPC_ERR_INVALID, "saturate/weight need ymax > 0");
    if ((cfg->flags & LDPC_GDBF_SMOOTH) && (cfg->windowsize < 0 || cfg->windowsize > 32767))
        return set_err(LDPC_ERR_INVALID, "windowsize out of range");
    return LDPC_OK;
}

static void rgdbf_fill(ldpc::RgdbfArgs &a, ldpc_ctx *c, const ldpc_rgdbf_cfg *cfg, int batch)
{
    redecode_fill(a, c, cfg, batch);
    a.maxphase = cfg->maxphase;
}

static int rgdbf_run(ldpc_ctx *c, const ldpc::RgdbfArgs &a, bool f64)
{
    const ldpc::OptScope os(c->opts);
    const ldpc::RgdbfChoice ch = ldpc::rgdbf_choose(c->dg, f64, c->g->maxdv, c->g->maxdc);
    return run_with_slots(*c, c->gscratch, ch, a.batch, 2 * c->num_cus, [&](void *scratch, int slots) {
        return ldpc::rgdbf_launch(c->dg, a, f64, ch, scratch, slots, c->num_cus, c->stream);
    });
}

int ldpc_rgdbf_decode_batch(ldpc_ctx *c, const void *y, const void *pert, int batch, const ldpc_rgdbf_cfg *cfg,
                            const int8_t *cw, int8_t *d_out, ldpc_frame_result *frames, ldpc_counts *counts)
{
    if (!c || !y) return set_err(LDPC_ERR_INVALID, "null argument");
    RC_TRY(rgdbf_check_cfg(cfg));
    RC_TRY(check_batch(*c, batch));
    const bool noise = cfg->flags & LDPC_GDBF_NOISE;
    if (noise && !pert) return set_err(LDPC_ERR_INVALID, "NOISE needs pert");
    RC_TRY(c->enter());
    const bool f64 = cfg->precision == LDPC_F64;
    ldpc::RgdbfArgs a;
    rgdbf_fill(a, c, cfg, batch);
    SyncCall s(*c);
    RC_TRY(stage_given(s, c, a, f64, y, noise ? pert : nullptr,
                       (size_t)batch * c->g->N * (size_t)cfg->T * (size_t)cfg->maxphase, &a.pert, cw));
    RC_TRY(bind_decisions(s, c, a, d_out, frames));
    RC_TRY(s.snapshot());
    RC_TRY(rgdbf_run(c, a, f64));
    return s.finish(counts);
}

// After the checks and enter().
static int rgdbf_sim_run(ldpc_ctx *c, const SimCall &q, const ldpc_rgdbf_cfg *cfg, ldpc_frame_result *frames_dev)
{
    ldpc::RgdbfArgs a;
    rgdbf_fill(a, c, cfg, q.batch);
    fill_sim(a, *c, q);                                       // RNGDBF.cpp:167-168
    fill_cw_table(a, *c);
    a.frame_res = (int4 *)frames_dev;
    a.noise_sigma = a.sigma * cfg->noise_scale;               // :308
    return rgdbf_run(c, a, cfg->precision == LDPC_F64);
}

int ldpc_rgdbf_sim_launch(ldpc_ctx *c, double ebn0_db, double R, const ldpc_rgdbf_cfg *cfg, uint64_t seed,
                          uint32_t stream_id, uint64_t first_cw, int batch, ldpc_frame_result *frames_dev)
{
    const SimCall q{ebn0_db, R, seed, stream_id, first_cw, batch};
    RC_TRY(check_sim(c, [&] { return rgdbf_check_cfg(cfg); }, q, true));
    RC_TRY(require_device(frames_dev, kFramesDev));
    RC_TRY(c->enter());
    return rgdbf_sim_run(c, q, cfg, frames_dev);
}

int ldpc_rgdbf_sim_batch(ldpc_ctx *c, double ebn0_db, double R, const ldpc_rgdbf_cfg *cfg, uint64_t seed,
                         uint32_t stream_id, uint64_t first_cw, int batch, ldpc_frame_result *frames,
                         ldpc_counts *accum)
{
    const SimCall q{ebn0_db, R, seed, stream_id, first_cw, batch};
    RC_TRY(check_sim(c, [&] { return rgdbf_check_cfg(cfg); }, q, true));
    return sim_batch_frames(c, batch, frames, accum, [&](ldpc_frame_result *w) { return rgdbf_sim_run(c, q, cfg, w); });
}

int ldpc_rgdbf_kernel_info(ldpc_ctx *c, const ldpc_rgdbf_cfg *cfg, char *name, int name_len, int *lds_bytes)
{
    RC_TRY(rgdbf_check_cfg(cfg));
    if (!c) return set_err(LDPC_ERR_INVALID, "ctx is null");
    const ldpc::OptScope os(c->opts);
    return report_choice(ldpc::rgdbf_choose(c->dg, cfg->precision == LDPC_F64, c->g->maxdv, c->g->maxdc), name, name_len,
                         lds_bytes);
}

// ----------------------------------------------------------------- every attempt of every frame
static int rstat_check_cfg(const ldpc_rstat_cfg *cfg)
{
    if (!cfg) return set_err(LDPC_ERR_INVALID, "cfg is null");
    if (cfg->precision != LDPC_F32 && cfg->precision != LDPC_F64)
        return set_err(LDPC_ERR_INVALID, "bad precision %d", cfg->precision);
    if (cfg->flags & ~511) return set_err(LDPC_ERR_INVALID, "unknown GDBF flags 0x%x", cfg->flags);
    if (cfg->flags & ~ldpc::kRgdbfFlags)
        return set_err(LDPC_ERR_UNSUPPORTED, "the every-attempt decoder takes NOISE|ADAPT|WEIGHT|SMOOTH|SATURATE only");
    // T >= 1 as ldpc_rgdbf_cfg; 4094: the 12-bit iteration field of the Philox stream word
    if (cfg->T < 1 || cfg->T > 4094) return set_err(LDPC_ERR_INVALID, "T must be in 1..4094");
    if (cfg->attempts < 1) return set_err(LDPC_ERR_INVALID, "attempts must be >= 1");
    if (cfg->first_attempt < 0) return set_err(LDPC_ERR_INVALID, "first_attempt must be >= 0");
    if ((int64_t)cfg->first_attempt + cfg->attempts > INT32_MAX)
        return set_err(LDPC_ERR_INVALID, "first_attempt + attempts must be <= 2^31 - 1");
    // a frame's iterations, summed over its attempts, are an int32 (ldpc_frame_result.iters)
    if ((int64_t)cfg->attempts * cfg->T > INT32_MAX)
        return set_err(LDPC_ERR_INVALID, "attempts * T must be <= 2^31 - 1");
    if ((cfg->flags & (LDPC_GDBF_SATURATE | LDPC_GDBF_WEIGHT)) && !(cfg->ymax > 0))
        return set_err(LDPC_ERR_INVALID, "saturate/weight need ymax > 0");
    if ((cfg->flags & LDPC_GDBF_SMOOTH) && (cfg->windowsize < 0 || cfg->windowsize > 32767))
        return set_err(LDPC_ERR_INVALID, "windowsize out of range");
    return LDPC_OK;
}

static int rstat_check_batch(ldpc_ctx *c, const ldpc_rstat_cfg *cfg, int batch)
{
    RC_TRY(check_batch(*c, batch));
    if ((int64_t)batch * cfg->attempts > INT32_MAX)
        return set_err(LDPC_ERR_INVALID, "batch * attempts must be <= 2^31 - 1");
    return LDPC_OK;
}

// The refusals of the ldpc_rstat_sim_* calls that need no device.
static int rstat_check_sim(ldpc_ctx *c, const ldpc_rstat_cfg *cfg, const SimCall &q)
{
    if (!c) return set_err(LDPC_ERR_INVALID, "ctx is null");
    RC_TRY(rstat_check_cfg(cfg));
    RC_TRY(rstat_check_batch(c, cfg, q.batch));
    RC_TRY(check_sim_point(q, true));
    // the attempt index takes the high word of the frame number in the Philox counter
    if (q.first_cw > (1ull << 32) - (uint64_t)q.batch)
        return set_err(LDPC_ERR_INVALID, "first_cw + batch must be <= 2^32");
    return LDPC_OK;
}

static void rstat_fill(ldpc::RstatArgs &a, ldpc_ctx *c, const ldpc_rstat_cfg *cfg, int batch)
{
    redecode_fill(a, c, cfg, batch);
    a.attempts = cfg->attempts;
    a.first_attempt = cfg->first_attempt;
}

static void rstat_traces(const ldpc_rstat_trace *trace, void *tp[4])
{
    tp[0] = trace ? trace->err_trace : nullptr;
    tp[1] = trace ? trace->unsat_trace : nullptr;
    tp[2] = trace ? trace->d_trace : nullptr;
    tp[3] = trace ? trace->s_trace : nullptr;
}

// Binds attempts_out (the kernels write it whether or not the caller wants it) and the
// traces, and puts the "not run" values into the traces.
static int rstat_outs(SyncCall &s, ldpc_ctx *c, ldpc::RstatArgs &a, ldpc_attempt_result *attempts_out,
                      const ldpc_rstat_trace *trace)
{
    const size_t items = (size_t)a.batch * a.attempts, rows = items * (size_t)a.T;
    RC_TRY(s.out(attempts_out, c->rs_att_stage, sizeof(ldpc_attempt_result) * items, a.attempt_res, true));
    HIP_TRY(c->rs_unc.ensure(sizeof(int) * (size_t)a.batch));
    a.frame_unc = (int *)c->rs_unc.p;
    const size_t tb[4] = {rows * 4, rows * 4, rows * (size_t)c->g->N, rows * (size_t)c->g->M};
    void *tp[4], *dev[4];
    rstat_traces(trace, tp);
    for (int k = 0; k < 4; ++k) {
        RC_TRY(s.out(tp[k], c->rs_tr_stage[k], tb[k], dev[k]));
        if (dev[k]) HIP_TRY(hipMemsetAsync(dev[k], k < 2 ? 0xFF : 0, tb[k], c->stream));   // -1 / 0: not run
    }
    a.err_trace = (int32_t *)dev[0];
    a.unsat_trace = (int32_t *)dev[1];
    a.d_trace = (int8_t *)dev[2];
    a.s_trace = (int8_t *)dev[3];
    return LDPC_OK;
}

static int rstat_run(ldpc_ctx *c, const ldpc::RstatArgs &a, bool f64)
{
    const ldpc::OptScope os(c->opts);
    const bool trace = a.err_trace || a.unsat_trace || a.d_trace || a.s_trace;
    const ldpc::RstatChoice ch = ldpc::rstat_choose(c->dg, f64, trace, c->g->maxdv, c->g->maxdc);
    return run_with_slots(*c, c->gscratch, ch, (int64_t)a.batch * a.attempts, 2 * c->num_cus, [&](void *scratch, int slots) {
        return ldpc::rstat_launch(c->dg, a, f64, ch, scratch, slots, c->num_cus, c->stream);
    });
}

int ldpc_rstat_decode_batch(ldpc_ctx *c, const void *y, const void *pert, int batch, const ldpc_rstat_cfg *cfg,
                            const int8_t *cw, ldpc_attempt_result *attempts_out, const ldpc_rstat_trace *trace,
                            int8_t *d_out, ldpc_frame_result *frames, ldpc_counts *counts)
{
    if (!c || !y) return set_err(LDPC_ERR_INVALID, "null argument");
    RC_TRY(rstat_check_cfg(cfg));
    RC_TRY(rstat_check_batch(c, cfg, batch));
    const bool noise = cfg->flags & LDPC_GDBF_NOISE;
    if (noise && !pert) return set_err(LDPC_ERR_INVALID, "NOISE needs pert");
    RC_TRY(c->enter());
    const bool f64 = cfg->precision == LDPC_F64;
    ldpc::RstatArgs a;
    rstat_fill(a, c, cfg, batch);
    SyncCall s(*c);
    RC_TRY(bind_decisions(s, c, a, d_out, frames));   // fetched first
    RC_TRY(rstat_outs(s, c, a, attempts_out, trace));
    RC_TRY(stage_given(s, c, a, f64, y, noise ? pert : nullptr,
                       (size_t)batch * c->g->N * (size_t)cfg->attempts * (size_t)cfg->T, &a.pert, cw));
    RC_TRY(s.snapshot());
    RC_TRY(rstat_run(c, a, f64));
    return s.finish(counts);
}

// After the checks and enter(); `a` holds the outputs.
static int rstat_sim_run(ldpc_ctx *c, const SimCall &q, const ldpc_rstat_cfg *cfg, ldpc::RstatArgs &a)
{
    fill_sim(a, *c, q);                                       // newstat.cpp:192-193
    fill_cw_table(a, *c);
    a.noise_sigma = a.sigma * cfg->noise_scale;               // :336
    return rstat_run(c, a, cfg->precision == LDPC_F64);
}

int ldpc_rstat_sim_launch(ldpc_ctx *c, double ebn0_db, double R, const ldpc_rstat_cfg *cfg, uint64_t seed,
                          uint32_t stream_id, uint64_t first_cw, int batch, ldpc_attempt_result *attempts_dev,
                          const ldpc_rstat_trace *trace_dev, ldpc_frame_result *frames_dev)
{
    const SimCall q{ebn0_db, R, seed, stream_id, first_cw, batch};
    RC_TRY(rstat_check_sim(c, cfg, q));
    RC_TRY(require_device(frames_dev, kFramesDev));
    RC_TRY(require_device(attempts_dev, "attempts_out must be a device pointer"));
    void *tp[4];
    rstat_traces(trace_dev, tp);
    for (void *p : tp) RC_TRY(require_device(p, "the traces must be device pointers"));
    RC_TRY(c->enter());
    ldpc::RstatArgs a;
    rstat_fill(a, c, cfg, batch);
    SyncCall s(*c);   // device pointers only: nothing is staged, nothing to fetch
    RC_TRY(rstat_outs(s, c, a, attempts_dev, trace_dev));
    a.frame_res = (int4 *)frames_dev;
    return rstat_sim_run(c, q, cfg, a);
}

int ldpc_rstat_sim_trace(ldpc_ctx *c, double ebn0_db, double R, const ldpc_rstat_cfg *cfg, uint64_t seed,
                         uint32_t stream_id, uint64_t first_cw, int batch, void *y_out, void *pert_out,
                         ldpc_attempt_result *attempts_out, const ldpc_rstat_trace *trace, int8_t *d_out,
                         ldpc_frame_result *frames, ldpc_counts *accum)
{
    const SimCall q{ebn0_db, R, seed, stream_id, first_cw, batch};
    RC_TRY(rstat_check_sim(c, cfg, q));
    RC_TRY(c->enter());
    ldpc::RstatArgs a;
    rstat_fill(a, c, cfg, batch);
    SyncCall s(*c);
    RC_TRY(s.snapshot());
    const size_t fsz = cfg->precision == LDPC_F64 ? 8 : 4, nb = (size_t)batch * c->g->N;
    const size_t pb = nb * (size_t)cfg->attempts * (size_t)cfg->T * fsz;
    RC_TRY(s.out(y_out, c->y_stage, nb * fsz, a.y_out));
    RC_TRY(s.out(pert_out, c->p_stage, pb, a.pert_out));
    RC_TRY(bind_decisions(s, c, a, d_out, frames));
    if (a.pert_out) HIP_TRY(hipMemsetAsync(a.pert_out, 0, pb, c->stream));   // rows that are not drawn
    RC_TRY(rstat_outs(s, c, a, attempts_out, trace));
    RC_TRY(rstat_sim_run(c, q, cfg, a));
    return s.finish(accum);
}

int ldpc_rstat_sim_batch(ldpc_ctx *c, double ebn0_db, double R, const ldpc_rstat_cfg *cfg, uint64_t seed,
                         uint32_t stream_id, uint64_t first_cw, int batch, ldpc_attempt_result *attempts_out,
                         const ldpc_rstat_trace *trace, ldpc_frame_result *frames, ldpc_counts *accum)
{
    return ldpc_rstat_sim_trace(c, ebn0_db, R, cfg, seed, stream_id, first_cw, batch, nullptr, nullptr, attempts_out,
                                trace, nullptr, frames, accum);
}

int ldpc_rstat_kernel_info(ldpc_ctx *c, const ldpc_rstat_cfg *cfg, int with_trace, char *name, int name_len,
                           int *lds_bytes)
{
    RC_TRY(rstat_check_cfg(cfg));
    if (!c) return set_err(LDPC_ERR_INVALID, "ctx is null");
    const ldpc::OptScope os(c->opts);
    return report_choice(ldpc::rstat_choose(c->dg, cfg->precision == LDPC_F64, with_trace != 0, c->g->maxdv, c->g->maxdc),
                         name, name_len, lds_bytes);
}

// ----------------------------------------------------------------- fixed-point NGDBF hardware model
// N < 0: no graph at hand (kernel_info with a null context), qlen is checked against N later.
static int hwgdbf_check_cfg(const ldpc_hwgdbf_cfg *cfg, int N)
{
    if (!cfg) return set_err(LDPC_ERR_INVALID, "cfg is null");
    if (cfg->precision != LDPC_F32 && cfg->precision != LDPC_F64)
        return set_err(LDPC_ERR_INVALID, "bad precision %d", cfg->precision);
    if (cfg->reserved != 0) return set_err(LDPC_ERR_INVALID, "reserved must be 0");
    if (cfg->T < 1) return set_err(LDPC_ERR_INVALID, "T must be >= 1");
    if (cfg->maxphase < 1) return set_err(LDPC_ERR_INVALID, "maxphase must be >= 1");
    if ((int64_t)cfg->maxphase * cfg->T > INT32_MAX) return set_err(LDPC_ERR_INVALID, "maxphase * T overflows");
    if (cfg->nq < 2 || cfg->nq > 7) return set_err(LDPC_ERR_INVALID, "nq must be in 2..7");
    if (cfg->qlen < 1) return set_err(LDPC_ERR_INVALID, "qlen must be > N");
    if (!(cfg->w > 0) || !std::isfinite(cfg->w)) return set_err(LDPC_ERR_INVALID, "w must be > 0");
    if (!(cfg->ymax > 0) || !std::isfinite(cfg->ymax)) return set_err(LDPC_ERR_INVALID, "ymax must be > 0");
    // NGDBFhw.cpp reads qprime[i + qpointer] out of bounds there (:583 with :357)
    if (N >= 0 && cfg->qlen <= N) return set_err(LDPC_ERR_INVALID, "qlen %d must be > N = %d", cfg->qlen, N);
    return LDPC_OK;
}

// pack(quantize(2.0), +1) then unpack (NGDBFhw.cpp:178, :640-677), in double.
static int hwgdbf_theta(double lmax, int nq)
{
    const double NL = std::pow(2.0, nq) - 1.0;
    const long m = (long)std::floor(2.0 * NL / (2.0 * lmax));
    const long code = m & ((1l << nq) - 1);
    const int mag = (int)(((code & ((1l << (nq - 1)) - 1)) << 1) | 1);
    return (code >> (nq - 1)) & 1 ? -mag : mag;
}

// The kernel instance for cfg->qlen on the context's graph, or the refusal when one codeword's state exceeds LDS.
static int hwgdbf_pick(ldpc_ctx *c, const ldpc_hwgdbf_cfg *cfg, ldpc::HwgdbfChoice &ch)
{
    const ldpc::OptScope os(c->opts);
    ch = ldpc::hwgdbf_choose(c->dg, c->g->E, cfg->qlen);
    if (!ch.name[0])
        return set_err(LDPC_ERR_UNSUPPORTED,
                       "NGDBFhw keeps a codeword in LDS: N + qlen + N + M = %d bytes exceed the bound of %d", ch.cw_bytes,
                       ldpc::kHwgdbfMaxLds);
    return LDPC_OK;
}

// Host work only (its refusals come before enter()).
static int hwgdbf_fill(ldpc::HwgdbfArgs &a, ldpc::HwgdbfChoice &ch, ldpc_ctx *c, const ldpc_hwgdbf_cfg *cfg, int batch)
{
    std::memset((void *)&a, 0, sizeof a);
    a.batch = batch;
    a.T = cfg->T;
    a.maxphase = cfg->maxphase;
    a.nq = cfg->nq;
    a.qlen = cfg->qlen;
    a.two_w = 2.0 * cfg->w;
    a.ymax = cfg->ymax;
    a.lmax = cfg->ymax / (2.0 * cfg->w);                          // :175
    a.theta0 = cfg->theta0;
    const double NL = std::pow(2.0, cfg->nq) - 1.0;
    const double sm = std::round(NL / a.lmax);                    // :179
    if (!(sm >= 0 && sm <= 65535)) return set_err(LDPC_ERR_INVALID, "Smult = round(NL / lmax) = %g out of range", sm);
    a.smult = (int)sm;
    a.theta = hwgdbf_theta(a.lmax, cfg->nq);
    fill_accounting(a, *c);
    return hwgdbf_pick(c, cfg, ch);
}

static int hwgdbf_run(ldpc_ctx *c, const ldpc::HwgdbfArgs &a, const ldpc::HwgdbfChoice &ch, bool f64)
{
    RC_TRY(c->begin_launch());
    HIP_TRY(ldpc::hwgdbf_launch(c->dg, a, f64, ch, c->g->E, c->num_cus, c->stream));
    return c->end_launch();
}

int ldpc_hwgdbf_decode_batch(ldpc_ctx *c, const void *y, const void *q, const int32_t *qptr0, int batch,
                             const ldpc_hwgdbf_cfg *cfg, const int8_t *cw, int8_t *d_out, ldpc_frame_result *frames,
                             int32_t *iters_run, ldpc_counts *counts)
{
    if (!c || !y || !q) return set_err(LDPC_ERR_INVALID, "null argument");
    RC_TRY(hwgdbf_check_cfg(cfg, c->g->N));
    RC_TRY(check_batch(*c, batch));
    ldpc::HwgdbfArgs a;
    ldpc::HwgdbfChoice ch;
    RC_TRY(hwgdbf_fill(a, ch, c, cfg, batch));
    const int N = c->g->N;
    if (qptr0 && !is_device_ptr(qptr0))   // a device array is clamped by the kernel
        for (int b = 0; b < batch; ++b)
            if (qptr0[b] < 0 || qptr0[b] >= cfg->qlen - N)
                return set_err(LDPC_ERR_INVALID, "qptr0[%d] = %d outside [0, qlen - N = %d)", b, qptr0[b], cfg->qlen - N);
    RC_TRY(c->enter());
    const bool f64 = cfg->precision == LDPC_F64;
    SyncCall s(*c);
    RC_TRY(stage_given(s, c, a, f64, y, q, (size_t)batch * cfg->qlen, &a.q, cw));
    RC_TRY(s.in(qptr0, sizeof(int32_t) * (size_t)batch, c->hw_ptr_stage, a.qptr0));
    RC_TRY(bind_decisions(s, c, a, d_out, frames));
    RC_TRY(s.out(iters_run, c->hw_it_stage, sizeof(int32_t) * (size_t)batch, a.iters_run));
    RC_TRY(s.snapshot());
    RC_TRY(hwgdbf_run(c, a, ch, f64));
    return s.finish(counts);
}

// The refusals of the ldpc_hwgdbf_sim_* calls that need no device, and the launch arguments of cfg.
static int hwgdbf_sim_setup(ldpc_ctx *c, const SimCall &q, const ldpc_hwgdbf_cfg *cfg, ldpc::HwgdbfArgs &a,
                            ldpc::HwgdbfChoice &ch)
{
    RC_TRY(check_sim(c, [&] { return hwgdbf_check_cfg(cfg, c->g->N); }, q, true));
    RC_TRY(hwgdbf_fill(a, ch, c, cfg, q.batch));
    const SimPoint pt = fill_sim(a, *c, q);                   // NGDBFhw.cpp:127-129
    fill_cw_table(a, *c);
    a.noise_sigma = pt.sigma * cfg->noise_scale;
    return LDPC_OK;
}

int ldpc_hwgdbf_sim_launch(ldpc_ctx *c, double ebn0_db, double R, const ldpc_hwgdbf_cfg *cfg, uint64_t seed,
                           uint32_t stream_id, uint64_t first_cw, int batch, ldpc_frame_result *frames_dev)
{
    ldpc::HwgdbfArgs a;
    ldpc::HwgdbfChoice ch;
    RC_TRY(hwgdbf_sim_setup(c, {ebn0_db, R, seed, stream_id, first_cw, batch}, cfg, a, ch));
    RC_TRY(require_device(frames_dev, kFramesDev));
    RC_TRY(c->enter());
    a.frame_res = (int4 *)frames_dev;
    return hwgdbf_run(c, a, ch, cfg->precision == LDPC_F64);
}

int ldpc_hwgdbf_sim_trace(ldpc_ctx *c, double ebn0_db, double R, const ldpc_hwgdbf_cfg *cfg, uint64_t seed,
                          uint32_t stream_id, uint64_t first_cw, int batch, void *y_out, void *q_out, int8_t *d_out,
                          ldpc_frame_result *frames, ldpc_counts *accum)
{
    ldpc::HwgdbfArgs a;
    ldpc::HwgdbfChoice ch;
    RC_TRY(hwgdbf_sim_setup(c, {ebn0_db, R, seed, stream_id, first_cw, batch}, cfg, a, ch));
    RC_TRY(c->enter());
    SyncCall s(*c);
    RC_TRY(s.snapshot());
    const size_t fsz = cfg->precision == LDPC_F64 ? 8 : 4;
    RC_TRY(s.out(y_out, c->y_stage, (size_t)batch * c->g->N * fsz, a.y_out));
    RC_TRY(s.out(q_out, c->p_stage, (size_t)batch * cfg->qlen * fsz, a.q_out));
    RC_TRY(bind_decisions(s, c, a, d_out, frames));
    RC_TRY(hwgdbf_run(c, a, ch, cfg->precision == LDPC_F64));
    return s.finish(accum);
}

int ldpc_hwgdbf_sim_batch(ldpc_ctx *c, double ebn0_db, double R, const ldpc_hwgdbf_cfg *cfg, uint64_t seed,
                          uint32_t stream_id, uint64_t first_cw, int batch, ldpc_frame_result *frames,
                          ldpc_counts *accum)
{
    return ldpc_hwgdbf_sim_trace(c, ebn0_db, R, cfg, seed, stream_id, first_cw, batch, nullptr, nullptr, nullptr, frames,
                                 accum);
}

int ldpc_hwgdbf_kernel_info(ldpc_ctx *c, const ldpc_hwgdbf_cfg *cfg, char *name, int name_len, int *lds_bytes)
{
    RC_TRY(hwgdbf_check_cfg(cfg, c ? c->g->N : -1));
    if (!c) return set_err(LDPC_ERR_INVALID, "ctx is null");
    ldpc::HwgdbfChoice ch;
    RC_TRY(hwgdbf_pick(c, cfg, ch));
    return report_choice(ch, name, name_len, lds_bytes);
}

}  // extern "C"

// ----------------------------------------------------------------- fixed-point min-sum, flooding and layered
// One set of entry points over a traits type X: Cfg and Args, the cfg check, the arguments
// beyond fx_fill, the kernel instance for the cfg on the context's graph (or the refusal when
// one codeword's state exceeds LDS), what a launch needs first, and the launch.
struct FxmsApi {
    using Cfg = ldpc_fxms_cfg;
    using Args = ldpc::FxmsArgs;
    using Choice = ldpc::FxmsChoice;
    static int check_cfg(const Cfg *cfg)
    {
        return fx_check_cfg(cfg, [&] { return cfg->reserved != 0 ? set_err(LDPC_ERR_INVALID, "reserved must be 0") : LDPC_OK; });
    }
    static void fill_extra(Args &, const Cfg *) {}
    static int pick(ldpc_ctx *c, const Cfg *cfg, Choice &ch)
    {
        ch = ldpc::fxms_choose(c->dg, c->g->E, cfg->msg_bits);
        if (!ch.name[0])
            return set_err(LDPC_ERR_UNSUPPORTED,
                           "fixed-point min-sum keeps a codeword in LDS: maxdc * M messages + 2 N = %d bytes exceed the "
                           "bound of %d",
                           ch.cw_bytes, ldpc::kFxmsMaxLds);
        return LDPC_OK;
    }
    static int prepare(ldpc_ctx *, const Args &, const Choice &, bool) { return LDPC_OK; }
    static hipError_t launch(ldpc_ctx *c, const Args &a, const Choice &ch, bool f64)
    {
        return ldpc::fxms_launch(c->dg, a, f64, ch, c->g->E, c->num_cus, c->stream);
    }
};

struct FxlmsApi {
    using Cfg = ldpc_fxlms_cfg;
    using Args = ldpc::FxlmsArgs;
    using Choice = ldpc::FxlmsChoice;
    static int check_cfg(const Cfg *cfg)
    {
        RC_TRY(fx_check_cfg(cfg, [] { return LDPC_OK; }));
        if (cfg->app_bits < cfg->msg_bits || cfg->app_bits > 16)
            return set_err(LDPC_ERR_INVALID, "app_bits must be in msg_bits..16 = %d..16", cfg->msg_bits);
        return LDPC_OK;
    }
    static void fill_extra(Args &a, const Cfg *cfg) { a.amax = (1 << (cfg->app_bits - 1)) - 1; }
    // (The choice reads the graph's sizes only: no schedule, no device.) LDPC_OPT_KERNEL = 3
    // ("global") takes the workgroup kernel, whose row state is in global memory (fxlms_wg.hip).
    static int pick(ldpc_ctx *c, const Cfg *cfg, Choice &ch)
    {
        ldpc::FxlmsSched sizes;
        sizes.N = c->g->N;
        sizes.M = c->g->M;
        sizes.dcs = c->g->maxdc > 0 ? c->g->maxdc : 1;
        if (c->opts.v[LDPC_OPT_KERNEL] == 3) {
            ch = ldpc::fxlms_wg_choose(sizes, cfg->app_bits);
            if (!ch.name[0])
                return set_err(LDPC_ERR_UNSUPPORTED,
                               "layered fixed-point min-sum with LDPC_OPT_KERNEL = 3 keeps a codeword's APPs in LDS: N APPs + "
                               "%d bytes of scratch = %d bytes exceed the bound of %d",
                               ldpc::kFxlmsWgRed, ch.cw_bytes, (int)ldpc::kWaveCwLds);
            return LDPC_OK;
        }
        ch = ldpc::fxlms_choose(sizes, cfg->app_bits);
        if (!ch.name[0])
            return set_err(LDPC_ERR_UNSUPPORTED,
                           "layered fixed-point min-sum keeps a codeword in LDS: N APPs + the packed state of M rows = %d "
                           "bytes exceed the bound of %d; LDPC_OPT_KERNEL = 3 (global) selects the kernel that keeps the "
                           "rows' state in global memory",
                           ch.cw_bytes, ldpc::kFxlmsMaxLds);
        return LDPC_OK;
    }
    // The layered row order on the device, built and uploaded by the context's first fxlms launch (after
    // enter()), so that a context that never decodes with fxlms is created as before.
    // The workgroup kernel's global slots, one per workgroup of this launch, grow with the grid.
    static int prepare(ldpc_ctx *c, const Args &a, const Choice &ch, bool f64)
    {
        RC_TRY(prepare_sched(c));
        if (!ch.wg) return LDPC_OK;
        c->fxl_wg_grid = ldpc::fxlms_wg_grid(a, f64, ch, c->num_cus);
        HIP_TRY(c->gscratch.ensure((size_t)ch.slot_bytes * (size_t)c->fxl_wg_grid));
        return LDPC_OK;
    }
    static int prepare_sched(ldpc_ctx *c)
    {
        if (c->has_fxl) return LDPC_OK;
        ldpc::FloodSchedule fh;
        ldpc::LayerSchedule lh;
        std::string err;
        try {
            err = ldpc::build_flood_schedule(*c->g, fh, ldpc::kMaxRowDegree);
            if (err.empty()) err = ldpc::build_layers(*c->g, fh, lh);
        } catch (const std::bad_alloc &) {
            return set_err(LDPC_ERR_NOMEM, "layer schedule out of memory");
        }
        if (!err.empty()) return set_err(LDPC_ERR_UNSUPPORTED, "no layer schedule for this graph: %s", err.c_str());
        HIP_TRY(upload_fxlms_sched(*c->g, lh, c->fxl_sched, c->fxl));
        c->has_fxl = true;
        return LDPC_OK;
    }
    static hipError_t launch(ldpc_ctx *c, const Args &a, const Choice &ch, bool f64)
    {
        if (ch.wg) return ldpc::fxlms_wg_launch(c->fxl, a, f64, ch, c->gscratch.p, c->fxl_wg_grid, c->stream);
        return ldpc::fxlms_launch(c->fxl, a, f64, ch, c->num_cus, c->stream);
    }
};

// Host work only (its refusals come before enter()).
template <class X>
static int fx_setup(typename X::Args &a, typename X::Choice &ch, ldpc_ctx *c, const typename X::Cfg *cfg, int batch)
{
    fx_fill(a, c, cfg, batch);
    X::fill_extra(a, cfg);
    return X::pick(c, cfg, ch);
}

template <class X> static int fx_run(ldpc_ctx *c, const typename X::Args &a, const typename X::Choice &ch, bool f64)
{
    RC_TRY(X::prepare(c, a, ch, f64));
    RC_TRY(c->begin_launch());
    HIP_TRY(X::launch(c, a, ch, f64));
    return c->end_launch();
}

template <class X>
static int fx_decode_batch(ldpc_ctx *c, const void *y, int batch, const typename X::Cfg *cfg, const int8_t *cw, int8_t *d_out,
                           ldpc_frame_result *frames, ldpc_counts *counts)
{
    if (!c || !y) return set_err(LDPC_ERR_INVALID, "null argument");
    RC_TRY(X::check_cfg(cfg));
    RC_TRY(check_batch(*c, batch));
    typename X::Args a;
    typename X::Choice ch;
    RC_TRY(fx_setup<X>(a, ch, c, cfg, batch));
    RC_TRY(c->enter());
    const bool f64 = cfg->precision == LDPC_F64;
    SyncCall s(*c);
    RC_TRY(stage_given(s, c, a, f64, y, nullptr, 0, nullptr, cw));
    RC_TRY(bind_decisions(s, c, a, d_out, frames));
    RC_TRY(s.snapshot());
    RC_TRY(fx_run<X>(c, a, ch, f64));
    return s.finish(counts);
}

// The refusals of the sim_* calls that need no device, and the launch arguments of cfg.
template <class X>
static int fx_sim_setup(ldpc_ctx *c, const SimCall &q, const typename X::Cfg *cfg, typename X::Args &a, typename X::Choice &ch)
{
    RC_TRY(check_sim(c, [&] { return X::check_cfg(cfg); }, q, false));
    RC_TRY(fx_setup<X>(a, ch, c, cfg, q.batch));
    fill_sim(a, *c, q);
    fill_cw_table(a, *c);
    return LDPC_OK;
}

template <class X>
static int fx_sim_launch(ldpc_ctx *c, const SimCall &q, const typename X::Cfg *cfg, ldpc_frame_result *frames_dev)
{
    typename X::Args a;
    typename X::Choice ch;
    RC_TRY(fx_sim_setup<X>(c, q, cfg, a, ch));
    RC_TRY(require_device(frames_dev, kFramesDev));
    RC_TRY(c->enter());
    a.frame_res = (int4 *)frames_dev;
    return fx_run<X>(c, a, ch, cfg->precision == LDPC_F64);
}

template <class X>
static int fx_sim_trace(ldpc_ctx *c, const SimCall &q, const typename X::Cfg *cfg, void *y_out, int8_t *ycode_out,
                        int8_t *d_out, ldpc_frame_result *frames, ldpc_counts *accum)
{
    typename X::Args a;
    typename X::Choice ch;
    RC_TRY(fx_sim_setup<X>(c, q, cfg, a, ch));
    RC_TRY(c->enter());
    SyncCall s(*c);
    RC_TRY(s.snapshot());
    const size_t nb = (size_t)q.batch * c->g->N;
    RC_TRY(s.out(y_out, c->y_stage, nb * (cfg->precision == LDPC_F64 ? 8 : 4), a.y_out));
    RC_TRY(s.out(ycode_out, c->fx_code_stage, nb, a.ycode_out));
    RC_TRY(bind_decisions(s, c, a, d_out, frames));
    RC_TRY(fx_run<X>(c, a, ch, cfg->precision == LDPC_F64));
    return s.finish(accum);
}

template <class X>
static int fx_kernel_info(ldpc_ctx *c, const typename X::Cfg *cfg, char *name, int name_len, int *lds_bytes)
{
    RC_TRY(X::check_cfg(cfg));
    if (!c) return set_err(LDPC_ERR_INVALID, "ctx is null");
    typename X::Choice ch;
    RC_TRY(X::pick(c, cfg, ch));
    return report_choice(ch, name, name_len, lds_bytes);
}

extern "C" {

int ldpc_fxms_decode_batch(ldpc_ctx *c, const void *y, int batch, const ldpc_fxms_cfg *cfg, const int8_t *cw,
                           int8_t *d_out, ldpc_frame_result *frames, ldpc_counts *counts)
{
    return fx_decode_batch<FxmsApi>(c, y, batch, cfg, cw, d_out, frames, counts);
}
int ldpc_fxms_sim_launch(ldpc_ctx *c, double ebn0_db, double R, const ldpc_fxms_cfg *cfg, uint64_t seed,
                         uint32_t stream_id, uint64_t first_cw, int batch, ldpc_frame_result *frames_dev)
{
    return fx_sim_launch<FxmsApi>(c, {ebn0_db, R, seed, stream_id, first_cw, batch}, cfg, frames_dev);
}
int ldpc_fxms_sim_trace(ldpc_ctx *c, double ebn0_db, double R, const ldpc_fxms_cfg *cfg, uint64_t seed,
                        uint32_t stream_id, uint64_t first_cw, int batch, void *y_out, int8_t *ycode_out, int8_t *d_out,
                        ldpc_frame_result *frames, ldpc_counts *accum)
{
    return fx_sim_trace<FxmsApi>(c, {ebn0_db, R, seed, stream_id, first_cw, batch}, cfg, y_out, ycode_out, d_out, frames, accum);
}
int ldpc_fxms_sim_batch(ldpc_ctx *c, double ebn0_db, double R, const ldpc_fxms_cfg *cfg, uint64_t seed,
                        uint32_t stream_id, uint64_t first_cw, int batch, ldpc_frame_result *frames, ldpc_counts *accum)
{
    return fx_sim_trace<FxmsApi>(c, {ebn0_db, R, seed, stream_id, first_cw, batch}, cfg, nullptr, nullptr, nullptr, frames, accum);
}
int ldpc_fxms_kernel_info(ldpc_ctx *c, const ldpc_fxms_cfg *cfg, char *name, int name_len, int *lds_bytes)
{
    return fx_kernel_info<FxmsApi>(c, cfg, name, name_len, lds_bytes);
}

int ldpc_fxlms_decode_batch(ldpc_ctx *c, const void *y, int batch, const ldpc_fxlms_cfg *cfg, const int8_t *cw,
                            int8_t *d_out, ldpc_frame_result *frames, ldpc_counts *counts)
{
    return fx_decode_batch<FxlmsApi>(c, y, batch, cfg, cw, d_out, frames, counts);
}
int ldpc_fxlms_sim_launch(ldpc_ctx *c, double ebn0_db, double R, const ldpc_fxlms_cfg *cfg, uint64_t seed,
                          uint32_t stream_id, uint64_t first_cw, int batch, ldpc_frame_result *frames_dev)
{
    return fx_sim_launch<FxlmsApi>(c, {ebn0_db, R, seed, stream_id, first_cw, batch}, cfg, frames_dev);
}
int ldpc_fxlms_sim_trace(ldpc_ctx *c, double ebn0_db, double R, const ldpc_fxlms_cfg *cfg, uint64_t seed,
                         uint32_t stream_id, uint64_t first_cw, int batch, void *y_out, int8_t *ycode_out, int8_t *d_out,
                         ldpc_frame_result *frames, ldpc_counts *accum)
{
    return fx_sim_trace<FxlmsApi>(c, {ebn0_db, R, seed, stream_id, first_cw, batch}, cfg, y_out, ycode_out, d_out, frames, accum);
}
int ldpc_fxlms_sim_batch(ldpc_ctx *c, double ebn0_db, double R, const ldpc_fxlms_cfg *cfg, uint64_t seed,
                         uint32_t stream_id, uint64_t first_cw, int batch, ldpc_frame_result *frames, ldpc_counts *accum)
{
    return fx_sim_trace<FxlmsApi>(c, {ebn0_db, R, seed, stream_id, first_cw, batch}, cfg, nullptr, nullptr, nullptr, frames, accum);
}
int ldpc_fxlms_kernel_info(ldpc_ctx *c, const ldpc_fxlms_cfg *cfg, char *name, int name_len, int *lds_bytes)
{
    return fx_kernel_info<FxlmsApi>(c, cfg, name, name_len, lds_bytes);
}

}  // extern "C"
