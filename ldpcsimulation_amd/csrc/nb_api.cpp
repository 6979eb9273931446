// nb_api.cpp -- C ABI of the non-binary GF(q) EMS decoder (include/ldpc_hip.h,
// "non-binary" section): NB alist loading with the semantics of the
// reference's SystemC/NB-LDPC/src/alist.cpp:23-56 (plus validation), device
// contexts, decode of given channel samples and the fused Monte-Carlo.
#include "ldpc_hip.h"
#include "nb.h"
#include "nb_graph.h"
#include "host_rt.h"
#include "kernels.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

using namespace ldpc;   // host_rt.h: set_err, HIP_TRY, DevBuf, CtxCore, Blob and the call skeleton

struct ldpc_nb_ctx : CtxCore {
    const ldpc_nb_graph *g = nullptr;
    ldpc::NbDevGraph dg{};
    DevBuf graph, y_stage, c_stage, d_stage, fr_stage, scratch;
    const uint8_t *col_h_swz = nullptr;   // device: col_h with the slot swizzles (nb_swizzled_coefficients)
    ldpc::NbDevSched ds{};                // device: the packed schedule (ems_global_sched reads it in place)
};

// LDPC_OPT_EMS_SWIZZLE = 1 keeps the plain message layout (A/B).
static bool nb_swizzle_enabled() { return ldpc::opt(LDPC_OPT_EMS_SWIZZLE) != 1; }

extern "C" {

int ldpc_nb_graph_create(int N, int M, int q, const int *num_nlist, const int *const *nlist, const int *const *nvals,
                         const int *num_mlist, const int *const *mlist, const int *const *mvals, ldpc_nb_graph **out)
{
    if (!out || !num_nlist || !nlist || !nvals || !num_mlist || !mlist || !mvals)
        return set_err(LDPC_ERR_INVALID, "null argument");
    *out = nullptr;
    if (N <= 0 || M <= 0) return set_err(LDPC_ERR_GRAPH, "bad dimensions N=%d M=%d", N, M);
    try {
        ldpc::NbLists cols(N), rows(M);
        for (int i = 0; i < N; ++i)
            for (int k = 0; k < num_nlist[i]; ++k) cols[i].push_back({nlist[i][k] - 1, nvals[i][k]});
        for (int j = 0; j < M; ++j)
            for (int k = 0; k < num_mlist[j]; ++k) rows[j].push_back({mlist[j][k] - 1, mvals[j][k]});
        std::unique_ptr<ldpc_nb_graph> g(new ldpc_nb_graph());
        std::string msg;
        const int rc = ldpc::nb_build_graph(N, M, q, cols, rows, *g, msg);
        if (rc) return set_err(rc, "%s", msg.c_str());
        *out = g.release();
    } catch (const std::bad_alloc &) {
        return set_err(LDPC_ERR_NOMEM, "graph build out of memory");
    }
    return LDPC_OK;
}

int ldpc_nb_graph_load_alist(const char *path, ldpc_nb_graph **out)
{
    if (!path || !out) return set_err(LDPC_ERR_INVALID, "null argument");
    *out = nullptr;
    try {
        std::unique_ptr<ldpc_nb_graph> g(new ldpc_nb_graph());
        std::string msg;
        const int rc = ldpc::nb_read_alist(path, *g, msg);
        if (rc) return set_err(rc, "%s", msg.c_str());
        *out = g.release();
    } catch (const std::bad_alloc &) {
        return set_err(LDPC_ERR_NOMEM, "alist load out of memory");
    }
    return LDPC_OK;
}

int ldpc_nb_graph_info(const ldpc_nb_graph *g, int *N, int *M, int *q, int *E, int *maxdv, int *maxdc)
{
    if (!g) return set_err(LDPC_ERR_INVALID, "graph is null");
    if (N) *N = g->N;
    if (M) *M = g->M;
    if (q) *q = g->q;
    if (E) *E = g->E;
    if (maxdv) *maxdv = g->maxdv;
    if (maxdc) *maxdc = g->maxdc;
    return LDPC_OK;
}

void ldpc_nb_graph_destroy(ldpc_nb_graph *g) { delete g; }

// Everything ldpc_nb_ctx_create puts on the device; on failure the caller frees the context.
static int nb_ctx_init(ldpc_nb_ctx *c, int device, const ldpc_nb_graph *g, int max_batch)
{
    c->g = g;
    RC_TRY(c->init(device, max_batch));
    // graph upload: row_ptr | row_col | col_ptr | col_slot | row_h | gf_mul | gf_inv | pslot | colh | colh_swz
    //               | cn_d | vn | vslot
    ldpc::NbTables tb;
    ldpc::nb_tables(*g, tb);
    Blob b(16);
    const size_t o_rp = b.add(g->row_ptr), o_rc = b.add(g->row_col), o_cp = b.add(g->col_ptr),
                 o_cs = b.add(g->col_slot), o_h = b.add(g->row_h), o_mul = b.add(tb.mul), o_inv = b.add(tb.inv),
                 o_ps = b.add(tb.pslot), o_ch = b.add(tb.colh), o_chs = b.add(tb.colh_swz),
                 o_cd = b.add(tb.cn_d), o_vn = b.add(tb.vn), o_vs = b.add(tb.vslot);
    HIP_TRY(upload(b, c->graph));
    const auto *base = (const uint8_t *)c->graph.p;
    c->dg.N = g->N;
    c->dg.M = g->M;
    c->dg.q = g->q;
    c->dg.m = g->m;
    c->dg.E = g->E;
    c->dg.row_ptr = (const int32_t *)(base + o_rp);
    c->dg.row_col = (const int32_t *)(base + o_rc);
    c->dg.col_ptr = (const int32_t *)(base + o_cp);
    c->dg.col_slot = (const int32_t *)(base + o_cs);
    c->dg.row_h = base + o_h;
    c->dg.gf_mul = base + o_mul;
    c->dg.gf_inv = base + o_inv;
    c->dg.col_pslot = (const int32_t *)(base + o_ps);
    c->dg.col_h = base + o_ch;
    c->col_h_swz = base + o_chs;
    c->ds.cn_d = base + o_cd;
    c->ds.vn = (const uint32_t *)(base + o_vn);
    c->ds.vslot = (const uint16_t *)(base + o_vs);
    c->dg.maxdc = g->maxdc;
    if (!ldpc::nb_choose(c->dg, g->maxdc).ok)
        return set_err(LDPC_ERR_UNSUPPORTED, "code too large for the EMS kernels (N=%d, M=%d, E=%d, q=%d)", g->N, g->M,
                       g->E, g->q);
    return LDPC_OK;
}

int ldpc_nb_ctx_create(int device, const ldpc_nb_graph *g, int max_batch, ldpc_nb_ctx **out)
{
    if (!g || !out) return set_err(LDPC_ERR_INVALID, "null argument");
    *out = nullptr;
    if (max_batch <= 0) return set_err(LDPC_ERR_INVALID, "max_batch must be > 0");
    if (!ldpc::nb_q_supported(g->q))
        return set_err(LDPC_ERR_UNSUPPORTED, "the EMS kernels are built for GF(4), GF(8) and GF(16), got q=%d (%s)", g->q,
                       g->q == 2 ? "binary codes have their own decoders" : "its check lanes would not hold their vectors");
    if (g->maxdc > ldpc::kNbMaxDc) return set_err(LDPC_ERR_UNSUPPORTED, "row degree %d > %d", g->maxdc, ldpc::kNbMaxDc);
    if (g->maxdv > 255) return set_err(LDPC_ERR_UNSUPPORTED, "column degree %d > 255", g->maxdv);
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return set_err(LDPC_ERR_INVALID, "device %d outside 0..%d", device, ndev - 1);
    auto *c = new (std::nothrow) ldpc_nb_ctx();
    if (!c) return set_err(LDPC_ERR_NOMEM, "context allocation failed");
    const int rc = nb_ctx_init(c, device, g, max_batch);
    if (rc) {
        ldpc_nb_ctx_destroy(c);
        return rc;
    }
    *out = c;
    return LDPC_OK;
}

int ldpc_nb_ctx_set_stream(ldpc_nb_ctx *c, void *hip_stream)
{
    return c ? c->set_stream(hip_stream) : set_err(LDPC_ERR_INVALID, "ctx is null");
}

void ldpc_nb_ctx_destroy(ldpc_nb_ctx *c)
{
    if (!c) return;
    c->destroy({&c->graph, &c->y_stage, &c->c_stage, &c->d_stage, &c->fr_stage, &c->scratch});
    delete c;
}

static int check_ems(const ldpc_nb_ctx *c, const ldpc_ems_cfg *cfg, int batch)
{
    if (!c || !cfg) return set_err(LDPC_ERR_INVALID, "null argument");
    RC_TRY(check_batch(*c, batch));
    if (cfg->T < 0) return set_err(LDPC_ERR_INVALID, "T must be >= 0");
    if (cfg->nm < 1) return set_err(LDPC_ERR_INVALID, "nm must be >= 1");
    if (!(cfg->offset >= 0)) return set_err(LDPC_ERR_INVALID, "offset must be >= 0");
    return LDPC_OK;
}

static int run(ldpc_nb_ctx *c, const ldpc::NbArgs &a)
{
    const ldpc::OptScope os(c->opts);
    const ldpc::NbChoice ch = ldpc::nb_choose(c->dg, c->g->maxdc);
    ldpc::NbDevGraph dg = c->dg;
    // untruncated messages (nm >= q): the XOR-swizzled layout; truncation ranks
    // entries by symbol on ties, so it keeps the plain one (nb.hip vn_lane)
    if (a.nm >= dg.q && nb_swizzle_enabled()) dg.col_h = c->col_h_swz;
    return run_with_slots(*c, c->scratch, ch, a.batch, c->num_cus, [&](void *scratch, int slots) {
        return ldpc::nb_launch(dg, a, ch, c->ds, scratch, slots, c->num_cus, c->stream);
    });
}

static void fill_cfg(ldpc::NbArgs &a, ldpc_nb_ctx *c, const ldpc_ems_cfg *cfg, int batch)
{
    std::memset(&a, 0, sizeof a);
    a.batch = batch;
    a.T = cfg->T;
    a.nm = cfg->nm;
    a.early_stop = cfg->early_stop ? 1 : 0;
    a.offset = (float)cfg->offset;
    a.counts = (unsigned long long *)c->counts.p;
    a.ticket = c->ticket();
}

// The decided symbols and the frame records, host or device.
static int bind_decisions(SyncCall &s, ldpc_nb_ctx *c, ldpc::NbArgs &a, uint8_t *d_out, ldpc_frame_result *frames)
{
    RC_TRY(s.out(d_out, c->d_stage, (size_t)a.batch * c->g->N, a.d_out));
    return s.out(frames, c->fr_stage, sizeof(ldpc_frame_result) * (size_t)a.batch, a.frame_res);
}

int ldpc_ems_decode_batch(ldpc_nb_ctx *c, const float *y, int batch, double n0, const ldpc_ems_cfg *cfg,
                          const uint8_t *cw, uint8_t *d_out, ldpc_frame_result *frames, ldpc_nb_counts *counts)
{
    RC_TRY(check_ems(c, cfg, batch));
    if (!y) return set_err(LDPC_ERR_INVALID, "y is null");
    if (!(n0 > 0)) return set_err(LDPC_ERR_INVALID, "n0 must be > 0");
    RC_TRY(c->enter());
    const int N = c->g->N, m = c->g->m;
    ldpc::NbArgs a;
    fill_cfg(a, c, cfg, batch);
    a.src = ldpc::SRC_GIVEN;
    a.n0 = (float)n0;
    const size_t nb = (size_t)batch * N;
    SyncCall s(*c);
    RC_TRY(s.in(y, nb * m * sizeof(float), c->y_stage, a.y));
    RC_TRY(s.in(cw, nb, c->c_stage, a.c));
    if (a.c != cw)   // staged, so cw is host memory: its symbols can be checked (before anything reads the copy)
        for (size_t i = 0; i < nb; ++i)
            if (cw[i] >= (unsigned)c->g->q)
                return set_err(LDPC_ERR_INVALID, "codeword symbol %zu is %d (q=%d)", i, cw[i], c->g->q);
    RC_TRY(bind_decisions(s, c, a, d_out, frames));
    RC_TRY(s.snapshot());
    RC_TRY(run(c, a));
    return s.finish(counts);
}

// The refusals of the ldpc_ems_sim_* calls that need no device (check_ems keeps its own order).
static int check_ems_sim(const ldpc_nb_ctx *c, const ldpc_ems_cfg *cfg, const SimCall &q)
{
    RC_TRY(check_ems(c, cfg, q.batch));
    return check_sim_point(q, false);
}

// After the checks and enter(); `a` holds the outputs.
static int sim_run(ldpc_nb_ctx *c, const SimCall &q, ldpc::NbArgs &a)
{
    a.n0 = (float)fill_sim(a, *c, q).N0;   // decodeMinSum.cpp:146-147
    return run(c, a);
}

int ldpc_ems_sim_launch(ldpc_nb_ctx *c, double ebn0_db, double R, const ldpc_ems_cfg *cfg, uint64_t seed,
                        uint32_t stream_id, uint64_t first_cw, int batch, ldpc_frame_result *frames_dev)
{
    const SimCall q{ebn0_db, R, seed, stream_id, first_cw, batch};
    RC_TRY(check_ems_sim(c, cfg, q));
    RC_TRY(require_device(frames_dev, "frames_dev must be device memory"));
    RC_TRY(c->enter());
    ldpc::NbArgs a;
    fill_cfg(a, c, cfg, batch);
    a.frame_res = (int4 *)frames_dev;
    return sim_run(c, q, a);
}

int ldpc_ems_sim_trace(ldpc_nb_ctx *c, double ebn0_db, double R, const ldpc_ems_cfg *cfg, uint64_t seed,
                       uint32_t stream_id, uint64_t first_cw, int batch, float *y_out, uint8_t *d_out,
                       ldpc_frame_result *frames, ldpc_nb_counts *accum)
{
    const SimCall q{ebn0_db, R, seed, stream_id, first_cw, batch};
    RC_TRY(check_ems_sim(c, cfg, q));
    RC_TRY(c->enter());
    ldpc::NbArgs a;
    fill_cfg(a, c, cfg, batch);
    SyncCall s(*c);
    RC_TRY(s.out(y_out, c->y_stage, (size_t)batch * c->g->N * c->g->m * sizeof(float), a.y_out));
    RC_TRY(bind_decisions(s, c, a, d_out, frames));
    RC_TRY(s.snapshot());
    RC_TRY(sim_run(c, q, a));
    return s.finish(accum);
}

int ldpc_ems_sim_batch(ldpc_nb_ctx *c, double ebn0_db, double R, const ldpc_ems_cfg *cfg, uint64_t seed,
                       uint32_t stream_id, uint64_t first_cw, int batch, ldpc_frame_result *frames,
                       ldpc_nb_counts *accum)
{
    return ldpc_ems_sim_trace(c, ebn0_db, R, cfg, seed, stream_id, first_cw, batch, nullptr, nullptr, frames, accum);
}

int ldpc_nb_ctx_read_counts(ldpc_nb_ctx *c, ldpc_nb_counts *out, int reset)
{
    if (!c || !out) return set_err(LDPC_ERR_INVALID, "null argument");
    RC_TRY(c->enter());
    return c->read_counts(out, reset);
}

int ldpc_nb_ctx_last_kernel_ms(ldpc_nb_ctx *c, float *ms)
{
    return c ? c->last_kernel_ms(ms) : set_err(LDPC_ERR_INVALID, "null argument");
}

int ldpc_ems_kernel_info(ldpc_nb_ctx *c, char *name, int name_len, int *lds_bytes)
{
    if (!c) return set_err(LDPC_ERR_INVALID, "ctx is null");
    const ldpc::OptScope os(c->opts);
    return report_choice(ldpc::nb_choose(c->dg, c->g->maxdc), name, name_len, lds_bytes);
}

int ldpc_nb_ctx_set_option(ldpc_nb_ctx *c, int option, int value)
{
    return c ? c->set_option(option, value, true) : set_err(LDPC_ERR_INVALID, "ctx is null");
}

}  // extern "C"
