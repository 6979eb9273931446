// host_rt.h -- the host runtime under both C ABIs (api.cpp: binary codes; nb_api.cpp:
// GF(q)): error reporting, device buffers, blob uploads, CtxCore, the part of a context the two share (device, streams,
// launch events, options, counters), and the call skeleton of the decoder entry points
// (the checks every family makes, the simulated point, SyncCall, run_with_slots). Header
// only: both files include it.
#pragma once
#include "ldpc_hip.h"
#include "blob.h"
#include "check.h"
#include "kernels.h"
#include "options.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <initializer_list>
#include <string>

namespace ldpc {

// ldpc_last_error() of api.cpp.
int set_last_error(int code, const std::string &msg);

inline int set_err(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
inline int set_err(int code, const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return set_last_error(code, buf);
}

// In a function that returns an ABI status: a failed HIP call ends it with LDPC_ERR_DEVICE ...
#define HIP_TRY(expr)                                                                                 \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess) {                                                                       \
            (void)hipGetLastError();                                                                  \
            return ::ldpc::set_err(LDPC_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                   __FILE__, __LINE__);                                               \
        }                                                                                             \
    } while (0)
// ... and a failed step (its last error is set) with that step's status.
#define RC_TRY(expr)                        \
    do {                                    \
        if (const int rc_ = (expr)) return rc_; \
    } while (0)

#ifdef LDPC_CHECK
// checked builds: every launch is synchronised and its indices' record read (check.h)
#define LDPC_CHECK_AFTER_LAUNCH(stream)                                                                       \
    do {                                                                                                      \
        char m_[192];                                                                                         \
        const long n_ = ::ldpc::check_collect((stream), m_, sizeof m_);                                       \
        if (n_ < 0) return ::ldpc::set_err(LDPC_ERR_DEVICE, "check_collect: %s", hipGetErrorString((hipError_t)-n_)); \
        if (n_ > 0) return ::ldpc::set_err(LDPC_ERR_DEVICE, "%s; %ld violations", m_, n_);                    \
    } while (0)
#else
#define LDPC_CHECK_AFTER_LAUNCH(stream) ((void)0)
#endif

// A grow-only device allocation.
struct DevBuf {
    void *p = nullptr;
    size_t n = 0;
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= n) return hipSuccess;
        release();
        hipError_t e = hipMalloc(&p, bytes);
        if (e == hipSuccess) n = bytes;
        return e;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
};

inline bool is_device_ptr(const void *p)
{
    if (!p) return false;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged;
}

// The device copy of a blob: one allocation, one copy; sections are at buf.p + their offsets.
inline hipError_t upload(const Blob &b, DevBuf &buf)
{
    const hipError_t e = buf.ensure(b.size());
    return e != hipSuccess || !b.size() ? e : hipMemcpy(buf.p, b.data(), b.size(), hipMemcpyHostToDevice);
}

// The device counters of a context are 8 words: bit, frame, uncoded bit errors, frames,
// iterations, syndrome failures (the fields ldpc_counts and ldpc_nb_counts share, in
// order), symbol errors (GF(q) only) and the codeword ticket of the GDBF / EMS launches
// (which each launch clears itself). Counts are reported as differences of two reads.
constexpr int kCountWords = 8;
template <class Counts>
void add_shared_counts(Counts *acc, const unsigned long long *after, const unsigned long long *before)
{
    int64_t *const f[6] = {&acc->bit_err, &acc->frame_err, &acc->uncoded_bit_err,
                           &acc->frames,  &acc->iters,     &acc->syndrome_fail};
    for (int i = 0; i < 6; ++i) *f[i] += (int64_t)(after[i] - before[i]);
}
inline void add_counts(ldpc_counts *acc, const unsigned long long *after, const unsigned long long *before)
{
    add_shared_counts(acc, after, before);
}
inline void add_counts(ldpc_nb_counts *acc, const unsigned long long *after, const unsigned long long *before)
{
    add_shared_counts(acc, after, before);
    acc->symbol_err += (int64_t)(after[6] - before[6]);
}

// What ldpc_ctx and ldpc_nb_ctx share. Every ABI function that touches the device calls
// enter() first; a launch is bracketed by begin_launch() / end_launch().
struct CtxCore {
    int device = 0, max_batch = 0, num_cus = 0;
    hipStream_t own = nullptr, stream = nullptr;   // the context's own stream; the one launches go to
    hipEvent_t ev0 = nullptr, ev1 = nullptr;       // around the last launch (last_kernel_ms)
    hipEvent_t handoff = nullptr;                  // orders the launches of a context across set_stream
    bool timed = false;
    Options opts;                                  // kernel-selection options (set_option), tests and A/B only
    DevBuf counts;
    // the codeword ticket: the eighth counter word (above), of which a launch uses 32 bits
    unsigned *ticket() const { return reinterpret_cast<unsigned *>((unsigned long long *)counts.p + (kCountWords - 1)); }

    int init(int dev, int batch)
    {
        device = dev;
        max_batch = batch;
        RC_TRY(enter());
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, device));
        num_cus = prop.multiProcessorCount;
        HIP_TRY(hipStreamCreateWithFlags(&own, hipStreamNonBlocking));
        stream = own;
        HIP_TRY(hipEventCreate(&ev0));
        HIP_TRY(hipEventCreate(&ev1));
        HIP_TRY(counts.ensure(kCountWords * sizeof(unsigned long long)));
        HIP_TRY(hipMemset(counts.p, 0, counts.n));
        return LDPC_OK;
    }
    // Waits for the current stream, then frees `bufs` and everything init() made. Any
    // partly initialised context is fine: this is also the failure path of the *_create calls.
    void destroy(std::initializer_list<DevBuf *> bufs)
    {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        for (DevBuf *b : bufs) b->release();
        counts.release();
        for (hipEvent_t ev : {ev0, ev1, handoff})
            if (ev) (void)hipEventDestroy(ev);
        if (own) (void)hipStreamDestroy(own);
    }
    int enter()
    {
        HIP_TRY(hipSetDevice(device));
        return LDPC_OK;
    }
    int set_stream(void *s)
    {
        const hipStream_t ns = s ? (hipStream_t)s : own;
        if (ns != stream) {
            // The launches of one context share its counters (the GDBF / EMS codeword ticket
            // included), staging and re-decode buffers: the new stream starts after everything
            // already queued on the old one, so launches never overlap across a stream change.
            RC_TRY(enter());
            if (!handoff) HIP_TRY(hipEventCreateWithFlags(&handoff, hipEventDisableTiming));
            HIP_TRY(hipEventRecord(handoff, stream));
            HIP_TRY(hipStreamWaitEvent(ns, handoff, 0));
        }
        stream = ns;
        return LDPC_OK;
    }
    int begin_launch()
    {
        HIP_TRY(hipEventRecord(ev0, stream));
        return LDPC_OK;
    }
    int end_launch()
    {
        HIP_TRY(hipEventRecord(ev1, stream));
        timed = true;
        LDPC_CHECK_AFTER_LAUNCH(stream);
        return LDPC_OK;
    }
    int last_kernel_ms(float *ms)
    {
        if (!ms) return set_err(LDPC_ERR_INVALID, "null argument");
        if (!timed) return set_err(LDPC_ERR_INVALID, "no kernel launched yet");
        RC_TRY(enter());
        HIP_TRY(hipEventSynchronize(ev1));
        HIP_TRY(hipEventElapsedTime(ms, ev0, ev1));
        return LDPC_OK;
    }
    // The EMS options belong to the GF(q) context and only there (options.h).
    int set_option(int option, int value, bool ems)
    {
        const bool ok = option_value_ok(option, value);
        if (ems) {
            if (!option_is_ems(option)) return set_err(LDPC_ERR_INVALID, "option %d is not an EMS option", option);
            if (!ok) return set_err(LDPC_ERR_INVALID, "option %d: value %d out of range", option, value);
        } else {
            if (!ok) return set_err(LDPC_ERR_INVALID, "option %d: unknown, or value %d out of range", option, value);
            if (option_is_ems(option))
                return set_err(LDPC_ERR_INVALID, "option %d is an EMS option (ldpc_nb_ctx_set_option)", option);
        }
        opts.v[option] = value;
        return LDPC_OK;
    }
    // The counters once everything queued on the stream has run (waits for it).
    int read_counts_raw(unsigned long long v[kCountWords])
    {
        HIP_TRY(hipMemcpyAsync(v, counts.p, kCountWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return LDPC_OK;
    }
    template <class Counts> int read_counts(Counts *out, int reset)
    {
        unsigned long long v[kCountWords];
        const unsigned long long zero[kCountWords] = {};
        RC_TRY(read_counts_raw(v));
        if (out) {
            *out = Counts{};
            add_counts(out, v, zero);
        }
        if (reset) HIP_TRY(hipMemsetAsync(counts.p, 0, counts.n, stream));   // stream-ordered: no wait
        return LDPC_OK;
    }
    // acc += what the launches since the read `before` counted (acc may be null; waits for the stream).
    template <class Counts> int counts_since(const unsigned long long *before, Counts *acc)
    {
        unsigned long long after[kCountWords];
        RC_TRY(read_counts_raw(after));
        if (acc) add_counts(acc, after, before);
        return LDPC_OK;
    }
};

// ---- The call skeleton of the decoder entry points. Every family refuses in one order:
// null context or required pointer, cfg, batch, the simulated point (R, stream_id,
// first_cw), device-pointer requirements; then enter() and the first device call.
inline int check_batch(const CtxCore &c, int batch)
{
    if (batch <= 0 || batch > c.max_batch)
        return set_err(LDPC_ERR_INVALID, "batch %d outside 1..max_batch=%d", batch, c.max_batch);
    return LDPC_OK;
}
// The arguments every fused Monte-Carlo entry point takes: frames first_cw .. first_cw + batch - 1
// of the Philox stream (seed, stream_id) at Eb/N0 for rate R.
struct SimCall {
    double ebn0_db, R;
    uint64_t seed;
    uint32_t stream_id;
    uint64_t first_cw;
    int batch;
};
// stream20: the GDBF families keep 20 bits of stream_id beside the iteration in a Philox word.
inline int check_sim_point(const SimCall &q, bool stream20)
{
    if (!(q.R > 0)) return set_err(LDPC_ERR_INVALID, "rate must be > 0");
    if (stream20 && q.stream_id >= (1u << 20)) return set_err(LDPC_ERR_INVALID, "stream_id must be < 2^20");
    return LDPC_OK;
}
// The refusals of a *_sim_* call that need no device, in order; check_cfg() is the family's own.
template <class Ctx, class CheckCfg> int check_sim(const Ctx *c, CheckCfg check_cfg, const SimCall &q, bool stream20)
{
    if (!c) return set_err(LDPC_ERR_INVALID, "ctx is null");
    RC_TRY(check_cfg());
    RC_TRY(check_batch(*c, q.batch));
    return check_sim_point(q, stream20);
}
// What an asynchronous launch writes must be device memory (null: not wanted).
inline int require_device(const void *p, const char *refusal)
{
    return p && !is_device_ptr(p) ? set_err(LDPC_ERR_INVALID, "%s", refusal) : LDPC_OK;
}

// N0 and sigma of Eb/N0 at rate R, in double as every reference program has them
// (decodeMinSum.cpp:146-147, decodeGDBF.cpp:175-176, RNGDBF.cpp:167-168, newstat.cpp:192-193,
// NGDBFhw.cpp:127-129).
struct SimPoint {
    double N0, sigma;
};
inline SimPoint sim_point(double ebn0_db, double R)
{
    const double N0 = std::pow(10.0, -ebn0_db / 10.0) / R;
    return {N0, std::sqrt(N0 / 2.0)};
}

// The *Args of the kernel families spell their common fields alike. The accounting of the
// binary GDBF families: counters, error-weight histogram, codeword ticket.
template <class Args, class Ctx> void fill_accounting(Args &a, Ctx &c)
{
    a.counts = (unsigned long long *)c.counts.p;
    a.hist = (unsigned long long *)c.hist.p;
    a.ticket = c.ticket();
}
// The fused Monte-Carlo source of a launch; returns the point for the family's own noise terms.
template <class Args, class Ctx> SimPoint fill_sim(Args &a, Ctx &c, const SimCall &q)
{
    const SimPoint pt = sim_point(q.ebn0_db, q.R);
    a.src = SRC_PHILOX;
    a.sigma = (decltype(a.sigma))pt.sigma;
    a.seed = q.seed;
    a.stream_id = q.stream_id;
    a.first_cw = q.first_cw;
    return pt;
}
// ... and the codeword table it sends (the binary contexts; null: the all-zero codeword).
template <class Args, class Ctx> void fill_cw_table(Args &a, Ctx &c)
{
    a.cw_table = c.cw_rows ? (const int8_t *)c.cw_table.p : nullptr;
    a.cw_rows = c.cw_rows;
}

// A synchronous entry point: snapshot() reads the counters before the launch; out() gives
// the device address of an output the caller holds on the host or on the device (its own
// pointer, or the staging buffer when that is host memory; null: not wanted) and in() that
// of a given-sample input; finish() copies the staged outputs back in the order they were
// bound and adds what the launch counted to acc (null: not wanted; waits for the stream).
struct SyncCall {
    CtxCore &c;
    unsigned long long before[kCountWords];
    struct {
        void *user, *dev;
        size_t bytes;
    } staged[12];
    int n = 0;
    explicit SyncCall(CtxCore &ctx) : c(ctx) {}
    int snapshot() { return c.read_counts_raw(before); }
    // forced: the kernel needs the buffer although the caller does not want it
    template <class D> int out(void *user, DevBuf &stage, size_t bytes, D *&dev, bool forced = false)
    {
        dev = (D *)user;
        if (user ? is_device_ptr(user) : !forced) return LDPC_OK;
        HIP_TRY(stage.ensure(bytes));
        dev = (D *)stage.p;
        if (user) staged[n++] = {user, stage.p, bytes};
        return LDPC_OK;
    }
    template <class T> int in(const T *user, size_t bytes, DevBuf &stage, const T *&dev)
    {
        dev = user;
        if (!user || is_device_ptr(user)) return LDPC_OK;
        HIP_TRY(stage.ensure(bytes));
        dev = (const T *)stage.p;
        HIP_TRY(hipMemcpyAsync(stage.p, user, bytes, hipMemcpyHostToDevice, c.stream));
        return LDPC_OK;
    }
    template <class Counts> int finish(Counts *acc)
    {
        for (int i = 0; i < n; ++i)
            HIP_TRY(hipMemcpyAsync(staged[i].user, staged[i].dev, staged[i].bytes, hipMemcpyDeviceToHost, c.stream));
        return c.counts_since(before, acc);
    }
};

// A launch between the context's launch events, with the scratch of a kernel that keeps
// its state in global memory: choice.slot_bytes for each of min(items, max_slots) resident
// items (no bytes: no slots). launch(scratch, slots) queues the family's kernels.
template <class Choice, class Launch>
int run_with_slots(CtxCore &c, DevBuf &scratch, const Choice &ch, int64_t items, int max_slots, Launch launch)
{
    int slots = 0;
    if (ch.slot_bytes) {
        slots = (int)std::min<int64_t>(items, max_slots);
        HIP_TRY(scratch.ensure(ch.slot_bytes * (size_t)slots));
    }
    RC_TRY(c.begin_launch());
    HIP_TRY(launch(scratch.p, slots));
    return c.end_launch();
}

// The tail of the *_kernel_info calls.
template <class Choice> int report_choice(const Choice &ch, char *name, int name_len, int *lds_bytes)
{
    if (name && name_len > 0) std::snprintf(name, (size_t)name_len, "%s", ch.name);
    if (lds_bytes) *lds_bytes = ch.lds_bytes;
    return LDPC_OK;
}

}  // namespace ldpc
