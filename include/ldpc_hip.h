/*
 * ldpc_hip.h -- C ABI of the MI355X-native LDPC min-sum decoder
 * (libldpc_hip.so, built from ldpcsimulation_amd/csrc/).
 *
 * Drop-in boundary for the hot path of ereiss123/LDPCsimulation
 * (paths relative to C_implementations/):
 *   - ldpc_graph_create / ldpc_graph_load_alist replace the H-matrix loader
 *     loadFile() (src/alist.cpp:22-95, inc/alist.h:21-41) and the message
 *     memory setup setupSymMessages/setupCheckMessages (src/decodeMinSum.cpp
 *     :345-361). ldpc_graph_create takes exactly the arrays of an
 *     alist_struct (N, M, num_nlist, nlist, num_mlist, mlist; 1-based,
 *     zero padded), so an existing loadFile() result passes straight through.
 *   - ldpc_decode_batch replaces the per-frame decode loop
 *     initializeSymMessages + T x {checkNodeUpdates, applyNormalization |
 *     applyOffset, symNodeUpdates} + countDecisionErrors
 *     (src/decodeMinSum.cpp:240-270, functions at :364-370, :410-515,
 *     :382-393) for a batch of frames whose channel samples y are given
 *     (the reference's `y`/`yq` vectors, :214-238).
 *   - ldpc_sim_launch / ldpc_sim_batch replace the body of the Monte-Carlo
 *     frame loop (src/decodeMinSum.cpp:189-289: AWGN, quantise/saturate,
 *     decode, error accounting) with one fused device pass per batch; the
 *     stop rule (:189) stays with the caller, which reads ldpc_counts.
 *   The compile-time variants of the reference (-D normalizedMS, offsetMS,
 *   quantizeSamples, saturateSamples; src/decodeMinSum.cpp:26-32,
 *   Makefile:58-65) are runtime fields of ldpc_decoder_cfg.
 *   The belief-propagation decoder (src/decodeBP.cpp) is variant LDPC_BP.
 *   - ldpc_gdbf_decode_batch / ldpc_gdbf_sim_* replace the frame body of the
 *     GDBF / NGDBF bit-flipping decoders (src/decodeGDBF.cpp:250-399,
 *     checkNodeUpdates :517-534, symNodeUpdates :536-621), whose -D switches
 *     (Makefile:33-53) are the flags of ldpc_gdbf_cfg.
 *   - ldpc_fxms_decode_batch / ldpc_fxms_sim_* stand where ldpc_decode_batch /
 *     ldpc_sim_* do, for min-sum with integer messages of a chosen width (no
 *     reference program has them: its -D quantizeSamples quantises the samples
 *     only, src/decodeMinSum.cpp:480-489). ldpc_fxlms_* are their row-layered
 *     counterparts (a saturating posterior per bit, a message per edge).
 *   - ldpc_nb_* / ldpc_ems_* (ABI 5): non-binary GF(16) codes (BASELINE
 *     config 5). ldpc_nb_graph_create / _load_alist replace the NB-LDPC
 *     model's loadFile() (SystemC/NB-LDPC/src/alist.cpp:23-56,
 *     inc/alist.h:25-43: (index, GF value) pairs); the decode replaces its
 *     symbol/check node iteration (inc/nodes.h:82-166, :240-293; a q^dc-LUT
 *     BP there, which does not compile) with the Extended Min-Sum.
 *
 * Conventions: every function returns LDPC_OK (0) or a negative
 * ldpc_status; ldpc_last_error() gives a thread-local message. No C++
 * exception crosses the ABI. Buffers may be host or device pointers (the
 * library checks with hipPointerGetAttributes); the caller owns them and the
 * library never frees caller memory. A context is not thread-safe: one host
 * thread (or process) per GPU. Graphs are immutable after creation and may
 * be shared read-only between contexts.
 */
#ifndef LDPC_HIP_H
#define LDPC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LDPC_ABI_VERSION 11

typedef enum {
    LDPC_OK = 0,
    LDPC_ERR_INVALID = -1,     /* bad argument                         */
    LDPC_ERR_NOMEM = -2,       /* host or device allocation failed     */
    LDPC_ERR_DEVICE = -3,      /* HIP runtime / kernel error           */
    LDPC_ERR_UNSUPPORTED = -4, /* shape or option not supported        */
    LDPC_ERR_IO = -5,          /* file could not be read               */
    LDPC_ERR_GRAPH = -6        /* inconsistent / malformed H matrix    */
} ldpc_status;

/* Check-node rule: MS = decodeMinSum, NMS = -D normalizedMS (c2v /= alpha,
 * src/decodeMinSum.cpp:494-499), OMS = -D offsetMS (:503-515), BP = the
 * tanh rule of src/decodeBP.cpp (:353-409) with its LLR front-end
 * yq = 4*y/n0 clipped to +-max_llr (:184-197; quantize/saturate ignored,
 * flooding only). DDBMP = differential decoding with binary message passing
 * (src/decodeDDBMP.cpp: one-bit messages, one memory per edge, :350-423) with
 * the min-sum front-end (quantize / saturate / ymax / qbits; its CLI sets
 * quantize); alpha, delta, n0 and max_llr are ignored; flooding only; T is a
 * maximum, the decoder stops when H*d = 0 (:203-204). */
typedef enum { LDPC_MS = 0, LDPC_NMS = 1, LDPC_OMS = 2, LDPC_BP = 3, LDPC_DDBMP = 4 } ldpc_variant;

/* Message arithmetic. F64 is the reference's own precision and reproduces
 * its decisions bit-for-bit for identical y; F32 is the throughput path. */
typedef enum { LDPC_F32 = 0, LDPC_F64 = 1 } ldpc_precision;

/* Message-passing schedule. FLOODING is the reference's (all check nodes,
 * then all bit nodes: src/decodeMinSum.cpp:247-263). LAYERED is the
 * row-serial schedule of SURVEY §8(f) row 2 (BASELINE config 3; no
 * reference counterpart): rows in the order ldpc_graph_layers() returns,
 * each row updating the posteriors of its bits in place, bit-disjoint rows
 * of a layer in parallel. */
typedef enum { LDPC_FLOODING = 0, LDPC_LAYERED = 1 } ldpc_schedule;

typedef struct ldpc_graph ldpc_graph;
typedef struct ldpc_ctx ldpc_ctx;

/* Error accounting of src/decodeMinSum.cpp:167-172,270-288, int64 as the
 * reference's `long` counters, plus a syndrome check (H*d != 0). */
typedef struct {
    int64_t bit_err;         /* errors          */
    int64_t frame_err;       /* wordErrors      */
    int64_t uncoded_bit_err; /* uncodedErrors   */
    int64_t frames;          /* totalWords      */
    int64_t iters;           /* totalIterations */
    int64_t syndrome_fail;   /* frames whose hard decision is not a codeword */
} ldpc_counts;

/* Per-frame outcome (optional output), in frame order. */
typedef struct {
    int32_t bit_err;          /* newErrors of :270 (0 = frame decoded)  */
    int32_t uncoded_bit_err;  /* hard-decision errors before decoding    */
    int32_t syndrome_fail;    /* 1 if H*d != 0                          */
    int32_t iters;            /* GDBF: iterations run (`it`, decodeGDBF.cpp:399); DD-BMP:
                               * `it` of decodeDDBMP.cpp:230 (a frame that stops inside
                               * iteration index it counts it, one that never stops T);
                               * min-sum, BP: 0, or with cfg.early_stop the s of the
                               * returned D(s) (see ldpc_decoder_cfg.early_stop) */
} ldpc_frame_result;

typedef struct {
    int32_t variant;    /* ldpc_variant                                     */
    int32_t precision;  /* ldpc_precision                                   */
    int32_t T;          /* iterations (num_iterations): fixed, no early stop
                         * (early_stop = 1: the maximum); DD-BMP: the maximum
                         * (it always stops early)                            */
    int32_t quantize;   /* -D quantizeSamples: quantize(y, ymax, 2^qbits)   */
    int32_t saturate;   /* -D saturateSamples: clip at +-ymax               */
    int32_t qbits;      /* Q                                                */
    double  ymax;       /* Ymax                                             */
    double  alpha;      /* NMS divisor                                      */
    double  delta;      /* OMS offset                                       */
    int32_t schedule;   /* ldpc_schedule (ABI 2)                            */
    int32_t early_stop; /* MS / NMS / OMS / BP, flooding: 0 = T iterations, as the
                         * reference (decodeMinSum / decodeBP have no early stop);
                         * 1 = with D(t) what the decoder returns for the frame at
                         * T = t (decisions, bit_err, uncoded_bit_err, syndrome_fail),
                         * the frame's result is D(s) for the smallest s in 0..T with
                         * syndrome_fail == 0 (s = T when there is none): the syndrome
                         * is checked before every iteration and after the last.
                         * frames[].iters = s and counts->iters += s. A frame's result
                         * does not depend on the other frames, the batch size or the
                         * kernel. LDPC_ERR_UNSUPPORTED with LDPC_LAYERED and with
                         * LDPC_OPT_KERNEL = 2 (flood); ignored by DD-BMP. The field
                         * was `reserved` (0) before: same offset, ABI unchanged. */
    double  n0;         /* BP: noise density N0 of the LLR front-end 4*y/N0 (ABI 4);
                         * ldpc_decode_batch needs it > 0, the sim entry points
                         * compute it from Eb/N0 and R (:104)               */
    double  max_llr;    /* BP: MAXLLR message clip, 0 = the reference's 20 (:58) */
} ldpc_decoder_cfg;

int         ldpc_abi_version(void);
const char *ldpc_last_error(void);
/* (ABI 9) 1 when the fp64 NMS division m / alpha (applyNormalization,
 * decodeMinSum.cpp:494-499) runs as Markstein's q = m*r, q += fma(-q, alpha, m)*r
 * with r = RN(1/alpha) -- exact for alpha = P * 2^E, odd P < 2^20, 2^-900 < alpha
 * <= 2^60 -- else 0 (IEEE division). No device call. */
int         ldpc_f64_nms_fast_division(double alpha);
/* (ABI 11) The fp64 BP check node's transcendentals as the device computes
 * them (bp_math.h: tanh for th_k = tanh(v2c/2) and log for c2v = log((1+p)/(1-p)),
 * decodeBP.cpp:353-377), evaluated on device `device` for n host values x:
 * tanh_out[i] = tanh(x[i]), log_out[i] = log(x[i]) (either output may be NULL).
 * Verification only (tests/test_bp.py measures their ulp distance to glibc). */
int         ldpc_bp_math_probe(int device, const double *x, int n, double *tanh_out, double *log_out);
/* (ABI 11) The device bounds checks of the checked build (`make checked`,
 * ldpcsimulation_amd/lib/checked/libldpc_hip_checked.so; check.h): launches one
 * kernel that indexes past a bound on purpose and returns what every launch of
 * that build returns on a violation -- LDPC_ERR_DEVICE, ldpc_last_error() naming
 * the site, index and bound. The product library compiles no checks and returns
 * LDPC_ERR_UNSUPPORTED. */
int         ldpc_check_selftest(int device);

/* ---- graph (H matrix) ------------------------------------------------ */
/* Arrays exactly as alist_struct (inc/alist.h:21-36): nlist[i] has
 * num_nlist[i] 1-based check indices of bit i, mlist[j] has num_mlist[j]
 * 1-based bit indices of check j (entries beyond the weight are ignored).
 * Validates that both views describe the same edge set. */
int  ldpc_graph_create(int N, int M, const int *num_nlist, const int *const *nlist,
                       const int *num_mlist, const int *const *mlist, ldpc_graph **out);
/* MacKay alist file with the reference loader's fixed-width semantics
 * (src/alist.cpp:70-93). */
int  ldpc_graph_load_alist(const char *path, ldpc_graph **out);
int  ldpc_graph_info(const ldpc_graph *g, int *N, int *M, int *E, int *maxdv, int *maxdc);
void ldpc_graph_destroy(ldpc_graph *g);
/* Row order and layer partition of the LAYERED schedule: row_order[M] lists
 * the rows in serial order, layer_ptr[nlayers+1] delimits the layers (runs
 * of rows that share no bit). Either array may be NULL (query nlayers
 * first). Every graph has one (row degree up to 58; the floating-point LAYERED
 * kernels take row degree up to 26). No reference counterpart. */
int  ldpc_graph_layers(const ldpc_graph *g, int32_t *row_order, int32_t *layer_ptr, int *nlayers);

/* ---- device context --------------------------------------------------- */
int  ldpc_device_count(int *n);
/* One per device: uploads the graph, owns a HIP stream, counters, scratch.
 * max_batch bounds the frames of one decode/sim call. */
int  ldpc_ctx_create(int device, const ldpc_graph *g, int max_batch, ldpc_ctx **out);
/* Launch on an external hipStream_t (e.g. torch.cuda.current_stream()); NULL
 * restores the context's own stream. A context's launches share its counters and
 * buffers, so a stream change is ordered after the work already queued on the
 * previous stream (an event): one context's launches never overlap. Use one
 * context per stream for concurrent launches. */
int  ldpc_ctx_set_stream(ldpc_ctx *ctx, void *hip_stream);
int  ldpc_ctx_synchronize(ldpc_ctx *ctx);
void ldpc_ctx_destroy(ldpc_ctx *ctx);

/* Decode `batch` frames of given channel samples y[batch][N] (float for
 * LDPC_F32, double for LDPC_F64; host or device). The cfg front-end
 * (quantize / saturate) is applied to y first, as :218-229 does.
 * c: transmitted bipolar codewords [batch][N] (+1/-1, int8) or NULL for the
 *    all-zero codeword (c = +1, :159).
 * d_out [batch][N] int8 +1/-1 decisions and frames [batch] per-frame
 * results: optional (NULL). counts: optional, ACCUMULATED (+=). Synchronous. */
int  ldpc_decode_batch(ldpc_ctx *ctx, const void *y, int batch, const ldpc_decoder_cfg *cfg,
                       const int8_t *c, int8_t *d_out, ldpc_frame_result *frames,
                       ldpc_counts *counts);

/* Codeword-file mode (:136-143, :193-212): rows of 0/1 bits [rows][N];
 * frame with global index f transmits row f % rows. rows = 0 restores the
 * all-zero codeword. */
int  ldpc_sim_set_codewords(ldpc_ctx *ctx, const uint8_t *bits, int rows);

/* Fused on-device Monte-Carlo of one SNR point: BPSK, AWGN with
 * sigma = sqrt(10^(-ebn0/10)/R/2) (:146-147) from counter-based
 * Philox4x32-10 keyed by (seed, stream_id, global frame index, bit index)
 * and a Box-Muller transform in fp32 on the SIMD's transcendental instructions
 * (v_log/v_sqrt/v_sin/v_cos_f32; the normals widened to double for the fp64
 * decoders), front-end, T iterations, error accounting into the context's device
 * counters. Frames first_cw .. first_cw+batch-1; the result does not depend
 * on how frames are split across calls or devices. Asynchronous.
 * frames_dev: optional DEVICE pointer [batch] of per-frame results. */
int  ldpc_sim_launch(ldpc_ctx *ctx, double ebn0_db, double R, const ldpc_decoder_cfg *cfg,
                     uint64_t seed, uint32_t stream_id, uint64_t first_cw, int batch,
                     ldpc_frame_result *frames_dev);
/* Synchronising read of the accumulated device counters (reset != 0 zeroes them). */
int  ldpc_ctx_read_counts(ldpc_ctx *ctx, ldpc_counts *out, int reset);
/* Error-weight histogram (error_weight_hist, :173,:280): out[w-1] = frames
 * with w bit errors, N entries. */
int  ldpc_ctx_read_histogram(ldpc_ctx *ctx, int64_t *out, int reset);
/* ldpc_sim_launch + the batch's counts accumulated into *accum; frames
 * (optional) may be host or device. Synchronous. */
int  ldpc_sim_batch(ldpc_ctx *ctx, double ebn0_db, double R, const ldpc_decoder_cfg *cfg,
                    uint64_t seed, uint32_t stream_id, uint64_t first_cw, int batch,
                    ldpc_frame_result *frames, ldpc_counts *accum);

/* ldpc_sim_batch that also returns what the fused kernel generated: the
 * channel samples y_out [batch][N] (float for F32, double for F64, before
 * the front-end) and the decisions d_out [batch][N] (+1/-1). Either may be
 * NULL; host or device. For verification of the on-device channel. */
int  ldpc_sim_trace(ldpc_ctx *ctx, double ebn0_db, double R, const ldpc_decoder_cfg *cfg,
                    uint64_t seed, uint32_t stream_id, uint64_t first_cw, int batch,
                    void *y_out, int8_t *d_out, ldpc_frame_result *frames, ldpc_counts *accum);

/* Device time (ms) of the last decode kernel, from HIP events recorded on
 * the launch stream around it. Synchronises that stream. */
int  ldpc_ctx_last_kernel_ms(ldpc_ctx *ctx, float *ms);
/* Kernel chosen for a cfg ("rows_pp", "rows_fast", "rows", "rows_es", "lds", "flood",
 * "global", "layered_*", "bp_*", "ddbmp_rows" / "ddbmp_lds" / "ddbmp_global")
 * and its per-codeword LDS bytes. */
int  ldpc_ctx_kernel_info(ldpc_ctx *ctx, const ldpc_decoder_cfg *cfg, char *name, int name_len,
                          int *lds_bytes, int *blocks_per_cu);
/* Codewords of the last min-sum launch that the fast row kernel (fp64,
 * "rows_fast") handed to the exact path because its premise failed (huge or
 * non-finite values, minima below 2^-960; 0 for any launch that did not use
 * the fast kernel). Diagnostic of the fast/exact split; synchronises the
 * stream. No reference counterpart (the reference has one exact path). */
int  ldpc_ctx_redo_count(ldpc_ctx *ctx, int64_t *n);
/* The batch indices of those codewords, in the order the kernel listed them (any order):
 * *n = their number, the first min(*n, cap) of them to list[]. Synchronises the stream. */
int  ldpc_ctx_redo_list(ldpc_ctx *ctx, uint32_t *list, int64_t cap, int64_t *n);
/* Shape of the row kernel ("rows"/"rows_fast"/"rows_pp"/"rows_es") that decodes cfg, for the
 * on-chip (LDS) roofline model of bench.py: info[10] = {threads per block,
 * rows per thread, bit slots per thread, padded row degree, padded edge slots
 * e_pad, codewords per block, LDS bytes per block, blocks per CU, the low row
 * degree of rows_pp's degree-aware slots (0: every slot runs the padded degree),
 * check-node edge slots issued per codeword-iteration} (ABI 10: 10 entries).
 * LDPC_ERR_UNSUPPORTED when another kernel decodes cfg (always for BP and DD-BMP). Host-only, no device
 * call. No reference counterpart (diagnostic of decodeMinSum.cpp:247-263's
 * replacement). */
int  ldpc_ctx_row_sched_info(ldpc_ctx *ctx, const ldpc_decoder_cfg *cfg, int32_t *info);
/* The in-register bits of the ping-pong kernel for cfg: degree-2 bits whose two check rows
 * are held by one check thread never pass through LDS. info[4] = {in-register bits,
 * check-node edge slots that pass through LDS per codeword-iteration, padded bit-slot edges
 * the bit role walks, bit slots per thread}. Without such bits (a code with no pair,
 * fp32 pairs, LDPC_OPT_PP_SLOTS 1 or 2) info[0] is 0 and the rest describes ldpc_ctx_row_sched_info's
 * schedule. LDPC_ERR_UNSUPPORTED when the kernel that decodes cfg is not "rows_pp". Host-only.
 * No reference counterpart. */
int  ldpc_ctx_pp_inreg_info(ldpc_ctx *ctx, const ldpc_decoder_cfg *cfg, int32_t *info);
/* The check-row slots of the schedule the "rows_pp" kernel runs cfg on, read back from the
 * device (the in-register schedule where ldpc_ctx_pp_inreg_info reports bits, else
 * ldpc_ctx_row_sched_info's): slot j belongs to check thread j % threads as its row
 * j / threads; cols[8 * j + k] is the bit of its edge k (an entry >= N is a padding edge),
 * deg[j] its degree (0: an empty slot). *nslots = threads * rows per thread; cap is the room
 * of cols / 8 and deg. Diagnostic, for tests that aim at one row of a thread; synchronises
 * the stream. LDPC_ERR_UNSUPPORTED as above. No reference counterpart. */
int  ldpc_ctx_pp_row_slots(ldpc_ctx *ctx, const ldpc_decoder_cfg *cfg, uint16_t *cols, uint8_t *deg, int cap,
                           int *nslots);
/* The workgroup the "rows_pp" kernel launches for cfg: info[2] = {threads per block (1024: 8
 * check and 8 bit waves; 768: 8 check and 4 bit waves, the in-register schedule with 3 bit slots
 * per thread on codes that fit the fixed-stride LDS layout), dynamic LDS bytes of the launch (ldpc_ctx_kernel_info's
 * decoder state plus that layout's gaps)}. LDPC_ERR_UNSUPPORTED as above. Host-only. No
 * reference counterpart. */
int  ldpc_ctx_pp_block_info(ldpc_ctx *ctx, const ldpc_decoder_cfg *cfg, int32_t *info);
/* The rule behind the 768-thread block: info[2] = {1 when the fixed-stride LDS layout holds a
 * code of n_bits bits whose row schedule has e_pad padded edge slots (ldpc_ctx_row_sched_info's
 * e_pad) -- (n_bits + 3) * 8 <= 16384, (e_pad + 64) * 8 <= 65520 and the whole layout within
 * 160 KB -- else 0, the dynamic LDS bytes of that layout}. No context, no device call. No
 * reference counterpart. */
int  ldpc_pp_block_layout(int n_bits, int e_pad, int32_t *info);

/* ---- kernel-selection options (ABI 10) ------------------------------- */
/* The library picks the kernel for a cfg by itself (the reference fixes its
 * algorithm per binary at build time, C_implementations/Makefile:58-65). These
 * per-context options override that choice for tests and A/B measurements;
 * every alternative decodes bit-identically to the default (the GPU tests pin
 * that). 0 is the library's own choice for every option; the library never
 * reads them from the environment. Options take effect at the next launch. */
typedef enum {
    LDPC_OPT_ROWS64 = 1,           /* fp64 row graphs: 0 ping-pong (rows_pp), 1 rows_fast, 2 the row kernel   */
    LDPC_OPT_ROWS32 = 2,           /* fp32 MS / NMS row graphs: 0 rows_pp pairs, 1 rows_fast pairs, 2 the row kernel */
    LDPC_OPT_PP_SLOTS = 3,         /* rows_pp row slots: 0 degree-aware (when the code admits them) with the   */
                                   /* paired rows' degree-2 bits in registers (when it has pairs), 1 plain,   */
                                   /* 2 degree-aware with every bit in LDS, 3 as 0 but always on the 16-wave  */
                                   /* block (0 takes the 12-wave block where the code fits its LDS layout)    */
    LDPC_OPT_KERNEL = 4,           /* generic kernel: 0 auto, 1 lds, 2 flood (persistent), 3 global; 3 also   */
                                   /* makes ldpc_fxlms_* take the workgroup-per-codeword kernel (fxlms_wg_*)  */
    LDPC_OPT_FLOOD_MODE = 5,       /* codes beyond LDS: 0 one launch per phase, 1 the persistent kernel       */
    LDPC_OPT_FLOOD_MSG = 6,        /* phase flooding messages: 0 packed row state, 1 the c2v array            */
    LDPC_OPT_FLOOD_SPS_CHECK = 7,  /* phase flooding: resident slots per check-kernel step (0 = default)      */
    LDPC_OPT_FLOOD_SPS_BIT = 8,    /* phase flooding: resident slots per bit-kernel step (0 = default)        */
    LDPC_OPT_FLOOD_RESIDENT = 9,   /* phase flooding: resident codewords (0 = sized to the Infinity Cache)    */
    LDPC_OPT_FLOOD_STREAMS = 10,   /* phase flooding: 2 = the resident set in two halves on two streams       */
    LDPC_OPT_FLOOD_BPC = 11,       /* persistent flooding kernel: blocks per CU cap (0 = occupancy)           */
    LDPC_OPT_LAYERED_BPC = 12,     /* global layered kernel: blocks per CU (0 = 1, capped by the 208 MiB      */
                                   /* resident-state budget; set: that many per CU, no cap)                  */
    LDPC_OPT_LAYERED_LDS_POS = 13, /* global layered kernel: positions kept in LDS + 1 (0 = as many as fit)   */
    LDPC_OPT_LAYERED_ROWS64 = 14,  /* 512-thread global layered kernel, fp64 rows per pass: 1 or 2 (0 = 2)    */
    LDPC_OPT_LAYERED_THREADS = 15, /* global layered kernel threads: 512 or 1024 (0 = 1024)                   */
    LDPC_OPT_ROWS_BPC = 16,        /* row kernel (k_decode_rows, k_rows_es): blocks per CU cap (0 = occupancy) */
    LDPC_OPT_FAST_BPC = 17,        /* rows_fast: blocks per CU cap (0 = occupancy)                            */
    LDPC_OPT_BP_KERNEL = 18,       /* belief propagation: 0 bp_rows when the code fits, 1 the generic kernel  */
    LDPC_OPT_GDBF_KERNEL = 19,     /* GDBF: 0 gdbf_rows when the code and flags fit, 1 the generic kernel     */
    LDPC_OPT_EMS_THREADS = 20,     /* EMS (nb context), row degree 4 (q < 16: any): 0 = 1024 threads, 512     */
    LDPC_OPT_EMS_SWIZZLE = 21,     /* EMS (nb context): 0 swizzled message slots, 1 the plain layout          */
    LDPC_OPT_DDBMP_KERNEL = 22     /* DD-BMP: 0 ddbmp_rows when the code fits, 1 the generic kernel           */
} ldpc_option;
#define LDPC_OPT_COUNT 23
/* LDPC_ERR_INVALID for an unknown option, a value outside its range, or an
 * EMS option (LDPC_OPT_EMS_*: the nb context's, ldpc_nb_ctx_set_option). */
int  ldpc_ctx_set_option(ldpc_ctx *ctx, int option, int value);
int  ldpc_ctx_get_option(const ldpc_ctx *ctx, int option, int *value);

/* ---- GDBF / NGDBF bit flipping (BASELINE config 4) --------------------- */
/* src/decodeGDBF.cpp in its parallel-flip mode (mu = 1): syndrome check
 * nodes with early stop (:298-306, :517-534), energy E = d*yq + w*sum(s)
 * [+ perturbation] and flip when E < theta (:536-621). The compile-time
 * switches of C_implementations/Makefile:33-53 are runtime flags:
 * decodeMNGDBF = NOISE|ADAPT|WEIGHT|SATURATE, decodeSMNGDBF = the same|SMOOTH,
 * decodeATGDBF = ADAPT, decodeSATGDBF = ADAPT|SMOOTH, decodeSMGDBF = SMOOTH,
 * and (ABI 8, Makefile:24-31) decodeSGDBF = SEQUENTIAL, decodeMGDBF =
 * MODESWITCH, decodeStochasticNGDBF = QUANTIZE|QPROB|WEIGHT|SATURATE.
 * ADAPT with SEQUENTIAL/MODESWITCH and NOISE with QPROB are not supported
 * (no reference target combines them). */
typedef enum {
    LDPC_GDBF_NOISE = 1,      /* -D addNoise: E += noiseScale*sigma*n per bit and iteration */
    LDPC_GDBF_ADAPT = 2,      /* -D thresholdAdaptation: theta *= lambda when not flipped   */
    LDPC_GDBF_WEIGHT = 4,     /* -D weightSyndromes: syndrome weight alpha (else 1)         */
    LDPC_GDBF_SMOOTH = 8,     /* -D outputSmoothing: majority of the last windowsize d's    */
    LDPC_GDBF_SATURATE = 16,  /* -D saturateSamples: |yq| <= Ymax                           */
    LDPC_GDBF_QUANTIZE = 32,  /* -D quantizeSamples: quantize(yq) with NQ levels            */
    LDPC_GDBF_SEQUENTIAL = 64,   /* -D sequentialmode: flip only the first bit of least energy
                                    per iteration (mu = 0, :573-580, :619-620)              */
    LDPC_GDBF_MODESWITCH = 128,  /* -D modeswitching: parallel flips until, after Tswitch,
                                    the objective sum(d*yq)+sum(s) does not grow (:309-345);
                                    then sequential                                         */
    LDPC_GDBF_QPROB = 256        /* -D quantizeProbabilities: flip with probability
                                    normalCDF((theta-E)/qsigma) rounded to 8 levels (:562-597) */
} ldpc_gdbf_flag;

typedef struct {
    int32_t flags;        /* OR of ldpc_gdbf_flag                         */
    int32_t precision;    /* ldpc_precision                               */
    int32_t T;            /* num_iterations (maximum; early stop)         */
    int32_t windowsize;   /* outputSmoothing window                       */
    int32_t nq;           /* quantizeSamples NQ                           */
    int32_t tswitch;      /* MODESWITCH: Tswitch (0 in the reference, :51) */
    double  theta;        /* initial flip threshold                       */
    double  lambda;       /* threshold adaptation factor                  */
    double  alpha;        /* syndrome weight (weightSyndromes)            */
    double  noise_scale;  /* perturbation sigma = noise_scale * channel sigma */
    double  ymax;         /* saturation / quantizer range                 */
    double  qsigma;       /* QPROB, ldpc_gdbf_decode_batch only: the normalCDF sigma
                           * (noiseSigma = noise_scale * channel sigma, :296); the sim
                           * entry points compute it from Eb/N0 and R (ABI 8) */
} ldpc_gdbf_cfg;

/* Decode `batch` frames of given RAW channel samples y[batch][N] (float for
 * F32, double for F64; host or device): front-end (:254-267), then the
 * iterations with the caller's perturbations pert[batch][T][N] (iteration it
 * of frame b adds pert[b][it][i] to E_i; required with LDPC_GDBF_NOISE; with
 * LDPC_GDBF_QPROB pert[b][it][i] is instead the uniform draw ranu() of bit i
 * in iteration it (:588); else ignored). c, d_out, frames, counts as ldpc_decode_batch; frames[].iters and
 * counts->iters report the iterations run. Synchronous. Replaces the frame
 * body of decodeGDBF.cpp main() (:250-399). */
int  ldpc_gdbf_decode_batch(ldpc_ctx *ctx, const void *y, const void *pert, int batch, const ldpc_gdbf_cfg *cfg,
                            const int8_t *c, int8_t *d_out, ldpc_frame_result *frames, ldpc_counts *counts);
/* Fused on-device Monte-Carlo of one SNR point (as ldpc_sim_launch: the
 * channel of frame f is the same as the min-sum path's); perturbations from
 * Philox4x32-10 keyed by (seed; bit/4, frame, stream_id | (it+1) << 20).
 * stream_id < 2^20. Asynchronous; counts accumulate in the context. */
int  ldpc_gdbf_sim_launch(ldpc_ctx *ctx, double ebn0_db, double R, const ldpc_gdbf_cfg *cfg, uint64_t seed,
                          uint32_t stream_id, uint64_t first_cw, int batch, ldpc_frame_result *frames_dev);
/* ldpc_gdbf_sim_launch + counts accumulated into *accum; frames host or device. Synchronous. */
int  ldpc_gdbf_sim_batch(ldpc_ctx *ctx, double ebn0_db, double R, const ldpc_gdbf_cfg *cfg, uint64_t seed,
                         uint32_t stream_id, uint64_t first_cw, int batch, ldpc_frame_result *frames,
                         ldpc_counts *accum);
/* Kernel chosen for a GDBF cfg ("gdbf_lds" / "gdbf_global") and its LDS bytes. */
int  ldpc_gdbf_kernel_info(ldpc_ctx *ctx, const ldpc_gdbf_cfg *cfg, char *name, int name_len, int *lds_bytes);

/* ---- re-decoding NGDBF (decodeRSMNGDBF) --------------------------------- */
/* src/RNGDBF.cpp (-D redecode ...): a frame whose decoding attempt ends with
 * unsatisfied checks is decoded again, up to maxphase times (:277-400). Every
 * phase starts from the channel hard decision with theta_i = theta and runs up
 * to T parallel-flip iterations of the GDBF decoder above, with fresh
 * perturbations. The syndrome weight is per bit, w_i = alpha*Ymax/dv_i with
 * LDPC_GDBF_WEIGHT (:564-567) and 1 without. flags is a subset of
 * LDPC_GDBF_NOISE|ADAPT|WEIGHT|SMOOTH|SATURATE (decodeRSMNGDBF sets all five);
 * another ldpc_gdbf_flag is LDPC_ERR_UNSUPPORTED. T >= 1, maxphase >= 1 and
 * maxphase*T <= 4094. A failed phase runs exactly T iterations and a satisfied
 * one fewer, so a frame that reports `iters` iterations ran
 * min(maxphase, iters / T + 1) phases. */
typedef struct {
    int32_t flags;        /* OR of ldpc_gdbf_flag (the five above)        */
    int32_t precision;    /* ldpc_precision                               */
    int32_t T;            /* iterations per phase (maximum; early stop)   */
    int32_t maxphase;     /* decoding attempts per frame (maximum)        */
    int32_t windowsize;   /* SMOOTH: the last windowsize iterations of a phase */
    int32_t reserved;     /* 0                                            */
    double  theta;        /* flip threshold (start value with ADAPT)      */
    double  lambda;       /* ADAPT: threshold decay                       */
    double  alpha;        /* WEIGHT: w_i = alpha * ymax / dv_i            */
    double  noise_scale;  /* perturbation sigma = noise_scale * channel sigma */
    double  ymax;         /* saturation range; also scales the weight     */
} ldpc_rgdbf_cfg;

/* As ldpc_gdbf_decode_batch, with pert[batch][maxphase*T][N]: row phase*T + it
 * is added in iteration it of phase `phase` (required with LDPC_GDBF_NOISE).
 * d_out and frames[].bit_err are the last phase's; frames[].iters and
 * counts->iters are sums over the phases. Synchronous. Replaces the frame
 * body of RNGDBF.cpp main() (:247-404). */
int  ldpc_rgdbf_decode_batch(ldpc_ctx *ctx, const void *y, const void *pert, int batch, const ldpc_rgdbf_cfg *cfg,
                             const int8_t *c, int8_t *d_out, ldpc_frame_result *frames, ldpc_counts *counts);
/* As ldpc_gdbf_sim_launch; the perturbation of iteration it of phase `phase`
 * is keyed by stream_id | (phase*T + it + 1) << 20, so phase 0 draws what
 * ldpc_gdbf_sim_launch draws. stream_id < 2^20. Asynchronous. */
int  ldpc_rgdbf_sim_launch(ldpc_ctx *ctx, double ebn0_db, double R, const ldpc_rgdbf_cfg *cfg, uint64_t seed,
                           uint32_t stream_id, uint64_t first_cw, int batch, ldpc_frame_result *frames_dev);
/* ldpc_rgdbf_sim_launch + counts accumulated into *accum; frames host or device. Synchronous. */
int  ldpc_rgdbf_sim_batch(ldpc_ctx *ctx, double ebn0_db, double R, const ldpc_rgdbf_cfg *cfg, uint64_t seed,
                          uint32_t stream_id, uint64_t first_cw, int batch, ldpc_frame_result *frames,
                          ldpc_counts *accum);
/* Kernel chosen for a cfg ("rgdbf_rows" / "rgdbf_lds" / "rgdbf_global") and its LDS bytes.
 * Option LDPC_OPT_GDBF_KERNEL at 1 forces the generic kernels here too. */
int  ldpc_rgdbf_kernel_info(ldpc_ctx *ctx, const ldpc_rgdbf_cfg *cfg, char *name, int name_len, int *lds_bytes);

/* ---- every attempt of every frame (redecodeStatistics, replayGDBF) ------- */
/* src/newstat.cpp and src/replayGDBF.cpp: a frame is decoded `attempts` times
 * from the same channel samples, each attempt with perturbations of its own,
 * and every attempt runs whether or not an earlier one succeeded. An attempt
 * is exactly one phase of the re-decoding decoder above (maxphase 1): it starts
 * from the channel hard decision with theta_i = theta and dsum = 0 and runs up
 * to T iterations with early stop. flags as ldpc_rgdbf_cfg (another
 * ldpc_gdbf_flag is LDPC_ERR_UNSUPPORTED); 1 <= T <= 4094, attempts >= 1,
 * first_attempt >= 0, first_attempt + attempts <= 2^31 - 1 and attempts * T
 * <= 2^31 - 1 (a frame's summed iterations are an int32), else
 * LDPC_ERR_INVALID. Attempt indices are absolute: local attempt k of a call is
 * attempt first_attempt + k, so a caller may split the attempts over calls. */
typedef struct {           /* ldpc_rgdbf_cfg with the attempt range in place of maxphase */
    int32_t flags, precision, T, attempts, windowsize, first_attempt;
    double  theta, lambda, alpha, noise_scale, ymax;
} ldpc_rstat_cfg;
/* One attempt: the residual error weight (the outcome newstat.cpp logs), the
 * iterations run, whether the output fails a check, and whether the attempt
 * ended inside the smoothing window (it > T - windowsize). */
typedef struct { int32_t bit_err, iters, syndrome_fail, smoothing_used; } ldpc_attempt_result;
/* Per-iteration traces, each optional, host or device. Row `it` of an attempt
 * is what replayGDBF.cpp:370-373 prints after iteration it: the decisions after
 * the flips and the check products that iteration computed before them. The
 * iteration whose check step finds every check satisfied writes no row. */
typedef struct {           /* all optional; host or device */
    int32_t *err_trace;    /* [batch][attempts][T]: bits != codeword after iteration it; -1 not run */
    int32_t *unsat_trace;  /* [batch][attempts][T]: unsatisfied checks found by iteration it's check step; -1 */
    int8_t  *d_trace;      /* [batch][attempts][T][N] +-1 after iteration it; 0 not run */
    int8_t  *s_trace;      /* [batch][attempts][T][M] +-1, the syndrome that iteration used; 0 not run */
} ldpc_rstat_trace;

/* Decode `batch` frames of given raw channel samples y[batch][N] `attempts`
 * times each with pert[batch][attempts][T][N] (row (k, it) is added in iteration
 * it of local attempt k; required with LDPC_GDBF_NOISE). attempts_out
 * [batch][attempts] (host or device, optional) is the product. frames[] and
 * counts follow newstat.cpp:421-465: bit_err, syndrome_fail and d_out are the
 * LAST attempt's, iters the sum over the attempts, uncoded_bit_err is counted
 * once per frame. trace NULL: none. Synchronous. */
int  ldpc_rstat_decode_batch(ldpc_ctx *ctx, const void *y, const void *pert, int batch, const ldpc_rstat_cfg *cfg,
                             const int8_t *c, ldpc_attempt_result *attempts_out, const ldpc_rstat_trace *trace,
                             int8_t *d_out, ldpc_frame_result *frames, ldpc_counts *counts);
/* Fused Monte-Carlo: the channel of frame f is ldpc_rgdbf_sim_launch's; attempt
 * a of frame f draws the perturbations that phase 0 of frame f + (a << 32) draws
 * there (Philox counter (bit / 4, lo32(f), hi32(f) + a, stream_id | (it + 1) << 20)),
 * so attempt 0 is ldpc_rgdbf_sim_launch with maxphase 1. first_cw + batch <= 2^32
 * and stream_id < 2^20, else LDPC_ERR_INVALID. attempts_dev, the traces and
 * frames_dev are device pointers or NULL. Asynchronous. */
int  ldpc_rstat_sim_launch(ldpc_ctx *ctx, double ebn0_db, double R, const ldpc_rstat_cfg *cfg, uint64_t seed,
                           uint32_t stream_id, uint64_t first_cw, int batch, ldpc_attempt_result *attempts_dev,
                           const ldpc_rstat_trace *trace_dev, ldpc_frame_result *frames_dev);
/* ldpc_rstat_sim_launch + counts accumulated into *accum; outputs host or device. Synchronous. */
int  ldpc_rstat_sim_batch(ldpc_ctx *ctx, double ebn0_db, double R, const ldpc_rstat_cfg *cfg, uint64_t seed,
                          uint32_t stream_id, uint64_t first_cw, int batch, ldpc_attempt_result *attempts_out,
                          const ldpc_rstat_trace *trace, ldpc_frame_result *frames, ldpc_counts *accum);
/* ldpc_rstat_sim_batch that also returns the samples drawn, y_out[batch][N] and
 * pert_out[batch][attempts][T][N] (the cfg's precision; rows that were not drawn
 * are zero), and d_out (host or device; any may be NULL). */
int  ldpc_rstat_sim_trace(ldpc_ctx *ctx, double ebn0_db, double R, const ldpc_rstat_cfg *cfg, uint64_t seed,
                          uint32_t stream_id, uint64_t first_cw, int batch, void *y_out, void *pert_out,
                          ldpc_attempt_result *attempts_out, const ldpc_rstat_trace *trace, int8_t *d_out,
                          ldpc_frame_result *frames, ldpc_counts *accum);
/* Kernel chosen for a cfg, with or without traces: "rstat_rows" (the codes
 * rgdbf_rows takes: a persistent workgroup with the graph in registers) or
 * "rstat_wg" (a workgroup per attempt; lds_bytes 0: its state is in a global
 * slot). Traces and option LDPC_OPT_GDBF_KERNEL at 1 force rstat_wg. The cfg is
 * checked first, also with a NULL context. */
int  ldpc_rstat_kernel_info(ldpc_ctx *ctx, const ldpc_rstat_cfg *cfg, int with_trace, char *name, int name_len,
                            int *lds_bytes);

/* ---- fixed-point NGDBF hardware model (NGDBFhw) -------------------------- */
/* src/NGDBFhw.cpp: channel samples and perturbations are sign-magnitude nq-bit
 * codes expanded to odd integers Y_i, Q_k in +-(2^nq - 1) (:611-677); the
 * energy E_i = (1 - 2 d_i) Y_i + Smult * (satisfied checks of bit i) +
 * Q[i + qpointer] is an integer and bit i flips when E_i <= theta (:565-593),
 * with lmax = ymax / (2w), NL = 2^nq - 1, Smult = round(NL / lmax) and
 * theta = unpack(pack(quantize(2.0), +1)) (:174-179; 7 and 15 at the defaults).
 * The perturbation is a shift register of qlen samples drawn once per frame:
 * qpointer advances by one per iteration, wraps to 0 at qlen - N and carries
 * over from phase to phase. Every one of the maxphase phases starts from the
 * channel decision and runs up to T iterations (early stop); all phases run.
 * The reference's constants (:48-57, in the comments below) are compile-time
 * there, so only the defaults are pinned by recorded reference runs; other T,
 * maxphase, nq and qlen are pinned by the numpy restatement of the tests alone.
 * The front end (saturate, y / (2w), quantise, pack) runs on the device in
 * `precision`; F64 reproduces the reference bit for bit. */
typedef struct {
    int32_t precision;    /* front end: LDPC_F32 / LDPC_F64            */
    int32_t T;            /* 600  iterations per phase (early stop)     */
    int32_t maxphase;     /* 1                                          */
    int32_t nq;           /* 5    bits per sample, 2..7                 */
    int32_t qlen;         /* 2648 noise samples per frame, > N          */
    int32_t reserved;     /* 0                                          */
    double  w, ymax, noise_scale, theta0;   /* 0.185 1.625 0.95 -0.525 */
} ldpc_hwgdbf_cfg;

/* Decode `batch` frames of given RAW channel samples y[batch][N] and raw noise
 * draws q[batch][qlen] (noiseSigma * n; float for F32, double for F64; host or
 * device). qptr0[batch] (host, int32, or NULL = 0) is each frame's start
 * pointer, in [0, qlen - N). c (bipolar, NULL = all +1), d_out (bipolar, the
 * last phase's decisions) and counts as ldpc_decode_batch. frames[].bit_err is
 * the least error weight over the phases, frames[].iters the least iteration
 * count (counts->iters sums it), frames[].syndrome_fail whether the last phase
 * ended unsatisfied, frames[].uncoded_bit_err the channel decision's errors.
 * iters_run[batch] (host or device, optional): the sum of the phases' iteration
 * counts, which is what a caller adds to the pointer (mod qlen - N).
 * qlen <= N is LDPC_ERR_INVALID; a graph whose N + qlen + N + M bytes of state
 * exceed the 65536-byte LDS bound is LDPC_ERR_UNSUPPORTED. Synchronous.
 * Replaces the frame body of NGDBFhw.cpp main() (:218-373). */
int  ldpc_hwgdbf_decode_batch(ldpc_ctx *ctx, const void *y, const void *q, const int32_t *qptr0, int batch,
                              const ldpc_hwgdbf_cfg *cfg, const int8_t *c, int8_t *d_out, ldpc_frame_result *frames,
                              int32_t *iters_run, ldpc_counts *counts);
/* Fused on-device Monte-Carlo of one SNR point: the channel of frame f is the
 * min-sum path's for the same (seed, frame); noise sample k of a frame is
 * noise_scale * sigma * n with n from Philox4x32-10 keyed by
 * (seed; k / 4, frame, stream_id | 1 << 20). Every frame starts at pointer 0.
 * stream_id < 2^20. Asynchronous; counts accumulate in the context. */
int  ldpc_hwgdbf_sim_launch(ldpc_ctx *ctx, double ebn0_db, double R, const ldpc_hwgdbf_cfg *cfg, uint64_t seed,
                            uint32_t stream_id, uint64_t first_cw, int batch, ldpc_frame_result *frames_dev);
/* ldpc_hwgdbf_sim_launch + counts accumulated into *accum; frames host or device. Synchronous. */
int  ldpc_hwgdbf_sim_batch(ldpc_ctx *ctx, double ebn0_db, double R, const ldpc_hwgdbf_cfg *cfg, uint64_t seed,
                           uint32_t stream_id, uint64_t first_cw, int batch, ldpc_frame_result *frames,
                           ldpc_counts *accum);
/* ldpc_hwgdbf_sim_batch that also returns the samples drawn, y_out[batch][N] and
 * q_out[batch][qlen] (the cfg's precision), and d_out (host or device; any may be NULL). */
int  ldpc_hwgdbf_sim_trace(ldpc_ctx *ctx, double ebn0_db, double R, const ldpc_hwgdbf_cfg *cfg, uint64_t seed,
                           uint32_t stream_id, uint64_t first_cw, int batch, void *y_out, void *q_out,
                           int8_t *d_out, ldpc_frame_result *frames, ldpc_counts *accum);
/* Kernel chosen for a cfg ("hwgdbf_wave": a wavefront per codeword, "hwgdbf_wg": a
 * workgroup per codeword; the library takes the one that keeps more waves on a CU, and
 * option LDPC_OPT_GDBF_KERNEL at 1 forces hwgdbf_wg) and the LDS bytes of a workgroup. The cfg is checked first, also with a NULL context. */
int  ldpc_hwgdbf_kernel_info(ldpc_ctx *ctx, const ldpc_hwgdbf_cfg *cfg, char *name, int name_len, int *lds_bytes);

/* ---- fixed-point min-sum (fxms) ----------------------------------------- */
/* Flooding MS / NMS / OMS whose messages are msg_bits-wide saturating integers,
 * as a hardware min-sum decoder has them (the reference's min-sum programs only
 * quantise the channel samples, -D quantizeSamples; its messages stay double).
 * With Nq = 2^qbits, V = 2^(msg_bits - 1) - 1 and sgn(x) = x >= 0 ? +1 : -1
 * (decodeMinSum.cpp:518-523):
 *   front end  in `precision` (ymax rounded to it once), quantize() of
 *              decodeMinSum.cpp:480-489 in its order of operations, as an integer
 *              code: a = |y|, s = sgn(y); a > ymax: Y = s (Nq - 1); else
 *              Y = s 2 max(floor(a (Nq - 1) / (2 ymax)), 1). Y is never 0 and odd
 *              only when saturated. For ymax = (Nq - 1) 2^-s, Y 2^-s is the
 *              quantised sample of ldpc_decoder_cfg.quantize exactly. The uncoded
 *              decision is r = Y > 0 ? +1 : -1.
 *   start      v2c = clamp(Y_i, -V, V) on every edge of bit i.
 *   check j    P = prod sgn(v2c) over the row, m1 <= m2 the two smallest |v2c|
 *              (V where the row has fewer edges); for edge k, mag = m2 at the
 *              position of the minimum, else m1; MS: as is; NMS:
 *              (mag * nms_num) >> nms_shift; OMS: max(mag - beta, 0);
 *              c2v_k = P sgn(v2c_k) mag.
 *   bit i      S_i = Y_i + sum c2v in int32 (the unclamped Y_i);
 *              v2c_k = clamp(S_i - c2v_k, -V, V); d_i = S_i > 0 ? +1 : -1.
 * T flooding iterations (T = 0: d = r); early_stop as ldpc_decoder_cfg.early_stop
 * (the result is D(s) for the smallest s in 0..T with a zero syndrome, s = T when
 * there is none; frames[].iters = s and counts->iters += s; without it
 * frames[].iters = 0 and counts->iters += T). Everything after the front end is
 * integer, so results are exact on every kernel shape, and a decoder whose messages
 * never saturate reproduces fp64 MS / OMS on grid samples bit for bit.
 * A codeword's state -- the messages of maxdc * M slots (one byte each for
 * msg_bits <= 8, else two) and 2 N bytes -- lives in LDS: a graph where it exceeds
 * 65536 bytes is LDPC_ERR_UNSUPPORTED (DVB-S2 is out of scope: no global-memory
 * kernel). No reference program computes this decoder. */
typedef struct {
    int32_t variant;     /* LDPC_MS | LDPC_NMS | LDPC_OMS; another ldpc_variant: LDPC_ERR_UNSUPPORTED */
    int32_t precision;   /* front end only */
    int32_t T;           /* >= 0 */
    int32_t qbits;       /* 2..7  (|Y| <= 127) */
    int32_t msg_bits;    /* 2..16 */
    int32_t nms_num;     /* NMS: 1 <= nms_num <= 2^nms_shift */
    int32_t nms_shift;   /* NMS: 0..7 */
    int32_t beta;        /* OMS: >= 0 */
    int32_t early_stop;
    int32_t reserved;    /* 0 */
    double  ymax;        /* > 0 */
} ldpc_fxms_cfg;

/* Decode `batch` frames of given raw channel samples y[batch][N] (float for F32,
 * double for F64); every argument as ldpc_decode_batch. Synchronous. */
int  ldpc_fxms_decode_batch(ldpc_ctx *ctx, const void *y, int batch, const ldpc_fxms_cfg *cfg, const int8_t *c,
                            int8_t *d_out, ldpc_frame_result *frames, ldpc_counts *counts);
/* Fused on-device Monte-Carlo of one SNR point: the channel of frame f is the
 * min-sum path's for the same (seed, stream_id, frame), the codeword table of
 * ldpc_sim_set_codewords applies. Asynchronous; counts accumulate in the context. */
int  ldpc_fxms_sim_launch(ldpc_ctx *ctx, double ebn0_db, double R, const ldpc_fxms_cfg *cfg, uint64_t seed,
                          uint32_t stream_id, uint64_t first_cw, int batch, ldpc_frame_result *frames_dev);
/* ldpc_fxms_sim_launch + counts accumulated into *accum; frames host or device. Synchronous. */
int  ldpc_fxms_sim_batch(ldpc_ctx *ctx, double ebn0_db, double R, const ldpc_fxms_cfg *cfg, uint64_t seed,
                         uint32_t stream_id, uint64_t first_cw, int batch, ldpc_frame_result *frames,
                         ldpc_counts *accum);
/* ldpc_fxms_sim_batch that also returns the raw samples drawn, y_out[batch][N] (the
 * cfg's precision; ldpc_sim_trace's bit for bit), the integer codes
 * ycode_out[batch][N] and d_out (host or device; any may be NULL). */
int  ldpc_fxms_sim_trace(ldpc_ctx *ctx, double ebn0_db, double R, const ldpc_fxms_cfg *cfg, uint64_t seed,
                         uint32_t stream_id, uint64_t first_cw, int batch, void *y_out, int8_t *ycode_out,
                         int8_t *d_out, ldpc_frame_result *frames, ldpc_counts *accum);
/* Kernel chosen for a cfg ("fxms_i8": one-byte messages, msg_bits <= 8; "fxms_i16")
 * and the LDS bytes of a workgroup. The cfg is checked first, also with a NULL context. */
int  ldpc_fxms_kernel_info(ldpc_ctx *ctx, const ldpc_fxms_cfg *cfg, char *name, int name_len, int *lds_bytes);

/* ---- layered fixed-point min-sum (fxlms) -------------------------------- */
/* Row-layered MS / NMS / OMS in integers, as a hardware layered decoder computes it:
 * a saturating posterior (APP) of app_bits per bit and a message of msg_bits per edge,
 * updated in place row by row as Q = P - R_old, R_new = f(Q), P = Q + R_new. With
 * Nq = 2^qbits, V = 2^(msg_bits - 1) - 1, A = 2^(app_bits - 1) - 1 and
 * sgn(x) = x >= 0 ? +1 : -1:
 *   front end  exactly ldpc_fxms_cfg's: the integer code Y in `precision`; the
 *              uncoded decision is r = Y > 0 ? +1 : -1.
 *   start      app_i = clamp(Y_i, -A, A); every c2v = 0.
 *   iteration  for each check row j in the order ldpc_graph_layers() returns
 *              (row_order), serially, with b_k the bit of its edge k:
 *                x_k = clamp(app[b_k] - c2v[j][k], -V, V);
 *                P = prod sgn(x_k), m1 <= m2 the two smallest |x_k| (m2 = V when the
 *                row has one edge; a row of degree 0 does nothing);
 *                mag = m2 at the position of the minimum, else m1; f as in fxms: MS as
 *                is, NMS (mag * nms_num) >> nms_shift, OMS max(mag - beta, 0);
 *                c_k = P sgn(x_k) f(mag); c2v[j][k] = c_k;
 *                app[b_k] = clamp(x_k + c_k, -A, A), in int32 from the clamped x_k.
 *   decision   d_i = app_i > 0 ? +1 : -1.
 * T iterations (T = 0: d = r); early_stop as ldpc_fxms_cfg's: the result is D(s) for
 * the smallest s in 0..T whose decisions have a zero syndrome (checked between whole
 * iterations and after the last), s = T when there is none; frames[].iters = s and
 * counts->iters += s; without it frames[].iters = 0 and counts->iters += T.
 * Rows of one layer share no bit and integers commute exactly, so any parallel
 * execution of a layer gives these results, and the result of a frame depends on the
 * frame only. With app_bits = msg_bits + 1 and msg_bits >= qbits the APP clamp never
 * acts (|x + c| <= 2 V < A); a decoder whose clamps never act reproduces the fp64
 * LAYERED MS / OMS on grid samples bit for bit. A codeword's state -- N
 * APPs (one byte each for app_bits <= 8, else two) and the packed messages of M rows
 * (6 bytes a row, 8 with two-byte APPs, 4 more where a row has more than 26 edges) --
 * lives in LDS: a graph where it exceeds 65536 bytes is LDPC_ERR_UNSUPPORTED (DVB-S2)
 * unless the context's option LDPC_OPT_KERNEL is 3 ("global"). That value selects, on
 * every graph it can hold, the kernel that gives a codeword to a workgroup, keeps the
 * APPs in LDS and the rows' messages in global memory; it computes the same results and
 * is LDPC_ERR_UNSUPPORTED only where N APPs plus 256 bytes exceed the 163840 bytes of
 * LDS a workgroup may use (DVB-S2 N=64800 fits at either APP width). No reference
 * program computes this decoder. */
typedef struct {
    int32_t variant;     /* LDPC_MS | LDPC_NMS | LDPC_OMS; another ldpc_variant: LDPC_ERR_UNSUPPORTED */
    int32_t precision;   /* front end only */
    int32_t T;           /* >= 0 */
    int32_t qbits;       /* 2..7  (|Y| <= 127) */
    int32_t msg_bits;    /* 2..16 */
    int32_t app_bits;    /* msg_bits..16 */
    int32_t nms_num;     /* NMS: 1 <= nms_num <= 2^nms_shift */
    int32_t nms_shift;   /* NMS: 0..7 */
    int32_t beta;        /* OMS: >= 0 */
    int32_t early_stop;  /* 0 | 1 */
    double  ymax;        /* > 0 */
} ldpc_fxlms_cfg;

/* The five calls of fixed-point min-sum, argument for argument: given samples, the fused
 * Monte-Carlo (the channel of frame f is the min-sum path's for the same (seed, stream_id,
 * frame); the codeword table of ldpc_sim_set_codewords applies), its synchronous form, the
 * form that also returns the samples drawn and their integer codes, and the kernel chosen
 * ("fxlms_i8": one-byte APPs and messages, app_bits <= 8; "fxlms_i16"; with LDPC_OPT_KERNEL
 * at 3 "fxlms_wg_i8" / "fxlms_wg_i16") with the LDS bytes of a workgroup. The cfg is checked first, also with a NULL context. */
int  ldpc_fxlms_decode_batch(ldpc_ctx *ctx, const void *y, int batch, const ldpc_fxlms_cfg *cfg, const int8_t *c,
                             int8_t *d_out, ldpc_frame_result *frames, ldpc_counts *counts);
int  ldpc_fxlms_sim_launch(ldpc_ctx *ctx, double ebn0_db, double R, const ldpc_fxlms_cfg *cfg, uint64_t seed,
                           uint32_t stream_id, uint64_t first_cw, int batch, ldpc_frame_result *frames_dev);
int  ldpc_fxlms_sim_batch(ldpc_ctx *ctx, double ebn0_db, double R, const ldpc_fxlms_cfg *cfg, uint64_t seed,
                          uint32_t stream_id, uint64_t first_cw, int batch, ldpc_frame_result *frames,
                          ldpc_counts *accum);
int  ldpc_fxlms_sim_trace(ldpc_ctx *ctx, double ebn0_db, double R, const ldpc_fxlms_cfg *cfg, uint64_t seed,
                          uint32_t stream_id, uint64_t first_cw, int batch, void *y_out, int8_t *ycode_out,
                          int8_t *d_out, ldpc_frame_result *frames, ldpc_counts *accum);
int  ldpc_fxlms_kernel_info(ldpc_ctx *ctx, const ldpc_fxlms_cfg *cfg, char *name, int name_len, int *lds_bytes);

/* ---- non-binary GF(q) codes, Extended Min-Sum (BASELINE config 5) ------ */
/* Messages are reliabilities over GF(q) (0 = most likely symbol); check
 * nodes are the forward-backward EMS with messages truncated to the nm most
 * likely symbols and absent symbols filled with (largest kept value +
 * offset); symbol nodes add the channel reliabilities and the incoming
 * messages. Channel: each symbol is m = log2(q) BPSK bits (bit i of the
 * symbol's integer value, 0 -> +1), y = x(1 + sigma n), bit LLR 4y/N0.
 * Exact definition: DESIGN.md §11 and oracle/ems_oracle.c. No reference
 * counterpart computes this (parity unpinned); q = 2 reduces to min-sum.
 * Graphs take q = 2..64; the device kernels decode q = 4, 8 and 16 (the
 * reference's GF(4) and GF(8) codes among them). On-device noise: symbol v
 * makes one Philox call (counter word 0 = v) and its first m normals are the
 * symbol's bits 0..m-1. */
typedef struct ldpc_nb_graph ldpc_nb_graph;
typedef struct ldpc_nb_ctx ldpc_nb_ctx;

typedef struct {
    int32_t T;          /* maximum iterations                                */
    int32_t nm;         /* message truncation (>= q: full vectors)           */
    int32_t early_stop; /* stop when H*d = 0 (checked before each iteration)  */
    int32_t reserved;   /* 0                                                 */
    double  offset;     /* fill offset for truncated (absent) symbols        */
} ldpc_ems_cfg;

/* ldpc_counts + symbol errors; bit_err counts bits of the decided symbols. */
typedef struct {
    int64_t bit_err, frame_err, uncoded_bit_err, frames, iters, syndrome_fail, symbol_err;
} ldpc_nb_counts;

/* Arrays as the NB alist_struct (SystemC/NB-LDPC/inc/alist.h:25-43): nlist /
 * nvals per column (1-based check, GF value), mlist / mvals per row. q a
 * power of two (2..64), coefficients 1..q-1, check degree >= 2; both views
 * must describe the same edges and coefficients (else LDPC_ERR_GRAPH). */
int  ldpc_nb_graph_create(int N, int M, int q, const int *num_nlist, const int *const *nlist,
                          const int *const *nvals, const int *num_mlist, const int *const *mlist,
                          const int *const *mvals, ldpc_nb_graph **out);
int  ldpc_nb_graph_load_alist(const char *path, ldpc_nb_graph **out);
int  ldpc_nb_graph_info(const ldpc_nb_graph *g, int *N, int *M, int *q, int *E, int *maxdv, int *maxdc);
void ldpc_nb_graph_destroy(ldpc_nb_graph *g);

/* Device context: q in {4, 8, 16}, row degree <= 8, N <= 65535, maxdc * M <=
 * 65535, and the bit LLRs, decisions and syndrome of one codeword within LDS.
 * LDPC_ERR_UNSUPPORTED otherwise: q = 2 (binary codes have their own
 * decoders) and q = 32, 64 (a check lane cannot hold their vectors). */
int  ldpc_nb_ctx_create(int device, const ldpc_nb_graph *g, int max_batch, ldpc_nb_ctx **out);
int  ldpc_nb_ctx_set_stream(ldpc_nb_ctx *ctx, void *hip_stream);
void ldpc_nb_ctx_destroy(ldpc_nb_ctx *ctx);
int  ldpc_nb_ctx_read_counts(ldpc_nb_ctx *ctx, ldpc_nb_counts *out, int reset);
int  ldpc_nb_ctx_last_kernel_ms(ldpc_nb_ctx *ctx, float *ms);
/* "ems_lds" (messages in LDS), "ems_global" (a global slot per workgroup) or
 * "ems_global_sched" (that, and the schedule tables read from global memory:
 * codes whose tables exceed LDS, such as the reference's GF(4) code). */
int  ldpc_ems_kernel_info(ldpc_nb_ctx *ctx, char *name, int name_len, int *lds_bytes);
/* (ABI 10) The EMS options of ldpc_option (LDPC_OPT_EMS_*); the others are refused. */
int  ldpc_nb_ctx_set_option(ldpc_nb_ctx *ctx, int option, int value);

/* Decode given channel samples y[batch][N*m] (float, host or device) with
 * bit LLRs 4y/n0. c: transmitted symbols [batch][N] or NULL (all-zero).
 * d_out [batch][N] symbols, frames[].iters = iterations run. Synchronous. */
int  ldpc_ems_decode_batch(ldpc_nb_ctx *ctx, const float *y, int batch, double n0, const ldpc_ems_cfg *cfg,
                           const uint8_t *c, uint8_t *d_out, ldpc_frame_result *frames, ldpc_nb_counts *counts);
/* Fused Monte-Carlo of the all-zero codeword: Philox4x32-10 keyed by
 * (seed; symbol, frame, stream_id), sigma = sqrt(10^(-ebn0/10)/R/2).
 * Asynchronous; counts accumulate in the context. */
int  ldpc_ems_sim_launch(ldpc_nb_ctx *ctx, double ebn0_db, double R, const ldpc_ems_cfg *cfg, uint64_t seed,
                         uint32_t stream_id, uint64_t first_cw, int batch, ldpc_frame_result *frames_dev);
int  ldpc_ems_sim_batch(ldpc_nb_ctx *ctx, double ebn0_db, double R, const ldpc_ems_cfg *cfg, uint64_t seed,
                        uint32_t stream_id, uint64_t first_cw, int batch, ldpc_frame_result *frames,
                        ldpc_nb_counts *accum);
/* ldpc_ems_sim_batch that also returns the generated samples y_out [batch][N*m]
 * and decisions d_out [batch][N] (host or device; either may be NULL). */
int  ldpc_ems_sim_trace(ldpc_nb_ctx *ctx, double ebn0_db, double R, const ldpc_ems_cfg *cfg, uint64_t seed,
                        uint32_t stream_id, uint64_t first_cw, int batch, float *y_out, uint8_t *d_out,
                        ldpc_frame_result *frames, ldpc_nb_counts *accum);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_HIP_H */
