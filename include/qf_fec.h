/*
 * qf_fec.h -- C ABI of the MI355X-native GF(2^8) RLNC FEC library
 *             (libqf_fec.so, hand-written HIP kernels for gfx950).
 *
 * This is the drop-in boundary for QuicFuscate's src/fec hot path.  Every
 * entry point names the reference interface it replaces (paths relative to
 * the reference repository, Christopher-Schulze/QuicFuscate @ 2025-07-18).
 * INTEGRATION.md shows the Rust FFI a maintainer would add on the reference
 * side.
 *
 * Conventions
 *  - All functions return int status: QF_OK (0) or a negative QF_E* code.
 *    Nothing panics or aborts; the reference's panics (gf_inv(0), k + r > 256)
 *    become QF_ERANGE.
 *  - Buffers are caller-owned.  The library never frees or zeroes caller
 *    memory.  "_dev" pointers are device (HBM) pointers; "_host" pointers are
 *    host memory (pinned for full PCIe rate).
 *  - Work is enqueued asynchronously on the context's stream; qf_sync()
 *    waits.  One context per host thread; distinct contexts are independent.
 *  - Arithmetic is GF(2^8) with polynomial 0x11D and generator 2, table
 *    semantics (gf_tables.rs:47-57, 384-408).
 */
#ifndef QF_FEC_H
#define QF_FEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QF_OK 0
#define QF_EINVAL (-1)     /* bad argument / shape                               */
#define QF_ERANGE (-2)     /* gf_inv(0): k + r > 256, Cauchy undefined (F5)      */
#define QF_ENOTREADY (-3)  /* window not full / fewer than k rows received       */
#define QF_ERANK (-4)      /* decode matrix singular                             */
#define QF_EDEVICE (-5)    /* HIP runtime error                                  */
#define QF_ENOMEM (-6)     /* allocation failed                                  */
#define QF_ETOOSMALL (-7)  /* output buffer too short (quiche BufferTooShort)    */
#define QF_ESTALE (-8)     /* frame older than the generation its slot now holds */
#define QF_ECLOSED (-9)    /* frame of the slot's generation, which is closed    */

#define QF_ABI_VERSION 1
int qf_abi_version(void);
const char *qf_strerror(int status);
/* The cause of the calling thread's most recent QF_EDEVICE: the failing HIP
 * call's source file:line and error name, and, when a generated kernel's
 * launch checks refused the call, which check ("... (qf_bs.hip:339 launch
 * refused)").  Thread-local, like errno: kept until the next device failure on
 * this thread; "" if there was none.  No reference counterpart (the
 * reference's codec has no device). */
const char *qf_last_error(void);

/* ---------------------------------------------------------------------------
 * GF(2^8) scalar helpers (host).  These mirror the reference's public GF API
 * for callers and parity tests; the hot path never calls them.
 * ------------------------------------------------------------------------- */
/* replaces gf_tables.rs:392 init_gf_tables (idempotent) */
int qf_gf256_init(void);
/* replaces gf_tables.rs:283 gf_mul and :47 gf_mul_table (same result) */
uint8_t qf_gf256_mul(uint8_t a, uint8_t b);
/* replaces gf_tables.rs:327 gf_mul_add: a*b ^ c */
uint8_t qf_gf256_mul_add(uint8_t a, uint8_t b, uint8_t c);
/* replaces gf_tables.rs:304 gf_inv / :312 gf_inv_prefetch; QF_ERANGE for 0 */
int qf_gf256_inv(uint8_t a, uint8_t *out);
/* replaces decoder.rs:280-298 Encoder::generate_cauchy_coefficients for
 * repairs 0..r-1: out[j*k + i] = inv((u8)i ^ (u8)(k + j)).  QF_ERANGE where
 * the reference panics (k + r > 256). */
int qf_cauchy_coeffs(uint32_t k, uint32_t r, uint8_t *out_rxk);
/* No reference counterpart (the rule of qf_rank_batch below, on the host, no
 * device needed): n vectors of k bytes in arrival order, vectors_nxk[s*k + i].
 * innovative_out[s] (may be NULL) = 1 iff vector s is not in the GF(2^8) span
 * of vectors 0..s-1, *rank_out = the number of such vectors.  Plain
 * arrival-order elimination with table arithmetic.  QF_EINVAL for k == 0, a
 * NULL rank_out, or NULL vectors with n > 0. */
int qf_gf256_rank(uint32_t k, uint32_t n, const uint8_t *vectors_nxk,
                  uint8_t *innovative_out, uint32_t *rank_out);

/* ---------------------------------------------------------------------------
 * Context
 * ------------------------------------------------------------------------- */
typedef struct qf_ctx qf_ctx;
/* device: HIP device ordinal.  stream: hipStream_t to enqueue on (NULL = the
 * context creates its own non-blocking stream; QF_STREAM_NULL = the device's
 * null stream, ordered with other work on it, e.g. torch's default stream). */
#define QF_STREAM_NULL ((void *)1)
int qf_ctx_create(int device, void *stream, qf_ctx **out);
int qf_ctx_destroy(qf_ctx *ctx);
int qf_ctx_set_stream(qf_ctx *ctx, void *stream);
void *qf_ctx_stream(qf_ctx *ctx);
/* Split-phase decode.  The next qf_decode_batch on ctx enqueues its
 * acceptance pass (row indices only: first k rows win, slot map, LU/inverse
 * records -- the bookkeeping the reference's Decoder::add_packet does on
 * arrival, decoder.rs:678-701) at once, and makes its payload pass
 * (Decoder::try_decode / gaussian_elimination, decoder.rs:720-783) wait for
 * `event` (a hipEvent_t recorded on any stream, e.g. after the H2D copy of
 * the rows).  The setting is cleared when that qf_decode_batch returns;
 * NULL clears it.  No reference counterpart beyond the add_packet /
 * try_decode split. */
int qf_ctx_set_payload_wait(qf_ctx *ctx, void *event);
/* Split-phase decode on two streams.  The next qf_decode_batch on ctx keeps
 * its acceptance pass on the context's stream and enqueues its payload pass
 * on `stream` (a hipStream_t; QF_STREAM_NULL = the null stream) after it, so
 * a caller whose rows are produced on `stream` needs no cross-stream wait
 * before the payload and none after it: the call's work is complete when
 * `stream` reaches that point.  Combines with qf_ctx_set_payload_wait.  The
 * fused decode runs its payload kernel on `stream`; the other decode paths
 * finish on the context's stream and `stream` waits for them.  The context's
 * own stream also waits for the payload pass (an event, no host block), so a
 * later call on ctx -- the next decode rewriting the context's workspace,
 * qf_sync, qf_ctx_destroy -- is ordered after it.  Cleared when
 * that qf_decode_batch returns; NULL clears it.  qf_decode_batch_host and
 * qf_decode_batch_desc clear it and run on the context's stream. */
int qf_ctx_set_payload_stream(qf_ctx *ctx, void *stream);
int qf_sync(qf_ctx *ctx);

/* Kernel-path options of a context.  No reference counterpart: the
 * reference codec has no tuning knobs (core.rs:189-303 builds it with its
 * defaults), and the defaults here are the fastest measured paths.  They let
 * a host pin a kernel path per context (A/B, work-arounds); every call on the
 * context reads the context's values, and no call reads the environment.
 * qf_ctx_create sets each option to its default and then, once, to the
 * integer in the environment variable named in brackets when that is set
 * (tooling compatibility).  Values are clamped to the ranges given;
 * QF_EINVAL for an unknown option. */
enum {
    QF_OPT_FFT_KERNELS = 0,      /* 1: additive-FFT Cauchy kernels where generated; 0: one coefficient
                                    block per repair [QF_FFT_KERNELS; default 1] */
    QF_OPT_BITSLICED,            /* 0: no bit-sliced Cauchy kernels, v_perm paths only
                                    [QF_DISABLE_BS=1 sets 0; default 1] */
    QF_OPT_ENCODE_SMALL,         /* small-batch encode kernel: -1 auto, 0 never, 1 always [QF_ENCODE_SMALL] */
    QF_OPT_ENCODE_KSPLIT,        /* 1: row-split encode passes for <= 1 item per CU; 0 never [QF_ENCODE_KSPLIT] */
    QF_OPT_ENCODE_V,             /* 16-B units per lane of k_combine_uniform: 1 or 2 [QF_ENCODE_V] */
    QF_OPT_ENCODE_PD,            /* prefetch depth of k_combine_uniform, 1..3 [QF_ENCODE_PD; default 2] */
    QF_OPT_DECODE_PATH,          /* Cauchy decode: 0 fused lane-chunk, 1 syndromes + combine
                                    [QF_DECODE_SYN=1], 2 fused item layout [QF_DECODE_LEGACY=1] */
    QF_OPT_DECODE_KSPLIT,        /* 1: row-split fused decode for <= 1 item per CU; 0 never [QF_DECODE_KSPLIT] */
    QF_OPT_DECODE_SYNW,          /* 1: scalar-map syndrome passes at long rows (r > 16); 0 never
                                    [QF_DECODE_NO_SYNW=1 sets 0] */
    QF_OPT_DECODE_PD,            /* prefetch depth of k_combine_slots, 1..3 [QF_DECODE_PD; default 1] */
    QF_OPT_DECODE_CHUNK,         /* generations per chunk of the general decode, 0 = all [QF_DECODE_CHUNK] */
    QF_OPT_DECODE_OVERLAP,       /* 1: chunked general decode overlaps chunks on two streams [QF_DECODE_OVERLAP] */
    QF_OPT_COMBINE_BS,           /* 1: bit-sliced payload pass (qf_combine_bs) at long rows; 0 never [QF_COMBINE_BS] */
    QF_OPT_COMBINE_BS_MIN_Q,     /* its smallest row, in 32-B lane-chunks [QF_COMBINE_BS_MIN_Q; default 64] */
    QF_OPT_COMBINE_SPLIT,        /* 1: slot-split payload pass for <= 1 item per CU; 0 never [QF_COMBINE_SPLIT] */
    QF_OPT_PREPARE_GRID,         /* split-phase acceptance pass grid, 0 = one block per CU [QF_PREPARE_GRID] */
    QF_OPT_ENC_BLOCKS_PER_CU,    /* cap of the bit-sliced encode grid, 0 = none [QF_ENC_BLOCKS_PER_CU] */
    QF_OPT_DEC_BLOCKS_PER_CU,    /* cap of the fused decode grid, 0 = none [QF_DEC_BLOCKS_PER_CU] */
    QF_OPT_SEND_FUSED,           /* 1: one-launch per-packet send (k_send_window); 0 never [QF_SEND_FUSED] */
    QF_OPT_SEND_WINDOWS_MIN_TILES, /* send batches: tiles from which k_encode_windows is used [default 256] */
    QF_OPT_SEND_CHUNKS,          /* send batches: D2H chunks, 1..8 [QF_SEND_CHUNKS; default 1] */
    QF_OPT_SEND_PROFILE,         /* 1: phase timing of send batches on stderr at qf_ctx_destroy [QF_SEND_PROFILE] */
    QF_OPT_COPY_THREADS,         /* host copy-out workers of send/receive batches, -1 = auto.  Process-wide:
                                    the first batch call creates the pool [QF_COPY_THREADS] */
    QF_OPT_GF16_DYN,             /* 1: GF(2^16) decode launches shaped on the device; 0 from e_max [QF_GF16_DYN] */
    QF_OPT_GF16_LOGIFY,          /* 1: GF(2^16) inputs in log form for wide matvecs; 0 never [QF_GF16_LOGIFY] */
    QF_OPT_GF16_LOGIFY_MIN_BLOCKS, /* output blocks from which inputs are logified [QF_GF16_LOGIFY_MIN_BLOCKS] */
    QF_OPT_GF16_LDS_GJ,          /* 1: GF(2^16) Gauss-Jordan in LDS for e <= 64 [QF_GF16_LDS_GJ; default 0] */
    QF_OPT_GF16_BITSLICED,       /* 1: bit-sliced GF(2^16) Cauchy encode and decode syndromes where
                                    generated; 0 never [QF_GF16_BITSLICED; default 1] */
    QF_OPT_GF16_FFT,             /* additive-FFT GF(2^16) Cauchy encode / decode syndromes for
                                    k = 2^a in [16, 4096] (first + r <= k) without a bit-sliced kernel:
                                    1 where it needs ~9x fewer products than the matvec, 2 always,
                                    0 never [QF_GF16_FFT; default 1] */
    QF_OPT_WIEDEMANN_PROJ,       /* k > 256 decoder's projections: 1 = the reference's first init vector
                                    (decoder.rs:805-807, b = 0), then random vectors drawn per attempt
                                    from a per-process secret (a packet sender cannot craft a matrix
                                    that defeats them and forces the exact host fallback); 0 = the
                                    reference's init vectors b = 0..7 only [QF_WIEDEMANN_PROJ; default 1] */
    QF_OPT_GF16_FFT_BS,          /* the GF(2^16) additive FFT for k <= 2048 bit-sliced (field elements
                                    in 16 bit planes, no table lookups): 1 where a batch has items for
                                    a quarter of the CUs, 2 always, 3 always with two layers per LDS
                                    pass; 0 the log / Zech-table kernel for every k
                                    [QF_GF16_FFT_BS; default 1] */
    QF_OPT_PREPARE_LANES,        /* 1: the fused decode's acceptance pass runs one generation per lane
                                    (k_decode_prepare_lu_lanes); 0: one per wave [QF_PREPARE_LANES;
                                    default 1] */
    QF_OPT_ENCODE_MERGED,        /* 1: multi-pass work in ONE dispatch each: the encode passes of a
                                    code with more repairs than one kernel holds (C5 r > 22; a
                                    workgroup's waves run the passes on one item, so each source row
                                    is read from HBM once), and the decode's syndrome and payload
                                    passes (pass-major workgroup ranges); 0: one launch per pass
                                    [QF_ENCODE_MERGED; default 1] */
    QF_OPT_SYNW_SHARED,          /* 1: the additive-FFT syndrome passes of the C5 decode item-major in
                                    one dispatch, the passes' waves sharing the source rows' gather,
                                    transposes and chunk butterflies through LDS; 0: pass-major
                                    (each pass re-reads the sources) [QF_SYNW_SHARED; default 1] */
    QF_OPT_COMBINE_WIDE,         /* 1: a bit-sliced payload pass with 17-24 outputs (e_max) runs as one
                                    24-output pass reading two coefficient records per row; 0: two
                                    16-output passes (pass-major) [QF_COMBINE_WIDE; default 1] */
    QF_OPT_COMBINE_XCD,          /* 1: the pass-major payload pass item-major: the passes of one
                                    generation's lane-chunk run together on one XCD, so the later
                                    passes read the syndrome rows from its L2 instead of HBM; 0: pass
                                    p's workgroups after pass p - 1's [QF_COMBINE_XCD; default 0:
                                    where the last pass is short it runs ahead of the others and the
                                    reuse is lost, 5 % slower at e = 39 / 59, DESIGN 3.7] */
    QF_OPT_COMBINE_JUMP,         /* 1: the bit-sliced payload pass multiplies by a runtime coefficient c
                                    with a call into c's code block (8 destination-indexed 3-input
                                    XORs); 0: M0-indexed XORs, one index write per XOR
                                    [QF_COMBINE_JUMP; default 1] */
    QF_OPT_COMBINE_PM24,         /* 1: with QF_COMBINE_JUMP, a payload pass of 49-64 outputs (e_max) runs
                                    as 3 24-output passes in one launch instead of 4 16-output ones
                                    (the syndrome rows read and transposed once less);
                                    0: 16-output passes [QF_COMBINE_PM24; default 1] */
    QF_OPT_SLIDING_KERNELS,      /* 1: an encode batch whose generations overlap (generation stride
                                    below k row strides: sliding windows) runs the shape's sliding-window
                                    kernel where one is built (cached row loads; (48, 8) as the hybrid
                                    FFT pass); 0: the block kernels [QF_SLIDING_KERNELS; default 1] */
    QF_OPT_COUNT
};
int qf_ctx_set_option(qf_ctx *ctx, int option, int64_t value);
int qf_ctx_get_option(qf_ctx *ctx, int option, int64_t *value);

/* Kernel timing (no reference counterpart; benches/ replacement).  While on,
 * every kernel the context launches is bracketed by HIP events recorded on
 * the stream it runs on; totals accumulate per kernel name.  on != 0 clears
 * the totals and starts, on == 0 stops.  qf_ctx_profile_read synchronises
 * the pending events and returns the i-th kernel (first-launch order):
 * name (owned by ctx), number of launches, summed duration in ms;
 * QF_EINVAL once i >= number of kernels seen. */
int qf_ctx_profile(qf_ctx *ctx, int on);
int qf_ctx_profile_read(qf_ctx *ctx, uint32_t i, const char **name, uint32_t *launches,
                        double *total_ms);

/* ---------------------------------------------------------------------------
 * Element-wise slice multiply on the device.
 * replaces gf_tables.rs:255-274 gf_mul_slice (benches/gf_mul_slice_bench.rs)
 * out[i] = a[i] * b[i] for i < n (device pointers).
 * ------------------------------------------------------------------------- */
int qf_gf256_mul_slice_dev(qf_ctx *ctx, const uint8_t *a_dev, const uint8_t *b_dev,
                           uint8_t *out_dev, size_t n);

/* ---------------------------------------------------------------------------
 * Batched block encode (device resident).
 * replaces decoder.rs:172-275 Encoder::generate_repair_packet, for r repairs
 * of G independent generations in one launch:
 *   rep[g][j][t] = XOR_{i<k} C[j][i] * src[g][i][t]      (t < L, j < r)
 * Row i of generation g starts at src_dev + g*src_gen_stride + i*src_row_stride;
 * repair j at rep_dev + g*rep_gen_stride + j*rep_row_stride.  Exactly L bytes
 * per repair row are written (plus the zero tail with QF_ENCODE_ZERO_TAIL).  coeff_rxk (host, r*k bytes, row-major) or NULL
 * for the reference's Cauchy matrix (decoder.rs:280-298).
 * Sliding windows (adaptive.rs:519-562, one window per source packet) are the
 * special case src_gen_stride == src_row_stride.
 * Fast path: src/rep pointers and strides 16-byte aligned (any L).
 * ------------------------------------------------------------------------- */
/* qf_encode_shape.flags: the caller lets the library write zeros to bytes
 * [L, round_up(L, 128)) of every repair row when rep_row_stride covers them
 * (the reference's repair is a pool block that is zero beyond L,
 * decoder.rs:182/264 + optimize.rs:524).  With 128-B aligned repair rows this
 * lets the encode kernel store whole 128-B lines only.  When
 * L % 16 != 0 the kernel then also reads each source row's last 16-byte unit
 * whole (up to round_up(L, 16): inside the 16-byte row stride, and for the
 * buffer's last row within the same page); those extra bytes never reach the
 * output. */
#define QF_ENCODE_ZERO_TAIL 1u

typedef struct qf_encode_shape {
    uint32_t k;              /* generation (window) size, 1..255 */
    uint32_t r;              /* repairs per generation, k + r <= 256 for Cauchy */
    uint32_t L;              /* payload bytes per packet */
    uint32_t flags;          /* QF_ENCODE_* bits; 0: exactly L bytes per repair row */
    uint64_t src_row_stride;
    uint64_t src_gen_stride;
    uint64_t rep_row_stride;
    uint64_t rep_gen_stride;
} qf_encode_shape;

int qf_encode_batch(qf_ctx *ctx, const qf_encode_shape *shape, uint32_t G,
                    const uint8_t *src_dev, uint8_t *rep_dev, const uint8_t *coeff_rxk);

/* Same, host-resident src/rep (pinned memory recommended).  Chunks of
 * generations are streamed H2D -> encode -> D2H on several HIP streams with
 * device staging owned by the context.  Synchronous on return. */
int qf_encode_batch_host(qf_ctx *ctx, const qf_encode_shape *shape, uint32_t G,
                         const uint8_t *src_host, uint8_t *rep_host,
                         const uint8_t *coeff_rxk);

/* ---------------------------------------------------------------------------
 * Batched decode (device resident).
 * replaces decoder.rs:658-791 Decoder::{add_packet, try_decode,
 * gaussian_elimination, get_decoded_packets} for G independent generations:
 *  - rows: the received packets of generation g in arrival order,
 *    rows_dev + g*rows_gen_stride + slot*row_stride, slot < n_rows[g]
 *  - row_index_dev[g*max_rows + slot]: < k = systematic source index
 *    (the reference's id % k, decoder.rs:684); >= k = repair j = value - k
 *  - row_coeffs_dev: NULL (repair coefficients are the Cauchy row of j) or
 *    k coefficient bytes per slot at row_coeffs_dev + (g*max_rows + slot)*k
 *    (the packet's coefficient block, decoder.rs:694-696)
 *  - n_rows_dev: per-generation slot count, or NULL (= max_rows)
 * Acceptance follows decoder.rs:678-701: the first k rows win, duplicate
 * systematic rows are ignored (rows that may be linearly dependent, as
 * recoded traffic is: qf_decode_innovative_batch below).  For each generation
 * the erased source rows are recovered (ascending source index) into
 *   rec_dev + g*rec_gen_stride + m*rec_row_stride,  m < n_rec[g] <= min(k, r)
 * with rec_index_dev[g*min(k,r) + m] = source index of recovered row m and
 * status_dev[g] = QF_OK / QF_ENOTREADY / QF_ERANK / QF_ERANGE / QF_EINVAL.
 * Received systematic rows are not copied (they are already the payload).
 * Deviation from the reference: systematic rows carry their
 * payloads, so the recovered bytes are the original bytes.
 * ------------------------------------------------------------------------- */
typedef struct qf_decode_shape {
    uint32_t k;
    uint32_t r;              /* max repairs that may arrive (bounds n_rec) */
    uint32_t L;
    uint32_t max_rows;       /* slots per generation in row_index / rows   */
    uint64_t row_stride;
    uint64_t rows_gen_stride;
    uint64_t rec_row_stride;
    uint64_t rec_gen_stride;
} qf_decode_shape;

int qf_decode_batch(qf_ctx *ctx, const qf_decode_shape *shape, uint32_t G,
                    const uint8_t *rows_dev, const uint16_t *row_index_dev,
                    const uint32_t *n_rows_dev, const uint8_t *row_coeffs_dev,
                    uint8_t *rec_dev, uint16_t *rec_index_dev, uint32_t *n_rec_dev,
                    int32_t *status_dev);

/* Same, every buffer host-resident (pinned memory recommended): the receive
 * side starting from datagrams in host memory (core.rs:203-232).  Chunks of
 * about 64 MiB of rows are streamed H2D -> decode -> D2H on several HIP
 * streams; each chunk's acceptance pass starts once its indices have landed
 * and its payload pass once its rows have (qf_ctx_set_payload_wait).
 * Generation g's rows must lie in [g*rows_gen_stride, (g+1)*rows_gen_stride);
 * recovered rows must be dense per generation (rec_gen_stride ==
 * min(k, r) * rec_row_stride).  Bytes [0, L) of recovered rows
 * n_rec[g] .. min(k, r) - 1 of a generation are unspecified on return (the
 * device path leaves them untouched).  Synchronous on return. */
int qf_decode_batch_host(qf_ctx *ctx, const qf_decode_shape *shape, uint32_t G,
                         const uint8_t *rows_host, const uint16_t *row_index_host,
                         const uint32_t *n_rows_host, const uint8_t *row_coeffs_host,
                         uint8_t *rec_host, uint16_t *rec_index_host, uint32_t *n_rec_host,
                         int32_t *status_host);

/* ---------------------------------------------------------------------------
 * Batched recoding (relay).
 * No reference counterpart: the reference's nodes either hold all k sources
 * (Encoder) or decode (Decoder); a relay that holds a mix of systematic and
 * coded rows of a generation can only forward them.  Recoding emits m fresh
 * linear combinations of the n rows a relay holds, each with its coefficient
 * vector over the k sources, without decoding.  A receiver needs no change:
 * a recoded row enters qf_decode_batch as a row with any index >= k plus its
 * vector in row_coeffs_dev, qf_decoder_add_packet as a repair packet, and
 * qf_packet_to_raw as a repair frame (the reference's Decoder takes any
 * coefficient vector, decoder.rs:694-696).
 *
 * For generation g, n = n_rows_dev[g] (NULL: max_rows).  rows_dev,
 * row_index_dev, n_rows_dev and row_coeffs_dev are laid out as for
 * qf_decode_batch; all n rows are mixed (no acceptance filtering, duplicates
 * are legal).  The vector v(s) of slot s over the k sources:
 *   index < k                       unit vector of that index (row_coeffs not read)
 *   index >= k, row_coeffs_dev      the k bytes at (g*max_rows + s)*k
 *   index >= k, no row_coeffs_dev   Cauchy row index - k of (k, r); needs index - k < r
 * Mix matrix M (m x n): M[j][s] = mix_dev[(g*m + j)*max_rows + s], or with
 * mix_dev == NULL byte t = (g*m + j)*max_rows + s of what
 * qf_fill_splitmix_dev(dst, G*m*max_rows, seed, 0) writes (zero bytes kept).
 * Outputs, j < m:
 *   out[g][j][t]        = XOR_s M[j][s] * rows[g][s][t], t < L, at
 *                         out_dev + g*out_gen_stride + j*out_row_stride
 *                         (exactly L bytes per row are written)
 *   out_coeffs[g][j][i] = XOR_s M[j][s] * v(s)[i], i < k, at
 *                         out_coeffs_dev + (g*m + j)*k
 * status_dev[g]: QF_OK; QF_ENOTREADY when n == 0; QF_EINVAL when n > max_rows
 * or a row with index >= k has no coefficient vector.  In the non-OK cases
 * the generation's m rows (L bytes each) and m vectors are written as zeros;
 * other generations are unaffected.
 * Returns QF_EINVAL for a bad shape (k, m, max_rows or L out of range, flags
 * != 0, a row stride shorter than L, a NULL required pointer, pointers or
 * strides not 16-byte aligned) and QF_ERANGE for k + r > 256.
 * The payload runs ceil(m / 16) passes of the decode's payload kernel; each
 * pass reads every input row once.
 * ------------------------------------------------------------------------- */
typedef struct qf_recode_shape {
    uint32_t k;              /* generation size, 1..255 */
    uint32_t r;              /* Cauchy repairs that may appear among the inputs when
                                row_coeffs_dev is NULL (k + r <= 256); 0 = none */
    uint32_t L;              /* payload bytes per row, >= 1 */
    uint32_t max_rows;       /* input slots per generation, 1..255 */
    uint32_t m;              /* recoded packets per generation, 1..64 */
    uint32_t flags;          /* 0 */
    uint64_t row_stride;     /* inputs, as qf_decode_shape */
    uint64_t rows_gen_stride;
    uint64_t out_row_stride;
    uint64_t out_gen_stride;
} qf_recode_shape;

int qf_recode_batch(qf_ctx *ctx, const qf_recode_shape *shape, uint32_t G,
                    const uint8_t *rows_dev, const uint16_t *row_index_dev,
                    const uint32_t *n_rows_dev, const uint8_t *row_coeffs_dev,
                    const uint8_t *mix_dev, uint64_t seed,
                    uint8_t *out_dev, uint8_t *out_coeffs_dev, int32_t *status_dev);

/* ---------------------------------------------------------------------------
 * Recoding from rows that lie where they were received (relay, in place).
 * No reference counterpart.  qf_recode_batch with r = 0 over rows given as
 * (where, how long) instead of a strided array:
 *   rows[g][c] = the row_len_dev[g*max_rows + c] bytes at
 *                src_dev + g*src_gen_stride + row_off_dev[g*max_rows + c],
 *                zero padded to L
 * which is what qf_parse_frame_headers_dev leaves of a batch of received
 * frames (src_dev = frames_dev, src_gen_stride = max_rows * frame_stride).
 * row_index_dev, n_rows_dev (NULL: max_rows), row_coeffs_dev (required here),
 * mix_dev / seed (the splitmix stream indexed by the compacted slot), out_dev,
 * out_coeffs_dev, the QF_ENOTREADY / QF_EINVAL cases of status_dev and the
 * all-zero outputs of a generation that is not QF_OK are those of
 * qf_recode_batch, and the outputs are byte for byte what qf_recode_batch
 * writes for the rows defined above.
 * Further QF_EINVAL cases of status_dev[g] (zero outputs): one of the
 * generation's n rows has row_len > L, row_off % 16 != 0 or row_off + row_len
 * > src_gen_stride.  row_len == 0 is legal: the row contributes its vector
 * only.
 * out_len_dev (nullable), one u32 per output slot at g*m + j: the largest
 * row_len among the generation's n rows, 0 for a generation that is not
 * QF_OK -- the row_len_dev of qf_frame_rows_dev for the recoded rows.
 * Reads: only aligned 16-byte units of a source row that hold at least one of
 * its bytes; with the offsets and src_gen_stride multiples of 16 they lie
 * inside the generation's region.  Writes: exactly L bytes per output row.
 * src_dev is never written and must not overlap out_dev.
 * Returns QF_EINVAL for k or max_rows outside 1..255, m outside 1..64, L == 0,
 * flags or reserved != 0, out_row_stride < L, a NULL required pointer
 * (src_dev, row_off_dev, row_len_dev, row_index_dev, row_coeffs_dev, out_dev,
 * out_coeffs_dev, status_dev), src_dev, out_dev or a stride not 16-byte
 * aligned.  G == 0 is QF_OK.
 * The payload runs ceil(m / 16) passes of k_combine_rows_at, whatever the row
 * length (the generated bit-sliced payload kernels are not used); each pass
 * reads every input row once.
 * ------------------------------------------------------------------------- */
typedef struct qf_recode_frames_shape {
    uint32_t k;              /* generation size, 1..255 */
    uint32_t L;              /* payload bytes per output row, >= every row_len, >= 1 */
    uint32_t max_rows;       /* input slots per generation, 1..255 */
    uint32_t m;              /* recoded packets per generation, 1..64 */
    uint32_t flags;          /* 0 */
    uint32_t reserved;       /* 0 */
    uint64_t src_gen_stride; /* bytes of one generation's source region, % 16 == 0 */
    uint64_t out_row_stride;
    uint64_t out_gen_stride;
} qf_recode_frames_shape;

int qf_recode_frames_dev(qf_ctx *ctx, const qf_recode_frames_shape *shape, uint32_t G,
                         const uint8_t *src_dev, const uint32_t *row_off_dev,
                         const uint32_t *row_len_dev, const uint16_t *row_index_dev,
                         const uint32_t *n_rows_dev, const uint8_t *row_coeffs_dev,
                         const uint8_t *mix_dev, uint64_t seed,
                         uint8_t *out_dev, uint8_t *out_coeffs_dev, uint32_t *out_len_dev,
                         int32_t *status_dev);

/* ---------------------------------------------------------------------------
 * Rank-aware receive side for recoded traffic (opt-in extension).
 * No reference counterpart: the reference's Cauchy code makes any k distinct
 * rows independent, so its decoder takes the first k rows (decoder.rs:678-701)
 * and so does qf_decode_batch.  Recoded traffic (qf_recode_batch) carries
 * dependent rows as a matter of course; these calls apply the RLNC receive
 * rule instead: a row is accepted iff it is innovative.
 *
 * For generation g the slots s = 0 .. n-1 are taken in arrival order, with
 * n = min(n_rows_dev[g], max_rows) (NULL: max_rows) and the layouts of
 * qf_decode_batch.  The vector v(s) over the k sources is that of
 * qf_recode_batch:
 *   index < k                       unit vector of that index
 *   index >= k, row_coeffs_dev      the k bytes at (g*max_rows + s)*k; needs index - k < 256
 *   index >= k, no row_coeffs_dev   Cauchy row index - k of (k, r); needs index - k < r
 * A slot that breaks its "needs" gives the generation QF_EINVAL.  Slot s is
 * innovative iff v(s) is not in the GF(2^8) span of v(0) .. v(s-1): a zero
 * vector, a repeated systematic or Cauchy index, and every row after the rank
 * has reached k are not.  rank[g] = number of innovative slots.
 *
 * qf_rank_batch (control only, no payload):
 *   innovative_dev[g*max_rows + s] = 1 / 0 (0 for s >= n); may be NULL
 *   rank_dev[g]                    = rank of generation g
 *   status_dev[g]                  = QF_OK, or QF_EINVAL (rank and flags 0)
 * Returns QF_EINVAL for k outside 1..256, max_rows outside 1..4096, flags != 0
 * or a NULL required pointer, and QF_ERANGE for NULL row_coeffs_dev with r > 0
 * and k + r > 256.
 * ------------------------------------------------------------------------- */
typedef struct qf_rank_shape {
    uint32_t k;              /* generation size, 1..256 */
    uint32_t r;              /* Cauchy repairs that may appear when row_coeffs_dev is NULL */
    uint32_t max_rows;       /* slots per generation, 1..4096 */
    uint32_t flags;          /* 0 */
} qf_rank_shape;

int qf_rank_batch(qf_ctx *ctx, const qf_rank_shape *shape, uint32_t G,
                  const uint16_t *row_index_dev, const uint32_t *n_rows_dev,
                  const uint8_t *row_coeffs_dev, uint8_t *innovative_dev,
                  uint32_t *rank_dev, int32_t *status_dev);

/* qf_decode_batch over the innovative slots only: generation g's rec,
 * rec_index, n_rec and status are exactly what qf_decode_batch writes for the
 * same generation with the non-innovative slots removed and the order kept.
 * The accepted rows are independent, so QF_ERANK is never reported; rank < k
 * gives QF_ENOTREADY with n_rec = 0.  An erased source is one without an
 * accepted systematic row, which includes a systematic row dropped because
 * earlier coded rows already span it; more than min(k, r) of them is
 * QF_EINVAL.  The payload of a non-innovative slot reaches no output.
 * rank_dev and innovative_dev (both nullable) receive what qf_rank_batch
 * writes (the rank is reported for QF_ENOTREADY generations as well).
 * Shape limits, alignment rules and error returns are those of
 * qf_decode_batch's general path (k <= 256, min(k, r) <= 128, max_rows <=
 * 4096, 16-byte alignment), plus QF_ERANGE for NULL row_coeffs_dev with r > 0
 * and k + r > 256.  The call always runs that general path (the acceptance
 * kernel k_rank_filter, k_decode_prepare and the payload pass), also with
 * NULL row_coeffs_dev: pure Cauchy traffic keeps using qf_decode_batch and
 * its fused kernels.  It does not honour qf_ctx_set_payload_stream /
 * qf_ctx_set_payload_wait; it clears them, as the _host and _desc calls do. */
int qf_decode_innovative_batch(qf_ctx *ctx, const qf_decode_shape *shape, uint32_t G,
                               const uint8_t *rows_dev, const uint16_t *row_index_dev,
                               const uint32_t *n_rows_dev, const uint8_t *row_coeffs_dev,
                               uint8_t *rec_dev, uint16_t *rec_index_dev, uint32_t *n_rec_dev,
                               int32_t *status_dev, uint32_t *rank_dev, uint8_t *innovative_dev);

/* ---------------------------------------------------------------------------
 * The same decode from rows that lie where they were received (receiver, in
 * place).  No reference counterpart.  qf_decode_innovative_batch over rows
 * given as in qf_recode_frames_dev:
 *   rows[g][c] = the row_len_dev[g*max_rows + c] bytes at
 *                src_dev + g*src_gen_stride + row_off_dev[g*max_rows + c],
 *                zero padded to L
 * which is what qf_parse_frame_headers_dev leaves (src_dev = frames_dev,
 * src_gen_stride = max_rows * frame_stride).  rec_dev, rec_index_dev,
 * n_rec_dev, status_dev, rank_dev (nullable) and innovative_dev (nullable) are
 * byte for byte what qf_decode_innovative_batch writes for those rows with the
 * same k, r, max_rows, row_index_dev, n_rows_dev (NULL: max_rows) and
 * row_coeffs_dev (required here, as in qf_recode_frames_dev).
 * Writes: exactly L bytes per recovered row; rows n_rec[g] and above of a
 * generation, and all rows of a generation that is not QF_OK, are not written
 * (the device decode's rule; the recoder writes zeros instead).
 * Further QF_EINVAL cases of status_dev[g]: one of the generation's n rows has
 * row_len > L, row_off % 16 != 0 or row_off + row_len > src_gen_stride.  Such
 * a generation has n_rec 0 and no byte of rec_dev written; rank_dev and
 * innovative_dev still hold what qf_rank_batch writes (they depend on the
 * vectors only).  row_len == 0 is legal.
 * src_slot_dev (nullable), one u16 per source at g*k + i: for a QF_OK
 * generation the slot c of the accepted systematic row of source i (the packet
 * is the row_len_dev[g*max_rows + c] bytes at row_off_dev[g*max_rows + c]), or
 * 0xFFFF when source i was recovered (the packet is then row m of rec_dev with
 * rec_index_dev[m] == i); all k entries 0xFFFF for a generation that is not
 * QF_OK.  With it the k packets of a generation are found without a host scan.
 * Reads: only aligned 16-byte units of an accepted (innovative) row that hold
 * at least one of its bytes; the payload of a non-innovative slot is never
 * read (qf_decode_innovative_batch reads it and multiplies it by zero).
 * src_dev is never written and must not overlap rec_dev.
 * Returns QF_EINVAL for k outside 1..256, max_rows outside 1..1024, min(k, r) >
 * 128, L == 0, flags or reserved != 0, rec_row_stride < L, a NULL required
 * pointer (src_dev, row_off_dev, row_len_dev, row_index_dev, row_coeffs_dev,
 * n_rec_dev, status_dev, and rec_dev / rec_index_dev when min(k, r) > 0),
 * src_dev, rec_dev or a stride not 16-byte aligned, or a shape whose control
 * kernel would need more than 160 KB of LDS.  G == 0 is QF_OK.  The call
 * clears qf_ctx_set_payload_stream / qf_ctx_set_payload_wait, as
 * qf_decode_innovative_batch does.
 * The payload runs ceil(min(k, r) / 16) passes of k_combine_rows_at, whatever
 * the row length (the generated bit-sliced payload kernels are not used); a
 * pass in which no generation has a row to write costs a launch and no row
 * read.  Which sequence: for rows under 2,017 bytes use this one (with
 * qf_parse_frame_headers_dev 0.66 of the copy sequence's time at k = 64, L =
 * 1,200, 13 recovered rows; 0.92 with 64 recovered).  From 2,017 bytes on,
 * qf_decode_innovative_batch runs the bit-sliced payload kernel and
 * qf_parse_frames_coded_dev + qf_decode_innovative_batch is the faster
 * sequence (this one takes 1.14 of its time at (196, 59), L = 9,000;
 * DESIGN.md 3.13).
 * ------------------------------------------------------------------------- */
typedef struct qf_decode_frames_shape {
    uint32_t k;              /* generation size, 1..256 */
    uint32_t r;              /* bounds the recovered rows: up to min(k, r) <= 128 per generation */
    uint32_t L;              /* payload bytes per recovered row, >= every row_len, >= 1 */
    uint32_t max_rows;       /* input slots per generation, 1..1024 */
    uint32_t flags;          /* 0 */
    uint32_t reserved;       /* 0 */
    uint64_t src_gen_stride; /* bytes of one generation's source region, % 16 == 0 */
    uint64_t rec_row_stride;
    uint64_t rec_gen_stride;
} qf_decode_frames_shape;

int qf_decode_frames_dev(qf_ctx *ctx, const qf_decode_frames_shape *shape, uint32_t G,
                         const uint8_t *src_dev, const uint32_t *row_off_dev,
                         const uint32_t *row_len_dev, const uint16_t *row_index_dev,
                         const uint32_t *n_rows_dev, const uint8_t *row_coeffs_dev,
                         uint8_t *rec_dev, uint16_t *rec_index_dev, uint32_t *n_rec_dev,
                         int32_t *status_dev, uint32_t *rank_dev, uint8_t *innovative_dev,
                         uint16_t *src_slot_dev);

/* ---------------------------------------------------------------------------
 * Streaming receive: generations that fill over many calls.  No reference
 * counterpart.  The calls above start from an empty span and need all rows of
 * a generation in one call; a receiver or relay that polls gets a few rows of
 * many generations at a time.  Two pieces carry a generation from one poll to
 * the next: a rank state that qf_rank_update_batch resumes from and writes
 * back, and a row store that qf_store_append_dev fills with the rows the
 * state took.
 *
 * Rank state.  Generation g's state is the qf_rank_state_bytes(k) bytes at
 * state_dev + g * qf_rank_state_bytes(k); the buffer is the caller's and is
 * 16-byte aligned.  All-zero bytes mean "nothing received": a generation is
 * reset by zeroing its state (a memset; no library call).  The contents are
 * private, only the size is part of the ABI.  Two calls that touch the same
 * generation's state must be ordered: the same context, or a stream
 * dependency between their contexts.
 * ------------------------------------------------------------------------- */
/* No reference counterpart.  Bytes of one generation's rank state: a multiple
 * of 16, 0 for k outside 1..256.  Host only, no device. */
size_t qf_rank_state_bytes(uint32_t k);

/* No reference counterpart.  qf_rank_batch that resumes from state_dev:
 * row_index_dev, n_rows_dev, row_coeffs_dev, innovative_dev, the vectors v(s),
 * the index validity rules and the call-level errors are those of
 * qf_rank_batch (state_dev is a required pointer and must be 16-byte aligned:
 * QF_EINVAL).  Slot s of this call is innovative iff v(s) is not in the span
 * of (the span the state holds) and v(0) .. v(s-1) of this call; rank_dev[g]
 * is the rank afterwards, and the state afterwards holds the enlarged span.
 * So the flags of every QF_OK update since the state was zero, concatenated in
 * call order, and the last rank are what qf_rank_batch and qf_gf256_rank give
 * for the concatenated slots in one call.  Calls on one state may differ in
 * max_rows, in r and in whether row_coeffs_dev is given; k is recorded in the
 * state.
 * status_dev[g]: QF_OK; QF_EINVAL for a slot that breaks its "needs" -- the
 * call's slots of that generation are then ignored as a whole: flags 0, the
 * state byte for byte unchanged, rank_dev[g] the rank the state held; QF_EINVAL
 * also for a state that is neither zero nor a valid state for this k (flags 0,
 * rank 0, the state untouched).  Validity is decided from the state's 16-byte
 * header (zero, or the tag, this k and counts within 0..k) and a range check
 * of the stored pivot columns and unit-column map before any of them is used.
 * A generation with no slot in the call (n = 0) costs a read of that header:
 * its flags are zeroed, rank_dev / status_dev are written, the state is not.
 * The state is written only when the rank grew. */
int qf_rank_update_batch(qf_ctx *ctx, const qf_rank_shape *shape, uint32_t G,
                         const uint16_t *row_index_dev, const uint32_t *n_rows_dev,
                         const uint8_t *row_coeffs_dev, uint8_t *state_dev,
                         uint8_t *innovative_dev, uint32_t *rank_dev, int32_t *status_dev);

/* No reference counterpart.  Appends rows to a per-generation row store.  The
 * inputs are what qf_parse_frame_headers_dev leaves: rows[g][s] = the
 * row_len_dev[g*max_rows + s] bytes at src_dev + g*src_gen_stride +
 * row_off_dev[g*max_rows + s], with row_index_dev, n_rows_dev (NULL: max_rows)
 * and row_coeffs_dev (required).  take_dev (nullable): one byte per input slot
 * at g*max_rows + s, nonzero = take the row; NULL takes every row.  It is the
 * innovative_dev of qf_rank_update_batch.
 * The taken rows of generation g are appended in arrival order at store slots
 * c = store_n_dev[g], store_n_dev[g] + 1, ..:
 *   payload      to store_dev + g*store_gen_stride + c*store_row_stride:
 *                round_up(row_len, 16) bytes, those after row_len zero
 *   store_off_dev[g*cap + c]    = c * store_row_stride
 *   store_len_dev[g*cap + c], store_index_dev[g*cap + c] and the k bytes of
 *   store_coeffs_dev at (g*cap + c)*k  copied from the row
 * and store_n_dev[g] grows by the number of taken rows (the caller zeroes it
 * when it resets the generation).
 * The five store arrays with max_rows = cap and src_gen_stride =
 * store_gen_stride are the inputs of qf_decode_frames_dev (any cap in
 * 1..1024), and of qf_recode_frames_dev when cap <= 255, that call's max_rows
 * limit: a store with cap = 256 can be decoded but not recoded.
 * status_dev[g]: QF_OK; QF_EINVAL when n_rows_dev[g] > max_rows or a taken row
 * has row_len > L, row_off % 16 != 0 or row_off + row_len > src_gen_stride
 * (checked first); QF_ETOOSMALL when store_n_dev[g] + taken rows > cap.  A
 * generation that is not QF_OK appends nothing: no store byte, no metadata
 * entry and no count changes.  After such a failure the generation's rank
 * state (which took the rows) and its store disagree, and the caller resets
 * both.  With the outputs of qf_parse_frame_headers_dev and cap >= k it cannot
 * happen.
 * Reads: only aligned 16-byte units of a taken row that hold one of its bytes;
 * the payload of a row that is not taken is never read.  Writes: nothing
 * outside the appended rows' round_up(row_len, 16) bytes and their metadata
 * entries; slots below the old count and at or above the new one are
 * untouched.  src_dev must not overlap store_dev.
 * Returns QF_EINVAL for k outside 1..256, L == 0, max_rows or cap outside
 * 1..1024, flags or reserved != 0, a stride not a multiple of 16,
 * store_row_stride < round_up(L, 16), store_gen_stride < cap *
 * store_row_stride, cap * store_row_stride > 2^32 (the offsets are u32), a
 * NULL required pointer (all but n_rows_dev and take_dev), src_dev or
 * store_dev not 16-byte aligned.  G == 0 is QF_OK.
 * Two kernels: k_store_prepare (one wave per generation: checks, slots,
 * metadata, vectors) and k_store_rows (one lane per 16-byte unit). */
typedef struct qf_store_shape {
    uint32_t k;                /* generation size, 1..256 */
    uint32_t L;                /* payload bytes per row at most, >= 1 */
    uint32_t max_rows;         /* input slots per generation, 1..1024 */
    uint32_t cap;              /* store slots per generation, 1..1024 (k is enough when take = innovative) */
    uint32_t flags;            /* 0 */
    uint32_t reserved;         /* 0 */
    uint64_t src_gen_stride;   /* bytes of one generation's source region, % 16 == 0 */
    uint64_t store_row_stride; /* % 16 == 0, >= round_up(L, 16) */
    uint64_t store_gen_stride; /* % 16 == 0, >= cap * store_row_stride */
} qf_store_shape;

int qf_store_append_dev(qf_ctx *ctx, const qf_store_shape *shape, uint32_t G,
                        const uint8_t *src_dev, const uint32_t *row_off_dev,
                        const uint32_t *row_len_dev, const uint16_t *row_index_dev,
                        const uint32_t *n_rows_dev, const uint8_t *row_coeffs_dev,
                        const uint8_t *take_dev, uint8_t *store_dev, uint32_t *store_off_dev,
                        uint32_t *store_len_dev, uint16_t *store_index_dev,
                        uint8_t *store_coeffs_dev, uint32_t *store_n_dev, int32_t *status_dev);

/* ---------------------------------------------------------------------------
 * Streaming receive over a list of generations.  No reference counterpart.
 * A poll touches few of a receiver's generations, and so should the step
 * after it: qf_gen_select_dev builds a list of generations on the device,
 * qf_decode_frames_sel_dev / qf_recode_frames_sel_dev run the store-side calls
 * over the listed generations only, and qf_stream_reset_dev resets them.  No
 * step needs the host to look at a device value.
 * ------------------------------------------------------------------------- */
/* No reference counterpart.  Generation g of 0..G-1 matches iff rank_dev[g] >=
 * min_rank and (seen_dev == NULL or rank_dev[g] > seen_dev[g]).  The first
 * min(matches, n_max) matching generations are written to sel_dev[0..] in
 * ascending order of g, *n_sel_dev is that number and *n_match_dev (nullable)
 * the number of all matches; sel_dev entries at and above *n_sel_dev are not
 * written.  flags: 0 or QF_SELECT_MARK, which needs seen_dev and sets
 * seen_dev[g] = rank_dev[g] for the selected generations only (a match beyond
 * n_max is not marked, so it turns up in the next call); without it seen_dev
 * is only read.  Receiver: min_rank = k and seen zeroed at reset list a
 * generation once, in the poll in which it completes.  Relay: min_rank = 1
 * lists a generation in every poll in which its rank grew.
 * The list is deterministic (it does not depend on the order in which
 * workgroups run).  Two launches (k_gen_select_count, k_gen_select_scatter), no
 * workgroup waits for another.
 * Returns QF_EINVAL for unknown flag bits, QF_SELECT_MARK without seen_dev,
 * n_max == 0, G > 2^24, or a NULL required pointer (rank_dev when G > 0,
 * sel_dev, n_sel_dev).  G == 0 writes *n_sel_dev = 0 (and *n_match_dev) and is
 * QF_OK. */
#define QF_SELECT_MARK 1u
int qf_gen_select_dev(qf_ctx *ctx, uint32_t G, const uint32_t *rank_dev, uint32_t *seen_dev,
                      uint32_t min_rank, uint32_t flags, uint32_t n_max,
                      uint32_t *sel_dev, uint32_t *n_sel_dev, uint32_t *n_match_dev);

/* A list of generations of source arrays that hold G_src of them.  Let
 * n = min(*n_sel_dev, n_max) (n_sel_dev NULL: n_max).  Entries j < n are
 * listed; one with sel_dev[j] >= G_src is invalid; entries n..n_max-1 are
 * unused and their sel_dev values are never looked at.  Duplicates are legal
 * and the list need not be sorted. */
typedef struct qf_gen_sel {
    const uint32_t *sel_dev;    /* n_max entries, generation numbers of the source arrays */
    const uint32_t *n_sel_dev;  /* device count; nullable = n_max */
    uint32_t n_max;             /* entries the call is sized for, >= 1 */
    uint32_t G_src;             /* generations in the source arrays; an entry >= G_src is invalid */
} qf_gen_sel;

/* No reference counterpart.  qf_decode_frames_dev over a list.  The inputs
 * (src_dev, row_off_dev, row_len_dev, row_index_dev, n_rows_dev, row_coeffs_dev,
 * strides as in the shape) are the source arrays of sel->G_src generations and
 * are indexed by the generation number sel_dev[j].  Every output is compact,
 * indexed by the list position j in 0..n_max-1, and sized for n_max
 * generations: rec_dev, rec_index_dev, n_rec_dev, status_dev, rank_dev,
 * innovative_dev, src_slot_dev.
 * A listed entry j with sel_dev[j] < G_src is written byte for byte as
 * qf_decode_frames_dev writes generation j of a batch of n_max generations
 * whose generation j has the metadata of source generation sel_dev[j] and a
 * copy of its region.  An invalid entry gets status QF_EINVAL, n_rec 0, rank 0,
 * no flags and src_slot 0xFFFF, and nothing is read through it.  An unused
 * entry gets exactly what qf_decode_frames_dev writes for a generation with
 * n_rows_dev[g] = 0.
 * Reads: no payload byte of a generation that is not listed; within a listed
 * one the read rules of qf_decode_frames_dev.  The sources are only read.
 * Returns what qf_decode_frames_dev returns with n_max in the place of G, and
 * QF_EINVAL for a NULL sel or sel_dev, n_max == 0 or G_src == 0.
 * k_sel_gather (one wave per entry) copies the listed generations' metadata
 * and vectors into compact arrays in the context workspace, the control
 * kernels of qf_decode_frames_dev run over those, and k_combine_rows_at reads
 * each entry's rows from the region of its source generation. */
int qf_decode_frames_sel_dev(qf_ctx *ctx, const qf_decode_frames_shape *shape, const qf_gen_sel *sel,
                             const uint8_t *src_dev, const uint32_t *row_off_dev,
                             const uint32_t *row_len_dev, const uint16_t *row_index_dev,
                             const uint32_t *n_rows_dev, const uint8_t *row_coeffs_dev,
                             uint8_t *rec_dev, uint16_t *rec_index_dev, uint32_t *n_rec_dev,
                             int32_t *status_dev, uint32_t *rank_dev, uint8_t *innovative_dev,
                             uint16_t *src_slot_dev);

/* No reference counterpart.  qf_recode_frames_dev over a list, inputs and
 * compact outputs (out_dev, out_coeffs_dev, out_len_dev, status_dev) as in
 * qf_decode_frames_sel_dev; mix_dev, or the splitmix stream of seed, is indexed
 * by the list position j as well.  A listed entry with sel_dev[j] < G_src is
 * written byte for byte as qf_recode_frames_dev writes generation j of the
 * batch the list stands for.  An invalid entry is QF_EINVAL with zero rows,
 * zero vectors and out_len 0, as that call's other QF_EINVAL generations, and
 * nothing is read through it.  An unused entry gets status QF_ENOTREADY,
 * out_len 0 and zero out_coeffs, but its m payload rows are NOT written (the
 * dense call writes zero rows there): a caller that sizes n_max generously
 * does not pay n_max * m * L bytes of stores.
 * Returns what qf_recode_frames_dev returns with n_max in the place of G, and
 * QF_EINVAL for a NULL sel or sel_dev, n_max == 0 or G_src == 0. */
int qf_recode_frames_sel_dev(qf_ctx *ctx, const qf_recode_frames_shape *shape, const qf_gen_sel *sel,
                             const uint8_t *src_dev, const uint32_t *row_off_dev,
                             const uint32_t *row_len_dev, const uint16_t *row_index_dev,
                             const uint32_t *n_rows_dev, const uint8_t *row_coeffs_dev,
                             const uint8_t *mix_dev, uint64_t seed,
                             uint8_t *out_dev, uint8_t *out_coeffs_dev, uint32_t *out_len_dev,
                             int32_t *status_dev);

/* No reference counterpart.  Resets the listed generations: for every listed
 * entry with sel_dev[j] < G_src the qf_rank_state_bytes(k) state bytes of
 * generation sel_dev[j], store_n_dev[sel_dev[j]] and seen_dev[sel_dev[j]] are
 * zeroed, each where its pointer was given.  Nothing else is written; invalid
 * and unused entries are skipped; duplicates are harmless.  One kernel
 * (k_stream_reset), one lane per 16-byte unit of state.
 * Returns QF_EINVAL for k outside 1..256, a NULL sel or sel_dev, n_max == 0,
 * G_src == 0, all three pointers NULL, or state_dev not 16-byte aligned. */
int qf_stream_reset_dev(qf_ctx *ctx, uint32_t k, const qf_gen_sel *sel, uint8_t *state_dev,
                        uint32_t *store_n_dev, uint32_t *seen_dev);

/* ---------------------------------------------------------------------------
 * Streaming receive from a flat poll.  No reference counterpart.  A receive
 * ring delivers frames in arrival order, and the generation of a frame comes
 * from an outer header (Packet::to_raw carries none).  A flat poll is N frame
 * slots in that order plus one u32 generation tag per frame; the three calls
 * below take it to the rank states and the row stores without a host scan and
 * without a per-generation poll buffer, and touch only the generations the
 * poll holds:
 *   qf_parse_poll_headers_dev  the flat poll -> the list of touched generations (sel, n_sel)
 *                              and, per list entry, row_off, row_len, row_index, n_rows, row_coeffs
 *   qf_rank_update_sel_batch   the entries' rows against the listed generations' rank states
 *                              -> innovative; rank_dev[sel[j]] of a persistent rank array
 *   qf_store_append_sel_dev    take_dev = innovative, src_dev = the poll's frames_dev,
 *                              src_gen_stride = N_max * frame_stride
 *   qf_gen_select_dev          over the persistent rank array (QF_SELECT_MARK, seen_dev)
 *   qf_decode_frames_sel_dev   or qf_recode_frames_sel_dev over the store arrays
 *   qf_stream_reset_dev        state, store_n and seen of the finished generations, and a
 *                              second call with seen_dev = rank_dev (state_dev and
 *                              store_n_dev NULL), which clears their entries of the
 *                              persistent rank array
 * ------------------------------------------------------------------------- */
/* No reference counterpart.  Groups a flat poll by generation, stably, and
 * parses the headers where the frames lie.
 * Reads: frames_dev, N_max slots of frame_stride bytes in the payload-aligned
 * layout of qf_frame_payload_offset(k); frame_len_dev, frame_off_dev (nullable:
 * 0) and ids_dev per frame as for qf_parse_frame_headers_dev; frame_gen_dev,
 * one u32 generation tag per frame; n_frames_dev (nullable: N_max), a device
 * count: the call looks at frames 0 .. N-1, N = min(*n_frames_dev, N_max).  Of
 * a frame at most the 3 header bytes and the k vector bytes are read, all
 * inside its slot; no payload byte.
 * Writes, by list position j in 0..n_max-1:
 *   sel_dev[j], *n_sel_dev, *n_match_dev (nullable)  the touched generations,
 *       those with at least one frame tagged < G_src, ascending, the first
 *       n_max of them; semantics as qf_gen_select_dev (entries at and above
 *       *n_sel_dev are not written, *n_match_dev counts all touched)
 *   row_off_dev, row_len_dev, row_index_dev, row_coeffs_dev (max_rows slots
 *       per entry) and n_rows_dev[j]: byte for byte what
 *       qf_parse_frame_headers_dev writes for a generation whose frames are
 *       the entry's frames in arrival order (ascending frame number f), except
 *       that row_off is relative to frames_dev: f*frame_stride + frame_off + 1
 *       for a systematic frame, + 3 + k for a coded one.  n_rows_dev[j] = 0 for
 *       unused entries j >= *n_sel_dev; slots at or above n_rows_dev[j] are
 *       not written
 *   entry_status_dev[j]: QF_OK; QF_ETOOSMALL for a generation with more than
 *       max_rows tagged frames in this poll, valid or not: the entry is listed
 *       with n_rows 0 and none of its frames is ingested (so the rule does not
 *       depend on the order of arrival)
 * and per frame f < N (frames at or above N are not written):
 *   frame_status_dev[f]: the per-frame codes of qf_parse_frame_headers_dev;
 *       QF_EINVAL for a tag >= G_src; QF_ENOTREADY for a frame whose
 *       generation was not listed because the list was full, or whose
 *       generation has more than max_rows frames: the caller can present those
 *       frames again.
 * Every output is deterministic: none depends on the order in which waves or
 * atomics run.
 * Returns QF_EINVAL for k outside 1..256, L == 0, max_rows outside 1..1024,
 * G_src == 0 or > 2^24, n_max == 0, frame_stride % 16 != 0, N_max *
 * frame_stride > 2^32 (the offsets are u32), a NULL required pointer (all but
 * frame_off_dev, n_frames_dev and n_match_dev; the per-frame pointers only
 * when N_max > 0), or frames_dev not 16-byte aligned.
 * Kernels: k_poll_count (a lane per frame counts its tag), k_gen_select_count
 * and k_gen_select_scatter over the counts, k_poll_place (a lane per frame
 * finds its entry and claims one of its slots) and k_poll_headers (a wave per
 * entry sorts its frames and parses them in order). */
int qf_parse_poll_headers_dev(qf_ctx *ctx, uint32_t k, uint32_t L, uint32_t max_rows,
                              const uint8_t *frames_dev, uint64_t frame_stride, uint32_t N_max,
                              const uint32_t *frame_len_dev, const uint32_t *frame_off_dev,
                              const uint64_t *ids_dev, const uint32_t *frame_gen_dev,
                              const uint32_t *n_frames_dev, uint32_t G_src, uint32_t n_max,
                              uint32_t *sel_dev, uint32_t *n_sel_dev, uint32_t *n_match_dev,
                              uint16_t *row_index_dev, uint32_t *n_rows_dev, uint8_t *row_coeffs_dev,
                              uint32_t *row_len_dev, uint32_t *row_off_dev,
                              int32_t *entry_status_dev, int32_t *frame_status_dev);

/* No reference counterpart.  qf_rank_update_batch over a list: the slots
 * (row_index_dev, n_rows_dev, row_coeffs_dev) and the outputs innovative_dev,
 * status_dev and rank_sel_dev (nullable) are compact, indexed by the list
 * position j in 0..n_max-1 (shape->max_rows slots per entry); state_dev holds
 * the rank states of sel->G_src generations and is indexed by sel_dev[j], and
 * so is rank_dev (nullable), of which only rank_dev[sel_dev[j]] of listed
 * entries is written, so a persistent rank array feeds qf_gen_select_dev.
 * A listed entry with sel_dev[j] < G_src: flags, status, rank (in both places)
 * and the state bytes afterwards are byte for byte what qf_rank_update_batch
 * produces for that generation with the same slots.  An invalid entry gets
 * status QF_EINVAL, flags 0 and rank_sel 0, and nothing is read or written
 * through it.  An unused entry gets flags 0, status QF_OK and rank_sel 0.
 * The list entries must be distinct (the list of qf_parse_poll_headers_dev
 * is): for a generation listed twice the result is unspecified, but every
 * access stays in bounds.
 * Returns what qf_rank_update_batch returns with n_max in the place of G
 * (status_dev is required, rank_sel_dev and rank_dev are not), and QF_EINVAL
 * for a NULL sel or sel_dev, n_max == 0 or G_src == 0.
 * One kernel, k_rank_update_sel: k_rank_filter's resuming form with the list
 * in front. */
int qf_rank_update_sel_batch(qf_ctx *ctx, const qf_rank_shape *shape, const qf_gen_sel *sel,
                             const uint16_t *row_index_dev, const uint32_t *n_rows_dev,
                             const uint8_t *row_coeffs_dev, uint8_t *state_dev,
                             uint8_t *innovative_dev, uint32_t *rank_sel_dev, uint32_t *rank_dev,
                             int32_t *status_dev);

/* No reference counterpart.  qf_store_append_dev over a list: row_off_dev,
 * row_len_dev, row_index_dev, n_rows_dev, row_coeffs_dev, take_dev and
 * status_dev are compact, indexed by the list position j (shape->max_rows
 * slots per entry); the five store arrays and store_n_dev hold sel->G_src
 * generations and are indexed by sel_dev[j].  All entries' rows lie in one
 * source region: rows[j][s] = the row_len bytes at src_dev + row_off (what
 * qf_parse_poll_headers_dev leaves, with src_dev = its frames_dev), and
 * shape->src_gen_stride is that region's size in bytes, so the geometry rule
 * reads row_off + row_len > src_gen_stride -> QF_EINVAL.  No payload is copied
 * before the append.
 * A listed entry with sel_dev[j] < G_src: status, the appended bytes and
 * metadata and store_n_dev are byte for byte what qf_store_append_dev writes
 * for that generation with the same slots; QF_ETOOSMALL, "a generation that is
 * not QF_OK appends nothing" and the read and write rules are that call's.  An
 * invalid entry gets status QF_EINVAL and nothing is read or written through
 * it; an unused entry gets status QF_OK.  The list entries must be distinct:
 * for a generation listed twice the result is unspecified, but every access
 * stays in bounds.
 * Returns what qf_store_append_dev returns with n_max in the place of G, and
 * QF_EINVAL for a NULL sel or sel_dev, n_max == 0 or G_src == 0.
 * Two kernels: k_store_prepare_sel and k_store_rows_sel, the dense call's with
 * the list in front. */
int qf_store_append_sel_dev(qf_ctx *ctx, const qf_store_shape *shape, const qf_gen_sel *sel,
                            const uint8_t *src_dev, const uint32_t *row_off_dev,
                            const uint32_t *row_len_dev, const uint16_t *row_index_dev,
                            const uint32_t *n_rows_dev, const uint8_t *row_coeffs_dev,
                            const uint8_t *take_dev, uint8_t *store_dev, uint32_t *store_off_dev,
                            uint32_t *store_len_dev, uint16_t *store_index_dev,
                            uint8_t *store_coeffs_dev, uint32_t *store_n_dev, int32_t *status_dev);

/* ---------------------------------------------------------------------------
 * The generation window.  No reference counterpart.  A stream numbers its
 * generations without bound in the outer header; every call above counts
 * generations in slots 0 .. G_src-1.  The window is the persistent map from
 * wire ids to slots, kept on the device and decided there, in front of
 * qf_parse_poll_headers_dev: which frames belong to the generation a slot
 * holds, which slots a newer generation takes over (their state is reset
 * before the ingest), and which frames are dropped because their generation
 * is gone (QF_ESTALE) or was delivered (QF_ECLOSED).
 *
 * The window state is caller-owned: win_dev holds G_src entries of uint64_t,
 * 8-byte aligned, zeroed once by the caller (every slot empty).
 *   entry 0          the slot is empty
 *   otherwise        bits 0..62 = id + 1, bit 63 = the closed flag
 * Wire ids are 0 .. 2^62 - 1 (the QUIC varint range); the slot of id x is
 * x % G_src.  A host may read the entries.  Ids are monotone: there is no
 * wrap-around arithmetic and no expiry by age.
 *
 * One poll of a receiver:
 *   qf_gen_window_dev          the poll's ids -> frame_gen_dev (the ingest's tags), the evict list
 *   qf_stream_reset_dev        twice over the evict list, as at the end of a poll
 *   qf_parse_poll_headers_dev  with frame_gen_dev; a dropped frame (QF_GEN_NONE) gets its QF_EINVAL
 *   qf_rank_update_sel_batch, qf_store_append_sel_dev, qf_gen_select_dev, qf_decode_frames_sel_dev
 *   qf_gen_window_sel_dev      over the completed list with QF_WINDOW_CLOSE: the ids that label
 *                              what is delivered; a later frame of them is QF_ECLOSED
 *   qf_stream_reset_dev        twice over the completed list
 * A relay runs qf_recode_frames_sel_dev, reads the ids without closing, and
 * never closes.
 * ------------------------------------------------------------------------- */
#define QF_GEN_NONE 0xFFFFFFFFu
/* No reference counterpart.  Let N = min(*n_frames_dev, N_max) (n_frames_dev
 * NULL: N_max), frame_id_dev[f] the wire generation id of frame f, and W the
 * window before the call.
 * Newest id per slot.  For each slot s, newest[s] is the largest valid id
 * among frames f < N with id % G_src == s.  A valid id is < 2^62.  If that id
 * is larger than the id W[s] holds, or W[s] is empty, the entry becomes
 * newest[s] + 1, open, with bit 63 clear.  Otherwise the entry is unchanged
 * byte for byte.  Entries of slots that no frame of the poll maps to are not
 * written.
 * Evicted slots.  A slot whose entry was replaced and whose old entry was
 * non-empty and open is evicted.  The evicted slots are listed ascending in
 * evict_sel_dev[0..], *n_evict_dev is their number, and evict_id_dev[j], when
 * given, is the id that was displaced.  Entries at and above *n_evict_dev are
 * not written.  A displaced closed or empty entry is not listed: its state was
 * reset when it was closed.  The list is what qf_stream_reset_dev takes as a
 * qf_gen_sel with n_max = n_evict_max; the caller runs the reset twice, as at
 * the end of a poll, before the ingest.
 * Per-frame outputs, for frames f < N (frames at or above N are not written):
 *   id >= 2^62                                       QF_EINVAL   QF_GEN_NONE
 *   id equals the id of the updated entry, open      QF_OK       the slot
 *   id equals the id of the updated entry, closed    QF_ECLOSED  QF_GEN_NONE
 *   id smaller than the id of the updated entry      QF_ESTALE   QF_GEN_NONE
 * in frame_status_dev[f] and frame_gen_dev[f].
 * Newest wins within a poll.  Within one poll the newest id of a slot wins
 * whatever the arrival order: frames of x and of x + G_src in the same poll
 * make every frame of x stale.
 * Determinism.  No output depends on the order of waves or atomics.
 * Returns QF_EINVAL, before any device work, for a NULL context, G_src == 0 or
 * G_src > 2^24 (the select's limit), flags != 0, n_evict_max < min(N_max,
 * G_src) (an eviction needs a frame, so with this bound the list never
 * overflows and no eviction is lost), a NULL required pointer (win_dev,
 * evict_sel_dev, n_evict_dev, and the per-frame pointers when N_max > 0), or
 * win_dev not 8-byte aligned.  N_max == 0 writes *n_evict_dev = 0 and is
 * QF_OK.
 * Kernels: a memset of G_src u64 of workspace, k_window_max (a lane per frame,
 * one atomicMax on id + 1), k_window_apply (a lane per slot), k_gen_select_count
 * and k_gen_select_scatter over the evicted flags, k_window_tag (a lane per
 * frame, and lanes for evict_id_dev). */
int qf_gen_window_dev(qf_ctx *ctx, uint32_t G_src, uint32_t N_max,
                      const uint64_t *frame_id_dev, const uint32_t *n_frames_dev,
                      uint64_t *win_dev, uint32_t flags,
                      uint32_t *frame_gen_dev, int32_t *frame_status_dev,
                      uint32_t n_evict_max, uint32_t *evict_sel_dev, uint32_t *n_evict_dev,
                      uint64_t *evict_id_dev);

/* No reference counterpart.  The wire ids of a list, and closing it.  For a
 * listed entry with sel_dev[j] < G_src and a non-empty window entry,
 * ids_dev[j] (nullable, n_max entries) is the wire id that slot holds: the
 * receiver labels what it delivers with it, the relay the frames it emits.
 * For invalid, unused and empty entries ids_dev[j] = UINT64_MAX.
 * flags: 0 or QF_WINDOW_CLOSE, which sets bit 63 of the listed non-empty
 * entries; duplicates are harmless and nothing else is written.  Without the
 * flag the window is only read.
 * Returns QF_EINVAL for unknown flag bits, a NULL sel, sel_dev or win_dev,
 * n_max == 0, G_src == 0, or when there is neither the flag nor ids_dev.
 * One kernel, k_window_sel, a lane per entry. */
#define QF_WINDOW_CLOSE 1u
int qf_gen_window_sel_dev(qf_ctx *ctx, const qf_gen_sel *sel, uint64_t *win_dev,
                          uint32_t flags, uint64_t *ids_dev);

/* ---------------------------------------------------------------------------
 * Partial decode: what the rows of a generation determine, at any rank.  No
 * reference counterpart (Decoder::get_decoded_packets returns a full decode
 * only, decoder.rs:641, 785).  qf_decode_frames_dev answers a generation of
 * rank < k with QF_ENOTREADY and nothing else; a generation that is displaced
 * from the slot ring short of rank k, or still short when a stream ends or a
 * deadline passes, would lose every packet it holds.  These two calls return
 * every source that the held rows pin down.
 * Inputs, shape (flags 0), alignment rules, the call-level QF_EINVAL cases and
 * G == 0 are those of qf_decode_frames_dev; qf_decode_partial_frames_sel_dev
 * mirrors qf_decode_frames_sel_dev in the same way.
 * Per generation let
 *   A = the innovative slots (what qf_rank_batch flags),
 *   S = the sources with a systematic slot in A,
 *   c = the number of coded slots in A,
 *   D = { i not in S : the unit vector e_i lies in the span of the vectors of A }.
 * Outputs:
 *   rank_dev, innovative_dev (both nullable)  what qf_rank_batch writes, always
 *   src_slot_dev[g*k + i] (nullable)  the slot of source i's systematic row for
 *                       i in S, else 0xFFFF; filled for every generation whose
 *                       status is QF_OK or QF_ENOTREADY, all 0xFFFF for QF_EINVAL
 *   n_rec_dev[g]        |D|
 *   rec_index_dev[g*min(k, r) + m]  the m-th element of D, ascending
 *   rec_dev             row m = source rec_index[m], exactly L bytes; rows at and
 *                       above n_rec are not written
 *   status_dev[g]       QF_OK iff rank == k; QF_ENOTREADY iff rank < k (n == 0
 *                       included): the outputs above are valid and describe what
 *                       is known; QF_EINVAL for the row and index rules of
 *                       qf_decode_frames_dev, for c > min(k, 128) (the control
 *                       kernel's matrix rows) and for |D| > min(k, r) (the output
 *                       capacity), each with n_rec 0 and no row written.
 *                       QF_ERANK is never reported: A is independent.
 * For a generation of rank k every output byte equals what the mirrored call
 * writes: D is then the complement of S, ascending in both.  A systematic row
 * that arrives after coded rows have determined its source is not innovative;
 * that source is in D and comes through rec_dev, as in the mirrored call.
 * Listed form: invalid entries get QF_EINVAL, n_rec 0, rank 0, no flags and
 * src_slot 0xFFFF and nothing is read through them; unused entries get what
 * the dense call writes for n_rows = 0; duplicates are legal.
 * Reads:
 *   - no payload byte of a slot outside A is read;
 *   - no payload at all is read for a generation with |D| = 0;
 *   - the payload of a slot of A is not read when its coefficient is zero in
 *     every determined source: the payload pass is given only the rows that
 *     some output uses.  A generation displaced with 50 systematic rows and 3
 *     coded rows that determine nothing costs no row read.
 * Within a row that is read, the rule of qf_decode_frames_dev holds (aligned
 * 16-byte units that hold at least one of its bytes).
 * A call re-reports what it finds each time it runs: a source delivered by an
 * earlier call over the same rows is reported again.  Remembering what was
 * already delivered is the caller's business.
 * Both calls clear qf_ctx_set_payload_stream / qf_ctx_set_payload_wait.
 * Kernels: k_rank_filter, k_partial_prepare (one wave per generation: the
 * reduced row echelon form of the c coded rows over the unknown sources, free
 * columns skipped), then ceil(min(k, r) / 16) passes of k_combine_rows_at; the
 * listed form runs k_sel_gather first.  No output depends on the order of
 * waves.
 * ------------------------------------------------------------------------- */
int qf_decode_partial_frames_dev(qf_ctx *ctx, const qf_decode_frames_shape *shape, uint32_t G,
                                 const uint8_t *src_dev, const uint32_t *row_off_dev,
                                 const uint32_t *row_len_dev, const uint16_t *row_index_dev,
                                 const uint32_t *n_rows_dev, const uint8_t *row_coeffs_dev,
                                 uint8_t *rec_dev, uint16_t *rec_index_dev, uint32_t *n_rec_dev,
                                 int32_t *status_dev, uint32_t *rank_dev, uint8_t *innovative_dev,
                                 uint16_t *src_slot_dev);
int qf_decode_partial_frames_sel_dev(qf_ctx *ctx, const qf_decode_frames_shape *shape,
                                     const qf_gen_sel *sel,
                                     const uint8_t *src_dev, const uint32_t *row_off_dev,
                                     const uint32_t *row_len_dev, const uint16_t *row_index_dev,
                                     const uint32_t *n_rows_dev, const uint8_t *row_coeffs_dev,
                                     uint8_t *rec_dev, uint16_t *rec_index_dev, uint32_t *n_rec_dev,
                                     int32_t *status_dev, uint32_t *rank_dev, uint8_t *innovative_dev,
                                     uint16_t *src_slot_dev);

/* ---------------------------------------------------------------------------
 * Delivery: the source packets of a generation in source order, each once.  No
 * reference counterpart.  A decode leaves a generation as a src_slot map into
 * the row store, a rec_index list and rec rows; these two calls take those
 * outputs and the store and write each generation's packets, in source order,
 * into one contiguous output.  A small persistent "delivered" state per
 * generation slot makes every source packet of a wire generation leave exactly
 * once across deadline flushes, displacement and completion.
 * Dense form: everything is indexed by g in 0..G-1.  Listed form: src_dev,
 * row_off_dev, row_len_dev and delivered_dev are the arrays of sel->G_src
 * generations, indexed by sel_dev[j]; every other argument is compact, indexed
 * by the list position j and sized for n_max, exactly as
 * qf_decode_frames_sel_dev and qf_decode_partial_frames_sel_dev leave their
 * outputs and as qf_gen_window_sel_dev and evict_id_dev leave the ids.
 * Per generation (entry) j, when dec_status_dev[j] is QF_OK or QF_ENOTREADY
 * (both carry valid src_slot, n_rec and rec_index, from either decode):
 *   S     = { i : src_slot_dev[j*k + i] != 0xFFFF }
 *   D     = rec_index_dev[j*e_max + 0 .. n_rec_dev[j])
 *   known = S u D;  new = known minus the sources marked in the delivered state.
 * Delivered state (delivered_dev, nullable, 8-byte aligned, QF_DELIVERED_WORDS
 * u64 per generation, zeroed once by the caller): word 0 is a tag, id + 1 of
 * the wire generation the mask belongs to (0: empty); bit i of the 256 bits
 * behind it is source i.  With ids_dev a tag other than ids_dev[j] + 1 means
 * that the slot now holds another generation and the mask is taken as empty;
 * when something is delivered the tag is rewritten with the new mask, so a
 * slot that was displaced or reset needs no reset of this state.  An id of
 * UINT64_MAX or >= 2^62 makes the entry QF_EINVAL.  With ids_dev NULL the tag
 * is neither read nor written, and the caller zeroes a generation's words when
 * it resets it.  With delivered_dev NULL every known source is new and ids_dev
 * is ignored.  The state is written only when new is not empty.  With
 * delivered_dev the listed entries must be distinct (for a duplicate the
 * result is unspecified, every access stays in bounds: the rule of
 * qf_rank_update_sel_batch); without it duplicates are legal.
 * Outputs:
 *   out_dev             for i in new the packet at j*out_gen_stride +
 *                       i*out_row_stride: round_up(len, 16) bytes are written,
 *                       those after len zero; len is the slot's row_len for a
 *                       stored source and L for a recovered one.  No byte of
 *                       any other row is written.
 *   out_len_dev[j*k+i]  len for i in new, else 0
 *   out_state_dev[j*k+i]  QF_SRC_STORED / QF_SRC_RECOVERED for i in new, else
 *                       QF_SRC_EARLIER (marked in the state) or QF_SRC_UNKNOWN
 *   n_out_dev[j]        |new|
 *   n_known_dev[j]      (nullable) |known u the marked sources below k|
 *   status_dev[j]       QF_OK: everything known has left.  QF_ENOTREADY:
 *                       dec_status_dev[j] is another value or the entry is
 *                       unused; all outputs zero, nothing read.  QF_EINVAL: an
 *                       invalid entry (sel_dev[j] >= G_src), a bad id, or
 *                       inconsistent inputs -- a src_slot value >= max_rows
 *                       other than 0xFFFF, n_rec > e_max, a rec_index >= k, a
 *                       source twice in rec_index or in both rec_index and S,
 *                       a stored row (any source of S) with row_len > L,
 *                       row_off % 16 != 0 or row_off + row_len >
 *                       src_gen_stride; all outputs zero, no payload byte and
 *                       no state touched.  Every index is checked before it is
 *                       used.
 * Reads: only aligned 16-byte units of a delivered row that hold one of its
 * bytes, and no payload byte of a source that is not in new (so rec_dev must
 * reach to the end of its last row's last unit: rec_row_stride bytes per row
 * do).  src_dev and rec_dev are only read and must not overlap out_dev.
 * Returns QF_EINVAL for k outside 1..256, e_max > 128, L == 0, max_rows
 * outside 1..1024, flags or reserved != 0, G (n_max) > 2^24, a stride or
 * src_dev / rec_dev / out_dev not 16-byte aligned, rec_row_stride < L,
 * out_row_stride < round_up(L, 16), out_gen_stride < k * out_row_stride,
 * delivered_dev not 8-byte aligned, a NULL required pointer (all but ids_dev,
 * delivered_dev and n_known_dev; rec_dev and rec_index_dev only when e_max >
 * 0), and in the listed form a NULL sel or sel_dev, n_max == 0 or G_src == 0.
 * G == 0 is QF_OK.
 * Kernels: k_deliver_prepare (one wave per entry: checks, sets, state, one
 * record per delivered packet) and k_deliver_rows (the copy); no output
 * depends on the order of waves.
 * ------------------------------------------------------------------------- */
#define QF_DELIVERED_WORDS 5   /* u64 per generation slot: tag, then 256 bits, bit i = source i */

/* out_state values */
#define QF_SRC_UNKNOWN   0  /* not determined by what the generation holds            */
#define QF_SRC_STORED    1  /* delivered by this call from its systematic row         */
#define QF_SRC_RECOVERED 2  /* delivered by this call from rec_dev                    */
#define QF_SRC_EARLIER   3  /* determined, but delivered by an earlier call (not written) */

typedef struct qf_deliver_shape {
    uint32_t k;              /* 1..256 */
    uint32_t e_max;          /* rec rows per generation: the decode's min(k, r), 0..128 */
    uint32_t L;              /* >= 1, the decode's L */
    uint32_t max_rows;       /* slots per generation of the source arrays (the store's cap), 1..1024 */
    uint32_t flags;          /* 0 */
    uint32_t reserved;       /* 0 */
    uint64_t src_gen_stride; /* as the decode's */
    uint64_t rec_row_stride; /* as the decode's */
    uint64_t rec_gen_stride;
    uint64_t out_row_stride; /* % 16 == 0, >= round_up(L, 16) */
    uint64_t out_gen_stride; /* % 16 == 0, >= k * out_row_stride */
} qf_deliver_shape;

int qf_deliver_frames_dev(qf_ctx *ctx, const qf_deliver_shape *shape, uint32_t G,
                          const uint8_t *src_dev, const uint32_t *row_off_dev,
                          const uint32_t *row_len_dev, const uint8_t *rec_dev,
                          const uint16_t *rec_index_dev, const uint32_t *n_rec_dev,
                          const int32_t *dec_status_dev, const uint16_t *src_slot_dev,
                          const uint64_t *ids_dev, uint64_t *delivered_dev,
                          uint8_t *out_dev, uint32_t *out_len_dev, uint8_t *out_state_dev,
                          uint32_t *n_out_dev, uint32_t *n_known_dev, int32_t *status_dev);
int qf_deliver_frames_sel_dev(qf_ctx *ctx, const qf_deliver_shape *shape, const qf_gen_sel *sel,
                              const uint8_t *src_dev, const uint32_t *row_off_dev,
                              const uint32_t *row_len_dev, const uint8_t *rec_dev,
                              const uint16_t *rec_index_dev, const uint32_t *n_rec_dev,
                              const int32_t *dec_status_dev, const uint16_t *src_slot_dev,
                              const uint64_t *ids_dev, uint64_t *delivered_dev,
                              uint8_t *out_dev, uint32_t *out_len_dev, uint8_t *out_state_dev,
                              uint32_t *n_out_dev, uint32_t *n_known_dev, int32_t *status_dev);

/* ---------------------------------------------------------------------------
 * Streaming send: the listed rows as a flat frame queue.  No reference
 * counterpart.  The mirror of qf_parse_poll_headers_dev: it takes compact rows
 * by list position -- what qf_recode_frames_sel_dev leaves, or a source's
 * packets -- and appends each entry's frames to a flat queue of N_max frame
 * slots without a hole, with an emission budget per generation.  The queue's
 * arrays (frames_dev, frame_len_dev, frame_off_dev, frame_id_dev,
 * frame_pkt_dev, n_frames_dev) are exactly the flat poll that
 * qf_gen_window_dev (ids = frame_id_dev) and qf_parse_poll_headers_dev
 * (ids = frame_pkt_dev) of the next hop read, so a hop needs no host scan.
 * Inputs, indexed by the list position j in 0..n_max-1 (the input layout of
 * qf_frame_rows_dev with G = n_max): rows_dev (row s of entry j at
 * j*rows_gen_stride + s*row_stride), row_index_dev (nullable: every row coded),
 * n_rows_dev (nullable: max_rows), row_coeffs_dev ([n_max][max_rows][k];
 * nullable when row_index_dev is given), row_len_dev (nullable: L),
 * in_status_dev (nullable; the recode's status_dev) and ids_dev (the wire
 * generation ids, as qf_gen_window_sel_dev writes them).  rank_dev and sent_dev
 * (both or neither) are persistent arrays of sel->G_src generations, indexed by
 * sel_dev[j]: the budget.
 * Per entry j, with n = min(*n_sel_dev, n_max) and n_j = min(n_rows_dev[j],
 * max_rows), the first that applies:
 *   j >= n (unused)                       QF_ENOTREADY, count 0
 *   sel_dev[j] >= G_src, ids_dev[j] >= 2^62 (UINT64_MAX included), one of the
 *   first n_j rows with row_len > L or with index >= k while row_coeffs_dev is
 *   NULL (invalid)                        QF_EINVAL, count 0; nothing is read
 *                                         through a bad sel or id
 *   in_status_dev[j] != QF_OK             that status, count 0
 *   otherwise the entry wants c_j = n_j frames, with the budget c_j = min(n_j,
 *   rank_dev[g] - sent_dev[g]) (0 when rank <= sent), g = sel_dev[j]: its first
 *   c_j rows.
 * The queue: base = min(*n_frames_dev, N_max) with QF_EMIT_APPEND, else 0
 * (*n_frames_dev is then not read).  P_j = the sum of c over the entries before
 * j.  Entry j is emitted iff base + P_j + c_j <= N_max; P_j only grows, so the
 * emitted entries are a prefix of the wanting ones and the queue has no hole.
 * Row s of an emitted entry is frame base + P_j + s.
 *   entry_status_dev[j]  QF_OK for an emitted entry (also one with c_j = 0),
 *                        QF_ENOTREADY for one that does not fit, else as above
 *   entry_count_dev[j]   c_j for an emitted entry, else 0
 *   entry_first_dev[j]   base + P_j, 0xFFFFFFFF whenever the count is 0
 *   *n_frames_dev        the queue's new length: base + the emitted frames
 *   *n_left_dev          (nullable) the wanted frames that did not fit
 *                        (0xFFFFFFFF for more)
 *   sent_dev[g]          += c_j for emitted entries only: an entry that did not
 *                        fit leaves with a later call, qf_gen_select_dev(rank_dev,
 *                        seen_dev = sent_dev, min_rank 1, flags 0) lists exactly
 *                        the generations with budget left, and
 *                        qf_stream_reset_dev(seen_dev = sent_dev) clears it
 * With sent_dev the valid entries must be distinct (for a duplicate the result
 * is unspecified, every access stays in bounds: the rule of
 * qf_rank_update_sel_batch).
 * Per frame f in [base, *n_frames_dev), row s of entry j: the slot's bytes,
 * frame_len_dev[f] and frame_off_dev[f] are byte for byte what
 * qf_frame_rows_dev writes in copy mode for that row (the payload at byte P =
 * qf_frame_payload_offset(k) of slot f, the header in front of it; no byte of
 * the slot outside the frame is written); frame_id_dev[f] = ids_dev[j];
 * frame_pkt_dev[f] = the row's index for a systematic row and 0 for a coded
 * one, so that id % k in the parsers is the source index.  Nothing is written
 * below base or at and beyond the new length.
 * Reads: the metadata of the first n_j rows of entries with a valid sel and id;
 * of emitted rows only, the aligned 16-byte payload units that hold a byte of
 * the row (rows_dev must reach to the end of its last row's last unit) and
 * bytes of the row's own k-byte vector, through aligned dwords that lie inside
 * it, or singly.  rows_dev is only read and must not overlap frames_dev.
 * Returns QF_EINVAL for k outside 1..256, L == 0, max_rows outside 1..1024,
 * N_max == 0, unknown flag bits, reserved != 0, a stride or rows_dev /
 * frames_dev not 16-byte aligned, row_stride < L, frame_stride < P + L,
 * N_max * frame_stride > 2^32, one of rank_dev / sent_dev without the other,
 * row_index_dev and row_coeffs_dev both NULL, a NULL required pointer (all but
 * the nullable ones above), a NULL sel or sel_dev, n_max == 0, n_max > 2^24 or
 * G_src == 0.
 * Kernels: k_emit_count and k_emit_place (checks, counts and their prefix in
 * two launches as in qf_gen_select_dev, no workgroup waits for another) and
 * k_emit_frames (the bytes: four frames per wave); no output depends on the
 * order of waves or on atomics.
 * ------------------------------------------------------------------------- */
#define QF_EMIT_APPEND 1u   /* qf_emit_shape.flags: append at *n_frames_dev instead of starting at 0 */

typedef struct qf_emit_shape {
    uint32_t k;               /* 1..256 */
    uint32_t L;               /* >= 1, the longest row */
    uint32_t max_rows;        /* rows per entry, 1..1024 */
    uint32_t N_max;           /* frame slots of the queue, >= 1 */
    uint32_t flags;           /* 0 or QF_EMIT_APPEND */
    uint32_t reserved;        /* 0 */
    uint64_t row_stride;      /* % 16 == 0, >= L */
    uint64_t rows_gen_stride; /* % 16 == 0 */
    uint64_t frame_stride;    /* % 16 == 0, >= P + L, N_max * frame_stride <= 2^32 */
} qf_emit_shape;

int qf_emit_frames_sel_dev(qf_ctx *ctx, const qf_emit_shape *shape, const qf_gen_sel *sel,
                           const uint8_t *rows_dev, const uint16_t *row_index_dev,
                           const uint32_t *n_rows_dev, const uint8_t *row_coeffs_dev,
                           const uint32_t *row_len_dev, const int32_t *in_status_dev,
                           const uint64_t *ids_dev, const uint32_t *rank_dev, uint32_t *sent_dev,
                           uint8_t *frames_dev, uint32_t *frame_len_dev, uint32_t *frame_off_dev,
                           uint64_t *frame_id_dev, uint64_t *frame_pkt_dev, uint32_t *n_frames_dev,
                           uint32_t *n_left_dev, uint32_t *entry_first_dev,
                           uint32_t *entry_count_dev, int32_t *entry_status_dev);

/* ---------------------------------------------------------------------------
 * Streaming feedback: rank reports and the credit budget.  No reference
 * counterpart.  A receiver tells its sender what it holds of a generation in a
 * 16-byte record; the sender turns its own ranks, a redundancy ratio and those
 * records into credit_dev, the array that qf_gen_select_dev and
 * qf_emit_frames_sel_dev take as rank_dev beside sent_dev: "the number of
 * frames a generation may have sent in total".  The records travel back as
 * the feedback packets of qf_frame_reports_dev / qf_parse_report_frames_dev
 * below, or any other way the host likes.
 *   id        a wire generation id (< 2^62); UINT64_MAX is a hole the applier
 *             skips (with status QF_EINVAL)
 *   rank      what the reporting node holds of it, 0..k; k for a generation it
 *             has delivered and closed
 *   reserved  0
 *
 * qf_rank_report_sel_dev: the ranks of a list as reports.  n = min(*n_sel_dev,
 * n_max) (n_max with n_sel_dev NULL); base = min(*n_reports_dev, N_max) with
 * QF_REPORT_APPEND, else 0 (*n_reports_dev is then not read).  The record of
 * entry j < n goes to reports_dev[base + j] when base + j < N_max; for slot s =
 * sel_dev[j] it is
 *   s >= G_src, or win_dev[s] empty        {UINT64_MAX, 0, 0}
 *   win_dev[s] open                         {its id, min(rank_dev[s], k), 0}
 *   win_dev[s] closed                       {its id, k, 0}  (the closing reset
 *                                           zeroed the rank: the window
 *                                           remembers it)
 * *n_reports_dev = min(base + n, N_max); *n_left_dev (nullable) = the records
 * that did not fit, base + n - *n_reports_dev.  Nothing is written below base or
 * at and beyond the new length; win_dev and rank_dev are only read; a sel value
 * at or behind n is not looked at and nothing is read through one >= G_src.
 * Duplicates in the list give duplicate records.  Meant for the completed list
 * after qf_gen_window_sel_dev(QF_WINDOW_CLOSE) has closed it and, appended, for
 * the list of qf_gen_select_dev(rank_dev, NULL, min_rank 1, flags 0) after the
 * resets: every open generation that holds a row.
 * Returns QF_EINVAL for k outside 1..256, a NULL ctx, sel, sel_dev, win_dev,
 * rank_dev, reports_dev or n_reports_dev, n_max == 0, G_src == 0, N_max == 0,
 * unknown flag bits, or reports_dev not 16-byte aligned.
 * One kernel, k_report_sel, a lane per entry (an appending call copies
 * *n_reports_dev in front of it).
 *
 * qf_credit_update_dev: credit_dev[s] for every slot s < G, every call.
 * fb_state_dev holds 16 bytes per slot, {u64 owner; u32 peer; u32 reserved},
 * zeroed once by the caller and then owned by this call: owner is the id + 1 of
 * the generation the state belongs to (0: none), peer the highest rank reported
 * for it.  credit_dev is read as the previous credit of a slot whose state
 * belongs to the generation the slot holds, and is not read otherwise (so it
 * needs no initialisation).
 * Reports: N = min(*n_reports_dev, N_max) (N_max with n_reports_dev NULL).  For
 * f < N, with s = id % G, the first that applies:
 *   id >= 2^62, rank > k or reserved != 0         QF_EINVAL (nothing is read
 *                                                 through the id)
 *   win_dev[s] holds a larger id                  QF_ESTALE
 *   win_dev[s] is empty or holds a smaller id     QF_ENOTREADY
 *   win_dev[s] holds this id, open or closed      QF_OK
 * in report_status_dev[f] (nullable).  Reports at and above N are not looked at
 * and their status is not written.
 * Per slot s: an empty win_dev[s] gives credit 0 and the state {0, 0, 0}.
 * Otherwise, with r = min(rank_dev[s], k), ceil_rho(x) = ceil(x * num / den),
 * (p, previous) = (peer, credit_dev[s]) when owner == the held id + 1 and
 * (0, 0) when not, and fresh = the largest rank among this call's QF_OK
 * reports for the slot:
 *   1. peer = max(p, fresh)
 *   2. peer >= k: credit = sent_dev[s] (the peer is satisfied, nothing is left
 *      to send: qf_gen_select_dev(credit_dev, sent_dev, 1, 0) does not list it)
 *   3. else c = max(previous, ceil_rho(r))        (every unit of rank is worth
 *                                                 rho frames)
 *   4. with a QF_OK report in this call, c = max(c, sent_dev[s] +
 *      ceil_rho(max(0, r - peer)))                (a request for what the peer
 *      lacks of what this node holds; the same report twice in one call changes
 *      nothing, in a later call it asks again: when to report is the host's
 *      retransmission policy)
 *   5. credit = min(c, cap)
 * and the state becomes {held id + 1, peer, 0}.  With num == den and no report
 * credit = min(rank, k, cap), the budget rank - sent of qf_emit_frames_sel_dev.
 * win_dev, rank_dev, sent_dev and reports_dev are only read.
 * Returns QF_EINVAL for k outside 1..256, den == 0, num < den, num > 65535,
 * cap == 0, cap > 2^20, G == 0, G > 2^24, flags or reserved != 0, a NULL ctx,
 * shape, win_dev, rank_dev, sent_dev, fb_state_dev or credit_dev, reports_dev
 * NULL with N_max > 0, win_dev not 8-byte or reports_dev / fb_state_dev not
 * 16-byte aligned.
 * Kernels: a memset of G u32 of workspace, k_credit_reports (a lane per report:
 * one 32-bit atomicMax of rank + 1 per QF_OK report; not launched with N_max 0)
 * and k_credit_apply (a lane per slot).  A maximum does not depend on the
 * order, so no output depends on the order of waves.
 * ------------------------------------------------------------------------- */
typedef struct qf_rank_report {
    uint64_t id;
    uint32_t rank;
    uint32_t reserved;
} qf_rank_report; /* 16 bytes */

#define QF_REPORT_APPEND 1u   /* qf_rank_report_sel_dev flags: append at *n_reports_dev instead of starting at 0 */

int qf_rank_report_sel_dev(qf_ctx *ctx, uint32_t k, const qf_gen_sel *sel, const uint64_t *win_dev,
                           const uint32_t *rank_dev, uint32_t N_max, uint32_t flags,
                           qf_rank_report *reports_dev, uint32_t *n_reports_dev, uint32_t *n_left_dev);

typedef struct qf_credit_shape {
    uint32_t k;               /* 1..256 */
    uint32_t num;             /* rho = num / den >= 1, num <= 65535 */
    uint32_t den;             /* >= 1 */
    uint32_t cap;             /* the most a generation may ever have sent, 1..2^20 */
    uint32_t flags;           /* 0 */
    uint32_t reserved;        /* 0 */
} qf_credit_shape;

int qf_credit_update_dev(qf_ctx *ctx, const qf_credit_shape *shape, uint32_t G, const uint64_t *win_dev,
                         const uint32_t *rank_dev, const uint32_t *sent_dev, uint32_t N_max,
                         const qf_rank_report *reports_dev, const uint32_t *n_reports_dev,
                         uint8_t *fb_state_dev, uint32_t *credit_dev, int32_t *report_status_dev);

/* ---------------------------------------------------------------------------
 * The reports on the wire.  A feedback packet is
 *   byte 0       0x02  (a data frame starts with 0x00 coded / 0x01 systematic,
 *                so a demultiplexer can tell the two directions apart)
 *   bytes 1..2   c, the number of entries, big-endian u16, c >= 1
 *   c entries of 10 bytes: the wire generation id as a big-endian u64 (< 2^62),
 *                then the rank as a big-endian u16 (0..k; 256 needs the high byte)
 * so 3 + 10 c bytes, without padding, checksum or varint: integrity and
 * encryption belong to the outer transport, as they do for data frames.
 * qf_report_frame_capacity(max_len), host only: the entries a packet of at most
 * max_len bytes holds, (max_len - 3) / 10 for max_len 13..65535, else 0.
 * Packet slot p of pkts_dev is bytes [p * stride, p * stride + stride).
 *
 * qf_frame_reports_dev: a report array as packets.  N = min(*n_reports_dev,
 * N_max) (N_max with n_reports_dev NULL), per = qf_report_frame_capacity(
 * max_len).  A record is sendable iff id < 2^62, rank <= k and reserved == 0;
 * every other record, the hole UINT64_MAX included, is skipped.  The S sendable
 * records among the first N keep their order: number i is entry i % per of
 * packet i / per.  P = min(ceil(S / per), F_max) packets are written, packet p
 * from byte 0 of slot p with c_p = min(per, S - p * per) entries and
 * pkt_len_dev[p] = 3 + 10 c_p; *n_pkts_dev = P; *n_left_dev (nullable) = S -
 * min(S, F_max * per), the sendable records that did not fit; *n_skipped_dev
 * (nullable) = N - S.  No byte of a slot outside [0, pkt_len) is written, no
 * slot and no pkt_len_dev entry at or beyond P; the report array is only read,
 * and a record at or behind N is not looked at.
 * Returns QF_EINVAL, before any device work, for a NULL ctx, shape,
 * reports_dev, pkts_dev, pkt_len_dev or n_pkts_dev, k outside 1..256, max_len
 * outside 13..65535, F_max == 0, N_max == 0, N_max > 2^24, flags != 0, stride %
 * 16 != 0, stride < max_len, or reports_dev / pkts_dev not 16-byte aligned.
 * Kernels: k_fbw_count (a lane per record, the blocks' sums) and k_fbw_pack (the
 * prefix over the sums; ten byte stores per sendable record, the header and
 * the length from the lane with a packet's entry 0).
 *
 * qf_parse_report_frames_dev: a flat poll of packets as a report array.  F =
 * min(*n_pkts_dev, F_max) (F_max with n_pkts_dev NULL).  Packet f < F with len =
 * pkt_len_dev[f] is QF_OK iff 3 <= len <= min(max_len, stride), byte 0 is 0x02,
 * c >= 1 and len == 3 + 10 c; every other packet is QF_EINVAL and contributes
 * nothing (len 0 included, as an empty frame is for the frame parsers).  No
 * byte at or beyond min(len, stride) of a slot is read, and none when len < 3.
 * base = min(*n_reports_dev, N_max) with QF_REPORT_APPEND in flags, else 0.  The
 * entries of the QF_OK packets follow each other in packet order, then entry
 * order; entry i of all T goes to reports_dev[base + i] as {id, rank, 0} when
 * base + i < N_max.  *n_reports_dev = min(base + T, N_max); *n_left_dev
 * (nullable) = base + T - *n_reports_dev (saturating at UINT32_MAX).  Nothing is
 * written below base or at and beyond the new length.  For f < F only, each
 * nullable: pkt_status_dev[f] the status; pkt_first_dev[f] = base + the entries
 * of the QF_OK packets in front of f for a QF_OK packet (saturating at
 * 0xFFFFFFFE), 0xFFFFFFFF otherwise: with it a host attributes records to the
 * peer a packet came from; pkt_count_dev[f] = c for a QF_OK packet, else 0.
 * Entry values are not judged: an id >= 2^62 or a rank > k goes through and gets
 * its QF_EINVAL from qf_credit_update_dev, the one place that decides.
 * Returns QF_EINVAL, before any device work, for a NULL ctx, shape, pkts_dev,
 * pkt_len_dev, reports_dev or n_reports_dev, flag bits other than
 * QF_REPORT_APPEND, and otherwise as qf_frame_reports_dev.
 * Kernels: k_fbr_count (a lane per packet: the decision, the blocks' sums),
 * k_fbr_place (the prefix, the per-packet outputs, the lengths) and
 * k_fbr_records (a wave per 64 entries of a packet, a record per lane; an
 * appending call copies *n_reports_dev in front of them).
 *
 * qf_report_closed_dev: the report of a closed generation, again.  A receiver
 * reports a generation's closing once; when that report is lost the sender goes
 * on emitting, and the frames come back from qf_gen_window_dev as QF_ECLOSED.
 * frame_id_dev / frame_status_dev are that call's arrays of this poll, M =
 * min(*n_frames_dev, F_max) (F_max with n_frames_dev NULL).  Slot s < G_src is
 * marked iff some frame f < M has frame_status_dev[f] == QF_ECLOSED,
 * frame_id_dev[f] < 2^62, frame_id_dev[f] % G_src == s and win_dev[s] holds
 * exactly that id with the closed flag set: a status the window does not back
 * up is ignored, and nothing is read through a bad id.  One record {id, k, 0}
 * per marked slot, in ascending slot order, goes to reports_dev from base (0, or
 * min(*n_reports_dev, N_max) with QF_REPORT_APPEND) while it is below N_max;
 * *n_reports_dev and *n_left_dev (nullable) as in qf_rank_report_sel_dev.  Any
 * number of frames of a generation give one record.  Meant to run appended
 * behind the two report calls of a poll.
 * Returns QF_EINVAL for k outside 1..256, G_src == 0 or > 2^24, F_max == 0,
 * N_max == 0, unknown flag bits, a NULL ctx, frame_id_dev, frame_status_dev,
 * win_dev, reports_dev or n_reports_dev, win_dev not 8-byte or reports_dev not
 * 16-byte aligned.
 * Kernels: a memset of G_src u32 of workspace, k_closed_mark (a lane per frame;
 * every writer of a slot's flag writes the same value), the two kernels of
 * qf_gen_select_dev over the flags and k_report_sel over their list.  No output
 * depends on the order of waves.
 * ------------------------------------------------------------------------- */
typedef struct qf_report_wire_shape {
    uint32_t k;               /* 1..256 */
    uint32_t max_len;         /* the most bytes a feedback packet may have, 13..65535 */
    uint32_t F_max;           /* packet slots, >= 1 */
    uint32_t flags;           /* pack: 0; parse: 0 or QF_REPORT_APPEND */
    uint64_t stride;          /* bytes per packet slot, % 16 == 0, >= max_len */
} qf_report_wire_shape;

uint32_t qf_report_frame_capacity(uint32_t max_len);

int qf_frame_reports_dev(qf_ctx *ctx, const qf_report_wire_shape *shape, uint32_t N_max,
                         const qf_rank_report *reports_dev, const uint32_t *n_reports_dev,
                         uint8_t *pkts_dev, uint32_t *pkt_len_dev, uint32_t *n_pkts_dev,
                         uint32_t *n_left_dev, uint32_t *n_skipped_dev);

int qf_parse_report_frames_dev(qf_ctx *ctx, const qf_report_wire_shape *shape,
                               const uint8_t *pkts_dev, const uint32_t *pkt_len_dev, const uint32_t *n_pkts_dev,
                               uint32_t N_max, qf_rank_report *reports_dev, uint32_t *n_reports_dev,
                               uint32_t *n_left_dev, int32_t *pkt_status_dev,
                               uint32_t *pkt_first_dev, uint32_t *pkt_count_dev);

int qf_report_closed_dev(qf_ctx *ctx, uint32_t k, uint32_t G_src, uint32_t F_max,
                         const uint64_t *frame_id_dev, const int32_t *frame_status_dev, const uint32_t *n_frames_dev,
                         const uint64_t *win_dev, uint32_t N_max, uint32_t flags,
                         qf_rank_report *reports_dev, uint32_t *n_reports_dev, uint32_t *n_left_dev);

/* ---------------------------------------------------------------------------
 * Heterogeneous batches (SURVEY 8(b) qf_gen_desc): one call over generations
 * whose (k, r, L) and placement differ per generation -- the ASW-RLNC-X mix
 * of window sizes (adaptive.rs:124-153, BASELINE config C5).  Generations
 * are grouped by shape inside the call; each group runs the batch kernels
 * above with per-generation offset tables (no payload is copied).
 * replaces per-generation Encoder::generate_repair_packet (decoder.rs:171-275)
 * / Decoder::add_packet + try_decode (decoder.rs:678-791) calls.
 * ------------------------------------------------------------------------- */
typedef struct qf_gen_desc {
    uint32_t k, r, L;        /* generation size, repairs (k + r <= 256), payload bytes */
    uint32_t flags;          /* QF_ENCODE_ZERO_TAIL: bytes [L, 16*ceil8(L/16)) of each repair row may be zeroed */
    uint64_t src_offset;     /* source row i at src_dev + src_offset + i * src_row_stride */
    uint64_t src_row_stride;
    uint64_t rep_offset;     /* repair row j at rep_dev + rep_offset + j * rep_row_stride */
    uint64_t rep_row_stride;
} qf_gen_desc;
/* Offsets and strides are multiples of 16; QF_ERANGE if any k + r > 256. */
int qf_encode_batch_desc(qf_ctx *ctx, const qf_gen_desc *gens_host, uint32_t G, const uint8_t *src_dev,
                         uint8_t *rep_dev);

typedef struct qf_dec_desc {
    uint32_t k, r, L;
    uint32_t n_rows;            /* received rows of this generation (<= 255), arrival order */
    uint64_t rows_offset;       /* received row s at rows_dev + rows_offset + s * row_stride */
    uint64_t row_stride;
    uint64_t row_index_offset;  /* its n_rows indices (< k source, k + j repair j) at row_index_dev + this (elements) */
    uint64_t rec_offset;        /* recovered row m at rec_dev + rec_offset + m * rec_row_stride */
    uint64_t rec_row_stride;
    uint64_t rec_index_offset;  /* min(k, r) u16 entries at rec_index_dev + this (elements) */
} qf_dec_desc;
/* Cauchy-coded generations (repair coefficients = the Cauchy row of the
 * repair index, decoder.rs:280-298).  n_rec_dev / status_dev: one entry per
 * descriptor, in descriptor order (status as qf_decode_batch). */
int qf_decode_batch_desc(qf_ctx *ctx, const qf_dec_desc *gens_host, uint32_t G, const uint8_t *rows_dev,
                         const uint16_t *row_index_dev, uint8_t *rec_dev, uint16_t *rec_index_dev,
                         uint32_t *n_rec_dev, int32_t *status_dev);

/* ---------------------------------------------------------------------------
 * Per-connection objects mirroring the reference's Rust API one call at a
 * time (what core.rs drives).  Payload state lives in HBM.
 * ------------------------------------------------------------------------- */
typedef struct qf_encoder qf_encoder;
/* replaces decoder.rs:156 Encoder::new(k, n); max_len bounds packet length */
int qf_encoder_new(qf_ctx *ctx, uint32_t k, uint32_t n, uint32_t max_len, qf_encoder **out);
int qf_encoder_free(qf_encoder *enc);
/* replaces decoder.rs:164 Encoder::add_source_packet (slides the window) */
int qf_encoder_add_source_packet(qf_encoder *enc, uint64_t id, const uint8_t *data,
                                 uint32_t len);
/* replaces decoder.rs:172 Encoder::generate_repair_packet(j).  QF_ENOTREADY
 * while the window holds fewer than k packets (the reference's None).
 * out_data receives len = window[0].len bytes, out_coeffs k bytes,
 * *out_id = last.id + 1 + j. */
int qf_encoder_generate_repair_packet(qf_encoder *enc, uint32_t repair_index,
                                      uint8_t *out_data, uint32_t out_cap,
                                      uint32_t *out_len, uint8_t *out_coeffs,
                                      uint64_t *out_id);
/* All repairs first..first+count-1 of the current window in one launch
 * (adaptive.rs:546-562 emit_repairs). out_data rows are out_stride apart. */
int qf_encoder_generate_repairs(qf_encoder *enc, uint32_t first, uint32_t count,
                                uint8_t *out_data, uint32_t out_stride, uint32_t *out_len,
                                uint8_t *out_coeffs, uint64_t *out_ids);
int qf_encoder_window_len(const qf_encoder *enc);

typedef struct qf_decoder qf_decoder;
/* Largest k of a GF(2^8) decoder: the largest window any mode uses
 * (Extreme, adaptive.rs:131-133).  k > 256 needs explicit coefficients on
 * every repair row (the reference's u8 Cauchy rows wrap there). */
#define QF_DECODER_MAX_K 4096
/* replaces decoder.rs:659 Decoder::new(k, pool): k <= 256 decodes by
 * Gauss-Jordan (or the Cauchy kernels), 256 < k <= QF_DECODER_MAX_K by the
 * Wiedemann strategy (decoder.rs:660-664, 794-975; qf_wiedemann.hip). */
int qf_decoder_new(qf_ctx *ctx, uint32_t k, uint32_t max_len, qf_decoder **out);
/* replaces decoder.rs:520-524 DecodingStrategy: 0 GaussianElimination,
 * 1 Wiedemann, as Decoder::new chose it; QF_EINVAL for NULL. */
#define QF_STRATEGY_GAUSSIAN 0
#define QF_STRATEGY_WIEDEMANN 1
int qf_decoder_strategy(const qf_decoder *dec);
/* Projections the last Wiedemann solve of this decoder tried (1..8; 9 = none
 * verified and exact elimination decided); 0 before any
 * Wiedemann solve and for k <= 256 decoders. */
int qf_decoder_solve_attempts(const qf_decoder *dec);
/* No reference counterpart (opt-in, off by default): with the mode on,
 * qf_decoder_add_packet takes a packet only if it is innovative (the rule of
 * qf_rank_batch) and drops any other one, returning 0.  The decision is made
 * on the host against an incremental basis of at most k * k bytes (the
 * elimination of qf_gf256_rank), no device call per packet.  The k rows kept
 * are then independent, so the generation decodes when the rank reaches k.  A
 * systematic packet dropped because coded packets already span it is
 * reconstructed like any erased source (out_ids[i] = i).  QF_EINVAL for NULL,
 * for k > 256 decoders and once a packet has been accepted. */
int qf_decoder_set_innovative(qf_decoder *dec, int on);
/* Rank of the packets accepted so far (0..k).  With the mode on it is the
 * number of accepted packets; with the mode off it is computed on the host
 * from the stored rows on each call.  QF_EINVAL for NULL and k > 256. */
int qf_decoder_rank(const qf_decoder *dec);
int qf_decoder_free(qf_decoder *dec);
/* replaces decoder.rs:678 Decoder::add_packet.  Returns 1 when the generation
 * is decoded, 0 when more packets are needed, QF_EINVAL for a repair packet
 * without coefficients ("Repair packet missing coefficients.").  A singular
 * matrix leaves the decoder undecoded, as in the reference. */
int qf_decoder_add_packet(qf_decoder *dec, uint64_t id, int is_systematic,
                          const uint8_t *data, uint32_t len, const uint8_t *coeffs,
                          uint32_t coeff_len);
/* replaces the decoder.rs:532 field is_decoded */
int qf_decoder_is_decoded(const qf_decoder *dec);
/* replaces decoder.rs:785 get_decoded_packets: drains the k source packets in
 * index order.  out_data holds k rows of out_stride bytes; out_len[i] and
 * out_ids[i] describe row i; *count = number of packets returned (k, or 0 if
 * not decoded or already drained). */
int qf_decoder_get_decoded_packets(qf_decoder *dec, uint8_t *out_data, uint32_t out_stride,
                                   uint32_t *out_len, uint64_t *out_ids, uint32_t *count);

/* ---------------------------------------------------------------------------
 * Adaptive FEC driver (adaptive.rs:44-631, mod.rs:56-79): loss estimator
 * (EMA + burst window + optional Kalman filter), PID-driven mode manager with
 * dwell time, hysteresis, emergency override and dynamic window, and the
 * per-connection sliding-window codec with a 32-packet cross-fade between
 * configurations.  The arithmetic is f32 exactly as the reference (no FP
 * contraction).  Time is in seconds on a monotonic clock; the *_at variants
 * take it explicitly (deterministic tests), the others read CLOCK_MONOTONIC.
 *
 * Codec: the GF(2^8) encoder/decoder objects above, and in Extreme mode the
 * GF(2^16) ones (decoder.rs:96-102; coefficient blocks of 2k bytes, so
 * coeff_stride >= 2k there).  A configuration the field cannot realise
 * (GF(2^8): k + r > 256, where the reference panics in gf_inv(0); GF(2^16):
 * k > 4096 or n > 65536) has no codec: on_send still emits the systematic
 * packet and returns QF_ERANGE.
 * ------------------------------------------------------------------------- */
#define QF_MODE_ZERO 0
#define QF_MODE_LIGHT 1
#define QF_MODE_NORMAL 2
#define QF_MODE_MEDIUM 3
#define QF_MODE_STRONG 4
#define QF_MODE_EXTREME 5
#define QF_CROSS_FADE_LEN 32   /* ModeManager::CROSS_FADE_LEN (adaptive.rs:114) */

typedef struct qf_fec_config {   /* FecConfig (adaptive.rs:338-349) */
    float lambda;                /* EMA smoothing factor */
    uint32_t burst_window;       /* burst-detection window (packets) */
    float hysteresis;
    float kp, ki, kd;            /* PidConfig */
    int32_t initial_mode;
    int32_t kalman_enabled;
    float kalman_q, kalman_r;
    uint32_t window_sizes[6];    /* initial window W0 per mode */
    uint32_t max_len;            /* payload capacity of the codec objects (bytes) */
} qf_fec_config;

/* FecConfig::default (adaptive.rs:435-452) + default_windows (352-362);
 * max_len = 1500. */
void qf_fec_config_default(qf_fec_config *cfg);
/* FecConfig::validate (adaptive.rs:455-471): QF_EINVAL on a bad field. */
int qf_fec_config_validate(const qf_fec_config *cfg);
/* ModeManager::params_for (adaptive.rs:149-153): k = window,
 * n = ceil(window * overhead_ratio(mode)) in f32. */
int qf_mode_params_for(int32_t mode, uint32_t window, uint32_t *k, uint32_t *n);
/* ModeManager::window_range (adaptive.rs:124-133). */
int qf_mode_window_range(int32_t mode, uint32_t *lo, uint32_t *hi);
/* ModeManager::overhead_ratio (adaptive.rs:135-147). */
float qf_mode_overhead_ratio(int32_t mode);

typedef struct qf_packet_desc {
    uint64_t id;
    uint32_t len;            /* payload bytes */
    uint32_t coeff_len;      /* coefficient bytes of a repair packet, else 0 */
    int32_t is_systematic;
    uint32_t reserved;
} qf_packet_desc;

typedef struct qf_adaptive qf_adaptive;
/* AdaptiveFec::new (adaptive.rs:473-508).  ctx may be NULL: controller only
 * (no codec objects; on_send emits the systematic packet, on_receive
 * recovers nothing) -- the mode logic then runs without a GPU. */
int qf_adaptive_new(qf_ctx *ctx, const qf_fec_config *cfg, qf_adaptive **out);
int qf_adaptive_new_at(qf_ctx *ctx, const qf_fec_config *cfg, double now_s, qf_adaptive **out);
int qf_adaptive_free(qf_adaptive *a);
/* current_mode / is_transitioning (adaptive.rs:510-517) and the rest of the
 * controller state (any pointer may be NULL). */
int qf_adaptive_state(const qf_adaptive *a, int32_t *mode, uint32_t *window, uint32_t *k,
                      uint32_t *n, int32_t *transitioning, uint32_t *transition_left,
                      float *estimated_loss);
/* Largest number of packets one on_send can emit (1 + repairs of the
 * current and the cross-fade configuration). */
uint32_t qf_adaptive_max_send_packets(const qf_adaptive *a);
/* Largest number of packets one on_receive can recover: the k of the
 * current decoder plus the k of the cross-fade decoder (both may complete
 * on the same packet, adaptive.rs:566-599).  A host sizes its reusable
 * receive buffers from it (INTEGRATION.md AdaptiveFec). */
uint32_t qf_adaptive_max_receive_packets(const qf_adaptive *a);
/* Smallest coeff_stride on_send accepts for the current and cross-fade
 * encoders: k bytes (GF(2^8)) or 2 k bytes (GF(2^16) Extreme windows). */
uint32_t qf_adaptive_max_coeff_bytes(const qf_adaptive *a);
/* AdaptiveFec::on_send (adaptive.rs:519-544) + emit_repairs (546-562): the
 * systematic packet, then the cross-fade configuration's repairs (while more
 * than CROSS_FADE_LEN/2 packets of the fade remain), then the current
 * configuration's repairs.  Packet i goes to out_data + i*out_stride (and
 * its coefficients to out_coeffs + i*coeff_stride); *n_out packets.
 * QF_ETOOSMALL if out_cap is too small (nothing is consumed then). */
int qf_adaptive_on_send(qf_adaptive *a, uint64_t id, const uint8_t *data, uint32_t len,
                        uint8_t *out_data, uint32_t out_stride, uint8_t *out_coeffs,
                        uint32_t coeff_stride, qf_packet_desc *out_desc, uint32_t out_cap,
                        uint32_t *n_out);
/* on_send for M connections at once (the server side of many QUIC
 * connections, core.rs:170-188 per packet): conns[m] sends packet (ids[m],
 * data[m], lens[m]).  The result is that of calling qf_adaptive_on_send for
 * m = 0..M-1 in order -- connection m's packets occupy out_data rows
 * [first_m, first_m + n_out[m]) with first_m = n_out[0] + ... + n_out[m-1],
 * and statuses[m] (nullable) gets that call's status -- but the steady-state
 * GF(2^8) connections of one context share one upload, one small-batch
 * encode launch per (k, n) class and one download.  A connection may appear
 * more than once (its packets are taken in order): a burst of one
 * connection's packets is one launch too, its overlapping windows read from
 * a staging copy of the ring's newest k - 1 rows and the burst (Normal mode,
 * 1,200-B packets: 18.5 us per packet alone, 1.2 us at 256 per call).  out_cap must cover the
 * sum of qf_adaptive_max_send_packets; out_stride / coeff_stride follow
 * qf_adaptive_on_send.  An argument error fails the whole call before any
 * state changes (QF_EINVAL / QF_ETOOSMALL); otherwise QF_OK. */
int qf_adaptive_on_send_batch(qf_adaptive *const *conns, uint32_t M, const uint64_t *ids,
                              const uint8_t *const *data, const uint32_t *lens, uint8_t *out_data,
                              uint32_t out_stride, uint8_t *out_coeffs, uint32_t coeff_stride,
                              qf_packet_desc *out_desc, uint32_t out_cap, uint32_t *n_out,
                              int32_t *statuses);
/* AdaptiveFec::on_receive (adaptive.rs:566-599): recovered packets (the
 * whole generation when a decoder completes, in source order: a received
 * systematic packet keeps its id, a reconstructed one gets id = i,
 * decoder.rs:688/771).  QF_EINVAL for a repair packet without coefficients. */
int qf_adaptive_on_receive(qf_adaptive *a, uint64_t id, int is_systematic, const uint8_t *data,
                           uint32_t len, const uint8_t *coeffs, uint32_t coeff_len,
                           uint8_t *out_data, uint32_t out_stride, qf_packet_desc *out_desc,
                           uint32_t out_cap, uint32_t *n_out);
/* on_receive for M connections at once: conns[m] receives packet m (ids,
 * is_systematic, data/lens, coeffs/coeff_lens: coeffs and coeff_lens may be
 * NULL when no packet carries coefficients).  The result is that of calling
 * qf_adaptive_on_receive for m = 0..M-1 in order -- connection m's recovered
 * packets occupy out_data rows [first_m, first_m + n_out[m]), first_m =
 * n_out[0] + ... + n_out[m-1], statuses[m] (nullable) gets that call's status
 * (e.g. QF_EINVAL for a repair without coefficients; such a packet is
 * dropped and the batch goes on) -- but the GF(2^8) decoders of one context
 * take their rows in one upload, and the generations that complete in the
 * call decode in one heterogeneous decode with one download.  out_cap must
 * cover the sum over connections of their decoders' k (the most one
 * on_receive can recover).  An argument error fails the whole call before any
 * state changes. */
int qf_adaptive_on_receive_batch(qf_adaptive *const *conns, uint32_t M, const uint64_t *ids,
                                 const int32_t *is_systematic, const uint8_t *const *data,
                                 const uint32_t *lens, const uint8_t *const *coeffs,
                                 const uint32_t *coeff_lens, uint8_t *out_data, uint32_t out_stride,
                                 qf_packet_desc *out_desc, uint32_t out_cap, uint32_t *n_out,
                                 int32_t *statuses);
/* AdaptiveFec::report_loss (adaptive.rs:602-630).  QF_EINVAL if lost > total
 * (the reference underflows). */
int qf_adaptive_report_loss(qf_adaptive *a, uint32_t lost, uint32_t total);
int qf_adaptive_report_loss_at(qf_adaptive *a, uint32_t lost, uint32_t total, double now_s);

/* ---------------------------------------------------------------------------
 * Wire framing, byte-compatible with encoder.rs:124-152 (to_raw) and
 * encoder.rs:18-68 (from_raw): [u8 sys(1/0)] [u16 BE coeff_len][coeffs] payload
 * (the coefficient header is present only when coeffs != NULL).
 * ------------------------------------------------------------------------- */
int qf_packet_to_raw(int is_systematic, const uint8_t *coeffs, uint32_t coeff_len,
                     const uint8_t *payload, uint32_t len, uint8_t *out, uint32_t out_cap,
                     uint32_t *out_len);
/* Parses a frame; pointers returned point into raw.  coeffs is NULL for
 * systematic frames. */
int qf_packet_from_raw(const uint8_t *raw, uint32_t raw_len, int *is_systematic,
                       const uint8_t **coeffs, uint32_t *coeff_len,
                       const uint8_t **payload, uint32_t *len);
/* replaces Packet::from_block (encoder.rs:72-121), the receive path of
 * core.rs:219-224: a frame of `len` valid bytes in a block of block_len bytes
 * is parsed in place; the coefficients are copied to coeffs_out (coeffs_cap
 * bytes) and the payload is moved to the front of the block (copy_within).
 * QF_EINVAL: len == 0 or len > block_len ("Invalid raw packet length");
 * QF_ETOOSMALL: coefficient length or coefficients truncated, or longer than
 * coeffs_cap / the block (where the reference would panic). */
int qf_packet_from_block(uint8_t *block, uint32_t block_len, uint32_t len, int *is_systematic,
                         uint8_t *coeffs_out, uint32_t coeffs_cap, uint32_t *coeff_len,
                         uint32_t *payload_len);

/* ---------------------------------------------------------------------------
 * Wire framing on the device (encoder.rs:18-152): the
 * step between UDP datagrams and the batch codec.
 * ------------------------------------------------------------------------- */
/* Frames of an encode batch, as Packet::to_raw writes them (encoder.rs:124-152):
 * generation g's k sources then its r repairs, frame f = g*(k+r) + i at
 * frames_dev + f*frame_stride:
 *   source i  0x01 | payload (L bytes)                                1 + L bytes
 *   repair j  0x00 | k as BE u16 | C[j][0..k) | payload (L bytes)     3 + k + L bytes
 * with C the reference's Cauchy rows (decoder.rs:280-298).  frame_len_dev
 * (may be NULL) receives each frame's length.  frame_stride % 16 == 0,
 * >= 3 + k + L; bytes of a frame past its length are not written. */
int qf_frame_batch_dev(qf_ctx *ctx, const qf_encode_shape *shape, uint32_t G, const uint8_t *src_dev,
                       const uint8_t *rep_dev, uint8_t *frames_dev, uint64_t frame_stride,
                       uint32_t *frame_len_dev);
/* Received frames -> qf_decode_batch input (Packet::from_raw, encoder.rs:18-68,
 * then Decoder::add_packet's column rule, decoder.rs:684).  Frame s of
 * generation g: frames_dev + (g*max_rows + s)*frame_stride, frame_len_dev[g*max_rows+s]
 * bytes, transport id ids_dev[g*max_rows+s]; n_frames_dev[g] frames (NULL: max_rows).
 * Valid frames are compacted in arrival order into rows_dev (payload zero
 * padded to L) with row_index_dev = id % k for a systematic frame, k + j for a
 * repair whose coefficient vector is Cauchy row j < r; n_rows_dev[g] = their
 * count.  frame_status_dev: QF_OK, QF_EINVAL (empty, payload > L),
 * QF_ETOOSMALL (coefficient length or coefficients truncated), QF_ERANGE
 * (coefficients are not a Cauchy row of this (k, r)).  max_rows <= 1024. */
int qf_parse_frames_dev(qf_ctx *ctx, uint32_t k, uint32_t r, uint32_t L, uint32_t G, uint32_t max_rows,
                        const uint8_t *frames_dev, uint64_t frame_stride, const uint32_t *frame_len_dev,
                        const uint64_t *ids_dev, const uint32_t *n_frames_dev, uint8_t *rows_dev,
                        uint64_t row_stride, uint64_t rows_gen_stride, uint16_t *row_index_dev,
                        uint32_t *n_rows_dev, int32_t *frame_status_dev);

/* ---------------------------------------------------------------------------
 * Device framing of coded rows that carry their coefficient vectors: the wire
 * step of a relay (qf_recode_batch) and of a receiver of recoded traffic
 * (qf_decode_innovative_batch).  The two calls above frame and accept Cauchy
 * repairs only.
 *
 * The payload-aligned layout: a frame slot is frame_stride bytes,
 * frame_stride % 16 == 0 and >= P + L with P = qf_frame_payload_offset(k) =
 * round_up(3 + k, 16).  The payload of every frame sits at byte P of its slot,
 * whatever the frame's kind, and the frame's bytes (Packet::to_raw,
 * encoder.rs:124-152) directly in front of it:
 *   systematic  starts at slot byte P - 1:      0x01 | payload
 *   coded       starts at slot byte P - 3 - k:  0x00 | k as BE u16 | k coefficient bytes | payload
 * A sender transmits frame_len bytes starting at frame_off.  The payload
 * position is 16-byte aligned and does not depend on the kind, so the payload
 * kernels write straight into frame slots: qf_recode_batch with out_dev =
 * frames_dev + P, out_row_stride = frame_stride and out_gen_stride = m *
 * frame_stride, and framing then costs the header bytes only.
 *
 * Relay step, frames in and frames out, all on the device:
 *   qf_parse_frames_coded_dev   frames -> rows, row_index, n_rows, row_coeffs
 *   qf_recode_batch             m fresh rows per generation, written into the frame slots
 *   qf_frame_rows_dev           QF_FRAME_IN_PLACE, row_index NULL, row_coeffs = out_coeffs_dev
 * The same step without the copy of the payloads out of their slots (the
 * received frames in this layout, so every payload starts at a multiple of 16):
 *   qf_parse_frame_headers_dev  frames -> row_off, row_len, row_index, n_rows, row_coeffs
 *   qf_recode_frames_dev        src_dev = frames_in, src_gen_stride = max_rows * frame_stride,
 *                               out_dev = frames_out + P; out_len_dev = the rows' lengths
 *   qf_frame_rows_dev           QF_FRAME_IN_PLACE, row_len_dev = out_len_dev
 * Receiver:
 *   qf_parse_frames_coded_dev   then qf_decode_innovative_batch on its outputs
 * The same without the copy of the payloads out of their slots (the faster
 * receiver sequence for rows under 2,017 bytes; the one above from there on):
 *   qf_parse_frame_headers_dev  then qf_decode_frames_dev with src_dev = frames_in,
 *                               src_gen_stride = max_rows * frame_stride
 * Streaming receiver or relay, a few frames of many generations per poll:
 *   qf_parse_frame_headers_dev  the poll's frames -> row_off, row_len, row_index, n_rows, row_coeffs
 *   qf_rank_update_batch        the same rows against the generations' rank states -> innovative, rank
 *   qf_store_append_dev         take_dev = innovative: the new rows join the generations' stores
 * and, once rank_dev[g] reaches k (a relay may recode sooner):
 *   qf_decode_frames_dev        over the store arrays, max_rows = cap, src_gen_stride = store_gen_stride
 *   qf_recode_frames_dev        the same at a relay (cap <= 255)
 * The same from a flat poll (frames in arrival order, one generation tag per
 * frame), touching the poll's generations only and with no host sort:
 *   qf_parse_poll_headers_dev   the flat poll -> the list of touched generations and, per entry,
 *                               row_off, row_len, row_index, n_rows, row_coeffs
 *   qf_rank_update_sel_batch    the listed generations' rank states; rank_dev is persistent
 *   qf_store_append_sel_dev     src_dev = the flat poll's frames_dev
 * then qf_gen_select_dev over the persistent rank_dev, the listed decode or
 * recode, and qf_stream_reset_dev twice: once for state_dev, store_n_dev and
 * seen_dev, once more with seen_dev = rank_dev (the other two NULL), which
 * clears the listed generations' ranks.
 * The send step of a relay, behind the append: qf_gen_select_dev(rank_dev,
 * seen_dev = sent_dev, min_rank 1, flags 0) lists the generations with budget
 * left, then
 *   qf_recode_frames_sel_dev    m fresh combinations per listed generation, compact by list position
 *   qf_gen_window_sel_dev       flags 0: the listed generations' wire ids
 *   qf_emit_frames_sel_dev      the first min(m, rank - sent) rows of each as frames, one behind the
 *                               other in a flat queue; sent_dev grows by what was emitted
 * and the queue's arrays are the flat poll of the next hop.  A source emits its
 * packets as systematic rows, then its repairs with QF_EMIT_APPEND.
 * Over a lossy hop qf_credit_update_dev runs in front of that select and its
 * credit_dev stands where rank_dev stood in the select and in the emit; the
 * receiver writes the reports it reads with qf_rank_report_sel_dev over the
 * completed list and, appended, over the list of qf_gen_select_dev(rank_dev,
 * NULL, min_rank 1, flags 0), after its resets.
 * The intermediate rows belong to the caller.
 * ------------------------------------------------------------------------- */
/* No reference counterpart (a layout rule): P = round_up(3 + k, 16) for k in
 * 1..256, 0 otherwise.  Host only, no device. */
uint32_t qf_frame_payload_offset(uint32_t k);

#define QF_FRAME_IN_PLACE 1u   /* the payloads already sit at byte P of their slots */

typedef struct qf_frame_rows_shape {
    uint32_t k;              /* generation size, 1..256 */
    uint32_t r;              /* Cauchy repairs that may appear when row_coeffs_dev is NULL */
    uint32_t L;              /* payload bytes per row at most, >= 1 */
    uint32_t max_rows;       /* slots per generation, 1..1024 */
    uint32_t flags;          /* 0 or QF_FRAME_IN_PLACE */
    uint32_t reserved;       /* 0 */
    uint64_t row_stride;     /* inputs, as qf_decode_shape; not read in place */
    uint64_t rows_gen_stride;
    uint64_t frame_stride;   /* % 16 == 0, >= P + L */
} qf_frame_rows_shape;

/* Rows with index and vector -> frames (replaces Packet::to_raw,
 * encoder.rs:124-152, per row of a batch; the batch itself has no reference
 * counterpart).  rows_dev, row_index_dev, n_rows_dev (NULL: max_rows) and
 * row_coeffs_dev (nullable) are laid out as for qf_decode_batch and
 * qf_recode_batch; row_index_dev NULL means every row is coded, which with
 * max_rows = m and row_coeffs_dev = out_coeffs_dev is the recoder's output.
 * row_len_dev (nullable, one u32 per slot) is the payload bytes of the row;
 * NULL means L.  Frame f = g*max_rows + s goes to frames_dev + f*frame_stride
 * in the layout above; frame_len_dev[f] (required) and frame_off_dev[f]
 * (nullable) receive its length and its start inside the slot.  The vector of
 * a slot is v(s) of qf_recode_batch: index < k a systematic frame (no vector
 * is read); index >= k the k bytes at (g*max_rows + s)*k of row_coeffs_dev,
 * or without row_coeffs_dev Cauchy row index - k of (k, r).
 * A slot gets frame_len = 0 (frame_off = 0) and no byte written when s >= n,
 * when its row_len > L, or when its index >= k has neither a vector nor
 * index - k < r.
 * flags 0: the payload is copied from rows_dev to byte P of the slot (16-byte
 * loads and stores).  QF_FRAME_IN_PLACE: the payloads already sit there,
 * rows_dev is ignored (may be NULL) and only the header bytes are written.
 * In both modes no byte of a slot outside [frame_off, frame_off + frame_len)
 * is written.
 * Returns QF_EINVAL for k outside 1..256, max_rows outside 1..1024, L == 0,
 * unknown flags, reserved != 0, a NULL required pointer, pointers or strides
 * not 16-byte aligned, a row stride shorter than L or frame_stride < P + L;
 * QF_ERANGE for NULL row_coeffs_dev with r > 0 and k + r > 256.  G == 0 is
 * QF_OK. */
int qf_frame_rows_dev(qf_ctx *ctx, const qf_frame_rows_shape *shape, uint32_t G,
                      const uint8_t *rows_dev, const uint16_t *row_index_dev,
                      const uint32_t *n_rows_dev, const uint8_t *row_coeffs_dev,
                      const uint32_t *row_len_dev, uint8_t *frames_dev,
                      uint32_t *frame_len_dev, uint32_t *frame_off_dev);

/* Received frames -> rows plus row_coeffs, the input of qf_recode_batch,
 * qf_rank_batch and qf_decode_innovative_batch (Packet::from_raw,
 * encoder.rs:18-68, then Decoder::add_packet's column rule, decoder.rs:684,
 * which takes any coefficient vector, decoder.rs:694-696).  Arguments as
 * qf_parse_frames_dev without r, plus:
 *   frame_off_dev   (nullable) the start of frame s inside its slot, so the
 *                   output of qf_frame_rows_dev parses directly; NULL means 0
 *   row_coeffs_dev  (required) k bytes per output slot at (g*max_rows + slot)*k
 *   row_len_dev     (nullable) the payload bytes of the row before zero padding
 * A systematic frame gives row_index = id % k and the unit vector of that
 * column, so row_coeffs_dev is fully defined.  A repair frame whose
 * coefficient length is k is accepted whatever its vector (an all-zero vector
 * is a legal row; the rank filter drops it): row_index = k and the k bytes
 * are copied.  frame_status_dev: QF_OK; QF_EINVAL (empty, frame_off +
 * frame_len > frame_stride, payload > L); QF_ETOOSMALL (coefficient length or
 * coefficients truncated); QF_ERANGE (coefficient length other than k).
 * Valid frames are compacted in arrival order and zero padded to L, with
 * n_rows_dev[g] their count; output slots >= n_rows_dev[g] are not written.
 * No byte outside [slot, slot + frame_stride) of a frame is read.
 * k 1..256, max_rows 1..1024; alignment rules and call-level errors as
 * qf_parse_frames_dev, with row_coeffs_dev among the required pointers. */
int qf_parse_frames_coded_dev(qf_ctx *ctx, uint32_t k, uint32_t L, uint32_t G, uint32_t max_rows,
                              const uint8_t *frames_dev, uint64_t frame_stride,
                              const uint32_t *frame_len_dev, const uint32_t *frame_off_dev,
                              const uint64_t *ids_dev, const uint32_t *n_frames_dev,
                              uint8_t *rows_dev, uint64_t row_stride, uint64_t rows_gen_stride,
                              uint16_t *row_index_dev, uint32_t *n_rows_dev, uint8_t *row_coeffs_dev,
                              uint32_t *row_len_dev, int32_t *frame_status_dev);

/* qf_parse_frames_coded_dev that reads the headers only and leaves every
 * payload in its slot, for qf_recode_frames_dev.  No reference counterpart
 * beyond that call's.  Arguments as qf_parse_frames_coded_dev without
 * rows_dev, row_stride and rows_gen_stride, with row_len_dev required, plus:
 *   row_off_dev  (required) one u32 per output slot at g*max_rows + c: the
 *                byte offset of compacted row c's payload from the start of
 *                generation g's frame region, frames_dev + g*max_rows*
 *                frame_stride; that is slot*frame_stride + frame_off + 1 for a
 *                systematic frame and + 3 + k for a coded one
 * row_index_dev, n_rows_dev, row_coeffs_dev, row_len_dev and frame_status_dev
 * receive exactly what qf_parse_frames_coded_dev writes for the same frames
 * (valid frames compacted in arrival order, output slots >= n_rows_dev[g] not
 * written), with one more per-frame status: a frame that is otherwise valid
 * but whose payload does not start at a multiple of 16 in its slot is
 * QF_EINVAL and is not compacted (never the case in the payload-aligned
 * layout).
 * No payload byte is read: at most the 3 header bytes and the k vector bytes
 * of a frame, all inside [slot, slot + frame_stride).
 * k 1..256, max_rows 1..1024; alignment rules and call-level errors as
 * qf_parse_frames_coded_dev, with row_len_dev and row_off_dev among the
 * required pointers, and QF_EINVAL when max_rows * frame_stride > 2^32 (the
 * offsets are u32). */
int qf_parse_frame_headers_dev(qf_ctx *ctx, uint32_t k, uint32_t L, uint32_t G, uint32_t max_rows,
                               const uint8_t *frames_dev, uint64_t frame_stride,
                               const uint32_t *frame_len_dev, const uint32_t *frame_off_dev,
                               const uint64_t *ids_dev, const uint32_t *n_frames_dev,
                               uint16_t *row_index_dev, uint32_t *n_rows_dev, uint8_t *row_coeffs_dev,
                               uint32_t *row_len_dev, uint32_t *row_off_dev, int32_t *frame_status_dev);

/* ---------------------------------------------------------------------------
 * GF(2^16) "Extreme mode" codec.
 * replaces gf_tables.rs:331-380 (gf16_mul / gf16_pow / gf16_inv / gf16_mul_add)
 * and decoder.rs:10-88 (Encoder16), 536-656 (Decoder16).  Field mod 0x1100B
 * with the reduction gf16_mul intends (as written its u16 test of bit 16
 * never fires).  Payload symbols are big-endian u16 byte pairs
 * (decoder.rs:42-54); L must be even.
 * ------------------------------------------------------------------------- */
/* gf_tables.rs:333 gf16_mul (host helper) */
uint16_t qf_gf16_mul(uint16_t a, uint16_t b);
/* gf_tables.rs:370 gf16_inv; QF_ERANGE for 0 (the reference panics) */
int qf_gf16_inv(uint16_t a, uint16_t *out);
/* decoder.rs:77-80: out[j*k + i] = gf16_inv((u16)i ^ (u16)(k + j));
 * QF_ERANGE when k + r > 65536 (gf16_inv(0)). */
int qf_cauchy16_coeffs(uint32_t k, uint32_t r, uint16_t *out_rxk);
/* replaces decoder.rs:21-75 Encoder16::generate_repair_packet for r repairs
 * of G generations (layout as qf_encode_batch, shape->flags must be 0);
 * coeff_rxk: host u16 r x k matrix or NULL for the Cauchy rows. */
int qf_encode16_batch(qf_ctx *ctx, const qf_encode_shape *shape, uint32_t G, const uint8_t *src_dev,
                      uint8_t *rep_dev, const uint16_t *coeff_rxk);
/* replaces decoder.rs:563-656 Decoder16::{add_packet, try_decode,
 * get_decoded_packets} for G generations (layout as qf_decode_batch).
 * Acceptance as Decoder16: the first k rows, row index < k = systematic
 * column (the reference's id % k), no duplicate filtering (a duplicated
 * column is singular: QF_ERANK).  row_coeffs_dev: NULL (row index k + j
 * carries Cauchy row j) or k u16 per slot at (g*max_rows + slot)*k (the
 * packet's big-endian coefficient block, converted).  r sizes the output:
 * up to min(k, r) erasures per generation (QF_ERANGE status beyond).
 * min(k, r) <= 64: all generations at once (Gauss-Jordan in LDS); larger:
 * one generation at a time (closed-form Cauchy inverse, or Gauss-Jordan in
 * the workspace for explicit coefficients).  k <= 4096, r >= 1,
 * max_rows <= 65536 (QF_EINVAL beyond).  Recovered rows: erased sources
 * ascending, with rec_index / n_rec / status as qf_decode_batch. */
int qf_decode16_batch(qf_ctx *ctx, const qf_decode_shape *shape, uint32_t G, const uint8_t *rows_dev,
                      const uint16_t *row_index_dev, const uint32_t *n_rows_dev,
                      const uint16_t *row_coeffs_dev, uint8_t *rec_dev, uint16_t *rec_index_dev,
                      uint32_t *n_rec_dev, int32_t *status_dev);

/* GF(2^16) per-connection objects (the Extreme-mode codec of
 * EncoderVariant / DecoderVariant, decoder.rs:90-153).  k <= 4096 (Extreme
 * windows, adaptive.rs:131).  Coefficient blocks are 2k bytes, big-endian u16
 * (decoder.rs:62-66). */
typedef struct qf_encoder16 qf_encoder16;
/* replaces decoder.rs:17 Encoder16::new(k, n) */
int qf_encoder16_new(qf_ctx *ctx, uint32_t k, uint32_t n, uint32_t max_len, qf_encoder16 **out);
int qf_encoder16_free(qf_encoder16 *enc);
/* replaces decoder.rs:25 Encoder16::add_source_packet (slides the window) */
int qf_encoder16_add_source_packet(qf_encoder16 *enc, uint64_t id, const uint8_t *data, uint32_t len);
/* replaces decoder.rs:33 Encoder16::generate_repair_packet(j): QF_ENOTREADY
 * while the window is not full (None); len = window[0].len (an odd last
 * byte is 0, decoder.rs:44); out_coeffs 2k bytes; id = last.id + 1 + j. */
int qf_encoder16_generate_repair_packet(qf_encoder16 *enc, uint32_t repair_index, uint8_t *out_data,
                                        uint32_t out_cap, uint32_t *out_len, uint8_t *out_coeffs,
                                        uint64_t *out_id);
/* Repairs first..first+count-1 of the window in one launch; coefficient
 * blocks packed 2k bytes apart.  QF_ERANGE when k + first + count > 65536. */
int qf_encoder16_generate_repairs(qf_encoder16 *enc, uint32_t first, uint32_t count, uint8_t *out_data,
                                  uint32_t out_stride, uint32_t *out_len, uint8_t *out_coeffs,
                                  uint64_t *out_ids);
int qf_encoder16_window_len(const qf_encoder16 *enc);
typedef struct qf_decoder16 qf_decoder16;
/* replaces decoder.rs:545 Decoder16::new(k, pool) */
int qf_decoder16_new(qf_ctx *ctx, uint32_t k, uint32_t max_len, qf_decoder16 **out);
int qf_decoder16_free(qf_decoder16 *dec);
/* replaces decoder.rs:555 Decoder16::add_packet: the first k packets are the
 * system (no duplicate filtering); decoding runs when the k-th arrives
 * (whatever its kind).  1 = decoded, 0 = not (yet, or singular: stays so),
 * QF_EINVAL for a repair without coefficients ("missing coeffs"). */
int qf_decoder16_add_packet(qf_decoder16 *dec, uint64_t id, int is_systematic, const uint8_t *data,
                            uint32_t len, const uint8_t *coeffs, uint32_t coeff_len);
int qf_decoder16_is_decoded(const qf_decoder16 *dec);
/* replaces decoder.rs:643 get_decoded_packets: drains the k source packets in
 * index order (as qf_decoder_get_decoded_packets). */
int qf_decoder16_get_decoded_packets(qf_decoder16 *dec, uint8_t *out_data, uint32_t out_stride,
                                     uint32_t *out_len, uint64_t *out_ids, uint32_t *count);

/* ---------------------------------------------------------------------------
 * Synthetic payload (bench / tests): byte t of the region is byte (t & 7) of
 * splitmix64(seed + word_offset + t/8), little endian.  Device kernel.
 * ------------------------------------------------------------------------- */
int qf_fill_splitmix_dev(qf_ctx *ctx, uint8_t *dst_dev, size_t n, uint64_t seed,
                         uint64_t word_offset);

/* ---------------------------------------------------------------------------
 * Host self-test of the split-index v_perm tables the kernels use: checks
 * T0[x&7]^T1[x>>3&7]^T2[x>>6] == gf_mul_table(c, x) for all 65,536 (c, x)
 * with a host emulation of v_perm_b32.  Returns QF_OK or QF_EINVAL.
 * ------------------------------------------------------------------------- */
int qf_selftest_split_tables(void);

#ifdef __cplusplus
}
#endif
#endif /* QF_FEC_H */
