// qf_internal.h -- context services for the library's other translation
// units (defined in qf_api.hip; not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <string>
#include <vector>

#include "qf_fec.h"

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline uint64_t round_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }

namespace qf {

// Locks the context and makes its device current.
int ctx_lock(qf_ctx* ctx, std::unique_lock<std::mutex>& lk);
hipStream_t ctx_stream(qf_ctx* ctx);
int ctx_num_cus(qf_ctx* ctx);
// The context's device workspace, grown to at least `bytes` (shared with the
// decode paths; valid until the next call on this context).
int ctx_work(qf_ctx* ctx, size_t bytes, uint8_t** out);
// GF(2^16) tables on the device, built on first use: log[65536] (log[0] =
// 0xFFFF, no product) and exp[2 * 65535] (exp[i + 65535] = exp[i]).
int ctx_gf16_tables(qf_ctx* ctx, const uint16_t** log, const uint16_t** exp);
// The Zech logarithms Z[d] = log(1 + alpha^d) of the same field, 65,536 entries
// (Z[0] and Z[65535] = 0xFFFF, log 0), beside the log table.
int ctx_gf16_zech(qf_ctx* ctx, const uint16_t** zech);
// The context's 256 split-table records (8 dwords each, gf256_tables.h).
const uint32_t* ctx_tab256(qf_ctx* ctx);
// A device buffer of >= bytes for GF(2^16) input rows in log form (its own
// allocation, so it can sit beside the workspace; valid until the next call).
int ctx_gf16_logrows(qf_ctx* ctx, size_t bytes, uint8_t** out);
// The context's exp[512] | log[256] tables of GF(2^8) on the device.
const uint8_t* ctx_explog(qf_ctx* ctx);
// One 16-output payload pass over coefficient records, on the kernel the
// decode paths would pick for the shape (k_combine_slots, its split variant
// for small batches, or the bit-sliced qf_combine_bs for long rows; prefetch
// depth from QF_OPT_DECODE_PD); *name receives the kernel's profile name.
struct CombineSlotsArgs;
hipError_t ctx_combine_payload(qf_ctx* ctx, const CombineSlotsArgs& a, hipStream_t st, std::string* name);
// Drops a pending qf_ctx_set_payload_stream / qf_ctx_set_payload_wait (they
// apply to qf_decode_batch only; the other decode calls clear them).  Takes
// the context lock.
void ctx_clear_payload_split(qf_ctx* ctx);
// The context's value of option `opt` (QF_OPT_*, qf_ctx_set_option).
int64_t ctx_opt(qf_ctx* ctx, int opt);
// qf_ctx_profile bracketing of a launch (QF_PROFILED below).
hipEvent_t ctx_prof_begin(qf_ctx* ctx, hipStream_t st);
void ctx_prof_end(qf_ctx* ctx, hipStream_t st, hipEvent_t ev, const std::string& name);

// The parts of one call's device workspace, each at a multiple of 256 bytes:
// take() in layout order, then one ctx_work(size()) for all of them.
struct WorkLayout {
    size_t end = 0;
    size_t take(size_t bytes) {
        const size_t off = round_up(end, 256);
        end = off + bytes;
        return off;
    }
    size_t size() const { return end; }
};

// A batch's rows described where they lie: row s of generation g is len bytes
// at off from the generation's source region, with its index and coefficient
// vector ([G][max_rows] each, coeffs [G][max_rows][k]) and n_rows[G] (nullptr:
// max_rows).  off / len are nullptr for the calls that read no payload.
struct RowArrays {
    const uint32_t* off;
    const uint32_t* len;
    const uint16_t* index;
    const uint32_t* n_rows;
    const uint8_t* coeffs;
};

// QF_LOCAL keeps a function that several translation units share out of the
// library's dynamic symbols, so that the exported list stays what it was (the
// older internals of this header predate it and are still exported).
#define QF_LOCAL __attribute__((visibility("hidden")))
// k_rank_filter over the rows, or with state != nullptr the walk resumed from
// and written back to the rank states (k_rank_update).  (qf_rank.hip)
QF_LOCAL hipError_t launch_rank(qf_ctx* ctx, const RowArrays& rows, uint32_t k, uint32_t r, uint32_t max_rows,
                                uint32_t G, uint8_t* state, uint8_t* innovative, uint32_t* rank, int32_t* status,
                                hipStream_t st);
// The two kernels of qf_gen_select_dev over any device array of G <= 2^24
// counts, without the seen condition: the first n_max entries >= min_rank,
// ascending, to sel, their number to *n_sel and the number of all to *n_match
// (nullable).  counts: gen_select_work_bytes(G) bytes of scratch.
// (qf_select.hip; the flat poll's list, qf_poll.hip)
QF_LOCAL size_t gen_select_work_bytes(uint32_t G);
QF_LOCAL hipError_t launch_gen_select_list(const uint32_t* rank, uint32_t G, uint32_t min_rank, uint32_t n_max,
                                           uint32_t* counts, uint32_t* sel, uint32_t* n_sel, uint32_t* n_match,
                                           hipStream_t st);
// The fields of k_decode_prepare's arguments that follow from the rows and the
// shape alike for every caller: the row arrays, the tables, k, e_max, e_lds,
// max_rows, max_rows_pad, passes and G.  The outputs, accept, coef_gen_stride,
// rep_limit and the row_off group are set by the caller, by name.
struct PrepareArgs;
QF_LOCAL void prepare_common(qf_ctx* ctx, PrepareArgs& pa, const RowArrays& rows, uint32_t k, uint32_t e_max,
                             uint32_t max_rows, uint32_t G);

}  // namespace qf

namespace qf {

// qf_encode16_batch over a ring of k source slots: window position i in slot
// (rot + i) % k, repairs = Cauchy rows first..first+r-1 (coeff_rxk must be
// NULL for first/rot != 0); coeff_be_dev (optional, device) receives each
// repair's big-endian coefficient block in window order.  (qf_gf16.hip)
int encode16_window(qf_ctx* ctx, const qf_encode_shape* sh, uint32_t G, const uint8_t* src, uint8_t* rep,
                    const uint16_t* coeff_rxk, uint32_t first, uint32_t rot, uint8_t* coeff_be_dev);

// Bit-sliced GF(2^16) Cauchy encode (qf_gf16_bs.hip, kernels generated by
// gf16_codegen.py): kGf16BsNone when (k, r) has no generated kernel.
constexpr int kGf16BsNone = 1;
int gf16_bs_encode(qf_ctx* ctx, hipStream_t st, uint32_t k, uint32_t r, uint32_t L, uint32_t G, const uint8_t* src,
                   uint64_t sgs, uint64_t srs, uint8_t* rep, uint64_t rgs, uint64_t rrs);
bool gf16_bs_has(uint32_t k, uint32_t r);
// Decode syndromes with the bit-sliced kernel of (k, r): syndrome a of
// generation g = C[k + j, S] x_S ^ the accepted row of repair k + j, for the
// generations with skip[g] == 0 (maps from k_dec16_bsmaps, qf_gf16.hip).
int gf16_bs_syndromes(qf_ctx* ctx, hipStream_t st, uint32_t k, uint32_t r, uint32_t L, uint32_t G,
                      const uint8_t* rows, uint64_t rgs, uint64_t rs, const uint16_t* smap, uint64_t smap_gs,
                      const uint16_t* rpos, const uint16_t* rslot, const uint32_t* skip, const uint8_t* zero,
                      uint8_t* synd, uint64_t synd_gs, uint64_t synd_rs);

// GF(2^16) Cauchy encode by the additive FFT (qf_gf16_fft.hip) for k = 2^a
// (16 <= k <= 4,096: the LDS strip, kFftLdsSymbols / 2) and repairs first ..
// first + r - 1 with first + r <= k,
// window position i in ring slot (rot + i) % k; kGf16BsNone otherwise.  work:
// >= 2 (2k + R) bytes of device workspace for the constants.
bool gf16_fft_has(uint32_t k, uint32_t r, uint32_t first);
// Whether the FFT beats the direct matvec for nout outputs over the first
// npoints coset points (QF_OPT_GF16_FFT 1; 2 forces the FFT wherever it applies).
bool gf16_fft_pays(uint32_t k, uint32_t nout, uint32_t npoints);
int gf16_fft_encode(qf_ctx* ctx, hipStream_t st, uint32_t k, uint32_t r, uint32_t first, uint32_t rot, uint32_t L,
                    uint32_t G, const uint8_t* src, uint64_t sgs, uint64_t srs, uint8_t* rep, uint64_t rgs,
                    uint64_t rrs, const uint16_t* glog, const uint16_t* gexp, uint8_t* work);

// Decode syndromes by the same FFT (k_dec16_bsmaps' maps, qf_gf16.hip):
// generation g's output row rpos[g r + t] = coset value t ^ the accepted row
// of repair k + t, sources gathered through smap (0xFFFF: zero), skip[g] != 0
// left alone.
int gf16_fft_syndromes(qf_ctx* ctx, hipStream_t st, uint32_t k, uint32_t r, uint32_t L, uint32_t G,
                       const uint8_t* rows, uint64_t rgs, uint64_t rs, const uint16_t* smap, const uint16_t* rpos,
                       const uint16_t* rslot, const uint32_t* skip, uint8_t* synd, uint64_t synd_gs, uint64_t synd_rs,
                       const uint16_t* glog, const uint16_t* gexp, uint8_t* work);

// x_E = C[J,E]^-1 s by the same FFT: (C^-1)_ba = D'_b / (J_a + E_b) D_a
// (closed form, logs of Qx, Px, Qy, Py in lprod), the FFT evaluating
// sum_a D_a s_a / ((J_a - k) + (k + E_b)).  Repairs J_a < 2k; generations with
// status != 0, e == 0 or solve_fb != 0 are left alone.
int gf16_fft_solve(qf_ctx* ctx, hipStream_t st, uint32_t k, uint32_t L, uint32_t G, const uint8_t* synd,
                   uint64_t synd_gs, uint64_t synd_rs, uint8_t* rec, uint64_t rec_gs, uint64_t rec_rs,
                   const uint32_t* st_e, uint32_t st_stride, const int32_t* status, const uint16_t* J,
                   const uint16_t* E, const uint32_t* lprod, uint64_t em, const uint32_t* solve_fb,
                   const uint16_t* glog, const uint16_t* gexp, uint8_t* work);

// One GF(2^8) window over a ring of k source slots (slot stride `stride`):
// window position i in slot (rot + i) % k; repairs = Cauchy rows
// first..first+count-1 into rep (row stride rep_stride), on the small-batch
// kernel.  QF_ERANGE when k + first + count > 256.  (qf_api.hip)
// fresh (fused per-packet send): window position k - 1 is the host packet
// fresh (fresh_units zero-padded 16-byte units, <= SEND_PKT_UNITS), passed in
// the kernel arguments and written into the ring slot fresh_dst; rep is then
// a host-coherent buffer of whole 16-byte units per row.
int encode_ring_window(qf_ctx* ctx, uint32_t k, uint32_t first, uint32_t count, uint32_t L,
                       const uint8_t* ring, uint64_t stride, uint32_t rot, uint8_t* rep, uint64_t rep_stride,
                       const uint8_t* fresh = nullptr, uint8_t* fresh_dst = nullptr, uint32_t fresh_units = 0);
// Whether the small-batch encode is enabled (QF_OPT_ENCODE_SMALL != 0).
bool small_encode_enabled(qf_ctx* ctx);

// Multi-connection send batches (qf_objects.hip).  The caller holds the
// context lock (ctx_lock) across these.
// The context's per-call metadata buffers, pinned host and device, `bytes`
// each, once the previous call's upload has landed.
int ctx_desc_buffers(qf_ctx* ctx, size_t bytes, uint8_t** h, uint8_t** d);
// The first `bytes` of the host buffer to the device buffer, on the context stream.
int ctx_desc_upload(qf_ctx* ctx, size_t bytes);
// Receive batches: pinned + device buffers of >= bytes each, once the
// previous user's host reads/writes are done (ctx_recv_release records that
// point on the context stream).  The caller does not hold the context lock.
int ctx_recv_buffers(qf_ctx* ctx, size_t bytes, uint8_t** h, uint8_t** d);
int ctx_recv_release(qf_ctx* ctx);
// At least n events of the context (download chunks of a send batch).
int ctx_send_events(qf_ctx* ctx, uint32_t n, hipEvent_t** out);
// QF_OPT_SEND_PROFILE: per-phase host wall time of this context's send
// batches (steady-state calls), printed when the context is destroyed.  A
// context serialises its own send batches, so the sums need no lock.
struct SendProfile {
    uint64_t calls = 0, seen = 0;
    double t[4] = {0, 0, 0, 0};   // stage, launch, wait, copy-out
    double u[4] = {0, 0, 0, 0};   // stage = host, buffers, packets, upload
};
SendProfile* ctx_send_profile(qf_ctx* ctx);
// Small-batch encode of G ring windows of one (k, r) class, repairs = Cauchy
// rows 0..r-1: window g per wins[g] (device records), rings addressed from
// src, repairs from rep; max_L (>= every window's L) sizes the grid.
int encode_ring_windows(qf_ctx* ctx, uint32_t k, uint32_t r, uint32_t G, uint32_t max_L, const uint8_t* src,
                        uint8_t* rep, const struct RingWin* wins);

// One connection's share of a send batch: a source packet for encoder e, and
// where repairs 0..n-k-1 of its window go when the add fills it.
struct EncSend {
    qf_encoder* e;
    uint64_t id;
    const uint8_t* data;
    uint32_t len;
    uint8_t* rep_data;            // rows rep_stride apart, >= window[0].len bytes each
    uint32_t rep_stride;
    uint8_t* rep_coeffs;          // nullable: k coefficient bytes per repair, coeff_stride apart
    uint32_t coeff_stride;
    qf_packet_desc* rep_desc;
    uint32_t n_rep;               // out: repairs emitted (0, or n - k)
};
// qf_encoder_add_source_packet + qf_encoder_generate_repairs(0, n - k) for M
// distinct encoders of ctx (lengths already checked): one upload, one ring
// scatter, one small-batch encode per (k, r) class, one download.  The
// caller does not hold the context lock.
int encoders_send_batch(qf_ctx* ctx, EncSend* v, uint32_t M);

// One packet for each of M distinct GF(2^8) decoders of ctx
// (qf_decoder_add_packet semantics, result per packet: 1 decoded, 0 not, < 0
// error): the accepted rows go up in one copy and one scatter; decoders that
// reach k rows decode together (one qf_decode_batch_desc over the Cauchy
// ones), with one download of all their outputs.
struct DecAdd {
    qf_decoder* d;
    uint64_t id;
    int is_systematic;
    const uint8_t* data;
    uint32_t len;
    const uint8_t* coeffs;
    uint32_t coeff_len;
    int result;
};
int decoders_add_batch(qf_ctx* ctx, DecAdd* v, uint32_t M);

// The k > 256 strategy of the GF(2^8) decoder (qf_wiedemann.hip,
// decoder.rs:794-975): k accepted rows on the device (slot q at q * stride,
// zero padded), e of them repairs with coefficient rows A_ek (e x k, host, in
// repair order), E the e erased sources ascending (host), slot[q] = source
// index of a systematic slot or 0x80000000 | repair ordinal (host).  Writes
// recovered row t (source E[t]) to d_rec + t * stride (L bytes, zero padded
// to 16).  QF_ERANK when the system is singular.  Takes the context lock;
// asynchronous on the context stream once it returns QF_OK.
int wiedemann_decode(qf_ctx* ctx, uint32_t k, uint32_t e, const uint8_t* A_ek, const uint16_t* E,
                     const uint32_t* slot, const uint8_t* d_rows, uint64_t stride, uint32_t L, uint8_t* d_rec,
                     uint32_t* tries_out);

// The host side of the innovative-row rule (qf_gf256_rank, the decoder
// object's innovative mode; qf_rank.hip): an incremental row-echelon basis
// over GF(2^8), at most k rows of k bytes, row c normalised with its first
// nonzero at column c.  add() reduces v (k bytes, clobbered) by the rows held,
// in column order, and keeps it when something is left.
class RankBasis {
  public:
    void reset(uint32_t k);
    bool add(uint8_t* v);
    uint32_t rank() const { return rank_; }

  private:
    uint32_t k_ = 0, rank_ = 0;
    std::vector<uint8_t> rows_;   // k x k, row c valid when has_[c]
    std::vector<uint8_t> has_;
};

}  // namespace qf

namespace qf {
// The cause of the calling thread's most recent QF_EDEVICE (qf_last_error):
// the failing HIP call's file:line and error name, plus the generated-kernel
// loader's refusal reason when a launch check refused it (qf_bs.hip).
int device_fail(const char* file, int line, hipError_t e);
void note_launch_refused(const char* what, int line);
const char* last_error_text();
}  // namespace qf

// every HIP call on the library's paths: a failure returns QF_EDEVICE and
// records its cause for qf_last_error
#define QF_CHECK_HIP(expr)                                                     \
    do {                                                                       \
        hipError_t _e = (expr);                                                \
        if (_e != hipSuccess) return qf::device_fail(__FILE__, __LINE__, _e);  \
    } while (0)

// One launch under qf_ctx_profile: begin, the launch (an expression of type
// hipError_t), its check, end under `name` (evaluated after the launch, so a
// launch that picks its kernel may set it).  Returns from the calling function
// on failure, with the caller's file and line as the cause.
#define QF_PROFILED(ctx, st, name, launch)                  \
    do {                                                    \
        hipEvent_t _ev = qf::ctx_prof_begin((ctx), (st));   \
        QF_CHECK_HIP(launch);                               \
        qf::ctx_prof_end((ctx), (st), _ev, (name));         \
    } while (0)
// (a kernel launched in place: hipLaunchKernelGGL as an expression of its error)
namespace qf {
template <class... Params, class... Args>
static inline hipError_t launch_kernel(void (*kern)(Params...), dim3 grid, dim3 block, size_t lds, hipStream_t st,
                                const Args&... args) {
    hipLaunchKernelGGL(kern, grid, block, lds, st, static_cast<Params>(args)...);
    return hipGetLastError();
}
}  // namespace qf
