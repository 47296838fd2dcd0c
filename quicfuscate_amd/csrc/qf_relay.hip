// qf_relay.hip -- a relay step that recodes straight from the received frame
// slots: qf_parse_frame_headers_dev leaves every payload in
// its slot and describes a row as (offset, length); qf_recode_frames_dev is
// qf_recode_batch over rows given that way, and qf_decode_frames_dev (DESIGN.md
// 3.13) qf_decode_innovative_batch over them, with the same payload pass.
//
//  k_combine_rows_at  the recode's payload pass, k_combine_slots with the rows
//                     read where they lie.  One lane per 16-byte unit of the
//                     output rows, the same 16-byte coefficient records and
//                     fma_rows_slots products, ceil(m / 16) passes.  Row s of
//                     a lane's generation comes from the {offset, length}
//                     that k_recode_prepare writes in front of the records
//                     of each slot pair (one 48-byte pair record: two
//                     offsets, two lengths, two coefficient records), so a
//                     slot pair costs five loads from two addresses against
//                     k_combine_slots' four from four, and the offsets of
//                     pair t + 2 are in flight while pair t multiplies.
//                     Full path (every lane of the wave has its whole unit
//                     inside every row of its generation: 16u + 16 <= the
//                     generation's shortest row): asm-pipelined loads as
//                     k_combine_slots, no masks.  Ragged path: a unit is
//                     loaded only when it holds a byte of the row and is
//                     masked to its valid bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <string>
#include <type_traits>

#include "qf_fec.h"
#include "qf_kernels.h"
#include "qf_gf_dev.h"
#include "qf_internal.h"

namespace qf {

namespace {

// Asm loads of a 48-byte pair record: the two row offsets (its first 8 bytes)
// and the two coefficient records (bytes 16 and 32).  The pair is the same for
// every lane, so its address is a scalar base (the pass's records + the pair's
// offset) plus the lane's 32-bit generation offset: no address arithmetic on
// the vector unit and one register per lane for all of a generation's records.
typedef uint32_t v2u __attribute__((ext_vector_type(2)));
QF_DEV void aload_offs(v2u& r, uint32_t gen_off, const uint8_t* pair) {
    asm volatile("global_load_dwordx2 %0, %1, %2" : "=v"(r) : "v"(gen_off), "s"(pair) : "memory");
}
QF_DEV void aload_rec_a(v4u& r, uint32_t gen_off, const uint8_t* pair) {
    asm volatile("global_load_dwordx4 %0, %1, %2 offset:16" : "=v"(r) : "v"(gen_off), "s"(pair) : "memory");
}
QF_DEV void aload_rec_b(v4u& r, uint32_t gen_off, const uint8_t* pair) {
    asm volatile("global_load_dwordx4 %0, %1, %2 offset:32" : "=v"(r) : "v"(gen_off), "s"(pair) : "memory");
}

// Counted waits of the full path's asm loads.  Issue order in the steady
// state, step t: D(t+2) Ca(t+1) Cb(t+1) | wait D(t+1) | Ra(t+1) Rb(t+1) |
// wait pair t | multiply pair t  (D row offsets, C records, R row units).
// Loads return in order: behind D(t+1) sit the four loads of pair t and the
// three just issued (7); behind Rb(t) sit D(t+2) and the four of pair t+1 (5).
// The prologue issues D(0) D(1) Ca(0) Cb(0) and waits for D(0) (3).
QF_DEV void wait_offs_first(v2u& d) { asm volatile("s_waitcnt vmcnt(3)" : "+v"(d)::"memory"); }
QF_DEV void wait_offs(v2u& d) { asm volatile("s_waitcnt vmcnt(7)" : "+v"(d)::"memory"); }
QF_DEV void wait_pair(v4u& a, v4u& b, v4u& c, v4u& d) {
    asm volatile("s_waitcnt vmcnt(5)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d)::"memory");
}
QF_DEV void wait_all(v2u& o, v4u& a, v4u& b, v4u& c, v4u& d) {
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(o), "+v"(a), "+v"(b), "+v"(c), "+v"(d)::"memory");
}

// One wave-item.  srcp: the lane's unit in its generation's source region at
// offset 0 (region + 16u); gen_off: the generation's pair records from a.coef
// (below 2^31, launch_combine_rows_at).  Pairs past the last one, (max_rows +
// 1) / 2, which holds zero slots only, are clamped to it.
template <int R, bool FULL>
QF_DEV void rows_at_item(const CombineRowsAtArgs& a, const uint32_t* __restrict__ tab256, const uint8_t* srcp,
                         uint8_t* outp, uint32_t gen_off, uint32_t u16, uint32_t nbytes, uint32_t e_lane,
                         uint32_t smax) {
    const uint32_t tz = (a.max_rows + 1) / 2;
    uint4 acc[R];
#pragma unroll
    for (int j = 0; j < R; ++j) acc[j] = make_uint4(0, 0, 0, 0);
    const uint32_t npairs = (smax + 1) / 2;
#define QF_PAIR(t) (a.coef + (uint64_t)((t) < tz ? (t) : tz) * kPairRecBytes)
    if (!FULL) {
        for (uint32_t t = 0; t < npairs; ++t) {
            const uint4* pr = reinterpret_cast<const uint4*>(QF_PAIR(t) + gen_off);
            const uint4 d = pr[0];   // off, off, len, len
            const uint4 xa = load_row_unit(srcp + (uint64_t)d.x, d.z, u16);
            const uint4 xb = load_row_unit(srcp + (uint64_t)d.y, d.w, u16);
            fma_rows_slots<R>(acc, tab256, xa, xb, pr[1], pr[2]);
        }
    } else {
        v2u d[2];
        v4u pa[2], pb[2], qa[2], qb[2];
        aload_offs(d[0], gen_off, QF_PAIR(0u));
        aload_offs(d[1], gen_off, QF_PAIR(1u));
        aload_rec_a(qa[0], gen_off, QF_PAIR(0u));
        aload_rec_b(qb[0], gen_off, QF_PAIR(0u));
        wait_offs_first(d[0]);
        aload16(pa[0], srcp + (uint64_t)d[0].x);
        aload16(pb[0], srcp + (uint64_t)d[0].y);
        for (uint32_t t = 0; t < npairs; t += 2) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int n = c ^ 1;
                const uint32_t tt = t + c;
                aload_offs(d[c], gen_off, QF_PAIR(tt + 2));
                aload_rec_a(qa[n], gen_off, QF_PAIR(tt + 1));
                aload_rec_b(qb[n], gen_off, QF_PAIR(tt + 1));
                wait_offs(d[n]);
                aload16(pa[n], srcp + (uint64_t)d[n].x);
                aload16(pb[n], srcp + (uint64_t)d[n].y);
                wait_pair(qa[c], qb[c], pa[c], pb[c]);
                fma_rows_slots<R>(acc, tab256, to_u4(pa[c]), to_u4(pb[c]), to_u4(qa[c]), to_u4(qb[c]));
            }
        }
        wait_all(d[0], pa[0], pb[0], qa[0], qb[0]);
        wait_all(d[1], pa[1], pb[1], qa[1], qb[1]);
    }
#undef QF_PAIR
#pragma unroll
    for (int j = 0; j < R; ++j) {
        if ((uint32_t)j < e_lane) {
            if (FULL) store_unit(outp + (uint64_t)j * a.dst_row_stride, acc[j], 16);
            else store_unit(outp + (uint64_t)j * a.dst_row_stride, acc[j], nbytes);
        }
    }
}

template <int R>
QF_DEV void rows_at_dispatch(const CombineRowsAtArgs& a, const uint32_t* tab256, const uint8_t* srcp, uint8_t* outp,
                             uint32_t gen_off, uint32_t u16, uint32_t nbytes, uint32_t e_lane, uint32_t smax,
                             bool full) {
    if (full) rows_at_item<R, true>(a, tab256, srcp, outp, gen_off, u16, nbytes, e_lane, smax);
    else rows_at_item<R, false>(a, tab256, srcp, outp, gen_off, u16, nbytes, e_lane, smax);
}

// PERGEN (the decode's pass, a.n_out_gen): the output rows of this pass differ
// per generation as in k_combine_slots: a lane whose generation has none
// contributes bound 0, a wave without an output row skips the item before it
// loads a row, and the unrolled width follows the wave's largest count.
// MAPPED (the calls over a list, a.gen_map): the source region
// of a lane's generation is region gen_map[g].  The records, counts and outputs
// stay indexed by g, so this is the one place the listed generation's number
// is needed, per lane: a wave spans several list entries when L < 1,024.
template <bool PERGEN, bool MAPPED = false>
__global__ void __launch_bounds__(256, 3)
k_combine_rows_at(typename std::conditional<MAPPED, CombineRowsAtMapArgs, CombineRowsAtArgs>::type a) {
    __shared__ __attribute__((aligned(16))) uint32_t tab256[256 * 8];
    {
        const uint4* g = reinterpret_cast<const uint4*>(a.tab256);
        uint4* l = reinterpret_cast<uint4*>(tab256);
        for (uint32_t w = threadIdx.x; w < 512; w += blockDim.x) l[w] = g[w];
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wpb = blockDim.x >> 6;
    const uint32_t wave = blockIdx.x * wpb + (threadIdx.x >> 6);
    const uint32_t nwaves = gridDim.x * wpb;
    for (uint64_t base = (uint64_t)wave * 64; base < a.total_units; base += (uint64_t)nwaves * 64) {
        // a lane past the last unit shadows the wave's first lane and stores nothing
        const bool active = base + lane < a.total_units;
        const uint64_t f = active ? base + lane : base;
        const uint64_t g = f / a.Lu;
        const uint32_t u = (uint32_t)(f - g * a.Lu);
        const uint32_t u16 = u * 16;
        uint64_t gs = g;
        if constexpr (MAPPED) gs = a.gen_map[g];
        const uint8_t* srcp = a.src + gs * a.src_gen_stride + u16;
        uint8_t* outp = a.dst + g * a.dst_gen_stride + u16;
        const uint32_t gen_off = (uint32_t)(g * a.coef_gen_stride);
        const uint32_t rem = a.L - u16;
        const uint32_t nbytes = rem < 16 ? rem : 16;
        uint32_t e_lane = active ? a.n_out : 0;
        uint32_t bound_lane = a.bound[g];
        uint32_t jmax = a.n_out;
        if (PERGEN) {
            // (a shadow lane has the first lane's generation, so its count changes no maximum)
            const uint32_t e = a.n_out_gen[g], lo = a.pass * 16;
            const uint32_t ep = e > lo ? (e - lo < 16 ? e - lo : 16) : 0;
            e_lane = active ? ep : 0;
            if (ep == 0) bound_lane = 0;
            jmax = wave_max_u32(ep);
            if (jmax == 0) continue;
        }
        const uint32_t smax = wave_max_u32(bound_lane);
        const bool full = __all(u16 + 16 <= a.min_len[g]);
        // smax == 0: every generation of the wave is not QF_OK; the ragged
        // path then stores the zero rows without a load
        if (jmax <= 4) rows_at_dispatch<4>(a, tab256, srcp, outp, gen_off, u16, nbytes, e_lane, smax, full);
        else if (jmax <= 8) rows_at_dispatch<8>(a, tab256, srcp, outp, gen_off, u16, nbytes, e_lane, smax, full);
        else if (jmax <= 12) rows_at_dispatch<12>(a, tab256, srcp, outp, gen_off, u16, nbytes, e_lane, smax, full);
        else if (PERGEN && jmax <= 13) rows_at_dispatch<13>(a, tab256, srcp, outp, gen_off, u16, nbytes, e_lane, smax, full);
        else if (PERGEN && jmax <= 14) rows_at_dispatch<14>(a, tab256, srcp, outp, gen_off, u16, nbytes, e_lane, smax, full);
        else rows_at_dispatch<16>(a, tab256, srcp, outp, gen_off, u16, nbytes, e_lane, smax, full);
    }
}

}  // namespace

hipError_t launch_combine_rows_at(const CombineRowsAtArgs& a, int num_cus, hipStream_t st, const uint32_t* gen_map) {
    if (a.total_units == 0) return hipSuccess;
    if (a.n_out == 0 || a.n_out > 16 || a.max_rows == 0 || a.Lu == 0 || a.Lu != (a.L + 15) / 16 || (a.src_gen_stride & 15) || (a.coef_gen_stride & 15) ||
        a.coef_gen_stride < ((uint64_t)(a.max_rows + 1) / 2 + 1) * kPairRecBytes || (gen_map && !a.n_out_gen))
        return hipErrorInvalidValue;
    const auto kern = a.n_out_gen ? k_combine_rows_at<true> : k_combine_rows_at<false>;
    int occ = 0;
    hipError_t e = gen_map ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_combine_rows_at<true, true>, 256, 0)
                           : hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kern, 256, 0);
    if (e != hipSuccess) return e;
    if (occ < 1) occ = 1;
    const uint64_t cap = (uint64_t)(num_cus > 0 ? num_cus : 1) * occ;
    // a lane addresses its generation's records by a 32-bit offset from
    // a.coef: batches whose records exceed 2 GiB go in several launches
    const uint64_t G = a.total_units / a.Lu;
    const uint64_t g_max = 0x7FFFFFFFull / a.coef_gen_stride;
    for (uint64_t g0 = 0; g0 < G; g0 += g_max) {
        const uint64_t gn = G - g0 < g_max ? G - g0 : g_max;
        CombineRowsAtArgs c = a;
        if (!gen_map) c.src += g0 * a.src_gen_stride;   // (the map holds source generation numbers: src stays)
        c.dst += g0 * a.dst_gen_stride;
        c.coef += g0 * a.coef_gen_stride;
        c.bound += g0;
        c.min_len += g0;
        if (c.n_out_gen) c.n_out_gen += g0;
        c.total_units = gn * a.Lu;
        const uint64_t waves = (c.total_units + 63) / 64;
        uint64_t blocks = (waves + 3) / 4;
        if (blocks > cap) blocks = cap;
        if (gen_map) {
            CombineRowsAtMapArgs cm{c, gen_map + g0};
            hipLaunchKernelGGL((k_combine_rows_at<true, true>), dim3((uint32_t)blocks), dim3(256), 0, st, cm);
        } else {
            hipLaunchKernelGGL(kern, dim3((uint32_t)blocks), dim3(256), 0, st, c);
        }
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace qf

extern "C" int qf_parse_frame_headers_dev(qf_ctx* ctx, uint32_t k, uint32_t L, uint32_t G, uint32_t max_rows,
                                          const uint8_t* frames, uint64_t frame_stride, const uint32_t* frame_len,
                                          const uint32_t* frame_off, const uint64_t* ids, const uint32_t* n_frames,
                                          uint16_t* row_index, uint32_t* n_rows, uint8_t* row_coeffs,
                                          uint32_t* row_len, uint32_t* row_off, int32_t* frame_status) {
    if (!ctx) return QF_EINVAL;
    if (k == 0 || k > 256) return QF_EINVAL;
    if (G == 0) return QF_OK;
    if (max_rows == 0 || max_rows > 1024 || L == 0) return QF_EINVAL;
    if (!frames || !frame_len || !ids || !row_index || !n_rows || !row_coeffs || !row_len || !row_off || !frame_status)
        return QF_EINVAL;
    if ((frame_stride & 15) || !aligned16(frames)) return QF_EINVAL;
    // row_off is a u32 offset into a generation's max_rows * frame_stride bytes
    if (frame_stride > (1ull << 32) / max_rows) return QF_EINVAL;
    std::unique_lock<std::mutex> lk;
    int s = qf::ctx_lock(ctx, lk);
    if (s) return s;
    hipStream_t st = qf::ctx_stream(ctx);
    qf::ParseHeadersArgs a{};
    a.frames = frames;
    a.frame_stride = frame_stride;
    a.frame_len = frame_len;
    a.frame_off = frame_off;
    a.ids = ids;
    a.n_frames = n_frames;
    a.row_index = row_index;
    a.n_rows = n_rows;
    a.row_coeffs = row_coeffs;
    a.row_len = row_len;
    a.row_off = row_off;
    a.frame_status = frame_status;
    a.k = k;
    a.L = L;
    a.max_rows = max_rows;
    QF_PROFILED(ctx, st, "k_parse_frame_headers", qf::launch_parse_frame_headers(a, G, st));
    return QF_OK;
}

// The arrays of k_sel_gather, taken behind a dense call's parts of the same
// layout: one ctx_work allocation holds both (a second ctx_work call may move
// the first).
struct SelWork {
    size_t off, len, index, n_rows, map, n_out, coeffs;
};
static SelWork sel_work(qf::WorkLayout& wl, uint32_t n_max, uint32_t max_rows, uint32_t k) {
    SelWork w;
    const size_t slots = (size_t)n_max * max_rows;
    w.off = wl.take(slots * 4);
    w.len = wl.take(slots * 4);
    w.index = wl.take(slots * 2);
    w.n_rows = wl.take((size_t)n_max * 4);
    w.map = wl.take((size_t)n_max * 4);
    w.n_out = wl.take((size_t)n_max * 4);
    w.coeffs = wl.take(slots * k);
    return w;
}
static bool sel_ok(const qf_gen_sel* sel) { return sel && sel->sel_dev && sel->n_max != 0 && sel->G_src != 0; }

// k_sel_gather: the batch of sel->n_max generations the list stands for, in the
// compact arrays at sw of the workspace w; *rows becomes those arrays and
// *gen_map the source generation of each entry.  invalid_n_rows: the n_rows
// that makes the call's control kernel answer an invalid entry with QF_EINVAL.
// n_out_gen (nullable) receives n_out_listed for a listed entry and 0 for an
// unused one.
static int sel_gather(qf_ctx* ctx, hipStream_t st, const qf_gen_sel* sel, const SelWork& sw, uint8_t* w, uint32_t k,
                      uint32_t max_rows, uint32_t invalid_n_rows, uint32_t n_out_listed, qf::RowArrays* rows,
                      const uint32_t** gen_map, const uint32_t** n_out_gen) {
    qf::SelGatherArgs ga{};
    ga.sel = sel->sel_dev;
    ga.n_sel = sel->n_sel_dev;
    ga.row_off = rows->off;
    ga.row_len = rows->len;
    ga.row_index = rows->index;
    ga.n_rows = rows->n_rows;
    ga.row_coeffs = rows->coeffs;
    ga.c_row_off = reinterpret_cast<uint32_t*>(w + sw.off);
    ga.c_row_len = reinterpret_cast<uint32_t*>(w + sw.len);
    ga.c_row_index = reinterpret_cast<uint16_t*>(w + sw.index);
    ga.c_n_rows = reinterpret_cast<uint32_t*>(w + sw.n_rows);
    ga.c_row_coeffs = w + sw.coeffs;
    ga.gen_map = reinterpret_cast<uint32_t*>(w + sw.map);
    if (n_out_gen) ga.n_out = reinterpret_cast<uint32_t*>(w + sw.n_out);
    ga.n_max = sel->n_max;
    ga.G_src = sel->G_src;
    ga.k = k;
    ga.max_rows = max_rows;
    ga.invalid_n_rows = invalid_n_rows;
    ga.n_out_listed = n_out_listed;
    QF_PROFILED(ctx, st, "k_sel_gather", qf::launch_sel_gather(ga, st));
    *rows = qf::RowArrays{ga.c_row_off, ga.c_row_len, ga.c_row_index, ga.c_n_rows, ga.c_row_coeffs};
    *gen_map = ga.gen_map;
    if (n_out_gen) *n_out_gen = ga.n_out;
    return QF_OK;
}

// The payload passes of both calls: pass p writes output rows 16 p .. of every
// generation from the pass's pair records, coef_gen_stride * G apart from a.coef.
// a holds what the passes share; a.n_out_gen == nullptr: m rows per generation.
static int rows_at_passes(qf_ctx* ctx, hipStream_t st, qf::CombineRowsAtArgs a, uint32_t passes, uint32_t G,
                          uint32_t m, const uint32_t* gen_map) {
    uint8_t* const dst = a.dst;
    const uint8_t* const coef = a.coef;
    a.tab256 = qf::ctx_tab256(ctx);
    a.Lu = (a.L + 15) / 16;
    a.total_units = (uint64_t)G * a.Lu;
    for (uint32_t p = 0; p < passes; ++p) {
        a.dst = dst + (uint64_t)p * 16 * a.dst_row_stride;
        a.coef = coef + (uint64_t)p * G * a.coef_gen_stride;
        a.n_out = 16;   // (with n_out_gen the per-generation count decides)
        if (a.n_out_gen) a.pass = p;
        else if (m - p * 16 < 16) a.n_out = m - p * 16;
        QF_PROFILED(ctx, st, "k_combine_rows_at", qf::launch_combine_rows_at(a, qf::ctx_num_cus(ctx), st, gen_map));
    }
    return QF_OK;
}

// qf_recode_frames_dev (sel == nullptr), and qf_recode_frames_sel_dev over the
// batch of G = sel->n_max generations that k_sel_gather makes of the list: the
// same control kernel over the compact arrays, and the payload pass in its
// per-generation-count form (m for a listed entry, 0 for an unused one), so
// that an unused entry stores no row.
static int recode_frames_run(qf_ctx* ctx, const qf_recode_frames_shape* sh, uint32_t G, const qf_gen_sel* sel,
                             const uint8_t* src, qf::RowArrays rows, const uint8_t* mix, uint64_t seed, uint8_t* out,
                             uint8_t* out_coeffs, uint32_t* out_len, int32_t* status) {
    const uint32_t k = sh->k, L = sh->L, max_rows = sh->max_rows, m = sh->m;
    if (k == 0 || k > 255 || max_rows == 0 || max_rows > 255 || m == 0 || m > 64 || L == 0 || sh->flags != 0 ||
        sh->reserved != 0)
        return QF_EINVAL;
    if (sh->out_row_stride < L) return QF_EINVAL;
    if (G == 0) return QF_OK;
    if (!src || !rows.off || !rows.len || !rows.index || !rows.coeffs || !out || !out_coeffs || !status)
        return QF_EINVAL;
    if (!aligned16(src) || (sh->src_gen_stride & 15) || !aligned16(out) || (sh->out_row_stride & 15) ||
        (sh->out_gen_stride & 15))
        return QF_EINVAL;
    std::unique_lock<std::mutex> lk;
    int s = qf::ctx_lock(ctx, lk);
    if (s) return s;
    hipStream_t st = qf::ctx_stream(ctx);
    // workspace: pair records [pass][G][((max_rows + 1) / 2 + 1) * 48] | n_out[G] | bound[G] | min_len[G]
    const uint32_t passes = (m + 15) / 16;
    const uint64_t coef_gen_stride = ((uint64_t)(max_rows + 1) / 2 + 1) * qf::kPairRecBytes;
    qf::WorkLayout wl;
    const size_t off_coef = wl.take((size_t)passes * G * coef_gen_stride);
    const size_t off_nout = wl.take((size_t)G * 4);
    const size_t off_bound = wl.take((size_t)G * 4);
    const size_t off_minlen = wl.take((size_t)G * 4);
    const SelWork sw = sel ? sel_work(wl, G, max_rows, k) : SelWork{};
    uint8_t* w = nullptr;
    s = qf::ctx_work(ctx, wl.size(), &w);
    if (s) return s;
    const uint32_t* gen_map = nullptr;
    const uint32_t* n_out_gen = nullptr;
    // (invalid entry: n_rows > max_rows, k_recode_prepare's QF_EINVAL)
    if (sel && (s = sel_gather(ctx, st, sel, sw, w, k, max_rows, 0xFFFFFFFFu, m, &rows, &gen_map, &n_out_gen)))
        return s;
    qf::RecodePrepareArgs pa{};
    pa.row_index = rows.index;
    pa.n_rows = rows.n_rows;
    pa.row_coeffs = rows.coeffs;
    pa.mix = mix;
    pa.explog = qf::ctx_explog(ctx);
    pa.seed = seed;
    pa.coef_out = w + off_coef;
    pa.coef_gen_stride = coef_gen_stride;
    pa.n_out = reinterpret_cast<uint32_t*>(w + off_nout);
    pa.bound = reinterpret_cast<uint32_t*>(w + off_bound);
    pa.out_coeffs = out_coeffs;
    pa.status = status;
    pa.k = k;
    pa.r = 0;
    pa.m = m;
    pa.max_rows = max_rows;
    pa.passes = passes;
    pa.G = G;
    pa.row_off = rows.off;
    pa.row_len = rows.len;
    pa.min_len = reinterpret_cast<uint32_t*>(w + off_minlen);
    pa.out_len = out_len;
    pa.src_gen_stride = sh->src_gen_stride;
    pa.L = L;
    QF_PROFILED(ctx, st, "k_recode_prepare", qf::launch_recode_prepare(pa, st));
    qf::CombineRowsAtArgs a{};
    a.src = src;
    a.src_gen_stride = sh->src_gen_stride;
    a.dst = out;
    a.dst_gen_stride = sh->out_gen_stride;
    a.dst_row_stride = sh->out_row_stride;
    a.coef = pa.coef_out;
    a.coef_gen_stride = coef_gen_stride;
    a.bound = pa.bound;
    a.min_len = pa.min_len;
    a.L = L;
    a.max_rows = max_rows;
    a.n_out_gen = n_out_gen;
    return rows_at_passes(ctx, st, a, passes, G, m, gen_map);
}

extern "C" int qf_recode_frames_dev(qf_ctx* ctx, const qf_recode_frames_shape* sh, uint32_t G, const uint8_t* src,
                                    const uint32_t* row_off, const uint32_t* row_len, const uint16_t* row_index,
                                    const uint32_t* n_rows, const uint8_t* row_coeffs, const uint8_t* mix,
                                    uint64_t seed, uint8_t* out, uint8_t* out_coeffs, uint32_t* out_len,
                                    int32_t* status) {
    if (!ctx || !sh) return QF_EINVAL;
    return recode_frames_run(ctx, sh, G, nullptr, src, {row_off, row_len, row_index, n_rows, row_coeffs}, mix, seed,
                             out, out_coeffs, out_len, status);
}

extern "C" int qf_recode_frames_sel_dev(qf_ctx* ctx, const qf_recode_frames_shape* sh, const qf_gen_sel* sel,
                                        const uint8_t* src, const uint32_t* row_off, const uint32_t* row_len,
                                        const uint16_t* row_index, const uint32_t* n_rows, const uint8_t* row_coeffs,
                                        const uint8_t* mix, uint64_t seed, uint8_t* out, uint8_t* out_coeffs,
                                        uint32_t* out_len, int32_t* status) {
    if (!ctx || !sh || !sel_ok(sel)) return QF_EINVAL;
    return recode_frames_run(ctx, sh, sel->n_max, sel, src, {row_off, row_len, row_index, n_rows, row_coeffs}, mix,
                             seed, out, out_coeffs, out_len, status);
}

// The receiver's step over the same row descriptions: k_rank_filter's flags as
// the accept mask, k_decode_prepare with pair records over the accepted rows,
// then ceil(min(k, r) / 16) passes of k_combine_rows_at with per-generation
// output counts.
// (sel as in recode_frames_run: the three control and payload kernels of the
// dense call over the compact arrays, the payload pass reading through the map)
// partial (qf_decode_partial_frames_dev): k_partial_prepare in
// the place of k_decode_prepare, over the same arguments and workspace; its
// records hold the rows some determined source uses, at most the accepted ones.
static int decode_frames_run(qf_ctx* ctx, const qf_decode_frames_shape* sh, uint32_t G, const qf_gen_sel* sel,
                             const uint8_t* src, qf::RowArrays rows, uint8_t* rec, uint16_t* rec_index,
                             uint32_t* n_rec, int32_t* status, uint32_t* rank, uint8_t* innovative,
                             uint16_t* src_slot, bool partial = false) {
    qf::ctx_clear_payload_split(ctx);   // as qf_decode_innovative_batch: they apply to qf_decode_batch only
    const uint32_t k = sh->k, r = sh->r, L = sh->L, max_rows = sh->max_rows;
    if (k == 0 || k > 256 || max_rows == 0 || max_rows > 1024 || L == 0 || sh->flags != 0 || sh->reserved != 0)
        return QF_EINVAL;
    const uint32_t e_max = k < r ? k : r;
    if (e_max > 128 || sh->rec_row_stride < L) return QF_EINVAL;
    if (G == 0) return QF_OK;
    if (!src || !rows.off || !rows.len || !rows.index || !rows.coeffs || !n_rec || !status) return QF_EINVAL;
    if (e_max && (!rec || !rec_index)) return QF_EINVAL;
    if (!aligned16(src) || (sh->src_gen_stride & 15) || !aligned16(rec) || (sh->rec_row_stride & 15) ||
        (sh->rec_gen_stride & 15))
        return QF_EINVAL;
    if ((partial ? qf::partial_prepare_lds_bytes(k, max_rows) : qf::prepare_lds_bytes(k, k < 128 ? k : 128, max_rows)) >
        160 * 1024)
        return QF_EINVAL;
    std::unique_lock<std::mutex> lk;
    int s = qf::ctx_lock(ctx, lk);
    if (s) return s;
    hipStream_t st = qf::ctx_stream(ctx);
    // workspace: pair records [pass][G][((min(k, max_rows) + 1) / 2 + 1) * 48] | bound[G] | min_len[G] |
    // the filter's flags [G][max_rows] unless the caller takes them
    const uint32_t passes = (e_max + 15) / 16;
    const uint32_t max_acc = k < max_rows ? k : max_rows;
    const uint64_t coef_gen_stride = ((uint64_t)(max_acc + 1) / 2 + 1) * qf::kPairRecBytes;
    qf::WorkLayout wl;
    const size_t off_coef = wl.take((size_t)(passes ? passes : 1) * G * coef_gen_stride);
    const size_t off_bound = wl.take((size_t)G * 4);
    const size_t off_minlen = wl.take((size_t)G * 4);
    const size_t off_flags = wl.take(innovative ? 0 : (size_t)G * max_rows);
    const SelWork sw = sel ? sel_work(wl, G, max_rows, k) : SelWork{};
    uint8_t* w = nullptr;
    s = qf::ctx_work(ctx, wl.size(), &w);
    if (s) return s;
    const uint32_t* gen_map = nullptr;
    // (invalid entry: one slot of index 0xFFFF, the control kernels' QF_EINVAL, rank 0)
    if (sel && (s = sel_gather(ctx, st, sel, sw, w, k, max_rows, 1, 0, &rows, &gen_map, nullptr))) return s;
    uint8_t* flags = innovative ? innovative : w + off_flags;
    // (no status from the filter: k_decode_prepare applies the same index rules and reports)
    QF_PROFILED(ctx, st, "k_rank_filter",
                qf::launch_rank(ctx, rows, k, r, max_rows, G, nullptr, flags, rank, nullptr, st));
    qf::PrepareArgs pa{};
    qf::prepare_common(ctx, pa, rows, k, e_max, max_rows, G);
    pa.accept = flags;
    pa.coef_out = w + off_coef;
    pa.coef_gen_stride = coef_gen_stride;
    pa.n_out = n_rec;
    pa.bound = reinterpret_cast<uint32_t*>(w + off_bound);
    pa.rec_index = rec_index;
    pa.status = status;
    pa.rep_limit = 256;
    pa.row_off = rows.off;
    pa.row_len = rows.len;
    pa.min_len = reinterpret_cast<uint32_t*>(w + off_minlen);
    pa.src_slot = src_slot;
    pa.src_gen_stride = sh->src_gen_stride;
    pa.L = L;
    if (partial) QF_PROFILED(ctx, st, "k_partial_prepare", qf::launch_partial_prepare(pa, st));
    else QF_PROFILED(ctx, st, "k_decode_prepare", qf::launch_decode_prepare(pa, st));
    qf::CombineRowsAtArgs a{};
    a.src = src;
    a.src_gen_stride = sh->src_gen_stride;
    a.dst = rec;
    a.dst_gen_stride = sh->rec_gen_stride;
    a.dst_row_stride = sh->rec_row_stride;
    a.coef = pa.coef_out;
    a.coef_gen_stride = coef_gen_stride;
    a.bound = pa.bound;
    a.min_len = pa.min_len;
    a.L = L;
    a.max_rows = max_acc;   // the records hold the accepted rows only
    a.n_out_gen = n_rec;
    return rows_at_passes(ctx, st, a, passes, G, 0, gen_map);
}

extern "C" int qf_decode_frames_dev(qf_ctx* ctx, const qf_decode_frames_shape* sh, uint32_t G, const uint8_t* src,
                                    const uint32_t* row_off, const uint32_t* row_len, const uint16_t* row_index,
                                    const uint32_t* n_rows, const uint8_t* row_coeffs, uint8_t* rec,
                                    uint16_t* rec_index, uint32_t* n_rec, int32_t* status, uint32_t* rank,
                                    uint8_t* innovative, uint16_t* src_slot) {
    if (!ctx || !sh) return QF_EINVAL;
    return decode_frames_run(ctx, sh, G, nullptr, src, {row_off, row_len, row_index, n_rows, row_coeffs}, rec,
                             rec_index, n_rec, status, rank, innovative, src_slot);
}

extern "C" int qf_decode_frames_sel_dev(qf_ctx* ctx, const qf_decode_frames_shape* sh, const qf_gen_sel* sel,
                                        const uint8_t* src, const uint32_t* row_off, const uint32_t* row_len,
                                        const uint16_t* row_index, const uint32_t* n_rows, const uint8_t* row_coeffs,
                                        uint8_t* rec, uint16_t* rec_index, uint32_t* n_rec, int32_t* status,
                                        uint32_t* rank, uint8_t* innovative, uint16_t* src_slot) {
    if (!ctx || !sh || !sel_ok(sel)) return QF_EINVAL;
    return decode_frames_run(ctx, sh, sel->n_max, sel, src, {row_off, row_len, row_index, n_rows, row_coeffs}, rec,
                             rec_index, n_rec, status, rank, innovative, src_slot);
}

extern "C" int qf_decode_partial_frames_dev(qf_ctx* ctx, const qf_decode_frames_shape* sh, uint32_t G,
                                            const uint8_t* src, const uint32_t* row_off, const uint32_t* row_len,
                                            const uint16_t* row_index, const uint32_t* n_rows,
                                            const uint8_t* row_coeffs, uint8_t* rec, uint16_t* rec_index,
                                            uint32_t* n_rec, int32_t* status, uint32_t* rank, uint8_t* innovative,
                                            uint16_t* src_slot) {
    if (!ctx || !sh) return QF_EINVAL;
    return decode_frames_run(ctx, sh, G, nullptr, src, {row_off, row_len, row_index, n_rows, row_coeffs}, rec,
                             rec_index, n_rec, status, rank, innovative, src_slot, true);
}

extern "C" int qf_decode_partial_frames_sel_dev(qf_ctx* ctx, const qf_decode_frames_shape* sh, const qf_gen_sel* sel,
                                                const uint8_t* src, const uint32_t* row_off, const uint32_t* row_len,
                                                const uint16_t* row_index, const uint32_t* n_rows,
                                                const uint8_t* row_coeffs, uint8_t* rec, uint16_t* rec_index,
                                                uint32_t* n_rec, int32_t* status, uint32_t* rank,
                                                uint8_t* innovative, uint16_t* src_slot) {
    if (!ctx || !sh || !sel_ok(sel)) return QF_EINVAL;
    return decode_frames_run(ctx, sh, sel->n_max, sel, src, {row_off, row_len, row_index, n_rows, row_coeffs}, rec,
                             rec_index, n_rec, status, rank, innovative, src_slot, true);
}
