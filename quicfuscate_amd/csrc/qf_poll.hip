// qf_poll.hip -- the streaming receiver's step into a poll:
// qf_parse_poll_headers_dev takes a flat poll, N frame slots in arrival order
// with one generation tag per frame, groups the frames by generation on the
// device and parses their headers where they lie.  The outputs are indexed by
// the position in the list of touched generations, which the listed update
// (qf_rank.hip) and the listed append (qf_store.hip) take.
//
//  k_poll_count    a lane per frame: one atomicAdd on its tag's entry of a
//                  zeroed count array.  The sums do not depend on the order.
//  (k_gen_select_count / k_gen_select_scatter of qf_select.hip over the
//                  counts with min_rank 1: the ascending list.)
//  k_poll_place    a lane per frame: a binary search of the list for its tag,
//                  one atomicAdd on the entry's cursor for a slot of the
//                  entry's scratch row, its frame number into that slot.  The
//                  slot a frame gets depends on the order, the set of frame
//                  numbers an entry ends up with does not.
//  k_poll_headers  a wave per entry: sorts the entry's frame numbers
//                  ascending in LDS (rank by counting), which restores the
//                  arrival order whatever k_poll_place did, then takes
//                  k_parse_frame_headers' decisions (qf_wire.hip) in that
//                  order, 64 frames at a time: status, ballot-prefix
//                  compaction, vector copy, the unit vector of a systematic
//                  frame.  The decision and the copy are the ones that
//                  kernel calls (frame_head and vector_block, qf_wire_dev.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>

#include "qf_fec.h"
#include "qf_internal.h"
#include "qf_wire_dev.h"

namespace qf {

namespace {

struct PollCountArgs {
    const uint32_t* frame_gen;
    const uint32_t* n_frames;   // nullptr: N_max
    uint32_t* counts;           // [G_src], zeroed
    uint32_t N_max, G_src;
};

struct PollPlaceArgs {
    const uint32_t* frame_gen;
    const uint32_t* n_frames;   // nullptr: N_max
    const uint32_t* counts;     // [G_src]
    const uint32_t* sel;        // ascending, min(*n_sel, n_max) entries
    const uint32_t* n_sel;
    uint32_t* cursor;           // [n_max], zeroed
    uint32_t* place;            // [n_max][max_rows] frame numbers, in claim order
    int32_t* frame_status;
    uint32_t N_max, G_src, n_max, max_rows;
};

struct PollHeadersArgs {
    const uint8_t* frames;
    uint64_t frame_stride;
    const uint32_t* frame_len;
    const uint32_t* frame_off;  // nullptr: 0
    const uint64_t* ids;
    const uint32_t* n_frames;   // nullptr: N_max
    const uint32_t* counts;
    const uint32_t* sel;
    const uint32_t* n_sel;
    const uint32_t* place;
    uint16_t* row_index;
    uint32_t* n_rows;
    uint8_t* row_coeffs;
    uint32_t* row_len;
    uint32_t* row_off;
    int32_t* entry_status;
    int32_t* frame_status;
    uint32_t k, L, max_rows, N_max, n_max;
};

QF_DEV uint32_t poll_frames(const uint32_t* n_frames, uint32_t N_max) {
    return n_frames ? min(*n_frames, N_max) : N_max;
}

__global__ void __launch_bounds__(256) k_poll_count(PollCountArgs a) {
    const uint32_t f = blockIdx.x * 256 + threadIdx.x;
    if (f >= poll_frames(a.n_frames, a.N_max)) return;
    const uint32_t tag = a.frame_gen[f];
    if (tag < a.G_src) atomicAdd(&a.counts[tag], 1u);
}

__global__ void __launch_bounds__(256) k_poll_place(PollPlaceArgs a) {
    const uint32_t f = blockIdx.x * 256 + threadIdx.x;
    if (f >= poll_frames(a.n_frames, a.N_max)) return;
    const uint32_t tag = a.frame_gen[f];
    if (tag >= a.G_src) {
        a.frame_status[f] = QF_EINVAL;
        return;
    }
    // the entry of the ascending list that holds the tag, if any
    uint32_t lo = 0, hi = min(*a.n_sel, a.n_max);
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a.sel[mid] < tag) lo = mid + 1;
        else hi = mid;
    }
    const uint32_t n_used = min(*a.n_sel, a.n_max);
    // not listed (the list was full), or more frames than an entry holds: the
    // caller presents the frame again
    if (lo >= n_used || a.sel[lo] != tag || a.counts[tag] > a.max_rows) {
        a.frame_status[f] = QF_ENOTREADY;
        return;
    }
    const uint32_t slot = atomicAdd(&a.cursor[lo], 1u);
    if (slot < a.max_rows) a.place[(uint64_t)lo * a.max_rows + slot] = f;   // (always: the count is the claims)
}

__global__ void __launch_bounds__(64) k_poll_headers(PollHeadersArgs a) {
    __shared__ uint32_t raw[1024];     // the entry's frame numbers as claimed
    __shared__ uint32_t srt[1024];     // ... ascending: the arrival order
    __shared__ uint32_t of_frame[64];  // accepted ordinal inside the chunk -> its frame,
    __shared__ uint32_t of_pay[64];    // payload start from the slot's first byte,
    __shared__ uint32_t of_idx[64];    // column of a systematic frame, k for a coded one
    const uint32_t j = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const uint32_t mr = a.max_rows;
    const uint32_t n_used = min(*a.n_sel, a.n_max);
    if (j >= n_used) {   // an unused entry: its sel value is not looked at
        if (lane == 0) {
            a.n_rows[j] = 0;
            a.entry_status[j] = QF_OK;
        }
        return;
    }
    const uint32_t g = a.sel[j];     // < G_src: it came from the count array
    const uint32_t c = a.counts[g];  // >= 1
    if (c > mr) {   // the frames were told QF_ENOTREADY by k_poll_place
        if (lane == 0) {
            a.n_rows[j] = 0;
            a.entry_status[j] = QF_ETOOSMALL;
        }
        return;
    }
    const uint32_t N = poll_frames(a.n_frames, a.N_max);
    for (uint32_t i = lane; i < c; i += 64) {
        raw[i] = a.place[(uint64_t)j * mr + i];
        srt[i] = 0xFFFFFFFFu;
    }
    __syncthreads();
    for (uint32_t i = lane; i < c; i += 64) {   // frame numbers are distinct: the ranks are a permutation
        const uint32_t v = raw[i];
        uint32_t r = 0;
        for (uint32_t t = 0; t < c; ++t) r += raw[t] < v;
        srt[r] = v;
    }
    __syncthreads();
    const uint64_t out0 = (uint64_t)j * mr;
    const uint32_t cpr = (a.k + 15) / 16;
    const uint64_t lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    uint32_t base = 0;
    for (uint32_t s0 = 0; s0 < c; s0 += 64) {   // c <= 1024: 16 chunks at most
        const uint32_t s = s0 + lane;
        FrameHead h{QF_OK, 0xFFFF, 0, 0};
        uint32_t f = 0;
        bool in = s < c;
        if (in) {
            f = srt[s];
            in = f < N;   // (always)
        }
        if (in) {
            h = frame_head(a.frames + (uint64_t)f * a.frame_stride, a.frame_len[f], a.frame_off ? a.frame_off[f] : 0,
                           a.frame_stride, a.ids + f, a.k, a.L, true);
            a.frame_status[f] = h.st;
        }
        const bool ok = in && h.st == QF_OK;
        const uint64_t bal = __ballot(ok);
        const uint32_t before = (uint32_t)__popcll(bal & lt_mask);
        const uint32_t cnt = (uint32_t)__popcll(bal);
        if (ok) {
            const uint64_t o = out0 + base + before;   // base + cnt <= c <= max_rows
            a.row_index[o] = (uint16_t)h.idx;
            a.row_len[o] = h.plen;
            a.row_off[o] = (uint32_t)((uint64_t)f * a.frame_stride) + h.pay;   // N_max * frame_stride <= 2^32
            of_frame[before] = f;
            of_pay[before] = h.pay;
            of_idx[before] = h.idx;
        }
        __syncthreads();
        // 16-byte blocks of the accepted rows' coefficient vectors (the unit
        // vector of a systematic frame)
        for (uint32_t w = lane; w < cnt * cpr; w += 64) {
            const uint32_t i = w / cpr, u = w - i * cpr;
            const uint8_t* fslot = a.frames + (uint64_t)of_frame[i] * a.frame_stride;
            // the readable bytes end with the vector (no payload byte is touched)
            vector_block(a.row_coeffs + (out0 + base + i) * a.k, u * 16, a.k, of_idx[i], fslot, of_pay[i], of_pay[i]);
        }
        __syncthreads();
        base += cnt;
    }
    if (lane == 0) {
        a.n_rows[j] = base;
        a.entry_status[j] = QF_OK;
    }
}

}  // namespace

}  // namespace qf

extern "C" int qf_parse_poll_headers_dev(qf_ctx* ctx, uint32_t k, uint32_t L, uint32_t max_rows,
                                         const uint8_t* frames, uint64_t frame_stride, uint32_t N_max,
                                         const uint32_t* frame_len, const uint32_t* frame_off, const uint64_t* ids,
                                         const uint32_t* frame_gen, const uint32_t* n_frames, uint32_t G_src,
                                         uint32_t n_max, uint32_t* sel, uint32_t* n_sel, uint32_t* n_match,
                                         uint16_t* row_index, uint32_t* n_rows, uint8_t* row_coeffs,
                                         uint32_t* row_len, uint32_t* row_off, int32_t* entry_status,
                                         int32_t* frame_status) {
    if (!ctx) return QF_EINVAL;
    if (k == 0 || k > 256 || L == 0 || max_rows == 0 || max_rows > 1024) return QF_EINVAL;
    if (G_src == 0 || G_src > (1u << 24) || n_max == 0) return QF_EINVAL;
    // row_off is a u32 offset into the poll's N_max * frame_stride bytes
    if ((frame_stride & 15) || (N_max && frame_stride > (1ull << 32) / N_max)) return QF_EINVAL;
    if (!sel || !n_sel || !row_index || !n_rows || !row_coeffs || !row_len || !row_off || !entry_status)
        return QF_EINVAL;
    if (N_max && (!frames || !frame_len || !ids || !frame_gen || !frame_status)) return QF_EINVAL;
    if (!aligned16(frames)) return QF_EINVAL;
    std::unique_lock<std::mutex> lk;
    int s = qf::ctx_lock(ctx, lk);
    if (s) return s;
    hipStream_t st = qf::ctx_stream(ctx);
    // workspace: counts [G_src] | cursors [n_max] (zeroed together) | the
    // select's block counts | frame numbers [n_max][max_rows]
    qf::WorkLayout wl;
    const size_t off_counts = wl.take((size_t)G_src * 4);
    const size_t off_cursor = wl.take((size_t)n_max * 4);
    const size_t zero_end = wl.size();
    const size_t off_blocks = wl.take(qf::gen_select_work_bytes(G_src));
    const size_t off_place = wl.take((size_t)n_max * max_rows * 4);
    uint8_t* w = nullptr;
    s = qf::ctx_work(ctx, wl.size(), &w);
    if (s) return s;
    uint32_t* counts = reinterpret_cast<uint32_t*>(w + off_counts);
    uint32_t* cursor = reinterpret_cast<uint32_t*>(w + off_cursor);
    uint32_t* place = reinterpret_cast<uint32_t*>(w + off_place);
    QF_CHECK_HIP(hipMemsetAsync(w + off_counts, 0, zero_end - off_counts, st));
    const dim3 fgrid((N_max + 255) / 256);
    if (N_max) {
        qf::PollCountArgs ca{};
        ca.frame_gen = frame_gen;
        ca.n_frames = n_frames;
        ca.counts = counts;
        ca.N_max = N_max;
        ca.G_src = G_src;
        QF_PROFILED(ctx, st, "k_poll_count", qf::launch_kernel(qf::k_poll_count, fgrid, dim3(256), 0, st, ca));
    }
    QF_PROFILED(ctx, st, "k_gen_select",
                qf::launch_gen_select_list(counts, G_src, 1, n_max, reinterpret_cast<uint32_t*>(w + off_blocks), sel,
                                           n_sel, n_match, st));
    if (N_max) {
        qf::PollPlaceArgs pa{};
        pa.frame_gen = frame_gen;
        pa.n_frames = n_frames;
        pa.counts = counts;
        pa.sel = sel;
        pa.n_sel = n_sel;
        pa.cursor = cursor;
        pa.place = place;
        pa.frame_status = frame_status;
        pa.N_max = N_max;
        pa.G_src = G_src;
        pa.n_max = n_max;
        pa.max_rows = max_rows;
        QF_PROFILED(ctx, st, "k_poll_place", qf::launch_kernel(qf::k_poll_place, fgrid, dim3(256), 0, st, pa));
    }
    qf::PollHeadersArgs ha{};
    ha.frames = frames;
    ha.frame_stride = frame_stride;
    ha.frame_len = frame_len;
    ha.frame_off = frame_off;
    ha.ids = ids;
    ha.n_frames = n_frames;
    ha.counts = counts;
    ha.sel = sel;
    ha.n_sel = n_sel;
    ha.place = place;
    ha.row_index = row_index;
    ha.n_rows = n_rows;
    ha.row_coeffs = row_coeffs;
    ha.row_len = row_len;
    ha.row_off = row_off;
    ha.entry_status = entry_status;
    ha.frame_status = frame_status;
    ha.k = k;
    ha.L = L;
    ha.max_rows = max_rows;
    ha.N_max = N_max;
    ha.n_max = n_max;
    QF_PROFILED(ctx, st, "k_poll_headers", qf::launch_kernel(qf::k_poll_headers, dim3(n_max), dim3(64), 0, st, ha));
    return QF_OK;
}
