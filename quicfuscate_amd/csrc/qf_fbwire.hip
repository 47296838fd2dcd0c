// qf_fbwire.hip -- the feedback direction of the streaming loop as bytes
// (DESIGN.md 3.22): the 16-byte rank reports of qf_rank_report_sel_dev packed
// into feedback packets at the receiving side (qf_frame_reports_dev), a flat
// poll of such packets turned back into a report array at the sending side
// (qf_parse_report_frames_dev), and the report of a closed generation written
// again when frames of it still arrive (qf_report_closed_dev).
//
// A feedback packet: 0x02 | c (BE u16, >= 1) | c entries of {id BE u64, rank BE
// u16}, 3 + 10 c bytes.  The entries sit at odd byte offsets of their slot, and
// a parser may not read a byte behind the packet, so both directions move the
// entry bytes one at a time.
//
// Both directions place their outputs by a two-launch prefix as k_emit_count /
// k_emit_place do: the first launch leaves every block's sum in the workspace,
// the second sums the blocks in front of it.  No block waits for another; the
// second launch is the only ordering.
//
//  k_fbw_count    one wave per kFbPerBlock records, a record per lane: whether
//                 the record is sendable, the block's number of them.
//  k_fbw_pack     the same blocks again: the sendable records in front of the
//                 lane's, hence its packet and entry; the lane writes its ten
//                 entry bytes, the lane with entry 0 of a packet also the three
//                 header bytes and the packet's length.  One lane writes the
//                 call's three counts.
//  k_fbr_count    a packet per lane: the header's decision, the packet's number
//                 of entries (0 for one that is not QF_OK), the block's sum.
//  k_fbr_place    the same blocks again: where every packet's records begin, the
//                 three per-packet outputs; one lane writes the new length.
//  k_fbr_records  a wave per 64 entries of a packet: ten byte loads and one
//                 16-byte store per lane.
//  k_closed_mark  a frame per lane: the slot of a QF_ECLOSED frame whose window
//                 entry is that generation, closed, gets its flag set.  Every
//                 writer of a flag writes the same value.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qf_fec.h"
#include "qf_kernels.h"

#ifndef QF_DEV
#define QF_DEV __device__ __forceinline__
#endif

namespace qf {

namespace {

constexpr uint64_t kFbClosed = 1ull << 63;    // the window's closed flag (qf_window.hip)
constexpr uint64_t kFbIdLimit = 1ull << 62;
constexpr uint32_t kFbNone = 0xFFFFFFFFu;

QF_DEV uint32_t fb_wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

QF_DEV uint64_t fb_wave_sum64(uint64_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, o, 64), hi = __shfl_xor((uint32_t)(v >> 32), o, 64);
        v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

// ---------------------------------------------------------------------------
// records -> packets
// ---------------------------------------------------------------------------
QF_DEV uint32_t fbw_n_used(const FbPackArgs& a) {
    uint32_t n = a.N_max;
    if (a.n_reports) n = min(*a.n_reports, n);
    return n;
}

// Record j < n: the record, and whether it is sendable.  A record at or behind
// n is not looked at.
QF_DEV bool fbw_sendable(const FbPackArgs& a, uint32_t j, uint32_t n, uint4* rec) {
    if (j >= n) return false;
    *rec = a.reports[j];
    const uint64_t id = ((uint64_t)rec->y << 32) | rec->x;
    return id < kFbIdLimit && rec->z <= a.k && rec->w == 0;
}

__global__ void __launch_bounds__(64) k_fbw_count(FbPackArgs a) {
    const uint32_t lane = threadIdx.x;
    const uint32_t j = blockIdx.x * kFbPerBlock + lane;   // N_max <= 2^24
    uint4 rec;
    const uint32_t sum = fb_wave_sum(fbw_sendable(a, j, fbw_n_used(a), &rec) ? 1u : 0u);
    if (lane == 0) a.sums[blockIdx.x] = sum;
}

__global__ void __launch_bounds__(64) k_fbw_pack(FbPackArgs a) {
    const uint32_t lane = threadIdx.x;
    // the sendable records of the blocks before this one, and of all: S <= 2^24
    uint32_t before = 0, all = 0;
    for (uint32_t b = lane; b < a.blocks; b += 64) {
        const uint32_t s = a.sums[b];
        all += s;
        if (b < blockIdx.x) before += s;
    }
    before = fb_wave_sum(before);
    all = fb_wave_sum(all);
    const uint32_t n = fbw_n_used(a);
    const uint32_t j = blockIdx.x * kFbPerBlock + lane;
    uint4 rec = make_uint4(0, 0, 0, 0);
    const bool ok = fbw_sendable(a, j, n, &rec);
    const uint64_t bal = __ballot(ok);
    const uint32_t i = before + (uint32_t)__popcll(bal & (lane == 0 ? 0ull : (~0ull >> (64 - lane))));
    if (blockIdx.x == 0 && lane == 0) {
        const uint64_t room = (uint64_t)a.F_max * a.per;
        const uint64_t pkts = ((uint64_t)all + a.per - 1) / a.per;
        *a.n_pkts = pkts < a.F_max ? (uint32_t)pkts : a.F_max;
        if (a.n_left) *a.n_left = all > room ? (uint32_t)(all - room) : 0;
        if (a.n_skipped) *a.n_skipped = n - all;
    }
    if (!ok) return;
    const uint32_t p = i / a.per, e = i - p * a.per;
    if (p >= a.F_max) return;   // left for the next call
    uint8_t* const slot = a.pkts + (uint64_t)p * a.stride;
    if (e == 0) {
        const uint32_t c = min(a.per, all - p * a.per);   // p * per <= i < all
        slot[0] = 2;
        slot[1] = (uint8_t)(c >> 8);
        slot[2] = (uint8_t)c;
        a.pkt_len[p] = 3 + 10 * c;
    }
    uint8_t* const d = slot + 3 + 10 * e;   // 3 + 10 e + 10 <= 3 + 10 per <= max_len <= stride
    d[0] = (uint8_t)(rec.y >> 24);
    d[1] = (uint8_t)(rec.y >> 16);
    d[2] = (uint8_t)(rec.y >> 8);
    d[3] = (uint8_t)rec.y;
    d[4] = (uint8_t)(rec.x >> 24);
    d[5] = (uint8_t)(rec.x >> 16);
    d[6] = (uint8_t)(rec.x >> 8);
    d[7] = (uint8_t)rec.x;
    d[8] = (uint8_t)(rec.z >> 8);
    d[9] = (uint8_t)rec.z;
}

// ---------------------------------------------------------------------------
// packets -> records
// ---------------------------------------------------------------------------
// Packet f < F_max: its number of entries when it is QF_OK, else 0 (a QF_OK
// packet has one entry at least).  Reads the length, and bytes 0..2 of a packet
// of 3 bytes or more that lies in its slot.
QF_DEV uint32_t fbr_entries(const FbParseArgs& a, uint32_t f) {
    uint32_t n = a.F_max;
    if (a.n_pkts) n = min(*a.n_pkts, n);
    if (f >= n) return 0;
    const uint32_t len = a.pkt_len[f];
    if (len < 3 || len > a.max_len || len > a.stride) return 0;
    const uint8_t* const slot = a.pkts + (uint64_t)f * a.stride;
    if (slot[0] != 2) return 0;
    const uint32_t c = ((uint32_t)slot[1] << 8) | slot[2];
    return len == 3 + 10 * c ? c : 0;   // (c == 0 gives len 3 and no entry: not QF_OK)
}

__global__ void __launch_bounds__(64) k_fbr_count(FbParseArgs a) {
    const uint32_t lane = threadIdx.x;
    const uint64_t f = (uint64_t)blockIdx.x * kFbPerBlock + lane;
    uint32_t c = 0;
    if (f < a.F_max) {
        c = fbr_entries(a, (uint32_t)f);
        a.cnt[f] = c;
    }
    const uint32_t sum = fb_wave_sum(c);   // <= 64 * 6553
    if (lane == 0) a.sums[blockIdx.x] = sum;
}

__global__ void __launch_bounds__(64) k_fbr_place(FbParseArgs a) {
    const uint32_t lane = threadIdx.x;
    uint64_t before = 0, all = 0;
    for (uint32_t b = lane; b < a.blocks; b += 64) {
        const uint32_t s = a.sums[b];
        all += s;
        if (b < blockIdx.x) before += s;
    }
    before = fb_wave_sum64(before);
    all = fb_wave_sum64(all);
    const uint32_t base = a.append ? min(a.head[0], a.N_max) : 0;
    const uint64_t f = (uint64_t)blockIdx.x * kFbPerBlock + lane;
    const bool in = f < a.F_max;
    const uint32_t c = in ? a.cnt[f] : 0;
    // the exclusive prefix of the lanes' counts over the wave
    uint32_t tot = c, pre = 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t other = __shfl_xor(tot, o, 64);
        if (lane & o) pre += other;
        tot += other;
    }
    if (blockIdx.x == 0 && lane == 0) {
        const uint64_t end = base + all;
        *a.n_reports = end < a.N_max ? (uint32_t)end : a.N_max;
        if (a.n_left) {
            const uint64_t left = end > a.N_max ? end - a.N_max : 0;
            *a.n_left = left > kFbNone ? kFbNone : (uint32_t)left;
        }
    }
    if (!in) return;
    uint32_t n = a.F_max;
    if (a.n_pkts) n = min(*a.n_pkts, n);
    const uint64_t at = base + before + pre;   // where the packet's records begin
    a.first[f] = at < a.N_max ? (uint32_t)at : a.N_max;
    if (f >= n) return;
    if (a.pkt_status) a.pkt_status[f] = c ? QF_OK : QF_EINVAL;
    if (a.pkt_first) a.pkt_first[f] = !c ? kFbNone : at < kFbNone ? (uint32_t)at : kFbNone - 1;
    if (a.pkt_count) a.pkt_count[f] = c;
}

__global__ void __launch_bounds__(64) k_fbr_records(FbParseArgs a) {
    const uint32_t lane = threadIdx.x;
    const uint64_t total = (uint64_t)a.F_max * a.chunks;
    for (uint64_t w = blockIdx.x; w < total; w += a.rec_blocks) {
        const uint64_t f = w / a.chunks;
        const uint32_t e = (uint32_t)(w - f * a.chunks) * 64 + lane;
        if (e >= a.cnt[f]) continue;   // (0 for a packet that is not QF_OK, or at and behind F)
        const uint32_t i = a.first[f] + e;   // <= 2^24 + 6553
        if (i >= a.N_max) continue;
        const uint8_t* const s = a.pkts + f * a.stride + 3 + 10 * e;   // 3 + 10 e + 10 <= len
        const uint32_t hi = ((uint32_t)s[0] << 24) | ((uint32_t)s[1] << 16) | ((uint32_t)s[2] << 8) | s[3];
        const uint32_t lo = ((uint32_t)s[4] << 24) | ((uint32_t)s[5] << 16) | ((uint32_t)s[6] << 8) | s[7];
        a.reports[i] = make_uint4(lo, hi, ((uint32_t)s[8] << 8) | s[9], 0);
    }
}

// ---------------------------------------------------------------------------
// the re-report
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_closed_mark(ClosedMarkArgs a) {
    const uint64_t f = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t n = a.F_max;
    if (a.n_frames) n = min(*a.n_frames, n);
    if (f >= n) return;
    if (a.frame_status[f] != QF_ECLOSED) return;
    const uint64_t id = a.frame_id[f];
    if (id >= kFbIdLimit) return;   // nothing is read through a bad id
    const uint32_t s = (uint32_t)(id % a.G_src);
    if (a.win[s] == ((id + 1) | kFbClosed)) a.flags[s] = 1;
}

}  // namespace

static bool fb_pack_ok(const FbPackArgs& a) {
    return a.reports && a.pkts && a.pkt_len && a.n_pkts && a.sums && a.k && a.k <= 256 && a.per && a.per <= 6553 &&
           a.F_max && a.N_max && a.N_max <= (1u << 24) && a.stride >= 3 + 10ull * a.per &&
           a.blocks == (a.N_max + kFbPerBlock - 1) / kFbPerBlock;
}

hipError_t launch_fbw_count(const FbPackArgs& a, hipStream_t st) {
    if (!fb_pack_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fbw_count, dim3(a.blocks), dim3(64), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_fbw_pack(const FbPackArgs& a, hipStream_t st) {
    if (!fb_pack_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fbw_pack, dim3(a.blocks), dim3(64), 0, st, a);
    return hipGetLastError();
}

uint32_t fb_parse_blocks(uint32_t F_max) { return (uint32_t)(((uint64_t)F_max + kFbPerBlock - 1) / kFbPerBlock); }

static bool fb_parse_ok(const FbParseArgs& a) {
    return a.pkts && a.pkt_len && a.reports && a.n_reports && a.cnt && a.first && a.sums && (!a.append || a.head) &&
           a.per && a.per <= 6553 && a.max_len >= 13 && a.max_len <= 65535 && a.F_max && a.N_max &&
           a.N_max <= (1u << 24) && a.stride >= a.max_len && a.blocks == fb_parse_blocks(a.F_max) &&
           a.chunks == (a.per + 63) / 64;
}

hipError_t launch_fbr_count(const FbParseArgs& a, hipStream_t st) {
    if (!fb_parse_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fbr_count, dim3(a.blocks), dim3(64), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_fbr_place(const FbParseArgs& a, hipStream_t st) {
    if (!fb_parse_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fbr_place, dim3(a.blocks), dim3(64), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_fbr_records(FbParseArgs a, hipStream_t st) {
    if (!fb_parse_ok(a)) return hipErrorInvalidValue;
    const uint64_t total = (uint64_t)a.F_max * a.chunks;
    a.rec_blocks = total < kFbRecordBlocks ? (uint32_t)total : kFbRecordBlocks;   // the rest is strided
    hipLaunchKernelGGL(k_fbr_records, dim3(a.rec_blocks), dim3(64), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_closed_mark(const ClosedMarkArgs& a, hipStream_t st) {
    if (!a.frame_id || !a.frame_status || !a.win || !a.flags || a.F_max == 0 || a.G_src == 0 || a.G_src > (1u << 24))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_closed_mark, dim3((uint32_t)(((uint64_t)a.F_max + 255) / 256)), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace qf

extern "C" uint32_t qf_report_frame_capacity(uint32_t max_len) {
    return max_len >= 13 && max_len <= 65535 ? (max_len - 3) / 10 : 0;
}

#ifndef QF_KERNEL_EMU   // (tests/kernel_emu builds the kernels and launchers above for the host)
#include <mutex>

#include "qf_internal.h"

static bool fb_shape_ok(const qf_report_wire_shape* sh, uint32_t N_max, uint32_t flags_allowed) {
    return sh->k >= 1 && sh->k <= 256 && sh->max_len >= 13 && sh->max_len <= 65535 && sh->F_max && N_max &&
           N_max <= (1u << 24) && !(sh->flags & ~flags_allowed) && sh->stride % 16 == 0 && sh->stride >= sh->max_len;
}

extern "C" int qf_frame_reports_dev(qf_ctx* ctx, const qf_report_wire_shape* sh, uint32_t N_max,
                                    const qf_rank_report* reports, const uint32_t* n_reports, uint8_t* pkts,
                                    uint32_t* pkt_len, uint32_t* n_pkts, uint32_t* n_left, uint32_t* n_skipped) {
    if (!ctx || !sh || !reports || !pkts || !pkt_len || !n_pkts) return QF_EINVAL;
    if (!fb_shape_ok(sh, N_max, 0) || !aligned16(reports) || !aligned16(pkts)) return QF_EINVAL;
    std::unique_lock<std::mutex> lk;
    int s = qf::ctx_lock(ctx, lk);
    if (s) return s;
    hipStream_t st = qf::ctx_stream(ctx);
    qf::FbPackArgs a{};
    a.blocks = (N_max + qf::kFbPerBlock - 1) / qf::kFbPerBlock;
    // workspace: the blocks' sums
    uint8_t* w = nullptr;
    s = qf::ctx_work(ctx, (size_t)a.blocks * 4, &w);
    if (s) return s;
    a.reports = reinterpret_cast<const uint4*>(reports);
    a.n_reports = n_reports;
    a.pkts = pkts;
    a.pkt_len = pkt_len;
    a.n_pkts = n_pkts;
    a.n_left = n_left;
    a.n_skipped = n_skipped;
    a.sums = reinterpret_cast<uint32_t*>(w);
    a.stride = sh->stride;
    a.N_max = N_max;
    a.k = sh->k;
    a.per = qf_report_frame_capacity(sh->max_len);
    a.F_max = sh->F_max;
    QF_PROFILED(ctx, st, "k_fbw_count", qf::launch_fbw_count(a, st));
    QF_PROFILED(ctx, st, "k_fbw_pack", qf::launch_fbw_pack(a, st));
    return QF_OK;
}

extern "C" int qf_parse_report_frames_dev(qf_ctx* ctx, const qf_report_wire_shape* sh, const uint8_t* pkts,
                                          const uint32_t* pkt_len, const uint32_t* n_pkts, uint32_t N_max,
                                          qf_rank_report* reports, uint32_t* n_reports, uint32_t* n_left,
                                          int32_t* pkt_status, uint32_t* pkt_first, uint32_t* pkt_count) {
    if (!ctx || !sh || !pkts || !pkt_len || !reports || !n_reports) return QF_EINVAL;
    if (!fb_shape_ok(sh, N_max, QF_REPORT_APPEND) || !aligned16(reports) || !aligned16(pkts)) return QF_EINVAL;
    std::unique_lock<std::mutex> lk;
    int s = qf::ctx_lock(ctx, lk);
    if (s) return s;
    hipStream_t st = qf::ctx_stream(ctx);
    qf::FbParseArgs a{};
    a.blocks = qf::fb_parse_blocks(sh->F_max);
    // workspace: cnt [F_max] | first [F_max] | the blocks' sums | the base of an appending call
    qf::WorkLayout wl;
    const size_t off_cnt = wl.take((size_t)sh->F_max * 4);
    const size_t off_first = wl.take((size_t)sh->F_max * 4);
    const size_t off_sums = wl.take((size_t)a.blocks * 4);
    const size_t off_head = wl.take(4);
    uint8_t* w = nullptr;
    s = qf::ctx_work(ctx, wl.size(), &w);
    if (s) return s;
    a.pkts = pkts;
    a.pkt_len = pkt_len;
    a.n_pkts = n_pkts;
    a.reports = reinterpret_cast<uint4*>(reports);
    a.n_reports = n_reports;
    a.n_left = n_left;
    a.pkt_status = pkt_status;
    a.pkt_first = pkt_first;
    a.pkt_count = pkt_count;
    a.cnt = reinterpret_cast<uint32_t*>(w + off_cnt);
    a.first = reinterpret_cast<uint32_t*>(w + off_first);
    a.sums = reinterpret_cast<uint32_t*>(w + off_sums);
    a.stride = sh->stride;
    a.F_max = sh->F_max;
    a.N_max = N_max;
    a.max_len = sh->max_len;
    a.per = qf_report_frame_capacity(sh->max_len);
    a.chunks = (a.per + 63) / 64;
    a.append = sh->flags & QF_REPORT_APPEND;
    if (a.append) {
        // the length the call appends at, taken before the kernel that overwrites it
        QF_CHECK_HIP(hipMemcpyAsync(w + off_head, n_reports, 4, hipMemcpyDeviceToDevice, st));
        a.head = reinterpret_cast<const uint32_t*>(w + off_head);
    }
    QF_PROFILED(ctx, st, "k_fbr_count", qf::launch_fbr_count(a, st));
    QF_PROFILED(ctx, st, "k_fbr_place", qf::launch_fbr_place(a, st));
    QF_PROFILED(ctx, st, "k_fbr_records", qf::launch_fbr_records(a, st));
    return QF_OK;
}

extern "C" int qf_report_closed_dev(qf_ctx* ctx, uint32_t k, uint32_t G_src, uint32_t F_max, const uint64_t* frame_id,
                                    const int32_t* frame_status, const uint32_t* n_frames, const uint64_t* win,
                                    uint32_t N_max, uint32_t flags, qf_rank_report* reports, uint32_t* n_reports,
                                    uint32_t* n_left) {
    if (!ctx || !frame_id || !frame_status || !win || !reports || !n_reports) return QF_EINVAL;
    if (k == 0 || k > 256 || G_src == 0 || G_src > (1u << 24) || F_max == 0 || N_max == 0) return QF_EINVAL;
    if ((flags & ~(uint32_t)QF_REPORT_APPEND) || (reinterpret_cast<uintptr_t>(win) & 7) || !aligned16(reports))
        return QF_EINVAL;
    std::unique_lock<std::mutex> lk;
    int s = qf::ctx_lock(ctx, lk);
    if (s) return s;
    hipStream_t st = qf::ctx_stream(ctx);
    // workspace: the slots' flags [G_src] (zeroed) | the list of the marked slots
    // [G_src] | its length | the select's block counts | the base of an appending call
    qf::WorkLayout wl;
    const size_t off_flags = wl.take((size_t)G_src * 4);
    const size_t off_list = wl.take((size_t)G_src * 4);
    const size_t off_n = wl.take(4);
    const size_t off_blocks = wl.take(qf::gen_select_work_bytes(G_src));
    const size_t off_head = wl.take(4);
    uint8_t* w = nullptr;
    s = qf::ctx_work(ctx, wl.size(), &w);
    if (s) return s;
    qf::ClosedMarkArgs m{};
    m.frame_id = frame_id;
    m.frame_status = frame_status;
    m.n_frames = n_frames;
    m.win = win;
    m.flags = reinterpret_cast<uint32_t*>(w + off_flags);
    m.F_max = F_max;
    m.G_src = G_src;
    qf::ReportSelArgs a{};
    a.sel = reinterpret_cast<const uint32_t*>(w + off_list);
    a.n_sel = reinterpret_cast<const uint32_t*>(w + off_n);
    a.win = win;
    a.rank = m.flags;   // every listed entry is closed, and a closed entry's rank is not used: any G_src words do
    a.reports = reinterpret_cast<uint4*>(reports);
    a.n_reports = n_reports;
    a.n_left = n_left;
    a.n_max = G_src;
    a.G_src = G_src;
    a.k = k;
    a.N_max = N_max;
    a.append = flags & QF_REPORT_APPEND;
    if (a.append) {
        QF_CHECK_HIP(hipMemcpyAsync(w + off_head, n_reports, 4, hipMemcpyDeviceToDevice, st));
        a.head = reinterpret_cast<const uint32_t*>(w + off_head);
    }
    QF_CHECK_HIP(hipMemsetAsync(w + off_flags, 0, (size_t)G_src * 4, st));
    QF_PROFILED(ctx, st, "k_closed_mark", qf::launch_closed_mark(m, st));
    QF_PROFILED(ctx, st, "k_gen_select",
                qf::launch_gen_select_list(m.flags, G_src, 1, G_src, reinterpret_cast<uint32_t*>(w + off_blocks),
                                           reinterpret_cast<uint32_t*>(w + off_list),
                                           reinterpret_cast<uint32_t*>(w + off_n), nullptr, st));
    QF_PROFILED(ctx, st, "k_report_sel", qf::launch_report_sel(a, st));
    return QF_OK;
}
#endif  // QF_KERNEL_EMU
