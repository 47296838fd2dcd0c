// qf_deliver.hip -- the last step of the streaming receive loop (DESIGN.md
// 3.19): qf_deliver_frames_dev takes a decode's outputs (src_slot, rec_index,
// n_rec, rec, status) and the row store and writes each generation's source
// packets in source order into one contiguous output, each packet of a wire
// generation once across calls (the delivered state: a tag and 256 bits per
// generation slot).
//
//  k_deliver_prepare  one wave per entry, four sources per lane (k <= 256).
//                     Checks every index it is about to use (the inputs are
//                     device arrays a caller may fill wrongly), counts per
//                     source in LDS how often S and rec_index name it (so a
//                     duplicate is found whatever the order of the lanes),
//                     merges with the delivered mask and tag, writes out_len,
//                     out_state, the counts, the status and the new state, and
//                     leaves one 16-byte record per packet to copy, compacted
//                     in ascending source order by a ballot prefix, plus the
//                     entry's count (qf_kernels.h, DeliverPrepareArgs).
//  k_deliver_rows     the copy.  A wave takes four records of one entry at a
//                     time (a "quad": the entry and the record position follow
//                     from one 32-bit division per quad, wave-uniform); the
//                     entry's count and the four records are loaded together,
//                     one round trip, and made scalar.  Its lanes stride over
//                     the 16-byte units of the four rows together: the four
//                     loads of a step carry no branch (a row without a byte in
//                     the lane's unit loads the quad's longest row's unit and
//                     drops it), so all four are in flight before the first
//                     store; a stored unit is masked to its row's bytes
//                     (load_row_unit's rule of qf_gf_dev.h, restated here: this
//                     file compiles for the host in tests/kernel_emu).  Only
//                     units that hold a byte of a delivered row are read.  The
//                     grid is bounded and strides over the remaining quads.
// Both kernels have a form over a list (k_deliver_prepare_sel /
// k_deliver_rows_sel in the profile): the source side is the listed
// generation's.  The copy is the same code for both, as the records carry
// whole offsets.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qf_kernels.h"

#define QF_DEV __device__ __forceinline__

namespace qf {

namespace {

// (the status values of qf_fec.h, which this part does not include)
constexpr int32_t kOk = 0, kEinval = -1, kEnotready = -3;
constexpr uint8_t kSrcStored = 1, kSrcRecovered = 2, kSrcEarlier = 3;

// An entry that delivers nothing: zero outputs, no record.
QF_DEV void deliver_nothing(const DeliverPrepareArgs& a, uint32_t j, uint32_t lane, int32_t status) {
    for (uint32_t i = lane; i < a.k; i += 64) {
        a.out_len[(uint64_t)j * a.k + i] = 0;
        a.out_state[(uint64_t)j * a.k + i] = 0;
    }
    if (lane == 0) {
        a.n_out[j] = 0;
        if (a.n_known) a.n_known[j] = 0;
        a.status[j] = status;
        a.cnt[j] = 0;
    }
}

// SEL: j is a list entry and gs its generation, which indexes the row arrays,
// the delivered state and the source region; without SEL gs is j.
template <bool SEL>
__global__ void __launch_bounds__(64) k_deliver_prepare(DeliverPrepareArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint32_t* count = reinterpret_cast<uint32_t*>(lds);           // 256: times source i is named
    uint16_t* rpos = reinterpret_cast<uint16_t*>(lds + 4 * 256);  // 256: the rec row of source i
    const uint32_t j = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const uint32_t k = a.k;
    uint32_t gs = j;
    int32_t status = kOk;
    if constexpr (SEL) {
        uint32_t n_used = a.G;
        if (a.n_sel) n_used = min(*a.n_sel, n_used);
        // an unused entry's sel value is not looked at; nothing is read or
        // written through an invalid one
        if (j >= n_used) status = kEnotready;
        else if ((gs = a.sel[j]) >= a.G_src) status = kEinval;
    }
    if (status == kOk) {
        const int32_t ds = a.dec_status[j];
        if (ds != kOk && ds != kEnotready) status = kEnotready;
    }
    const bool tagged = a.delivered && a.ids;
    uint64_t tag = 0;
    uint32_t n_rec = 0;
    if (status == kOk) {
        if (tagged) {
            const uint64_t id = a.ids[j];
            if (id >= (1ull << 62)) status = kEinval;   // UINT64_MAX (no generation) included
            tag = id + 1;
        }
        n_rec = a.n_rec[j];
        if (n_rec > a.e_max) status = kEinval;
    }
    if (status != kOk) {
        deliver_nothing(a, j, lane, status);
        return;
    }
    // S, and the count of every source
    bool bad = false;
    uint32_t slot[4], off[4], len[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t i = lane + 64 * q;
        slot[q] = 0xFFFF;
        off[q] = len[q] = 0;
        if (i < k) {
            const uint32_t s = a.src_slot[(uint64_t)j * k + i];
            if (s != 0xFFFF && s >= a.max_rows) bad = true;
            else slot[q] = s;
        }
        count[i] = slot[q] != 0xFFFF ? 1 : 0;
    }
    __syncthreads();
    for (uint32_t m = lane; m < n_rec; m += 64) {
        const uint32_t idx = a.rec_index[(uint64_t)j * a.e_max + m];
        if (idx >= k) bad = true;
        else {
            atomicAdd(&count[idx], 1u);
            rpos[idx] = (uint16_t)m;   // (named twice: QF_EINVAL below, and rpos is not used)
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t i = lane + 64 * q;
        if (count[i] > 1) bad = true;
        if (slot[q] != 0xFFFF) {
            off[q] = a.row_off[(uint64_t)gs * a.max_rows + slot[q]];
            len[q] = a.row_len[(uint64_t)gs * a.max_rows + slot[q]];
            if (len[q] > a.L || (off[q] & 15) || (uint64_t)off[q] + len[q] > a.src_gen_stride) bad = true;
        }
    }
    if (__any(bad)) {
        deliver_nothing(a, j, lane, kEinval);
        return;
    }
    // the delivered mask: that of another wire generation counts as empty
    uint64_t old[4] = {0, 0, 0, 0};
    uint64_t* dw = a.delivered ? a.delivered + (uint64_t)gs * 5 : nullptr;
    if (dw && (!tagged || dw[0] == tag)) {
#pragma unroll
        for (int q = 0; q < 4; ++q) old[q] = dw[1 + q];
    }
    const uint64_t lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    uint32_t n_new = 0, n_known = 0;
    uint64_t fresh[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t i = lane + 64 * q;
        const bool known = i < k && count[i] == 1;
        const bool earlier = i < k && ((old[q] >> lane) & 1);
        const bool isnew = known && !earlier;
        const bool stored = slot[q] != 0xFFFF;
        fresh[q] = __ballot(isnew);
        n_known += (uint32_t)__popcll(__ballot(known || earlier));
        if (i < k) {
            a.out_len[(uint64_t)j * k + i] = isnew ? (stored ? len[q] : a.L) : 0;
            a.out_state[(uint64_t)j * k + i] = isnew ? (stored ? kSrcStored : kSrcRecovered) : earlier ? kSrcEarlier : 0;
        }
        if (isnew) {
            const uint32_t t = n_new + (uint32_t)__popcll(fresh[q] & lt_mask);
            const uint64_t at = stored ? (uint64_t)gs * a.src_gen_stride + off[q]
                                       : (uint64_t)j * a.rec_gen_stride + (uint64_t)rpos[i] * a.rec_row_stride;
            a.rec[(uint64_t)j * k + t] = make_uint4((uint32_t)at, (uint32_t)(at >> 32) | (stored ? 0u : kDeliverFromRec),
                                                    stored ? len[q] : a.L, i);
        }
        n_new += (uint32_t)__popcll(fresh[q]);
    }
    if (lane == 0) {
        if (dw && n_new) {
            if (tagged) dw[0] = tag;
#pragma unroll
            for (int q = 0; q < 4; ++q) dw[1 + q] = old[q] | fresh[q];
        }
        a.n_out[j] = n_new;
        if (a.n_known) a.n_known[j] = n_known;
        a.status[j] = kOk;
        a.cnt[j] = n_new;
    }
}

// The bytes of a 16-byte unit that lie inside a row: v = the row's bytes at and
// after the unit's first (0: none, 16 and more: all), as load_row_unit of
// qf_gf_dev.h masks them, without a branch.
QF_DEV uint32_t low_bytes(uint32_t nb) { return nb >= 4 ? 0xFFFFFFFFu : (1u << (8 * nb)) - 1; }
QF_DEV uint4 mask_unit(uint4 x, uint32_t v) {
    x.x &= low_bytes(v);
    x.y &= low_bytes(v > 4 ? v - 4 : 0);
    x.z &= low_bytes(v > 8 ? v - 8 : 0);
    x.w &= low_bytes(v > 12 ? v - 12 : 0);
    return x;
}

// Global memory said so: a row's base is one of two buffers, and without the
// address space the select between them makes the loads flat ones.
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(1))) uint4* RowUnitPtr;
#else
typedef const uint4* RowUnitPtr;
#endif
QF_DEV uint4 load_global_unit(const uint8_t* p) {
    const RowUnitPtr g = (RowUnitPtr)(uintptr_t)p;
    return make_uint4(g->x, g->y, g->z, g->w);
}

__global__ void __launch_bounds__(256) k_deliver_rows(DeliverRowsArgs a) {
    const uint32_t lane = threadIdx.x & 63;
    // (wave-uniform by construction; said so, the quad's arithmetic is scalar)
    const uint32_t w0 = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    for (uint32_t q = w0; q < a.n_quads; q += a.n_waves) {
        const uint32_t j = q / a.kq, t0 = (q - j * a.kq) * 4;
        // the count and the four records in one round trip: the records are
        // loaded whether or not the count covers them (positions clamped to the
        // entry's k, so inside the workspace) and looked at only when it does
        const uint4* r = a.rec + (uint64_t)j * a.k;
        uint4 rr[4];
#pragma unroll
        for (int x = 0; x < 4; ++x) rr[x] = r[min(t0 + x, a.k - 1)];
        const uint32_t c = a.cnt[j];
        if (t0 >= c) continue;
        const uint32_t n = min(c - t0, 4u);
        uint8_t* const og = a.out + (uint64_t)j * a.out_gen_stride;
        const uint8_t* sp[4];
        uint8_t* dp[4];
        uint32_t len[4], longest = 0;
        const uint8_t* sp_long = a.src;
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            const bool used = (uint32_t)x < n;
            // (a record the count does not cover is not looked at: its row is the source base, length 0)
            const uint64_t at = used ? ((uint64_t)(rr[x].y & ~kDeliverFromRec) << 32) | rr[x].x : 0;
            sp[x] = (used && (rr[x].y & kDeliverFromRec) ? a.rec_rows : a.src) + at;
            dp[x] = og + (uint64_t)(used ? rr[x].w : 0) * a.out_row_stride;
            len[x] = used ? rr[x].z : 0;
            if (len[x] > longest) {
                longest = len[x];
                sp_long = sp[x];
            }
        }
        // Every lane in the loop has a unit of the longest row, so a row that
        // has no byte in the lane's unit loads the longest row's instead (a
        // unit that holds a byte of a delivered row, as the read rule wants)
        // and drops it: four loads without a branch between them, all issued
        // before the first is waited for.
        for (uint32_t u16 = lane * 16; u16 < longest; u16 += 64 * 16) {
            uint4 v[4];
#pragma unroll
            for (int x = 0; x < 4; ++x) v[x] = load_global_unit((len[x] > u16 ? sp[x] : sp_long) + u16);
#pragma unroll
            for (int x = 0; x < 4; ++x)
                if (len[x] > u16) *reinterpret_cast<uint4*>(dp[x] + u16) = mask_unit(v[x], len[x] - u16);
        }
    }
}

}  // namespace

hipError_t launch_deliver_prepare(const DeliverPrepareArgs& a, hipStream_t st) {
    if (a.G == 0) return hipSuccess;
    if (!a.row_off || !a.row_len || !a.n_rec || !a.dec_status || !a.src_slot || !a.out_len || !a.out_state ||
        !a.n_out || !a.status || !a.rec || !a.cnt || (a.e_max && !a.rec_index) || a.k == 0 || a.k > 256 ||
        a.max_rows == 0 || (a.sel && a.G_src == 0))
        return hipErrorInvalidValue;
    if (a.sel) hipLaunchKernelGGL(k_deliver_prepare<true>, dim3(a.G), dim3(64), kDeliverPrepareLds, st, a);
    else hipLaunchKernelGGL(k_deliver_prepare<false>, dim3(a.G), dim3(64), kDeliverPrepareLds, st, a);
    return hipGetLastError();
}

hipError_t launch_deliver_rows(DeliverRowsArgs a, uint32_t G, uint32_t grid_cap, hipStream_t st) {
    if (G == 0) return hipSuccess;
    if (!a.src || !a.out || !a.rec || !a.cnt || a.k == 0 || a.k > 256 || G > (1u << 24) || grid_cap == 0)
        return hipErrorInvalidValue;
    a.kq = (a.k + 3) / 4;
    a.n_quads = G * a.kq;   // <= 2^30
    const uint32_t need = (a.n_quads + 3) / 4;
    const uint32_t blocks = need < grid_cap ? need : grid_cap;
    a.n_waves = blocks * 4;
    hipLaunchKernelGGL(k_deliver_rows, dim3(blocks), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace qf

#ifndef QF_KERNEL_EMU   // (tests/kernel_emu builds the kernels and launchers above for the host)
#include <mutex>

#include "qf_fec.h"
#include "qf_internal.h"

// qf_deliver_frames_dev over G generations, and with `sel` qf_deliver_frames_sel_dev
// over its n_max entries (G = n_max).
static int deliver_run(qf_ctx* ctx, const qf_deliver_shape* sh, uint32_t G, const qf_gen_sel* sel,
                       const uint8_t* src, const uint32_t* row_off, const uint32_t* row_len, const uint8_t* rec,
                       const uint16_t* rec_index, const uint32_t* n_rec, const int32_t* dec_status,
                       const uint16_t* src_slot, const uint64_t* ids, uint64_t* delivered, uint8_t* out,
                       uint32_t* out_len, uint8_t* out_state, uint32_t* n_out, uint32_t* n_known, int32_t* status) {
    if (!ctx || !sh) return QF_EINVAL;
    const uint32_t k = sh->k, L = sh->L, max_rows = sh->max_rows, e_max = sh->e_max;
    if (k == 0 || k > 256 || e_max > 128 || L == 0 || max_rows == 0 || max_rows > 1024 || sh->flags != 0 ||
        sh->reserved != 0 || G > (1u << 24))
        return QF_EINVAL;
    if ((sh->src_gen_stride & 15) || (sh->rec_row_stride & 15) || (sh->rec_gen_stride & 15) ||
        (sh->out_row_stride & 15) || (sh->out_gen_stride & 15) || sh->rec_row_stride < L ||
        sh->out_row_stride < round_up(L, 16) || sh->out_gen_stride / k < sh->out_row_stride)
        return QF_EINVAL;
    if (G == 0) return QF_OK;
    if (!src || !row_off || !row_len || !n_rec || !dec_status || !src_slot || !out || !out_len || !out_state ||
        !n_out || !status || (e_max && (!rec || !rec_index)))
        return QF_EINVAL;
    if (!aligned16(src) || !aligned16(rec) || !aligned16(out) || (reinterpret_cast<uintptr_t>(delivered) & 7))
        return QF_EINVAL;
    std::unique_lock<std::mutex> lk;
    int s = qf::ctx_lock(ctx, lk);
    if (s) return s;
    hipStream_t st = qf::ctx_stream(ctx);
    // workspace: records [G][k] of 16 bytes | counts [G]
    qf::WorkLayout wl;
    const size_t off_rec = wl.take((size_t)G * k * sizeof(uint4));
    const size_t off_cnt = wl.take((size_t)G * 4);
    uint8_t* w = nullptr;
    s = qf::ctx_work(ctx, wl.size(), &w);
    if (s) return s;
    qf::DeliverPrepareArgs pa{};
    pa.row_off = row_off;
    pa.row_len = row_len;
    pa.rec_index = rec_index;
    pa.n_rec = n_rec;
    pa.dec_status = dec_status;
    pa.src_slot = src_slot;
    pa.ids = ids;
    pa.delivered = delivered;
    pa.out_len = out_len;
    pa.out_state = out_state;
    pa.n_out = n_out;
    pa.n_known = n_known;
    pa.status = status;
    pa.rec = reinterpret_cast<uint4*>(w + off_rec);
    pa.cnt = reinterpret_cast<uint32_t*>(w + off_cnt);
    pa.src_gen_stride = sh->src_gen_stride;
    pa.rec_row_stride = sh->rec_row_stride;
    pa.rec_gen_stride = sh->rec_gen_stride;
    pa.k = k;
    pa.e_max = e_max;
    pa.L = L;
    pa.max_rows = max_rows;
    pa.G = G;
    if (sel) {
        pa.sel = sel->sel_dev;
        pa.n_sel = sel->n_sel_dev;
        pa.G_src = sel->G_src;
    }
    QF_PROFILED(ctx, st, sel ? "k_deliver_prepare_sel" : "k_deliver_prepare", qf::launch_deliver_prepare(pa, st));
    qf::DeliverRowsArgs ra{};
    ra.src = src;
    ra.rec_rows = rec;
    ra.out = out;
    ra.rec = pa.rec;
    ra.cnt = pa.cnt;
    ra.out_row_stride = sh->out_row_stride;
    ra.out_gen_stride = sh->out_gen_stride;
    ra.k = k;
    // a wave per four records; the grid is bounded and strides over the rest
    const uint32_t cap = (uint32_t)(qf::ctx_num_cus(ctx) > 0 ? qf::ctx_num_cus(ctx) : 1) * qf::kDeliverGroupsPerCu;
    QF_PROFILED(ctx, st, sel ? "k_deliver_rows_sel" : "k_deliver_rows", qf::launch_deliver_rows(ra, G, cap, st));
    return QF_OK;
}

extern "C" int qf_deliver_frames_dev(qf_ctx* ctx, const qf_deliver_shape* sh, uint32_t G, const uint8_t* src,
                                     const uint32_t* row_off, const uint32_t* row_len, const uint8_t* rec,
                                     const uint16_t* rec_index, const uint32_t* n_rec, const int32_t* dec_status,
                                     const uint16_t* src_slot, const uint64_t* ids, uint64_t* delivered,
                                     uint8_t* out, uint32_t* out_len, uint8_t* out_state, uint32_t* n_out,
                                     uint32_t* n_known, int32_t* status) {
    return deliver_run(ctx, sh, G, nullptr, src, row_off, row_len, rec, rec_index, n_rec, dec_status, src_slot, ids,
                       delivered, out, out_len, out_state, n_out, n_known, status);
}

extern "C" int qf_deliver_frames_sel_dev(qf_ctx* ctx, const qf_deliver_shape* sh, const qf_gen_sel* sel,
                                         const uint8_t* src, const uint32_t* row_off, const uint32_t* row_len,
                                         const uint8_t* rec, const uint16_t* rec_index, const uint32_t* n_rec,
                                         const int32_t* dec_status, const uint16_t* src_slot, const uint64_t* ids,
                                         uint64_t* delivered, uint8_t* out, uint32_t* out_len, uint8_t* out_state,
                                         uint32_t* n_out, uint32_t* n_known, int32_t* status) {
    if (!sel || !sel->sel_dev || sel->n_max == 0 || sel->G_src == 0) return QF_EINVAL;
    return deliver_run(ctx, sh, sel->n_max, sel, src, row_off, row_len, rec, rec_index, n_rec, dec_status, src_slot,
                       ids, delivered, out, out_len, out_state, n_out, n_known, status);
}
#endif  // QF_KERNEL_EMU
