// qf_emit.hip -- the send step of the streaming loop:
// qf_emit_frames_sel_dev takes the compact rows of a list (a listed recode's
// outputs, or a source's packets), an emission budget per generation and a flat
// frame queue, and appends each entry's frames to the queue without a hole: the
// flat poll that qf_gen_window_dev / qf_parse_poll_headers_dev of the next hop
// read.
//
//  k_emit_count   one wave per kEmitPerBlock entries, one entry per lane.
//                 Checks every entry (the list value, the id,
//                 the metadata of its first n rows; every index before it is
//                 used), derives the number of frames it wants from its rows and
//                 the budget rank - sent, and leaves that number, the entry's
//                 status so far and the block's sum in the workspace.  Block 0
//                 snapshots the queue's base, which the next kernel overwrites.
//  k_emit_place   the same blocks again: each sums the blocks before it (and all
//                 of them, for the frames left over), scans its own entries and
//                 so knows where every entry's frames go.  An entry is emitted
//                 iff its last frame is inside the queue; the positions only
//                 grow, so the emitted entries are a prefix of those that want
//                 frames.  Writes the per-entry outputs, sent, the per-frame
//                 metadata, one 16-byte record per frame, and -- from the one
//                 entry at the cutoff, or from block 0 when everything fits --
//                 the queue's new length.  No block waits for another; the
//                 second launch is the only ordering.
//  k_emit_frames  the bytes.  A wave takes four consecutive frames of the queue
//                 at a time; the four records are loaded together and made
//                 scalar.  Its lanes stride over the 16-byte units of the four
//                 payloads together as k_deliver_rows does: four loads without a
//                 branch between them, all in flight before the first store; a
//                 whole unit is one store, the row's last bytes at most four
//                 stores (8, 4, 2, 1 bytes), so no byte behind the frame is
//                 written.  Then sixteen lanes per frame write its header's
//                 16-byte blocks: whole blocks of the coefficient vector through
//                 vector_copy_block of qf_wire_dev.h (an aligned 16-byte load, or
//                 aligned dwords joined with v_alignbit), the block that holds
//                 the frame's first bytes and a last block whose dwords would
//                 reach past the vector byte by byte.  The grid is bounded and
//                 strides over the remaining quads.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qf_kernels.h"
#include "qf_wire_dev.h"

namespace qf {

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;

QF_DEV uint32_t emit_wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

QF_DEV uint64_t emit_wave_sum64(uint64_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, o, 64), hi = __shfl_xor((uint32_t)(v >> 32), o, 64);
        v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

QF_DEV uint32_t emit_n_used(const EmitPlanArgs& a) {
    uint32_t n = a.n_max;
    if (a.n_sel) n = min(*a.n_sel, n);
    return n;
}

// Entry j < n_max: its status so far and the frames it wants.  An unused
// entry's sel value is not looked at, and nothing is read through an invalid
// entry.
QF_DEV int32_t emit_entry(const EmitPlanArgs& a, uint32_t j, uint32_t n_used, uint32_t* want) {
    *want = 0;
    if (j >= n_used) return QF_ENOTREADY;
    const uint32_t g = a.sel[j];
    if (g >= a.G_src) return QF_EINVAL;
    if (a.ids[j] >= (1ull << 62)) return QF_EINVAL;   // UINT64_MAX (no generation) included
    const uint32_t nj = a.n_rows ? min(a.n_rows[j], a.max_rows) : a.max_rows;
    bool bad = false;
    for (uint32_t s = 0; s < nj; ++s) {
        const uint64_t f = (uint64_t)j * a.max_rows + s;
        if (a.row_len && a.row_len[f] > a.L) bad = true;
        if (a.row_index && !a.has_coeffs && a.row_index[f] >= a.k) bad = true;   // a coded row without its vector
    }
    if (bad) return QF_EINVAL;
    if (a.in_status) {
        const int32_t st = a.in_status[j];
        if (st != QF_OK) return st;
    }
    uint32_t c = nj;
    if (a.rank) {
        const uint32_t rk = a.rank[g], sn = a.sent[g];
        c = rk > sn ? min(nj, rk - sn) : 0;
    }
    *want = c;
    return QF_OK;
}

__global__ void __launch_bounds__(64) k_emit_count(EmitPlanArgs a) {
    const uint32_t lane = threadIdx.x;
    const uint32_t j = blockIdx.x * kEmitPerBlock + lane;   // n_max <= 2^24
    uint32_t c = 0;
    if (j < a.n_max) {
        a.entry_status[j] = emit_entry(a, j, emit_n_used(a), &c);
        a.want[j] = c;
    }
    const uint32_t sum = emit_wave_sum(c);   // <= kEmitPerBlock * 1024
    if (lane == 0) {
        a.sums[blockIdx.x] = sum;
        if (blockIdx.x == 0) a.head[0] = a.append ? min(*a.n_frames, a.N_max) : 0;
    }
}

__global__ void __launch_bounds__(64) k_emit_place(EmitPlanArgs a) {
    const uint32_t lane = threadIdx.x;
    // the frames wanted by the blocks before this one, and by all
    uint64_t before = 0, all = 0;
    for (uint32_t b = lane; b < a.blocks; b += 64) {
        const uint32_t s = a.sums[b];
        all += s;
        if (b < blockIdx.x) before += s;
    }
    before = emit_wave_sum64(before);
    all = emit_wave_sum64(all);
    const uint32_t base = a.head[0];
    const uint64_t room = a.N_max - base;   // base <= N_max
    const uint32_t j = blockIdx.x * kEmitPerBlock + lane;
    const bool in_list = j < a.n_max;
    const uint32_t c = in_list ? a.want[j] : 0;
    int32_t st = in_list ? a.entry_status[j] : QF_ENOTREADY;
    // the exclusive prefix of the lanes' counts over the wave
    uint32_t tot = c, pre = 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t other = __shfl_xor(tot, o, 64);
        if (lane & o) pre += other;
        tot += other;
    }
    const uint64_t at = before + pre;   // frames wanted in front of entry j
    if (in_list) {
        uint32_t first = kNone, count = 0;
        if (st == QF_OK) {
            if (at + c <= room) {
                count = c;
                if (count) first = base + (uint32_t)at;
            } else {
                st = QF_ENOTREADY;
                if (at <= room) {
                    // the cutoff: every entry in front fits, none behind does
                    a.head[1] = (uint32_t)at;
                    *a.n_frames = base + (uint32_t)at;
                    if (a.n_left) *a.n_left = all - at > kNone ? kNone : (uint32_t)(all - at);
                }
            }
        }
        a.entry_first[j] = first;
        a.entry_count[j] = count;
        a.entry_status[j] = st;
        if (count) {
            // (the entry passed emit_entry: sel[j] < G_src, the rows' metadata in range)
            if (a.sent) a.sent[a.sel[j]] += count;
            const uint64_t id = a.ids[j];
            for (uint32_t s = 0; s < count; ++s) {
                const uint64_t f = (uint64_t)j * a.max_rows + s;
                const uint32_t rlen = a.row_len ? a.row_len[f] : a.L;
                const uint32_t idx = a.row_index ? a.row_index[f] : a.k;
                const bool sys = idx < a.k;
                const uint32_t foff = sys ? a.P - 1 : a.P - 3 - a.k;
                const uint32_t t = (uint32_t)at + s, q = base + t;   // q < N_max
                a.frame_len[q] = a.P - foff + rlen;
                a.frame_off[q] = foff;
                a.frame_id[q] = id;
                a.frame_pkt[q] = sys ? idx : 0;
                a.rec[t] = make_uint4(j, s, rlen, sys ? idx : a.k);
            }
        }
    }
    if (blockIdx.x == 0 && lane == 0 && all <= room) {
        a.head[1] = (uint32_t)all;
        *a.n_frames = base + (uint32_t)all;
        if (a.n_left) *a.n_left = 0;
    }
}

// The last v < 16 bytes of a row from its 16-byte unit x to p (16-byte aligned).
QF_DEV void store_tail(uint8_t* p, uint4 x, uint32_t v) {
    uint32_t w0 = x.x, w1 = x.y;
    if (v & 8) {
        *reinterpret_cast<uint64_t*>(p) = ((uint64_t)x.y << 32) | x.x;
        p += 8;
        w0 = x.z;
        w1 = x.w;
    }
    if (v & 4) {
        *reinterpret_cast<uint32_t*>(p) = w0;
        p += 4;
        w0 = w1;
    }
    if (v & 2) {
        *reinterpret_cast<uint16_t*>(p) = (uint16_t)w0;
        p += 2;
        w0 >>= 16;
    }
    if (v & 1) *p = (uint8_t)w0;
}

// Global memory said so, as in qf_deliver.hip: the loads' base is one of four
// rows, and without the address space the select makes them flat ones.
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(1))) uint4* EmitUnitPtr;
#else
typedef const uint4* EmitUnitPtr;
#endif
QF_DEV uint4 emit_load_unit(const uint8_t* p) {
    const EmitUnitPtr g = (EmitUnitPtr)(uintptr_t)p;
    return make_uint4(g->x, g->y, g->z, g->w);
}

// Header block blk (slot bytes [16 blk, 16 blk + 16), blk < P / 16) of a frame
// whose row has index idx and its vector at vec.
QF_DEV void emit_header_block(uint8_t* slot, uint32_t blk, uint32_t k, uint32_t P, uint32_t idx, const uint8_t* vec) {
    const uint32_t t0 = blk * 16;
    if (idx < k) {   // systematic: one byte in front of the payload
        if (t0 + 16 == P) slot[P - 1] = 1;
        return;
    }
    const uint32_t foff = P - 3 - k, v0 = P - k;
    if (t0 + 16 <= foff) return;   // in front of the frame
    if (t0 >= v0) {
        // 16 bytes of the vector to an aligned block: the vector as the "frame"
        // of vector_copy_block, read from the aligned address at or below it,
        // its readable bytes ending with its last.  (Not wide, so byte by byte,
        // where the first dword would begin in front of the vector.)
        const uintptr_t va = reinterpret_cast<uintptr_t>(vec);
        const uint32_t lead = (uint32_t)(va & 15), c0 = t0 - v0;
        uint8_t* const cd = slot + v0;
        vector_copy_block(cd, c0, k, reinterpret_cast<const uint8_t*>(va - lead), lead + k, lead + k,
                          wide_block(cd, c0, k) && ((lead + c0) & 3) <= c0);
        return;
    }
    // the block that holds the frame's first bytes: 0x00 | k (BE u16) | vector
    for (uint32_t t = t0 > foff ? t0 : foff; t < t0 + 16; ++t) {
        const uint32_t h = t - foff;
        slot[t] = h == 0 ? 0 : h == 1 ? (uint8_t)(k >> 8) : h == 2 ? (uint8_t)(k & 0xFF) : vec[h - 3];
    }
}

__global__ void __launch_bounds__(256) k_emit_frames(EmitFramesArgs a) {
    const uint32_t lane = threadIdx.x & 63;
    // (wave-uniform by construction; said so, the quad's arithmetic is scalar)
    const uint32_t w0 = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    const uint32_t base = a.head[0], n_rec = a.head[1];
    const uint32_t n_quads = (n_rec + 3) / 4;   // n_rec <= N_max <= 2^28
    const uint32_t hb = a.P / 16;
    for (uint32_t q = w0; q < n_quads; q += a.n_waves) {
        const uint32_t t0 = q * 4;
        const uint32_t n = min(n_rec - t0, 4u);
        // the four records in one round trip; one the count does not cover
        // repeats the last that it does and is not looked at
        uint4 rr[4];
#pragma unroll
        for (int x = 0; x < 4; ++x) rr[x] = a.rec[min(t0 + x, n_rec - 1)];
        const uint8_t* sp[4];
        uint8_t* dp[4];
        uint32_t len[4], longest = 0;
        const uint8_t* sp_long = a.rows;
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            const bool used = (uint32_t)x < n;
            sp[x] = a.rows + (uint64_t)rr[x].x * a.rows_gen_stride + (uint64_t)rr[x].y * a.row_stride;
            dp[x] = a.frames + (uint64_t)(base + t0 + (used ? x : 0)) * a.frame_stride;
            len[x] = used ? rr[x].z : 0;
            if (len[x] > longest) {
                longest = len[x];
                sp_long = sp[x];
            }
        }
        // Every lane in the loop has a unit of the longest row, so a row that
        // has no byte in the lane's unit loads the longest row's instead (a
        // unit that holds a byte of an emitted row, as the read rule wants) and
        // drops it: four loads without a branch between them, all issued before
        // the first is waited for.
        for (uint32_t u16 = lane * 16; u16 < longest; u16 += 64 * 16) {
            uint4 v[4];
#pragma unroll
            for (int x = 0; x < 4; ++x) v[x] = emit_load_unit((len[x] > u16 ? sp[x] : sp_long) + u16);
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                if (len[x] >= u16 + 16) *reinterpret_cast<uint4*>(dp[x] + a.P + u16) = v[x];
                else if (len[x] > u16) store_tail(dp[x] + a.P + u16, v[x], len[x] - u16);
            }
        }
        // the headers: sixteen lanes per frame, a lane per 16-byte block
        // (the frame of a lane is picked by four predicated copies of the code, not by
        // an index into the records: that would move them to LDS)
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            if ((lane >> 4) == (uint32_t)x && (uint32_t)x < n) {
                const uint8_t* const vec =
                    rr[x].w < a.k ? nullptr : a.row_coeffs + ((uint64_t)rr[x].x * a.max_rows + rr[x].y) * a.k;
                for (uint32_t blk = lane & 15; blk < hb; blk += 16) emit_header_block(dp[x], blk, a.k, a.P, rr[x].w, vec);
            }
        }
    }
}

}  // namespace

static bool emit_plan_ok(const EmitPlanArgs& a) {
    return a.sel && a.ids && a.frame_len && a.frame_off && a.frame_id && a.frame_pkt && a.n_frames && a.entry_first &&
           a.entry_count && a.entry_status && a.want && a.sums && a.head && a.rec && (!a.rank == !a.sent) &&
           (a.row_index || a.has_coeffs) && a.n_max && a.n_max <= (1u << 24) && a.G_src && a.k && a.k <= 256 &&
           a.max_rows && a.max_rows <= 1024 && a.N_max && a.P == (3 + a.k + 15) / 16 * 16 &&
           a.blocks == (a.n_max + kEmitPerBlock - 1) / kEmitPerBlock;
}

hipError_t launch_emit_count(const EmitPlanArgs& a, hipStream_t st) {
    if (!emit_plan_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_emit_count, dim3(a.blocks), dim3(64), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_emit_place(const EmitPlanArgs& a, hipStream_t st) {
    if (!emit_plan_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_emit_place, dim3(a.blocks), dim3(64), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_emit_frames(EmitFramesArgs a, uint64_t max_frames, uint32_t grid_cap, hipStream_t st) {
    if (!a.rows || !a.frames || !a.rec || !a.head || a.k == 0 || a.k > 256 || a.max_rows == 0 || max_frames == 0 ||
        max_frames > (1ull << 28) || grid_cap == 0 || a.P != (3 + a.k + 15) / 16 * 16)
        return hipErrorInvalidValue;
    const uint32_t need = (uint32_t)((max_frames + 15) / 16);   // four waves of four frames
    const uint32_t blocks = need < grid_cap ? need : grid_cap;
    a.n_waves = blocks * 4;
    hipLaunchKernelGGL(k_emit_frames, dim3(blocks), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace qf

#ifndef QF_KERNEL_EMU   // (tests/kernel_emu builds the kernels and launchers above for the host)
#include <mutex>

#include "qf_internal.h"

extern "C" int qf_emit_frames_sel_dev(qf_ctx* ctx, const qf_emit_shape* sh, const qf_gen_sel* sel, const uint8_t* rows,
                                      const uint16_t* row_index, const uint32_t* n_rows, const uint8_t* row_coeffs,
                                      const uint32_t* row_len, const int32_t* in_status, const uint64_t* ids,
                                      const uint32_t* rank, uint32_t* sent, uint8_t* frames, uint32_t* frame_len,
                                      uint32_t* frame_off, uint64_t* frame_id, uint64_t* frame_pkt, uint32_t* n_frames,
                                      uint32_t* n_left, uint32_t* entry_first, uint32_t* entry_count,
                                      int32_t* entry_status) {
    if (!ctx || !sh) return QF_EINVAL;
    if (!sel || !sel->sel_dev || sel->n_max == 0 || sel->G_src == 0 || sel->n_max > (1u << 24)) return QF_EINVAL;
    const uint32_t k = sh->k, L = sh->L, max_rows = sh->max_rows, N_max = sh->N_max;
    if (k == 0 || k > 256 || L == 0 || max_rows == 0 || max_rows > 1024 || N_max == 0 ||
        (sh->flags & ~(uint32_t)QF_EMIT_APPEND) || sh->reserved != 0)
        return QF_EINVAL;
    const uint32_t P = qf_frame_payload_offset(k);
    if ((sh->row_stride & 15) || (sh->rows_gen_stride & 15) || (sh->frame_stride & 15) || sh->row_stride < L ||
        sh->frame_stride < (uint64_t)P + L || sh->frame_stride > (1ull << 32) ||
        (uint64_t)N_max * sh->frame_stride > (1ull << 32))
        return QF_EINVAL;
    if (!rows || !ids || !frames || !frame_len || !frame_off || !frame_id || !frame_pkt || !n_frames || !entry_first ||
        !entry_count || !entry_status || (!row_index && !row_coeffs) || (!rank != !sent))
        return QF_EINVAL;
    if (!aligned16(rows) || !aligned16(frames) || (reinterpret_cast<uintptr_t>(ids) & 7) ||
        (reinterpret_cast<uintptr_t>(frame_id) & 7) || (reinterpret_cast<uintptr_t>(frame_pkt) & 7))
        return QF_EINVAL;
    std::unique_lock<std::mutex> lk;
    int s = qf::ctx_lock(ctx, lk);
    if (s) return s;
    hipStream_t st = qf::ctx_stream(ctx);
    const uint32_t n_max = sel->n_max;
    const uint32_t blocks = (n_max + qf::kEmitPerBlock - 1) / qf::kEmitPerBlock;
    const uint64_t most = (uint64_t)n_max * max_rows < N_max ? (uint64_t)n_max * max_rows : N_max;
    // workspace: wanted counts [n_max] | block sums | base, emitted | records, 16 bytes per frame
    qf::WorkLayout wl;
    const size_t off_want = wl.take((size_t)n_max * 4);
    const size_t off_sums = wl.take((size_t)blocks * 4);
    const size_t off_head = wl.take(2 * 4);
    const size_t off_rec = wl.take((size_t)most * sizeof(uint4));
    uint8_t* w = nullptr;
    s = qf::ctx_work(ctx, wl.size(), &w);
    if (s) return s;
    qf::EmitPlanArgs pa{};
    pa.sel = sel->sel_dev;
    pa.n_sel = sel->n_sel_dev;
    pa.row_index = row_index;
    pa.n_rows = n_rows;
    pa.row_len = row_len;
    pa.in_status = in_status;
    pa.ids = ids;
    pa.rank = rank;
    pa.sent = sent;
    pa.frame_len = frame_len;
    pa.frame_off = frame_off;
    pa.frame_id = frame_id;
    pa.frame_pkt = frame_pkt;
    pa.n_frames = n_frames;
    pa.n_left = n_left;
    pa.entry_first = entry_first;
    pa.entry_count = entry_count;
    pa.entry_status = entry_status;
    pa.want = reinterpret_cast<uint32_t*>(w + off_want);
    pa.sums = reinterpret_cast<uint32_t*>(w + off_sums);
    pa.head = reinterpret_cast<uint32_t*>(w + off_head);
    pa.rec = reinterpret_cast<uint4*>(w + off_rec);
    pa.n_max = n_max;
    pa.G_src = sel->G_src;
    pa.k = k;
    pa.L = L;
    pa.max_rows = max_rows;
    pa.N_max = N_max;
    pa.P = P;
    pa.append = sh->flags & QF_EMIT_APPEND;
    pa.has_coeffs = row_coeffs != nullptr;
    pa.blocks = blocks;
    QF_PROFILED(ctx, st, "k_emit_count", qf::launch_emit_count(pa, st));
    QF_PROFILED(ctx, st, "k_emit_place", qf::launch_emit_place(pa, st));
    qf::EmitFramesArgs fa{};
    fa.rows = rows;
    fa.row_coeffs = row_coeffs;
    fa.frames = frames;
    fa.rec = pa.rec;
    fa.head = pa.head;
    fa.row_stride = sh->row_stride;
    fa.rows_gen_stride = sh->rows_gen_stride;
    fa.frame_stride = sh->frame_stride;
    fa.k = k;
    fa.P = P;
    fa.max_rows = max_rows;
    // a wave per four frames; the grid is bounded and strides over the rest
    const uint32_t cap = (uint32_t)(qf::ctx_num_cus(ctx) > 0 ? qf::ctx_num_cus(ctx) : 1) * qf::kEmitGroupsPerCu;
    QF_PROFILED(ctx, st, "k_emit_frames", qf::launch_emit_frames(fa, most, cap, st));
    return QF_OK;
}
#endif  // QF_KERNEL_EMU
