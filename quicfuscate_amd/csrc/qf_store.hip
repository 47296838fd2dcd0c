// qf_store.hip -- the row store of a streaming receiver:
// qf_store_append_dev keeps the rows a poll brought and the rank state took
// (qf_rank_update_batch's flags) in a per-generation store of cap slots, in the
// (offset, length) form qf_decode_frames_dev and qf_recode_frames_dev read.
//
//  k_store_prepare  one wave per generation.  Pass 1 counts the taken slots
//                   and applies the geometry rules to them; a generation that
//                   fails writes its status and nothing else.  Pass 2 gives
//                   the taken slots their store slots in arrival order (a
//                   ballot prefix per chunk of 64, as k_parse_frame_headers
//                   compacts), writes the metadata entries, copies the
//                   vectors, and leaves one {offset, length} record per taken
//                   row plus {first store slot, count} per generation for
//                   the payload pass.
//  k_store_rows     one lane per 16-byte unit of (generation, taken row).  A
//                   lane past its generation's count or past its row's last
//                   unit ends after one or two loads; the others load the
//                   unit (masked to the row's bytes, so the tail of the last
//                   unit is zero) and store it.
// Both kernels have a second form over a list (qf_store_append_sel_dev, timed
// as k_store_prepare_sel / k_store_rows_sel): the rows of all
// entries lie in one flat poll buffer and the stores are the listed
// generations'.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <type_traits>

#include "qf_fec.h"
#include "qf_gf_dev.h"
#include "qf_internal.h"

namespace qf {

namespace {

struct StorePrepareArgs {
    const uint32_t* row_off;
    const uint32_t* row_len;
    const uint16_t* row_index;
    const uint32_t* n_rows;     // nullptr: max_rows
    const uint8_t* row_coeffs;
    const uint8_t* take;        // nullptr: every row
    uint32_t* store_off;
    uint32_t* store_len;
    uint16_t* store_index;
    uint8_t* store_coeffs;
    uint32_t* store_n;
    int32_t* status;
    uint2* rec;                 // [G][max_rows] {row_off, row_len} of the taken rows, compacted
    uint2* gen;                 // [G] {first store slot, taken rows}; count 0 unless QF_OK
    uint64_t src_gen_stride, store_row_stride;
    uint32_t k, L, max_rows, cap;
};

struct StoreRowsArgs {
    const uint8_t* src;
    uint8_t* store;
    const uint2* rec;
    const uint2* gen;
    uint64_t src_gen_stride, store_row_stride, store_gen_stride;
    uint64_t total;             // G * max_rows * Lu lanes
    uint32_t max_rows, Lu;
};

// The calls over a list (qf_store_append_sel_dev): the blocks
// are the n_max list entries; rows, take, status, rec and gen are indexed by
// the list position, the store arrays and store_n by the listed generation
// sel[j] < G_src.  Their own argument types, so the dense call's kernels keep
// their arguments.
struct StorePrepareSelArgs : StorePrepareArgs {
    const uint32_t* sel;
    const uint32_t* n_sel;      // nullptr: n_max
    uint32_t n_max, G_src;
};

struct StoreRowsSelArgs : StoreRowsArgs {
    const uint32_t* sel;        // read for entries with taken rows only: those are listed and valid
};

// SEL: g is a list entry and gs its generation, which indexes the store side
// only; without SEL gs is g and the code is the dense call's.
template <bool SEL>
__global__ void __launch_bounds__(64)
k_store_prepare(typename std::conditional<SEL, StorePrepareSelArgs, StorePrepareArgs>::type a) {
    __shared__ uint32_t src_of[64];   // taken ordinal inside the chunk -> its lane
    const uint32_t g = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const uint32_t mr = a.max_rows;
    uint32_t gs = g;
    if constexpr (SEL) {
        uint32_t n_used = a.n_max;
        if (a.n_sel) n_used = min(*a.n_sel, n_used);
        // an unused entry's sel value is not looked at; nothing is read or
        // written through an invalid one
        const bool unused = g >= n_used;
        if (!unused) gs = a.sel[g];
        if (unused || gs >= a.G_src) {
            if (lane == 0) {
                a.status[g] = unused ? QF_OK : QF_EINVAL;
                a.gen[g] = make_uint2(0, 0);
            }
            return;
        }
    }
    const uint32_t n = a.n_rows ? a.n_rows[g] : mr;
    const uint32_t c0 = a.store_n[gs];
    const uint64_t in0 = (uint64_t)g * mr;
    int32_t status = QF_OK;
    uint32_t taken = 0;
    if (n > mr) {
        status = QF_EINVAL;
    } else {
        bool bad = false;
        for (uint32_t s0 = 0; s0 < n; s0 += 64) {   // n <= 1024: 16 chunks at most
            const uint32_t s = s0 + lane;
            const bool tk = s < n && (!a.take || a.take[in0 + s]);
            if (tk) {
                const uint32_t off = a.row_off[in0 + s], len = a.row_len[in0 + s];
                if (len > a.L || (off & 15) || (uint64_t)off + len > a.src_gen_stride) bad = true;
            }
            taken += (uint32_t)__popcll(__ballot(tk));
        }
        if (__any(bad)) status = QF_EINVAL;
        else if (c0 > a.cap || taken > a.cap - c0) status = QF_ETOOSMALL;
    }
    if (status != QF_OK) {
        if (lane == 0) {
            a.status[g] = status;
            a.gen[g] = make_uint2(c0, 0);
        }
        return;
    }
    const uint64_t out0 = (uint64_t)gs * a.cap;
    const bool words = (a.k & 3) == 0 && ((reinterpret_cast<uintptr_t>(a.row_coeffs) |
                                           reinterpret_cast<uintptr_t>(a.store_coeffs)) & 3) == 0;
    const uint32_t per = words ? a.k / 4 : a.k;   // copy steps of one vector
    uint32_t base = 0;
    for (uint32_t s0 = 0; s0 < n; s0 += 64) {
        const uint32_t s = s0 + lane;
        const bool tk = s < n && (!a.take || a.take[in0 + s]);
        const uint64_t bal = __ballot(tk);
        const uint32_t before = (uint32_t)__popcll(bal & ((lane == 0) ? 0ull : (~0ull >> (64 - lane))));
        if (tk) {
            const uint32_t j = base + before, c = c0 + j;
            const uint32_t off = a.row_off[in0 + s], len = a.row_len[in0 + s];
            a.store_off[out0 + c] = (uint32_t)(c * a.store_row_stride);   // cap * store_row_stride <= 2^32
            a.store_len[out0 + c] = len;
            a.store_index[out0 + c] = a.row_index[in0 + s];
            a.rec[in0 + j] = make_uint2(off, len);
            src_of[before] = lane;
        }
        __syncthreads();
        const uint32_t cnt = (uint32_t)__popcll(bal);
        for (uint32_t w = lane; w < cnt * per; w += 64) {
            const uint32_t i = w / per, t = w - i * per;
            const uint64_t from = (in0 + s0 + src_of[i]) * a.k, to = (out0 + c0 + base + i) * a.k;
            if (words) reinterpret_cast<uint32_t*>(a.store_coeffs + to)[t] = reinterpret_cast<const uint32_t*>(a.row_coeffs + from)[t];
            else a.store_coeffs[to + t] = a.row_coeffs[from + t];
        }
        __syncthreads();
        base += cnt;
    }
    if (lane == 0) {
        a.status[g] = QF_OK;
        a.store_n[gs] = c0 + taken;
        a.gen[g] = make_uint2(c0, taken);
    }
}

template <bool SEL>
__global__ void __launch_bounds__(256)
k_store_rows(typename std::conditional<SEL, StoreRowsSelArgs, StoreRowsArgs>::type a) {
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; f < a.total; f += step) {
        const uint64_t row = f / a.Lu;   // g * max_rows + j
        const uint32_t u16 = (uint32_t)(f - row * a.Lu) * 16;
        const uint64_t g = row / a.max_rows;
        const uint32_t j = (uint32_t)(row - g * a.max_rows);
        const uint2 gn = a.gen[g];
        if (j >= gn.y) continue;
        const uint2 r = a.rec[row];      // {row_off, row_len}
        if (r.y <= u16) continue;        // no byte of the row in this unit
        if constexpr (SEL) {
            // every entry's rows lie in the one region at a.src; the store is the listed generation's
            const uint4 x = load_row_unit(a.src + r.x + u16, r.y, u16);
            const uint64_t gs = a.sel[g];
            *reinterpret_cast<uint4*>(a.store + gs * a.store_gen_stride + (uint64_t)(gn.x + j) * a.store_row_stride + u16) = x;
        } else {
            const uint4 x = load_row_unit(a.src + g * a.src_gen_stride + r.x + u16, r.y, u16);
            *reinterpret_cast<uint4*>(a.store + g * a.store_gen_stride + (uint64_t)(gn.x + j) * a.store_row_stride + u16) = x;
        }
    }
}

}  // namespace

}  // namespace qf

// qf_store_append_dev over G generations, and with `sel` qf_store_append_sel_dev
// over its n_max entries (G = n_max).
static int store_append_run(qf_ctx* ctx, const qf_store_shape* sh, uint32_t G, const qf_gen_sel* sel,
                            const uint8_t* src, const uint32_t* row_off, const uint32_t* row_len,
                            const uint16_t* row_index, const uint32_t* n_rows, const uint8_t* row_coeffs,
                            const uint8_t* take, uint8_t* store, uint32_t* store_off, uint32_t* store_len,
                            uint16_t* store_index, uint8_t* store_coeffs, uint32_t* store_n, int32_t* status) {
    if (!ctx || !sh) return QF_EINVAL;
    const uint32_t k = sh->k, L = sh->L, max_rows = sh->max_rows, cap = sh->cap;
    if (k == 0 || k > 256 || L == 0 || max_rows == 0 || max_rows > 1024 || cap == 0 || cap > 1024 ||
        sh->flags != 0 || sh->reserved != 0)
        return QF_EINVAL;
    if ((sh->src_gen_stride & 15) || (sh->store_row_stride & 15) || (sh->store_gen_stride & 15) ||
        sh->store_row_stride < round_up(L, 16))
        return QF_EINVAL;
    // store_off is a u32 offset into a generation's cap * store_row_stride bytes
    if (sh->store_row_stride > (1ull << 32) / cap || sh->store_gen_stride < cap * sh->store_row_stride)
        return QF_EINVAL;
    if (G == 0) return QF_OK;
    if (!src || !row_off || !row_len || !row_index || !row_coeffs || !store || !store_off || !store_len ||
        !store_index || !store_coeffs || !store_n || !status)
        return QF_EINVAL;
    if (!aligned16(src) || !aligned16(store)) return QF_EINVAL;
    std::unique_lock<std::mutex> lk;
    int s = qf::ctx_lock(ctx, lk);
    if (s) return s;
    hipStream_t st = qf::ctx_stream(ctx);
    // workspace: records [G][max_rows] {offset, length} | [G] {first store slot, count}
    qf::WorkLayout wl;
    const size_t off_rec = wl.take((size_t)G * max_rows * sizeof(uint2));
    const size_t off_gen = wl.take((size_t)G * sizeof(uint2));
    uint8_t* w = nullptr;
    s = qf::ctx_work(ctx, wl.size(), &w);
    if (s) return s;
    qf::StorePrepareSelArgs pa{};
    pa.row_off = row_off;
    pa.row_len = row_len;
    pa.row_index = row_index;
    pa.n_rows = n_rows;
    pa.row_coeffs = row_coeffs;
    pa.take = take;
    pa.store_off = store_off;
    pa.store_len = store_len;
    pa.store_index = store_index;
    pa.store_coeffs = store_coeffs;
    pa.store_n = store_n;
    pa.status = status;
    pa.rec = reinterpret_cast<uint2*>(w + off_rec);
    pa.gen = reinterpret_cast<uint2*>(w + off_gen);
    pa.src_gen_stride = sh->src_gen_stride;
    pa.store_row_stride = sh->store_row_stride;
    pa.k = k;
    pa.L = L;
    pa.max_rows = max_rows;
    pa.cap = cap;
    if (sel) {
        pa.sel = sel->sel_dev;
        pa.n_sel = sel->n_sel_dev;
        pa.n_max = sel->n_max;
        pa.G_src = sel->G_src;
        QF_PROFILED(ctx, st, "k_store_prepare_sel",
                    qf::launch_kernel(qf::k_store_prepare<true>, dim3(G), dim3(64), 0, st, pa));
    } else {
        QF_PROFILED(ctx, st, "k_store_prepare",
                    qf::launch_kernel(qf::k_store_prepare<false>, dim3(G), dim3(64), 0, st, pa));
    }
    qf::StoreRowsSelArgs ra{};
    ra.src = src;
    ra.store = store;
    ra.rec = pa.rec;
    ra.gen = pa.gen;
    ra.src_gen_stride = sh->src_gen_stride;
    ra.store_row_stride = sh->store_row_stride;
    ra.store_gen_stride = sh->store_gen_stride;
    ra.max_rows = max_rows;
    ra.Lu = (L + 15) / 16;
    ra.total = (uint64_t)G * max_rows * ra.Lu;
    // a lane per unit; the grid is bounded and strides over the rest
    const uint64_t need = (ra.total + 255) / 256;
    const uint64_t most = (uint64_t)(qf::ctx_num_cus(ctx) > 0 ? qf::ctx_num_cus(ctx) : 1) * 64;
    const dim3 grid((uint32_t)(need < most ? need : most));
    if (sel) {
        ra.sel = sel->sel_dev;
        QF_PROFILED(ctx, st, "k_store_rows_sel", qf::launch_kernel(qf::k_store_rows<true>, grid, dim3(256), 0, st, ra));
    } else {
        QF_PROFILED(ctx, st, "k_store_rows", qf::launch_kernel(qf::k_store_rows<false>, grid, dim3(256), 0, st, ra));
    }
    return QF_OK;
}

extern "C" int qf_store_append_dev(qf_ctx* ctx, const qf_store_shape* sh, uint32_t G, const uint8_t* src,
                                   const uint32_t* row_off, const uint32_t* row_len, const uint16_t* row_index,
                                   const uint32_t* n_rows, const uint8_t* row_coeffs, const uint8_t* take,
                                   uint8_t* store, uint32_t* store_off, uint32_t* store_len, uint16_t* store_index,
                                   uint8_t* store_coeffs, uint32_t* store_n, int32_t* status) {
    return store_append_run(ctx, sh, G, nullptr, src, row_off, row_len, row_index, n_rows, row_coeffs, take, store,
                            store_off, store_len, store_index, store_coeffs, store_n, status);
}

extern "C" int qf_store_append_sel_dev(qf_ctx* ctx, const qf_store_shape* sh, const qf_gen_sel* sel,
                                       const uint8_t* src, const uint32_t* row_off, const uint32_t* row_len,
                                       const uint16_t* row_index, const uint32_t* n_rows, const uint8_t* row_coeffs,
                                       const uint8_t* take, uint8_t* store, uint32_t* store_off, uint32_t* store_len,
                                       uint16_t* store_index, uint8_t* store_coeffs, uint32_t* store_n,
                                       int32_t* status) {
    if (!sel || !sel->sel_dev || sel->n_max == 0 || sel->G_src == 0) return QF_EINVAL;
    return store_append_run(ctx, sh, sel->n_max, sel, src, row_off, row_len, row_index, n_rows, row_coeffs, take,
                            store, store_off, store_len, store_index, store_coeffs, store_n, status);
}

