// qf_window.hip -- the generation window of the streaming receiver (DESIGN.md
// 3.17): the persistent map from the unbounded generation ids of the wire onto
// the G_src slots every other call counts in.  qf_gen_window_dev stands in
// front of qf_parse_poll_headers_dev (qf_poll.hip) and turns a poll's ids into
// that call's tags, qf_gen_window_sel_dev reads the ids of a list and closes
// its generations.
//
//  k_window_max    a lane per frame: one atomicMax on its slot's entry of a
//                  zeroed u64 array, on id + 1.  A maximum does not depend on
//                  the order.
//  k_window_apply  a lane per slot: the poll's newest id against the window
//                  entry; the new entry, an evicted flag and the displaced id.
//  (k_gen_select_count / k_gen_select_scatter of qf_select.hip over the flags
//                  with min_rank 1: the ascending list of evicted slots.)
//  k_window_tag    a lane per frame: its tag and status from the updated
//                  entry; further lanes copy the displaced ids of the list.
//  k_window_sel    a lane per list entry: the id its slot holds, and with
//                  QF_WINDOW_CLOSE the closed flag.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>

#include "qf_fec.h"
#include "qf_gf_dev.h"
#include "qf_internal.h"

namespace qf {

namespace {

constexpr uint64_t kWinClosed = 1ull << 63;
constexpr uint64_t kWinIdLimit = 1ull << 62;   // wire ids are 0 .. 2^62 - 1

struct WindowArgs {
    const uint64_t* frame_id;
    const uint32_t* n_frames;   // nullptr: N_max
    uint64_t* win;              // [G_src]
    unsigned long long* newest; // [G_src], zeroed: the poll's largest id + 1 per slot
    uint32_t* evicted;          // [G_src] 1 for an evicted slot
    uint64_t* displaced;        // [G_src] the id an evicted slot held
    uint32_t* frame_gen;
    int32_t* frame_status;
    const uint32_t* evict_sel;
    const uint32_t* n_evict;
    uint64_t* evict_id;         // nullable
    uint32_t N_max, G_src, n_evict_max, id_lanes;
};

struct WindowSelArgs {
    const uint32_t* sel;
    const uint32_t* n_sel;      // nullptr: n_max
    uint64_t* win;
    uint64_t* ids;              // nullable
    uint32_t n_max, G_src, close;
};

QF_DEV uint32_t window_frames(const uint32_t* n_frames, uint32_t N_max) {
    return n_frames ? min(*n_frames, N_max) : N_max;
}

__global__ void __launch_bounds__(256) k_window_max(WindowArgs a) {
    const uint32_t f = blockIdx.x * 256 + threadIdx.x;
    if (f >= window_frames(a.n_frames, a.N_max)) return;
    const uint64_t id = a.frame_id[f];
    if (id < kWinIdLimit) atomicMax(&a.newest[id % a.G_src], (unsigned long long)(id + 1));
}

__global__ void __launch_bounds__(256) k_window_apply(WindowArgs a) {
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= a.G_src) return;
    const uint64_t m = a.newest[s];   // 0: no frame of the poll maps to the slot
    uint32_t flag = 0;
    if (m) {
        const uint64_t w = a.win[s];
        if (w == 0 || m > (w & ~kWinClosed)) {
            a.win[s] = m;             // open
            if (w != 0 && !(w & kWinClosed)) {
                flag = 1;
                a.displaced[s] = w - 1;
            }
        }
    }
    a.evicted[s] = flag;
}

__global__ void __launch_bounds__(256) k_window_tag(WindowArgs a) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= a.N_max) {
        // the displaced ids, in list order
        const uint32_t j = t - a.N_max;
        if (j >= a.id_lanes || j >= min(*a.n_evict, a.n_evict_max)) return;
        a.evict_id[j] = a.displaced[a.evict_sel[j]];   // the list holds slots < G_src
        return;
    }
    if (t >= window_frames(a.n_frames, a.N_max)) return;
    const uint64_t id = a.frame_id[t];
    uint32_t tag = QF_GEN_NONE;
    int32_t st = QF_EINVAL;
    if (id < kWinIdLimit) {
        const uint32_t s = (uint32_t)(id % a.G_src);
        const uint64_t w = a.win[s];   // not empty: it holds this id or a larger one
        if (id + 1 != (w & ~kWinClosed)) {
            st = QF_ESTALE;
        } else if (w & kWinClosed) {
            st = QF_ECLOSED;
        } else {
            st = QF_OK;
            tag = s;
        }
    }
    a.frame_gen[t] = tag;
    a.frame_status[t] = st;
}

__global__ void __launch_bounds__(256) k_window_sel(WindowSelArgs a) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= a.n_max) return;
    uint32_t n = a.n_max;
    if (a.n_sel) {
        const uint32_t v = *a.n_sel;
        n = v < n ? v : n;
    }
    uint64_t id = UINT64_MAX;
    if (j < n) {   // an unused entry's sel value is not looked at
        const uint32_t g = a.sel[j];
        if (g < a.G_src) {
            const uint64_t w = a.win[g];
            if (w) {
                id = (w & ~kWinClosed) - 1;
                // a slot listed twice gets the same value from both lanes
                if (a.close) a.win[g] = w | kWinClosed;
            }
        }
    }
    if (a.ids) a.ids[j] = id;
}

}  // namespace

}  // namespace qf

extern "C" int qf_gen_window_dev(qf_ctx* ctx, uint32_t G_src, uint32_t N_max, const uint64_t* frame_id,
                                 const uint32_t* n_frames, uint64_t* win, uint32_t flags, uint32_t* frame_gen,
                                 int32_t* frame_status, uint32_t n_evict_max, uint32_t* evict_sel, uint32_t* n_evict,
                                 uint64_t* evict_id) {
    if (!ctx) return QF_EINVAL;
    if (G_src == 0 || G_src > (1u << 24) || flags != 0) return QF_EINVAL;
    // an eviction needs a frame of the poll and a slot of the window
    const uint32_t most = N_max < G_src ? N_max : G_src;
    if (n_evict_max < most) return QF_EINVAL;
    if (!win || !evict_sel || !n_evict) return QF_EINVAL;
    if (N_max && (!frame_id || !frame_gen || !frame_status)) return QF_EINVAL;
    if (reinterpret_cast<uintptr_t>(win) & 7) return QF_EINVAL;
    std::unique_lock<std::mutex> lk;
    int s = qf::ctx_lock(ctx, lk);
    if (s) return s;
    hipStream_t st = qf::ctx_stream(ctx);
    if (N_max == 0) {
        QF_CHECK_HIP(hipMemsetAsync(n_evict, 0, 4, st));
        return QF_OK;
    }
    // workspace: newest [G_src] u64 (zeroed) | displaced [G_src] u64 | evicted
    // [G_src] u32 | the select's block counts
    qf::WorkLayout wl;
    const size_t off_newest = wl.take((size_t)G_src * 8);
    const size_t off_disp = wl.take((size_t)G_src * 8);
    const size_t off_flags = wl.take((size_t)G_src * 4);
    const size_t off_blocks = wl.take(qf::gen_select_work_bytes(G_src));
    uint8_t* w = nullptr;
    s = qf::ctx_work(ctx, wl.size(), &w);
    if (s) return s;
    qf::WindowArgs a{};
    a.frame_id = frame_id;
    a.n_frames = n_frames;
    a.win = win;
    a.newest = reinterpret_cast<unsigned long long*>(w + off_newest);
    a.evicted = reinterpret_cast<uint32_t*>(w + off_flags);
    a.displaced = reinterpret_cast<uint64_t*>(w + off_disp);
    a.frame_gen = frame_gen;
    a.frame_status = frame_status;
    a.evict_sel = evict_sel;
    a.n_evict = n_evict;
    a.evict_id = evict_id;
    a.N_max = N_max;
    a.G_src = G_src;
    a.n_evict_max = n_evict_max;
    a.id_lanes = evict_id ? most : 0;
    QF_CHECK_HIP(hipMemsetAsync(w + off_newest, 0, (size_t)G_src * 8, st));
    const dim3 fgrid((uint32_t)(((uint64_t)N_max + 255) / 256));
    QF_PROFILED(ctx, st, "k_window_max", qf::launch_kernel(qf::k_window_max, fgrid, dim3(256), 0, st, a));
    QF_PROFILED(ctx, st, "k_window_apply",
                qf::launch_kernel(qf::k_window_apply, dim3((G_src + 255) / 256), dim3(256), 0, st, a));
    QF_PROFILED(ctx, st, "k_gen_select",
                qf::launch_gen_select_list(a.evicted, G_src, 1, n_evict_max, reinterpret_cast<uint32_t*>(w + off_blocks),
                                           evict_sel, n_evict, nullptr, st));
    const uint64_t lanes = (uint64_t)N_max + a.id_lanes;   // < 2^32 + 2^24
    QF_PROFILED(ctx, st, "k_window_tag",
                qf::launch_kernel(qf::k_window_tag, dim3((uint32_t)((lanes + 255) / 256)), dim3(256), 0, st, a));
    return QF_OK;
}

extern "C" int qf_gen_window_sel_dev(qf_ctx* ctx, const qf_gen_sel* sel, uint64_t* win, uint32_t flags,
                                     uint64_t* ids) {
    if (!ctx || !sel || !sel->sel_dev || !win || sel->n_max == 0 || sel->G_src == 0) return QF_EINVAL;
    if ((flags & ~(uint32_t)QF_WINDOW_CLOSE) || (!(flags & QF_WINDOW_CLOSE) && !ids)) return QF_EINVAL;
    std::unique_lock<std::mutex> lk;
    int s = qf::ctx_lock(ctx, lk);
    if (s) return s;
    hipStream_t st = qf::ctx_stream(ctx);
    qf::WindowSelArgs a{};
    a.sel = sel->sel_dev;
    a.n_sel = sel->n_sel_dev;
    a.win = win;
    a.ids = ids;
    a.n_max = sel->n_max;
    a.G_src = sel->G_src;
    a.close = flags & QF_WINDOW_CLOSE;
    QF_PROFILED(ctx, st, "k_window_sel",
                qf::launch_kernel(qf::k_window_sel, dim3((a.n_max + 255) / 256), dim3(256), 0, st, a));
    return QF_OK;
}
