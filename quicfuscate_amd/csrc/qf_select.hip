// qf_select.hip -- the streaming receiver's steps over a list of generations
// (DESIGN.md 3.15): qf_gen_select_dev builds the list on the device,
// qf_decode_frames_sel_dev / qf_recode_frames_sel_dev (qf_relay.hip) run the
// store-side calls over it through k_sel_gather, qf_stream_reset_dev resets it.
//
//  k_gen_select_count    a block of 256 lanes tests kSelPerBlock generations
//                        (ballot + popcount per wave) and leaves its number of
//                        matches in the workspace.
//  k_gen_select_scatter  the same blocks again: each sums the counts of the
//                        blocks before it, repeats its tests and writes its
//                        matches at their ranks among all matches, so the list
//                        ascends and does not depend on arrival order.  No
//                        block waits for another; the second launch is the
//                        only ordering.  The last block writes the counts.
//  k_sel_gather          one wave per list entry: the listed generations'
//                        metadata and vectors as a compact batch.
//  k_stream_reset        one lane per 16-byte unit of a listed generation's
//                        rank state; the first lane of an entry also zeroes
//                        its store_n and seen.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>

#include "qf_fec.h"
#include "qf_kernels.h"
#include "qf_gf_dev.h"
#include "qf_internal.h"

namespace qf {

namespace {

constexpr uint32_t kSelThreads = 256;
constexpr uint32_t kSelIters = 8;
constexpr uint32_t kSelPerBlock = kSelThreads * kSelIters;   // generations of one block
constexpr uint32_t kSelWaves = kSelThreads / 64;

struct GenSelectArgs {
    const uint32_t* rank;
    uint32_t* seen;          // nullptr: no "grew" condition
    uint32_t* counts;        // [blocks] matches per block
    uint32_t* sel;
    uint32_t* n_sel;
    uint32_t* n_match;       // nullable
    uint32_t G, min_rank, n_max, mark;
};

QF_DEV bool sel_match(const GenSelectArgs& a, uint32_t g, uint32_t* rank_out) {
    if (g >= a.G) return false;
    const uint32_t rk = a.rank[g];
    *rank_out = rk;
    return rk >= a.min_rank && (!a.seen || rk > a.seen[g]);
}

QF_DEV uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ void __launch_bounds__(kSelThreads) k_gen_select_count(GenSelectArgs a) {
    __shared__ uint32_t wsum[kSelWaves];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t g0 = blockIdx.x * kSelPerBlock;   // G <= 2^24
    uint32_t c = 0;
#pragma unroll
    for (uint32_t i = 0; i < kSelIters; ++i) {
        uint32_t rk;
        c += (uint32_t)__popcll(__ballot(sel_match(a, g0 + i * kSelThreads + threadIdx.x, &rk)));
    }
    if (lane == 0) wsum[wave] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (uint32_t w = 0; w < kSelWaves; ++w) t += wsum[w];
        a.counts[blockIdx.x] = t;
    }
}

__global__ void __launch_bounds__(kSelThreads) k_gen_select_scatter(GenSelectArgs a) {
    __shared__ uint32_t wsum[kSelWaves];
    __shared__ uint32_t cnt[kSelIters * kSelWaves];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // matches in the blocks before this one
    uint32_t before = 0;
    for (uint32_t b = threadIdx.x; b < blockIdx.x; b += kSelThreads) before += a.counts[b];
    before = wave_sum_u32(before);
    if (lane == 0) wsum[wave] = before;
    const uint32_t g0 = blockIdx.x * kSelPerBlock;
    bool m[kSelIters];
    uint32_t rk[kSelIters], below[kSelIters];
    const uint64_t lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
#pragma unroll
    for (uint32_t i = 0; i < kSelIters; ++i) {
        rk[i] = 0;
        m[i] = sel_match(a, g0 + i * kSelThreads + threadIdx.x, &rk[i]);
        const uint64_t bal = __ballot(m[i]);
        below[i] = (uint32_t)__popcll(bal & lt_mask);
        if (lane == 0) cnt[i * kSelWaves + wave] = (uint32_t)__popcll(bal);
    }
    __syncthreads();
    uint32_t base = 0;
    for (uint32_t w = 0; w < kSelWaves; ++w) base += wsum[w];
    // generation g0 + i * 256 + 64 * wave + lane: chunk i * kSelWaves + wave, in ascending order
    uint32_t run = base;
#pragma unroll
    for (uint32_t i = 0; i < kSelIters; ++i) {
        uint32_t at = run;
        for (uint32_t w = 0; w < kSelWaves; ++w) {
            const uint32_t c = cnt[i * kSelWaves + w];
            if (w < wave) at += c;
            run += c;
        }
        const uint32_t pos = at + below[i];
        if (m[i] && pos < a.n_max) {
            const uint32_t g = g0 + i * kSelThreads + threadIdx.x;
            a.sel[pos] = g;
            if (a.mark) a.seen[g] = rk[i];
        }
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        // run: the matches of every block
        *a.n_sel = run < a.n_max ? run : a.n_max;
        if (a.n_match) *a.n_match = run;
    }
}

__global__ void __launch_bounds__(64) k_sel_gather(SelGatherArgs a) {
    const uint32_t j = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const uint32_t mr = a.max_rows;
    uint32_t n = a.n_max;
    if (a.n_sel) {
        const uint32_t v = *a.n_sel;
        n = v < n ? v : n;
    }
    const uint64_t out0 = (uint64_t)j * mr;
    if (j >= n) {   // an unused entry: its sel value is not looked at
        if (lane == 0) {
            a.c_n_rows[j] = 0;
            a.gen_map[j] = 0;
            if (a.n_out) a.n_out[j] = 0;
        }
        return;
    }
    const uint32_t g = a.sel[j];
    if (g >= a.G_src) {   // nothing is read through an invalid entry
        if (lane == 0) {
            a.c_n_rows[j] = a.invalid_n_rows;
            a.c_row_index[out0] = 0xFFFF;
            a.c_row_off[out0] = 0;
            a.c_row_len[out0] = 0;
            a.gen_map[j] = 0;
            if (a.n_out) a.n_out[j] = a.n_out_listed;
        }
        return;
    }
    const uint32_t nr = a.n_rows ? a.n_rows[g] : mr;
    const uint32_t nc = nr < mr ? nr : mr;
    const uint64_t in0 = (uint64_t)g * mr;
    for (uint32_t s = lane; s < nc; s += 64) {
        a.c_row_off[out0 + s] = a.row_off[in0 + s];
        a.c_row_len[out0 + s] = a.row_len[in0 + s];
        a.c_row_index[out0 + s] = a.row_index[in0 + s];
    }
    // the nc vectors are contiguous on both sides (the compact side is 256-byte aligned)
    const uint8_t* from = a.row_coeffs + in0 * a.k;
    uint8_t* to = a.c_row_coeffs + out0 * a.k;
    const uint32_t bytes = nc * a.k;   // <= 1024 * 256
    if ((a.k & 3) == 0 && (reinterpret_cast<uintptr_t>(a.row_coeffs) & 3) == 0) {
        const uint32_t* f4 = reinterpret_cast<const uint32_t*>(from);
        uint32_t* t4 = reinterpret_cast<uint32_t*>(to);
        for (uint32_t w = lane; w < bytes / 4; w += 64) t4[w] = f4[w];
    } else {
        for (uint32_t w = lane; w < bytes; w += 64) to[w] = from[w];
    }
    if (lane == 0) {
        a.c_n_rows[j] = nr;
        a.gen_map[j] = g;
        if (a.n_out) a.n_out[j] = a.n_out_listed;
    }
}

struct StreamResetArgs {
    const uint32_t* sel;
    const uint32_t* n_sel;   // nullptr: n_max
    uint8_t* state;          // nullable
    uint32_t* store_n;       // nullable
    uint32_t* seen;          // nullable
    uint64_t total;          // n_max * units lanes
    uint32_t n_max, G_src, units, state_bytes;
};

__global__ void __launch_bounds__(256) k_stream_reset(StreamResetArgs a) {
    uint32_t n = a.n_max;
    if (a.n_sel) {
        const uint32_t v = *a.n_sel;
        n = v < n ? v : n;
    }
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; f < a.total; f += step) {
        const uint64_t j = f / a.units;
        const uint32_t u = (uint32_t)(f - j * a.units);
        if (j >= n) return;   // entries ascend with f
        const uint32_t g = a.sel[j];
        if (g >= a.G_src) continue;
        if (a.state)
            *reinterpret_cast<uint4*>(a.state + (uint64_t)g * a.state_bytes + (uint64_t)u * 16) = make_uint4(0, 0, 0, 0);
        if (u == 0) {
            if (a.store_n) a.store_n[g] = 0;
            if (a.seen) a.seen[g] = 0;
        }
    }
}

}  // namespace

// Both kernels of qf_gen_select_dev, in stream order.
static hipError_t launch_gen_select(const GenSelectArgs& a, uint32_t blocks, hipStream_t st) {
    hipLaunchKernelGGL(k_gen_select_count, dim3(blocks), dim3(kSelThreads), 0, st, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_gen_select_scatter, dim3(blocks), dim3(kSelThreads), 0, st, a);
    return hipGetLastError();
}

size_t gen_select_work_bytes(uint32_t G) { return (size_t)((G + kSelPerBlock - 1) / kSelPerBlock) * 4; }

hipError_t launch_gen_select_list(const uint32_t* rank, uint32_t G, uint32_t min_rank, uint32_t n_max,
                                  uint32_t* counts, uint32_t* sel, uint32_t* n_sel, uint32_t* n_match,
                                  hipStream_t st) {
    if (G == 0 || G > (1u << 24) || n_max == 0 || !rank || !counts || !sel || !n_sel) return hipErrorInvalidValue;
    GenSelectArgs a{};
    a.rank = rank;
    a.counts = counts;
    a.sel = sel;
    a.n_sel = n_sel;
    a.n_match = n_match;
    a.G = G;
    a.min_rank = min_rank;
    a.n_max = n_max;
    return launch_gen_select(a, (G + kSelPerBlock - 1) / kSelPerBlock, st);
}

hipError_t launch_sel_gather(const SelGatherArgs& a, hipStream_t st) {
    if (a.n_max == 0) return hipSuccess;
    if (!a.sel || a.k == 0 || a.k > 256 || a.max_rows == 0 || a.max_rows > 1024 || a.G_src == 0)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sel_gather, dim3(a.n_max), dim3(64), 0, st, a);
    return hipGetLastError();
}

}  // namespace qf

extern "C" int qf_gen_select_dev(qf_ctx* ctx, uint32_t G, const uint32_t* rank, uint32_t* seen, uint32_t min_rank,
                                 uint32_t flags, uint32_t n_max, uint32_t* sel, uint32_t* n_sel, uint32_t* n_match) {
    if (!ctx) return QF_EINVAL;
    if ((flags & ~(uint32_t)QF_SELECT_MARK) || ((flags & QF_SELECT_MARK) && !seen) || n_max == 0 || !sel || !n_sel)
        return QF_EINVAL;
    if (G > (1u << 24)) return QF_EINVAL;
    if (G && !rank) return QF_EINVAL;
    std::unique_lock<std::mutex> lk;
    int s = qf::ctx_lock(ctx, lk);
    if (s) return s;
    hipStream_t st = qf::ctx_stream(ctx);
    if (G == 0) {
        QF_CHECK_HIP(hipMemsetAsync(n_sel, 0, 4, st));
        if (n_match) QF_CHECK_HIP(hipMemsetAsync(n_match, 0, 4, st));
        return QF_OK;
    }
    const uint32_t blocks = (G + qf::kSelPerBlock - 1) / qf::kSelPerBlock;   // <= 8,192
    uint8_t* w = nullptr;
    s = qf::ctx_work(ctx, (size_t)blocks * 4, &w);
    if (s) return s;
    qf::GenSelectArgs a{};
    a.rank = rank;
    a.seen = seen;
    a.counts = reinterpret_cast<uint32_t*>(w);
    a.sel = sel;
    a.n_sel = n_sel;
    a.n_match = n_match;
    a.G = G;
    a.min_rank = min_rank;
    a.n_max = n_max;
    a.mark = flags & QF_SELECT_MARK;
    QF_PROFILED(ctx, st, "k_gen_select", qf::launch_gen_select(a, blocks, st));
    return QF_OK;
}

extern "C" int qf_stream_reset_dev(qf_ctx* ctx, uint32_t k, const qf_gen_sel* sel, uint8_t* state, uint32_t* store_n,
                                   uint32_t* seen) {
    if (!ctx || !sel || !sel->sel_dev || sel->n_max == 0 || sel->G_src == 0) return QF_EINVAL;
    if (k == 0 || k > 256 || (!state && !store_n && !seen)) return QF_EINVAL;
    if (reinterpret_cast<uintptr_t>(state) & 15) return QF_EINVAL;
    std::unique_lock<std::mutex> lk;
    int s = qf::ctx_lock(ctx, lk);
    if (s) return s;
    hipStream_t st = qf::ctx_stream(ctx);
    qf::StreamResetArgs a{};
    a.sel = sel->sel_dev;
    a.n_sel = sel->n_sel_dev;
    a.state = state;
    a.store_n = store_n;
    a.seen = seen;
    a.n_max = sel->n_max;
    a.G_src = sel->G_src;
    a.state_bytes = (uint32_t)qf_rank_state_bytes(k);   // a multiple of 16
    a.units = state ? a.state_bytes / 16 : 1;
    a.total = (uint64_t)a.n_max * a.units;
    // a lane per unit; the grid is bounded and strides over the rest
    const uint64_t need = (a.total + 255) / 256;
    const uint64_t most = (uint64_t)(qf::ctx_num_cus(ctx) > 0 ? qf::ctx_num_cus(ctx) : 1) * 64;
    const dim3 grid((uint32_t)(need < most ? need : most));
    QF_PROFILED(ctx, st, "k_stream_reset", qf::launch_kernel(qf::k_stream_reset, grid, dim3(256), 0, st, a));
    return QF_OK;
}
