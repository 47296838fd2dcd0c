// qf_credit.hip -- the feedback of the streaming loop: what a
// node holds of its generations, written as 16-byte rank reports at the
// receiving side (qf_rank_report_sel_dev), and at the sending side the step
// from the local ranks, a redundancy ratio and the peer's reports to the
// emission budget that qf_gen_select_dev and qf_emit_frames_sel_dev take where
// they took the rank (qf_credit_update_dev).
//
//  k_report_sel      a lane per list entry: the window entry and the rank of
//                    its slot as one record, one 16-byte store.  The base of an
//                    appending call is a copy the call made in front of the
//                    launch, so the one lane that writes the new length races
//                    with nobody.
//  k_credit_reports  a lane per report: one 16-byte load, the checks, the slot's
//                    window entry, the report's status, and for a report of the
//                    generation the slot holds one 32-bit atomicMax of rank + 1
//                    on the slot's word of a zeroed array (the scheme of
//                    k_window_max: a maximum does not depend on the order).
//  k_credit_apply    a lane per slot, the only writer of the slot's state and
//                    credit: one 16-byte load and store of the state, the rule.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qf_fec.h"
#include "qf_kernels.h"

#ifndef QF_DEV
#define QF_DEV __device__ __forceinline__
#endif

namespace qf {

namespace {

constexpr uint64_t kCreditClosed = 1ull << 63;   // the window's closed flag (qf_window.hip)
constexpr uint64_t kCreditIdLimit = 1ull << 62;

__global__ void __launch_bounds__(256) k_report_sel(ReportSelArgs a) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    uint32_t n = a.n_max;
    if (a.n_sel) n = min(*a.n_sel, n);
    const uint32_t base = a.append ? min(a.head[0], a.N_max) : 0;
    const uint64_t end = (uint64_t)base + n;
    if (j == 0) {
        *a.n_reports = end < a.N_max ? (uint32_t)end : a.N_max;
        if (a.n_left) *a.n_left = end > a.N_max ? (uint32_t)(end - a.N_max) : 0;
    }
    if (j >= n || (uint64_t)base + j >= a.N_max) return;   // an unused entry's sel value is not looked at
    const uint32_t s = a.sel[j];
    const bool in = s < a.G_src;
    const uint32_t at = in ? s : 0;                        // nothing is read through a bad slot
    const uint64_t w = a.win[at];
    const uint32_t r = a.rank[at];
    uint64_t id = UINT64_MAX;
    uint32_t held = 0;
    if (in && w != 0) {
        id = (w & ~kCreditClosed) - 1;
        held = (w & kCreditClosed) ? a.k : min(r, a.k);   // a closed generation's rank is zeroed: the window remembers it
    }
    a.reports[base + j] = make_uint4((uint32_t)id, (uint32_t)(id >> 32), held, 0);
}

__global__ void __launch_bounds__(256) k_credit_reports(CreditArgs a) {
    const uint32_t f = blockIdx.x * 256 + threadIdx.x;
    uint32_t n = a.N_max;
    if (a.n_reports) n = min(*a.n_reports, n);
    if (f >= n) return;
    const uint4 rec = a.reports[f];
    const uint64_t id = ((uint64_t)rec.y << 32) | rec.x;
    int32_t st = QF_EINVAL;
    if (id < kCreditIdLimit && rec.z <= a.k && rec.w == 0) {
        const uint32_t s = (uint32_t)(id % a.G);
        const uint64_t have = a.win[s] & ~kCreditClosed;   // 0, or the held id + 1
        st = have > id + 1 ? QF_ESTALE : have < id + 1 ? QF_ENOTREADY : QF_OK;
        if (st == QF_OK) atomicMax(&a.fresh[s], rec.z + 1);
    }
    if (a.report_status) a.report_status[f] = st;
}

// ceil(x * num / den): x <= 256 and den <= num <= 65535, so 32 bits hold it
QF_DEV uint32_t credit_scaled(uint32_t x, uint32_t num, uint32_t den) { return (x * num + den - 1) / den; }

__global__ void __launch_bounds__(256) k_credit_apply(CreditArgs a) {
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= a.G) return;
    const uint64_t have = a.win[s] & ~kCreditClosed;
    const uint4 state = a.state[s];                        // {owner lo, owner hi, peer, reserved}
    const uint32_t m = a.fresh[s];                         // 0, or the largest reported rank + 1
    const uint32_t r = min(a.rank[s], a.k);
    const uint32_t sent = a.sent[s];
    const uint32_t before = a.credit[s];
    // the state owns itself: another generation in the slot starts from nothing
    const bool mine = have == (((uint64_t)state.y << 32) | state.x);
    uint32_t peer = mine ? state.z : 0;
    const uint32_t prev = mine ? before : 0;
    if (m) peer = peer > m - 1 ? peer : m - 1;
    uint64_t c = credit_scaled(r, a.num, a.den);           // the open loop
    if (prev > c) c = prev;
    if (m) {
        // a report asks for what the peer lacks of what this node holds
        const uint64_t want = (uint64_t)sent + credit_scaled(r > peer ? r - peer : 0, a.num, a.den);
        if (want > c) c = want;
    }
    if (c > a.cap) c = a.cap;
    if (peer >= a.k) c = sent;                             // the peer is satisfied
    if (have == 0) {
        c = 0;
        peer = 0;
    }
    a.state[s] = make_uint4((uint32_t)have, (uint32_t)(have >> 32), peer, 0);
    a.credit[s] = (uint32_t)c;
}

}  // namespace

hipError_t launch_report_sel(const ReportSelArgs& a, hipStream_t st) {
    if (!a.sel || !a.win || !a.rank || !a.reports || !a.n_reports || (a.append && !a.head) || a.n_max == 0 ||
        a.G_src == 0 || a.N_max == 0 || a.k == 0 || a.k > 256)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_report_sel, dim3((uint32_t)(((uint64_t)a.n_max + 255) / 256)), dim3(256), 0, st, a);
    return hipGetLastError();
}

static bool credit_args_ok(const CreditArgs& a) {
    return a.win && a.rank && a.sent && a.state && a.credit && a.fresh && (a.reports || a.N_max == 0) && a.G &&
           a.G <= (1u << 24) && a.k && a.k <= 256 && a.den && a.num >= a.den && a.num <= 65535 && a.cap &&
           a.cap <= (1u << 20);
}

hipError_t launch_credit_reports(const CreditArgs& a, hipStream_t st) {
    if (!credit_args_ok(a) || a.N_max == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_credit_reports, dim3((uint32_t)(((uint64_t)a.N_max + 255) / 256)), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_credit_apply(const CreditArgs& a, hipStream_t st) {
    if (!credit_args_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_credit_apply, dim3((a.G + 255) / 256), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace qf

#ifndef QF_KERNEL_EMU   // (tests/kernel_emu builds the kernels and launchers above for the host)
#include <mutex>

#include "qf_internal.h"

static_assert(sizeof(qf_rank_report) == 16, "a report is one 16-byte record");

extern "C" int qf_rank_report_sel_dev(qf_ctx* ctx, uint32_t k, const qf_gen_sel* sel, const uint64_t* win,
                                      const uint32_t* rank, uint32_t N_max, uint32_t flags, qf_rank_report* reports,
                                      uint32_t* n_reports, uint32_t* n_left) {
    if (!ctx || !sel || !sel->sel_dev || !win || !rank || !reports || !n_reports) return QF_EINVAL;
    if (k == 0 || k > 256 || sel->n_max == 0 || sel->G_src == 0 || N_max == 0) return QF_EINVAL;
    if ((flags & ~(uint32_t)QF_REPORT_APPEND) || !aligned16(reports)) return QF_EINVAL;
    std::unique_lock<std::mutex> lk;
    int s = qf::ctx_lock(ctx, lk);
    if (s) return s;
    hipStream_t st = qf::ctx_stream(ctx);
    qf::ReportSelArgs a{};
    a.sel = sel->sel_dev;
    a.n_sel = sel->n_sel_dev;
    a.win = win;
    a.rank = rank;
    a.reports = reinterpret_cast<uint4*>(reports);
    a.n_reports = n_reports;
    a.n_left = n_left;
    a.n_max = sel->n_max;
    a.G_src = sel->G_src;
    a.k = k;
    a.N_max = N_max;
    a.append = flags & QF_REPORT_APPEND;
    if (a.append) {
        // the length the call appends at, taken before the kernel that overwrites it
        uint8_t* w = nullptr;
        s = qf::ctx_work(ctx, 4, &w);
        if (s) return s;
        QF_CHECK_HIP(hipMemcpyAsync(w, n_reports, 4, hipMemcpyDeviceToDevice, st));
        a.head = reinterpret_cast<const uint32_t*>(w);
    }
    QF_PROFILED(ctx, st, "k_report_sel", qf::launch_report_sel(a, st));
    return QF_OK;
}

extern "C" int qf_credit_update_dev(qf_ctx* ctx, const qf_credit_shape* sh, uint32_t G, const uint64_t* win,
                                    const uint32_t* rank, const uint32_t* sent, uint32_t N_max,
                                    const qf_rank_report* reports, const uint32_t* n_reports, uint8_t* fb_state,
                                    uint32_t* credit, int32_t* report_status) {
    if (!ctx || !sh || !win || !rank || !sent || !fb_state || !credit || (N_max && !reports)) return QF_EINVAL;
    if (sh->k == 0 || sh->k > 256 || sh->den == 0 || sh->num < sh->den || sh->num > 65535 || sh->cap == 0 ||
        sh->cap > (1u << 20) || G == 0 || G > (1u << 24) || sh->flags != 0 || sh->reserved != 0)
        return QF_EINVAL;
    if ((reinterpret_cast<uintptr_t>(win) & 7) || !aligned16(reports) || !aligned16(fb_state)) return QF_EINVAL;
    std::unique_lock<std::mutex> lk;
    int s = qf::ctx_lock(ctx, lk);
    if (s) return s;
    hipStream_t st = qf::ctx_stream(ctx);
    // workspace: per slot the call's largest reported rank + 1, zeroed
    uint8_t* w = nullptr;
    s = qf::ctx_work(ctx, (size_t)G * 4, &w);
    if (s) return s;
    qf::CreditArgs a{};
    a.win = win;
    a.rank = rank;
    a.sent = sent;
    a.reports = reinterpret_cast<const uint4*>(reports);
    a.n_reports = n_reports;
    a.fresh = reinterpret_cast<uint32_t*>(w);
    a.state = reinterpret_cast<uint4*>(fb_state);
    a.credit = credit;
    a.report_status = report_status;
    a.G = G;
    a.N_max = N_max;
    a.k = sh->k;
    a.num = sh->num;
    a.den = sh->den;
    a.cap = sh->cap;
    QF_CHECK_HIP(hipMemsetAsync(w, 0, (size_t)G * 4, st));
    if (N_max) QF_PROFILED(ctx, st, "k_credit_reports", qf::launch_credit_reports(a, st));
    QF_PROFILED(ctx, st, "k_credit_apply", qf::launch_credit_apply(a, st));
    return QF_OK;
}
#endif  // QF_KERNEL_EMU
