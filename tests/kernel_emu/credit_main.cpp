// k_report_sel, k_credit_reports and k_credit_apply on the host shim
// (hip/hip_runtime.h beside this file) -- TEST INFRASTRUCTURE ONLY
// (tests/test_credit_kernel_emu_cpu.py).  Includes csrc/qf_credit.hip as it is,
// with -DQF_KERNEL_EMU and the host sanitizers.
//   credit_emu IN OUT
// IN, mode 0 (qf_credit_update_dev's kernels): u32 0, G, N_max, k, num, den,
//      cap, n_reports (0xFFFFFFFF: NULL), has_status, 0, 0, 0; win u64[G]; rank,
//      sent u32[G]; reports 16 bytes[N_max]; then what the call starts from:
//      state 16 bytes[G], credit u32[G], status i32[N_max] (when given).
// OUT: state, credit, status (when given).
// IN, mode 1 (qf_rank_report_sel_dev's kernel): u32 1, k, n_max, G_src, N_max,
//      append, n_sel (0xFFFFFFFF: NULL), has_n_left, 0, 0, 0, 0; sel u32[n_max];
//      win u64[G_src]; rank u32[G_src]; then reports 16 bytes[N_max], n_reports
//      u32, n_left u32 (when given).
// OUT: reports, n_reports, n_left (when given).
// Every buffer is a heap block of exactly its size; the workspace of mode 0 is
// G zeroed u32 (the call's memset), that of mode 1 the copy of *n_reports.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <hip/hip_runtime.h>

// the 32-bit maximum of k_credit_reports: the lanes of the block are host threads
inline uint32_t atomicMax(uint32_t* p, uint32_t v) {
    std::lock_guard<std::mutex> lk(emu_mu);
    const uint32_t o = *p;
    if (v > o) *p = v;
    return o;
}

#include "qf_credit.hip"

thread_local EmuIdx threadIdx;
EmuIdx blockIdx;
uint8_t* emu_lds;
std::barrier<>* emu_bar;
uint64_t emu_pred[64];
uint32_t emu_xch[64];
std::mutex emu_mu;

template <class T>
static T* rd(FILE* f, size_t n) {
    T* p = static_cast<T*>(malloc(n * sizeof(T) ? n * sizeof(T) : 1));
    if (n && fread(p, sizeof(T), n, f) != n) {
        fprintf(stderr, "short input\n");
        exit(2);
    }
    return p;
}

static int credit(FILE* f, const uint32_t* h, const char* out) {
    const uint32_t G = h[1], N_max = h[2];
    qf::CreditArgs a{};
    a.win = rd<uint64_t>(f, G);
    a.rank = rd<uint32_t>(f, G);
    a.sent = rd<uint32_t>(f, G);
    a.reports = N_max ? rd<uint4>(f, N_max) : nullptr;
    a.state = rd<uint4>(f, G);
    a.credit = rd<uint32_t>(f, G);
    if (h[8]) a.report_status = rd<int32_t>(f, N_max);
    fclose(f);
    uint32_t n_reports = h[7];
    a.n_reports = n_reports == 0xFFFFFFFFu ? nullptr : &n_reports;
    a.fresh = static_cast<uint32_t*>(calloc(G, 4));
    a.G = G;
    a.N_max = N_max;
    a.k = h[3];
    a.num = h[4];
    a.den = h[5];
    a.cap = h[6];
    if (N_max && qf::launch_credit_reports(a, nullptr) != hipSuccess) return 3;
    if (qf::launch_credit_apply(a, nullptr) != hipSuccess) return 3;
    FILE* o = fopen(out, "wb");
    if (!o) return 2;
    fwrite(a.state, 16, G, o);
    fwrite(a.credit, 4, G, o);
    if (a.report_status) fwrite(a.report_status, 4, N_max, o);
    fclose(o);
    return 0;
}

static int report(FILE* f, const uint32_t* h, const char* out) {
    const uint32_t n_max = h[2], G_src = h[3], N_max = h[4];
    qf::ReportSelArgs a{};
    a.sel = rd<uint32_t>(f, n_max);
    a.win = rd<uint64_t>(f, G_src);
    a.rank = rd<uint32_t>(f, G_src);
    a.reports = rd<uint4>(f, N_max);
    a.n_reports = rd<uint32_t>(f, 1);
    if (h[7]) a.n_left = rd<uint32_t>(f, 1);
    fclose(f);
    uint32_t n_sel = h[6];
    a.n_sel = n_sel == 0xFFFFFFFFu ? nullptr : &n_sel;
    a.n_max = n_max;
    a.G_src = G_src;
    a.k = h[1];
    a.N_max = N_max;
    a.append = h[5];
    if (a.append) {
        uint32_t* head = static_cast<uint32_t*>(malloc(4));
        *head = *a.n_reports;
        a.head = head;
    }
    if (qf::launch_report_sel(a, nullptr) != hipSuccess) return 3;
    FILE* o = fopen(out, "wb");
    if (!o) return 2;
    fwrite(a.reports, 16, N_max, o);
    fwrite(a.n_reports, 4, 1, o);
    if (a.n_left) fwrite(a.n_left, 4, 1, o);
    fclose(o);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t h[12];
    if (fread(h, 4, 12, f) != 12) return 2;
    const int rc = h[0] == 0 ? credit(f, h, argv[2]) : report(f, h, argv[2]);
    if (rc == 3) fprintf(stderr, "a launch was refused\n");
    fflush(nullptr);
    _exit(rc);   // (the buffers live until here: no leak report wanted for them)
}
