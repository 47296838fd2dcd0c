// k_fbw_count / k_fbw_pack, k_fbr_count / k_fbr_place / k_fbr_records and
// k_closed_mark on the host shim (hip/hip_runtime.h beside this file) -- TEST
// INFRASTRUCTURE ONLY (tests/test_fbwire_kernel_emu_cpu.py).  Includes
// csrc/qf_fbwire.hip as it is, with -DQF_KERNEL_EMU and the host sanitizers.
//   fbwire_emu IN OUT
// IN, mode 0 (qf_frame_reports_dev's kernels): u32 0, k, max_len, F_max, stride,
//      N_max, n_reports (0xFFFFFFFF: NULL), has_n_left, has_n_skipped, 0, 0, 0;
//      reports 16 bytes[N_max]; then what the call starts from: pkts u8[F_max *
//      stride], pkt_len u32[F_max], n_pkts u32, n_left u32, n_skipped u32 (the
//      last two when given).
// OUT: pkts, pkt_len, n_pkts, n_left, n_skipped (when given).
// IN, mode 1 (qf_parse_report_frames_dev's kernels): u32 1, k, max_len, F_max,
//      stride, N_max, n_pkts (0xFFFFFFFF: NULL), append, has_n_left, has_status,
//      has_first, has_count; pkts u8[F_max * stride]; pkt_len u32[F_max]; then
//      reports 16 bytes[N_max], n_reports u32, and when given n_left u32,
//      pkt_status i32[F_max], pkt_first u32[F_max], pkt_count u32[F_max].
// OUT: reports, n_reports, n_left, pkt_status, pkt_first, pkt_count (when given).
// IN, mode 2 (k_closed_mark): u32 2, G_src, F_max, n_frames (0xFFFFFFFF: NULL), 0
//      ...; frame_id u64[F_max]; frame_status i32[F_max]; win u64[G_src].
// OUT: the flags u32[G_src] (the call's zeroed workspace after the kernel; the
//      select and report kernels that follow are those of their own files).
// Every buffer and every part of the workspace is a heap block of exactly its
// size.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <hip/hip_runtime.h>

#include "qf_fbwire.hip"

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

template <class T>
static T* ws(size_t n) {
    return static_cast<T*>(malloc(n * sizeof(T) ? n * sizeof(T) : 1));
}

static int pack(FILE* f, const uint32_t* h, const char* out) {
    const uint32_t F_max = h[3], stride = h[4], N_max = h[5];
    qf::FbPackArgs a{};
    a.reports = rd<uint4>(f, N_max);
    a.pkts = rd<uint8_t>(f, (size_t)F_max * stride);
    a.pkt_len = rd<uint32_t>(f, F_max);
    a.n_pkts = rd<uint32_t>(f, 1);
    if (h[7]) a.n_left = rd<uint32_t>(f, 1);
    if (h[8]) a.n_skipped = rd<uint32_t>(f, 1);
    fclose(f);
    uint32_t n_reports = h[6];
    a.n_reports = n_reports == 0xFFFFFFFFu ? nullptr : &n_reports;
    a.stride = stride;
    a.N_max = N_max;
    a.k = h[1];
    a.per = qf_report_frame_capacity(h[2]);
    a.F_max = F_max;
    a.blocks = (N_max + qf::kFbPerBlock - 1) / qf::kFbPerBlock;
    a.sums = ws<uint32_t>(a.blocks);
    if (qf::launch_fbw_count(a, nullptr) != hipSuccess || qf::launch_fbw_pack(a, nullptr) != hipSuccess) return 3;
    FILE* o = fopen(out, "wb");
    if (!o) return 2;
    fwrite(a.pkts, 1, (size_t)F_max * stride, o);
    fwrite(a.pkt_len, 4, F_max, o);
    fwrite(a.n_pkts, 4, 1, o);
    if (a.n_left) fwrite(a.n_left, 4, 1, o);
    if (a.n_skipped) fwrite(a.n_skipped, 4, 1, o);
    fclose(o);
    return 0;
}

static int parse(FILE* f, const uint32_t* h, const char* out) {
    const uint32_t F_max = h[3], stride = h[4], N_max = h[5];
    qf::FbParseArgs a{};
    a.pkts = rd<uint8_t>(f, (size_t)F_max * stride);
    a.pkt_len = rd<uint32_t>(f, F_max);
    a.reports = rd<uint4>(f, N_max);
    a.n_reports = rd<uint32_t>(f, 1);
    if (h[8]) a.n_left = rd<uint32_t>(f, 1);
    if (h[9]) a.pkt_status = rd<int32_t>(f, F_max);
    if (h[10]) a.pkt_first = rd<uint32_t>(f, F_max);
    if (h[11]) a.pkt_count = rd<uint32_t>(f, F_max);
    fclose(f);
    uint32_t n_pkts = h[6];
    a.n_pkts = n_pkts == 0xFFFFFFFFu ? nullptr : &n_pkts;
    a.stride = stride;
    a.F_max = F_max;
    a.N_max = N_max;
    a.max_len = h[2];
    a.per = qf_report_frame_capacity(h[2]);
    a.chunks = (a.per + 63) / 64;
    a.append = h[7];
    a.blocks = qf::fb_parse_blocks(F_max);
    a.cnt = ws<uint32_t>(F_max);
    a.first = ws<uint32_t>(F_max);
    a.sums = ws<uint32_t>(a.blocks);
    if (a.append) {
        uint32_t* head = ws<uint32_t>(1);
        *head = *a.n_reports;
        a.head = head;
    }
    if (qf::launch_fbr_count(a, nullptr) != hipSuccess || qf::launch_fbr_place(a, nullptr) != hipSuccess ||
        qf::launch_fbr_records(a, nullptr) != hipSuccess)
        return 3;
    FILE* o = fopen(out, "wb");
    if (!o) return 2;
    fwrite(a.reports, 16, N_max, o);
    fwrite(a.n_reports, 4, 1, o);
    if (a.n_left) fwrite(a.n_left, 4, 1, o);
    if (a.pkt_status) fwrite(a.pkt_status, 4, F_max, o);
    if (a.pkt_first) fwrite(a.pkt_first, 4, F_max, o);
    if (a.pkt_count) fwrite(a.pkt_count, 4, F_max, o);
    fclose(o);
    return 0;
}

static int mark(FILE* f, const uint32_t* h, const char* out) {
    const uint32_t G_src = h[1], F_max = h[2];
    qf::ClosedMarkArgs a{};
    a.frame_id = rd<uint64_t>(f, F_max);
    a.frame_status = rd<int32_t>(f, F_max);
    a.win = rd<uint64_t>(f, G_src);
    fclose(f);
    uint32_t n_frames = h[3];
    a.n_frames = n_frames == 0xFFFFFFFFu ? nullptr : &n_frames;
    a.flags = static_cast<uint32_t*>(calloc(G_src, 4));
    a.F_max = F_max;
    a.G_src = G_src;
    if (qf::launch_closed_mark(a, nullptr) != hipSuccess) return 3;
    FILE* o = fopen(out, "wb");
    if (!o) return 2;
    fwrite(a.flags, 4, G_src, o);
    fclose(o);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t h[12];
    if (fread(h, 4, 12, f) != 12) return 2;
    const int rc = h[0] == 0 ? pack(f, h, argv[2]) : h[0] == 1 ? parse(f, h, argv[2]) : mark(f, h, argv[2]);
    if (rc == 3) fprintf(stderr, "a launch was refused\n");
    fflush(nullptr);
    _exit(rc);   // (the buffers live until here: no leak report wanted for them)
}
