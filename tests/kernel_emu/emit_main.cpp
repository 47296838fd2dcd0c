// k_emit_count, k_emit_place and k_emit_frames on the host shim
// (hip/hip_runtime.h and deliver_emu.h beside this file) -- TEST INFRASTRUCTURE
// ONLY (tests/test_emit_kernel_emu_cpu.py).  Includes csrc/qf_emit.hip as it
// is, with -DQF_KERNEL_EMU and the host sanitizers.
//   emit_emu IN OUT
// IN:  u32 k, L, max_rows, n_max, G_src, N_max, append, n_sel (0xFFFFFFFF:
//      NULL), has_row_index, has_n_rows, has_coeffs, has_row_len, has_in_status,
//      has_budget, has_n_left, grid_cap; u64 row_stride, rows_gen_stride,
//      frame_stride, rows_bytes; rows; sel u32[n_max]; ids u64[n_max]; then, each
//      when it is given, row_index u16[n_max][max_rows], n_rows u32[n_max],
//      row_coeffs u8[n_max][max_rows][k], row_len u32[n_max][max_rows],
//      in_status i32[n_max], rank and sent u32[G_src]; then what the outputs
//      hold before the call: frames u8[N_max * frame_stride], frame_len,
//      frame_off u32[N_max], frame_id, frame_pkt u64[N_max], n_frames u32,
//      n_left u32 (when given), entry_first, entry_count u32[n_max],
//      entry_status i32[n_max].
// OUT: the outputs in that order, then sent (when given).
// Every buffer is a heap block of exactly its size; the workspace starts as 0xCC.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "deliver_emu.h"
#include "qf_emit.hip"

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
static T* filled(size_t n) {
    T* p = static_cast<T*>(malloc(n * sizeof(T) ? n * sizeof(T) : 1));
    memset(p, 0xCC, n * sizeof(T));
    return p;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t h[16];
    uint64_t s[4];
    if (fread(h, 4, 16, f) != 16 || fread(s, 8, 4, f) != 4) return 2;
    const uint32_t k = h[0], mr = h[2], n_max = h[3], G_src = h[4], N_max = h[5];
    const size_t nr = (size_t)n_max * mr;
    const uint8_t* rows = rd<uint8_t>(f, s[3]);
    qf::EmitPlanArgs a{};
    a.sel = rd<uint32_t>(f, n_max);
    a.ids = rd<uint64_t>(f, n_max);
    uint32_t n_sel = h[7];
    a.n_sel = n_sel == 0xFFFFFFFFu ? nullptr : &n_sel;
    if (h[8]) a.row_index = rd<uint16_t>(f, nr);
    if (h[9]) a.n_rows = rd<uint32_t>(f, n_max);
    const uint8_t* coeffs = h[10] ? rd<uint8_t>(f, nr * k) : nullptr;
    if (h[11]) a.row_len = rd<uint32_t>(f, nr);
    if (h[12]) a.in_status = rd<int32_t>(f, n_max);
    if (h[13]) {
        a.rank = rd<uint32_t>(f, G_src);
        a.sent = rd<uint32_t>(f, G_src);
    }
    const size_t frame_bytes = (size_t)N_max * s[2];
    uint8_t* frames = rd<uint8_t>(f, frame_bytes);
    a.frame_len = rd<uint32_t>(f, N_max);
    a.frame_off = rd<uint32_t>(f, N_max);
    a.frame_id = rd<uint64_t>(f, N_max);
    a.frame_pkt = rd<uint64_t>(f, N_max);
    a.n_frames = rd<uint32_t>(f, 1);
    if (h[14]) a.n_left = rd<uint32_t>(f, 1);
    a.entry_first = rd<uint32_t>(f, n_max);
    a.entry_count = rd<uint32_t>(f, n_max);
    a.entry_status = rd<int32_t>(f, n_max);
    fclose(f);
    a.n_max = n_max;
    a.G_src = G_src;
    a.k = k;
    a.L = h[1];
    a.max_rows = mr;
    a.N_max = N_max;
    a.P = (3 + k + 15) / 16 * 16;
    a.append = h[6];
    a.has_coeffs = coeffs != nullptr;
    a.blocks = (n_max + qf::kEmitPerBlock - 1) / qf::kEmitPerBlock;
    const uint64_t most = nr < N_max ? nr : N_max;
    a.want = filled<uint32_t>(n_max);
    a.sums = filled<uint32_t>(a.blocks);
    a.head = filled<uint32_t>(2);
    a.rec = filled<uint4>(most);
    if (qf::launch_emit_count(a, nullptr) != hipSuccess || qf::launch_emit_place(a, nullptr) != hipSuccess) {
        fprintf(stderr, "a planning launch was refused\n");
        return 3;
    }
    qf::EmitFramesArgs fa{};
    fa.rows = rows;
    fa.row_coeffs = coeffs;
    fa.frames = frames;
    fa.rec = a.rec;
    fa.head = a.head;
    fa.row_stride = s[0];
    fa.rows_gen_stride = s[1];
    fa.frame_stride = s[2];
    fa.k = k;
    fa.P = a.P;
    fa.max_rows = mr;
    if (qf::launch_emit_frames(fa, most, h[15], nullptr) != hipSuccess) {
        fprintf(stderr, "the copy's launch was refused\n");
        return 3;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(frames, 1, frame_bytes, o);
    fwrite(a.frame_len, 4, N_max, o);
    fwrite(a.frame_off, 4, N_max, o);
    fwrite(a.frame_id, 8, N_max, o);
    fwrite(a.frame_pkt, 8, N_max, o);
    fwrite(a.n_frames, 4, 1, o);
    if (a.n_left) fwrite(a.n_left, 4, 1, o);
    fwrite(a.entry_first, 4, n_max, o);
    fwrite(a.entry_count, 4, n_max, o);
    fwrite(a.entry_status, 4, n_max, o);
    if (a.sent) fwrite(a.sent, 4, G_src, o);
    fclose(o);
    _exit(0);   // (the buffers live until here: no leak report wanted for them)
}
