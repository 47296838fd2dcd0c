// k_deliver_prepare and k_deliver_rows on the host shim (hip/hip_runtime.h and
// deliver_emu.h beside this file) -- TEST INFRASTRUCTURE ONLY.  The test writes
// qf_deliver_emu.inc, the text of csrc/qf_deliver.hip with its dynamic LDS
// declaration replaced by `uint8_t* lds = emu_lds;`, and builds this program
// with -DQF_KERNEL_EMU and the host sanitizers.
//   deliver_prepare_emu IN OUT
// IN:  u32 k, e_max, L, max_rows, G, G_src, has_sel, n_sel (0xFFFFFFFF: NULL),
//      has_ids, has_delivered, has_n_known, grid_cap; u64 src_gen_stride,
//      rec_row_stride, rec_gen_stride, out_row_stride, out_gen_stride,
//      src_bytes, rec_bytes, out_bytes; src; row_off and row_len u32[G_src]
//      [max_rows]; rec; rec_index u16[G][e_max]; n_rec u32[G]; dec_status
//      i32[G]; src_slot u16[G][k]; sel u32[G], ids u64[G] and delivered
//      u64[G_src][5], each when it is given.
// OUT: out; out_len u32[G][k]; out_state u8[G][k]; n_out, n_known u32[G];
//      status i32[G]; delivered (when given); the counts u32[G].
// Every buffer is a heap block of exactly its size (rec and rec_index are NULL
// when e_max is 0); outputs and the workspace start as 0xCC.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "deliver_emu.h"
#include "qf_deliver_emu.inc"

thread_local EmuIdx threadIdx;
EmuIdx blockIdx;
uint8_t* emu_lds;
std::barrier<>* emu_bar;
uint64_t emu_pred[64];
uint32_t emu_xch[64];
std::mutex emu_mu;

template <class T>
static T* rd(FILE* f, size_t n) {
    if (!n) return nullptr;
    T* p = static_cast<T*>(malloc(n * sizeof(T)));
    if (fread(p, sizeof(T), n, f) != n) {
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
    uint32_t h[12];
    uint64_t s[8];
    if (fread(h, 4, 12, f) != 12 || fread(s, 8, 8, f) != 8) return 2;
    const uint32_t k = h[0], e_max = h[1], mr = h[3], G = h[4], G_src = h[5];
    const uint8_t* src = rd<uint8_t>(f, s[5]);
    qf::DeliverPrepareArgs a{};
    a.row_off = rd<uint32_t>(f, (size_t)G_src * mr);
    a.row_len = rd<uint32_t>(f, (size_t)G_src * mr);
    const uint8_t* rec = rd<uint8_t>(f, s[6]);
    a.rec_index = rd<uint16_t>(f, (size_t)G * e_max);
    a.n_rec = rd<uint32_t>(f, G);
    a.dec_status = rd<int32_t>(f, G);
    a.src_slot = rd<uint16_t>(f, (size_t)G * k);
    uint32_t n_sel = h[7];
    if (h[6]) {
        a.sel = rd<uint32_t>(f, G);
        a.n_sel = n_sel == 0xFFFFFFFFu ? nullptr : &n_sel;
        a.G_src = G_src;
    }
    if (h[8]) a.ids = rd<uint64_t>(f, G);
    if (h[9]) a.delivered = rd<uint64_t>(f, (size_t)G_src * 5);
    fclose(f);
    uint8_t* out = filled<uint8_t>(s[7]);
    a.out_len = filled<uint32_t>((size_t)G * k);
    a.out_state = filled<uint8_t>((size_t)G * k);
    a.n_out = filled<uint32_t>(G);
    a.n_known = h[10] ? filled<uint32_t>(G) : nullptr;
    a.status = filled<int32_t>(G);
    a.rec = filled<uint4>((size_t)G * k);
    a.cnt = filled<uint32_t>(G);
    a.src_gen_stride = s[0];
    a.rec_row_stride = s[1];
    a.rec_gen_stride = s[2];
    a.k = k;
    a.e_max = e_max;
    a.L = h[2];
    a.max_rows = mr;
    a.G = G;
    if (qf::launch_deliver_prepare(a, nullptr) != hipSuccess) {
        fprintf(stderr, "the control launch was refused\n");
        return 3;
    }
    qf::DeliverRowsArgs ra{};
    ra.src = src;
    ra.rec_rows = rec;
    ra.out = out;
    ra.rec = a.rec;
    ra.cnt = a.cnt;
    ra.out_row_stride = s[3];
    ra.out_gen_stride = s[4];
    ra.k = k;
    if (qf::launch_deliver_rows(ra, G, h[11], nullptr) != hipSuccess) {
        fprintf(stderr, "the copy's launch was refused\n");
        return 3;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(out, 1, s[7], o);
    fwrite(a.out_len, 4, (size_t)G * k, o);
    fwrite(a.out_state, 1, (size_t)G * k, o);
    fwrite(a.n_out, 4, G, o);
    if (a.n_known) fwrite(a.n_known, 4, G, o);
    fwrite(a.status, 4, G, o);
    if (a.delivered) fwrite(a.delivered, 8, (size_t)G_src * 5, o);
    fwrite(a.cnt, 4, G, o);
    fclose(o);
    _exit(0);   // (the buffers live until here: no leak report wanted for them)
}
