// k_partial_prepare on the host shim (hip/hip_runtime.h beside this file) -- TEST
// INFRASTRUCTURE ONLY.  The test writes qf_partial_emu.inc, the text of
// csrc/qf_partial.hip with its dynamic LDS declaration replaced by `uint8_t* lds
// = emu_lds;`, and builds this program with the host sanitizers.
//   partial_prepare_emu IN OUT
// IN:  u32 k, e_max, max_rows, G, L, passes, rep_limit, 0; u64 src_gen_stride,
//      coef_gen_stride; explog[768]; row_index u16[G][max_rows]; n_rows u32[G];
//      row_coeffs u8[G][max_rows][k]; accept u8[G][max_rows]; row_off and row_len
//      u32[G][max_rows].
// OUT: status i32[G]; n_out, bound, min_len u32[G]; rec_index u16[G][e_max];
//      src_slot u16[G][k]; the pair records u8[max(passes, 1)][G][coef_gen_stride].
// Every buffer is a heap block of exactly its size; outputs start as 0xCC.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "qf_partial_emu.inc"

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
    uint32_t h[8];
    uint64_t s[2];
    if (fread(h, 4, 8, f) != 8 || fread(s, 8, 2, f) != 2) return 2;
    const uint32_t k = h[0], e_max = h[1], mr = h[2], G = h[3], passes = h[5];
    const size_t slots = (size_t)G * mr;
    qf::PrepareArgs a{};
    a.explog = rd<uint8_t>(f, 768);
    a.row_index = rd<uint16_t>(f, slots);
    a.n_rows = rd<uint32_t>(f, G);
    a.row_coeffs = rd<uint8_t>(f, slots * k);
    a.accept = rd<uint8_t>(f, slots);
    a.row_off = rd<uint32_t>(f, slots);
    a.row_len = rd<uint32_t>(f, slots);
    fclose(f);
    const size_t ncoef = (size_t)(passes ? passes : 1) * G * s[1];
    a.coef_out = filled<uint8_t>(ncoef);
    a.coef_gen_stride = s[1];
    a.n_out = filled<uint32_t>(G);
    a.bound = filled<uint32_t>(G);
    a.min_len = filled<uint32_t>(G);
    a.status = filled<int32_t>(G);
    a.rec_index = filled<uint16_t>((size_t)G * e_max);
    a.src_slot = filled<uint16_t>((size_t)G * k);
    a.k = k;
    a.e_max = e_max;
    a.rep_limit = h[6];
    a.e_lds = k < 128 ? k : 128;
    a.max_rows = mr;
    a.max_rows_pad = (mr + 7) & ~7u;
    a.passes = passes;
    a.G = G;
    a.src_gen_stride = s[0];
    a.L = h[4];
    if (qf::launch_partial_prepare(a, nullptr) != hipSuccess) {
        fprintf(stderr, "the launch was refused\n");
        return 3;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(a.status, 4, G, o);
    fwrite(a.n_out, 4, G, o);
    fwrite(a.bound, 4, G, o);
    fwrite(a.min_len, 4, G, o);
    fwrite(a.rec_index, 2, (size_t)G * e_max, o);
    fwrite(a.src_slot, 2, (size_t)G * k, o);
    fwrite(a.coef_out, 1, ncoef, o);
    fclose(o);
    _exit(0);   // (the buffers live until here: no leak report wanted for them)
}
