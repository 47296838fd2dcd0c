// The per-lane pieces of csrc/qf_wire_dev.h on the host shim (hip/hip_runtime.h
// beside this file) -- TEST INFRASTRUCTURE ONLY (tests/test_wire_dev_emu_cpu.py
// builds this program with the host sanitizers).  frame_head and vector_block
// are barrier-free, so they run in plain loops: the decision for every frame
// slot in order, then every 16-byte block of every accepted row's vector.
//   wire_dev_emu IN OUT
// IN:  u32 k, L, N, pay16, end_with_payload, 0; u64 frame_stride; frame_len and
//      frame_off u32[N]; ids u64[N]; frames u8[N][frame_stride].
// OUT: status i32[N]; idx, pay, plen u32[N] (as returned); n u32;
//      row_coeffs u8[n][k] in slot order.
// The frames are one heap block of exactly N * frame_stride bytes and
// row_coeffs one of exactly n * k (0xCC before the copy), so the host address
// sanitizer sees a read past a slot of the last frame or a write past a row.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "qf_wire_dev.h"

template <class T>
static T* rd(FILE* f, size_t n) {
    T* p = static_cast<T*>(malloc(n * sizeof(T) ? n * sizeof(T) : 1));
    if (n && fread(p, sizeof(T), n, f) != n) {
        fprintf(stderr, "short input\n");
        exit(2);
    }
    return p;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t h[6];
    uint64_t fs;
    if (fread(h, 4, 6, f) != 6 || fread(&fs, 8, 1, f) != 1) return 2;
    const uint32_t k = h[0], L = h[1], N = h[2];
    const bool pay16 = h[3] != 0, with_payload = h[4] != 0;
    const uint32_t* flen = rd<uint32_t>(f, N);
    const uint32_t* foff = rd<uint32_t>(f, N);
    const uint64_t* ids = rd<uint64_t>(f, N);
    const uint8_t* frames = rd<uint8_t>(f, (size_t)N * fs);
    fclose(f);
    qf::FrameHead* head = static_cast<qf::FrameHead*>(malloc(N * sizeof(qf::FrameHead)));
    uint32_t n = 0;
    for (uint32_t s = 0; s < N; ++s) {
        head[s] = qf::frame_head(frames + s * fs, flen[s], foff[s], fs, ids + s, k, L, pay16);
        n += head[s].st == QF_OK;
    }
    uint8_t* coeffs = static_cast<uint8_t*>(malloc((size_t)n * k ? (size_t)n * k : 1));
    memset(coeffs, 0xCC, (size_t)n * k);
    uint32_t slot = 0;
    for (uint32_t s = 0; s < N; ++s) {
        if (head[s].st != QF_OK) continue;
        const uint32_t end = head[s].pay + (with_payload ? head[s].plen : 0);
        for (uint32_t c0 = 0; c0 < k; c0 += 16)
            qf::vector_block(coeffs + (size_t)slot * k, c0, k, head[s].idx, frames + s * fs, head[s].pay, end);
        ++slot;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    for (uint32_t s = 0; s < N; ++s) fwrite(&head[s].st, 4, 1, o);
    for (uint32_t s = 0; s < N; ++s) fwrite(&head[s].idx, 4, 1, o);
    for (uint32_t s = 0; s < N; ++s) fwrite(&head[s].pay, 4, 1, o);
    for (uint32_t s = 0; s < N; ++s) fwrite(&head[s].plen, 4, 1, o);
    fwrite(&n, 4, 1, o);
    fwrite(coeffs, 1, (size_t)n * k, o);
    fclose(o);
    _exit(0);   // (the buffers live until here: no leak report wanted for them)
}
