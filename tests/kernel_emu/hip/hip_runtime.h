// A host stand-in for the few HIP pieces a one-wave control kernel uses -- TEST
// INFRASTRUCTURE ONLY (tests/test_partial_kernel_emu_cpu.py).  A launch runs the
// kernel's 64 lanes as 64 host threads per block; __syncthreads, __ballot, __any
// and __shfl_xor meet at a barrier, so a kernel whose lanes reach them together
// (a single wave with uniform control flow) computes what it computes on the
// device.  Dynamic LDS is one heap block of exactly the launch's size, so the
// host address sanitizer sees an access past it.  Between two barriers the
// threads run in any order: the shim checks results and bounds, not the
// ordering of LDS accesses within a phase.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include <barrier>
#include <mutex>
#include <thread>
#include <vector>

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __shared__
#define __launch_bounds__(...)

typedef int hipError_t;
typedef void* hipStream_t;
typedef void* hipEvent_t;
constexpr hipError_t hipSuccess = 0, hipErrorInvalidValue = 1;
constexpr int hipFuncAttributeMaxDynamicSharedMemorySize = 8;
inline hipError_t hipFuncSetAttribute(const void*, int, int) { return hipSuccess; }
inline hipError_t hipGetLastError() { return hipSuccess; }

struct uint4 {
    uint32_t x, y, z, w;
};
inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
struct dim3 {
    uint32_t x, y, z;
    dim3(uint32_t a = 1, uint32_t b = 1, uint32_t c = 1) : x(a), y(b), z(c) {}
};
struct EmuIdx {
    uint32_t x;
};
// defined by the program that includes the kernel
extern thread_local EmuIdx threadIdx;
extern EmuIdx blockIdx;
extern uint8_t* emu_lds;          // the block's dynamic LDS (the kernel's `lds` array)
extern std::barrier<>* emu_bar;
extern uint64_t emu_pred[64];
extern uint32_t emu_xch[64];
extern std::mutex emu_mu;

inline uint32_t min(uint32_t a, uint32_t b) { return a < b ? a : b; }
inline void __syncthreads() { emu_bar->arrive_and_wait(); }
inline uint64_t __ballot(bool p) {
    emu_pred[threadIdx.x] = p;
    emu_bar->arrive_and_wait();
    uint64_t m = 0;
    for (int i = 0; i < 64; ++i) m |= (uint64_t)(emu_pred[i] != 0) << i;
    emu_bar->arrive_and_wait();
    return m;
}
inline bool __any(bool p) { return __ballot(p) != 0; }
inline uint32_t __shfl_xor(uint32_t v, int o, int) {
    emu_xch[threadIdx.x] = v;
    emu_bar->arrive_and_wait();
    const uint32_t r = emu_xch[threadIdx.x ^ o];
    emu_bar->arrive_and_wait();
    return r;
}
inline uint32_t atomicMin(uint32_t* p, uint32_t v) {
    std::lock_guard<std::mutex> lk(emu_mu);
    const uint32_t o = *p;
    if (v < o) *p = v;
    return o;
}
#define __popcll __builtin_popcountll
// v_alignbit_b32: the low dword of {hi, lo} >> (sh & 31)
inline uint32_t emu_alignbit(uint32_t hi, uint32_t lo, uint32_t sh) {
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (sh & 31));
}
#define __builtin_amdgcn_alignbit emu_alignbit

template <class K, class A>
void hipLaunchKernelGGL(K kern, dim3 grid, dim3 block, size_t lds, hipStream_t, A args) {
    for (uint32_t b = 0; b < grid.x; ++b) {
        blockIdx.x = b;
        emu_lds = static_cast<uint8_t*>(malloc(lds ? lds : 1));
        std::barrier<> bar(block.x);
        emu_bar = &bar;
        std::vector<std::thread> th;
        for (uint32_t t = 0; t < block.x; ++t)
            th.emplace_back([=] {
                threadIdx.x = t;
                kern(args);
            });
        for (auto& x : th) x.join();
        free(emu_lds);
    }
}
