// What k_deliver_prepare and k_deliver_rows use beyond hip/hip_runtime.h beside
// this file -- TEST INFRASTRUCTURE ONLY (tests/test_deliver_kernel_emu_cpu.py).
#pragma once
#include <hip/hip_runtime.h>

// an LDS counter: the lanes of the block are host threads
inline uint32_t atomicAdd(uint32_t* p, uint32_t v) {
    std::lock_guard<std::mutex> lk(emu_mu);
    const uint32_t o = *p;
    *p = o + v;
    return o;
}
// v_readfirstlane_b32 of a value that is the same in every lane of the wave
inline uint32_t emu_readfirstlane(uint32_t v) { return v; }
#define __builtin_amdgcn_readfirstlane emu_readfirstlane
