// qf_gf_dev.h -- device helpers shared by the .hip files.  For all of them:
// QF_DEV (the one definition) and the unit loads and stores, among them the
// masked row-unit load of qf_relay.hip and qf_store.hip.  For the v_perm
// payload kernels of qf_kernels.hip (k_combine_uniform, k_combine_slots, ...)
// and qf_relay.hip (k_combine_rows_at): the split-table multiply-add of
// gf256_tables.h, the asm streaming load and the wave maximum.  Everything
// here is inline device code: a file that uses none of it emits none of it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qf {

#define QF_DEV __device__ __forceinline__

QF_DEV uint32_t vperm(uint32_t hi, uint32_t lo, uint32_t sel) {
    return __builtin_amdgcn_perm(hi, lo, sel);
}
QF_DEV uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}

QF_DEV uint32_t comp(const uint4& v, int c) {
    return c == 0 ? v.x : (c == 1 ? v.y : (c == 2 ? v.z : v.w));
}
QF_DEV void set_comp(uint4& v, int c, uint32_t x) {
    if (c == 0) v.x = x;
    else if (c == 1) v.y = x;
    else if (c == 2) v.z = x;
    else v.w = x;
}

// Load 16 bytes (nb valid, the rest zero).  nb == 16 is the fast path.
QF_DEV uint4 load_unit(const uint8_t* p, uint32_t nb) {
    if (nb >= 16) return *reinterpret_cast<const uint4*>(p);
    uint4 r = make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int b = 0; b < 16; ++b) {
        if ((uint32_t)b < nb) {
            uint32_t w = comp(r, b >> 2) | ((uint32_t)p[b] << (8 * (b & 3)));
            set_comp(r, b >> 2, w);
        }
    }
    return r;
}

QF_DEV uint32_t low_bytes_mask(uint32_t nb) { return nb >= 4 ? 0xFFFFFFFFu : (1u << (8 * nb)) - 1; }

// The unit at p of a row of len bytes, u16 = 16 * unit index: the bytes of the
// unit at and after len are zero, and a unit without a valid byte is not loaded.
QF_DEV uint4 load_row_unit(const uint8_t* p, uint32_t len, uint32_t u16) {
    uint4 x = make_uint4(0, 0, 0, 0);
    if (len > u16) {
        x = *reinterpret_cast<const uint4*>(p);
        const uint32_t v = len - u16;
        if (v < 16) {
            x.x &= low_bytes_mask(v);
            x.y &= low_bytes_mask(v > 4 ? v - 4 : 0);
            x.z &= low_bytes_mask(v > 8 ? v - 8 : 0);
            x.w &= low_bytes_mask(v > 12 ? v - 12 : 0);
        }
    }
    return x;
}

QF_DEV void store_unit(uint8_t* p, const uint4& v, uint32_t nb) {
    if (nb >= 16) {
        *reinterpret_cast<uint4*>(p) = v;
        return;
    }
#pragma unroll
    for (int b = 0; b < 16; ++b)
        if ((uint32_t)b < nb) p[b] = (uint8_t)(comp(v, b >> 2) >> (8 * (b & 3)));
}

// ---------------------------------------------------------------------------
// Explicitly pipelined streaming loads.  hipcc sinks loop-carried loads down
// to their first use (exposing the whole HBM latency per step), so the hot
// loops issue global_load_dwordx4 through inline asm and wait with a counted
// s_waitcnt vmcnt(N) whose asm operands are the destination registers: the
// data dependency orders every use after the wait, and hipcc's own counters
// never see these loads (the loops contain no other vector-memory ops).
// ---------------------------------------------------------------------------
typedef uint32_t v4u __attribute__((ext_vector_type(4)));

QF_DEV void aload16(v4u& r, const uint8_t* p) {
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(r) : "v"(p) : "memory");
}

QF_DEV uint4 to_u4(const v4u& v) { return make_uint4(v.x, v.y, v.z, v.w); }

struct Sel {
    uint4 s0, s1, s2;
};
QF_DEV Sel selectors(const uint4& x) {
    Sel s;
    s.s0 = make_uint4(x.x & 0x07070707u, x.y & 0x07070707u, x.z & 0x07070707u, x.w & 0x07070707u);
    s.s1 = make_uint4((x.x >> 3) & 0x07070707u, (x.y >> 3) & 0x07070707u,
                      (x.z >> 3) & 0x07070707u, (x.w >> 3) & 0x07070707u);
    s.s2 = make_uint4((x.x >> 6) & 0x03030303u, (x.y >> 6) & 0x03030303u,
                      (x.z >> 6) & 0x03030303u, (x.w >> 6) & 0x03030303u);
    return s;
}

// acc ^= ca * xa ^ cb * xb  for the four dwords of one unit.
// A = {T0lo,T0hi,T1lo,T1hi} of ca, a2 = T2 of ca; same for cb.
QF_DEV void fma_pair(uint4& acc, const uint4& A, uint32_t a2, const Sel& sa, const uint4& B,
                     uint32_t b2, const Sel& sb) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        uint32_t t = comp(acc, c);
        t = xor3(t, vperm(A.y, A.x, comp(sa.s0, c)), vperm(A.w, A.z, comp(sa.s1, c)));
        t = xor3(t, vperm(a2, a2, comp(sa.s2, c)), vperm(B.y, B.x, comp(sb.s0, c)));
        t = xor3(t, vperm(B.w, B.z, comp(sb.s1, c)), vperm(b2, b2, comp(sb.s2, c)));
        set_comp(acc, c, t);
    }
}

QF_DEV uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        uint32_t o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return __builtin_amdgcn_readfirstlane(v);
}

// Two slots of a payload pass over 16-byte coefficient records: acc[j] ^=
// ca[j] * xa ^ cb[j] * xb, the split tables of a coefficient value read from
// the 256 records in LDS.
template <int R>
QF_DEV void fma_rows_slots(uint4 (&acc)[R], const uint32_t* __restrict__ tab256, const uint4& xa,
                           const uint4& xb, const uint4& ca, const uint4& cb) {
    const Sel sa = selectors(xa), sb = selectors(xb);
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const uint32_t wa = comp(ca, j >> 2), wb = comp(cb, j >> 2);
        // record address = coefficient * 32 bytes
        const uint32_t oa = ((wa >> (8 * (j & 3))) & 0xFF) << 5;
        const uint32_t ob = ((wb >> (8 * (j & 3))) & 0xFF) << 5;
        const uint8_t* base = reinterpret_cast<const uint8_t*>(tab256);
        const uint4 A = *reinterpret_cast<const uint4*>(base + oa);
        const uint32_t a2 = *reinterpret_cast<const uint32_t*>(base + oa + 16);
        const uint4 B = *reinterpret_cast<const uint4*>(base + ob);
        const uint32_t b2 = *reinterpret_cast<const uint32_t*>(base + ob + 16);
        fma_pair(acc[j], A, a2, sa, B, b2, sb);
    }
}

}  // namespace qf
