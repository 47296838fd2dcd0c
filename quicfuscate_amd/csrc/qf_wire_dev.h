// qf_wire_dev.h -- the device pieces that turn a received wire frame into a
// row, shared by the parsers of qf_wire.hip (k_parse_frames,
// k_parse_frames_coded, k_parse_frame_headers) and qf_poll.hip
// (k_poll_headers): the unaligned loads, the header decision, one 16-byte
// block of a row's coefficient vector and the block-wide compaction prefix.
// This is the code that decides which bytes of an untrusted datagram are read
// and where they go, so it exists once.  Everything here is inline device
// code (tests/test_wire_dev_emu_cpu.py compiles it for the host).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qf_fec.h"

// qf_gf_dev.h's definition, repeated here instead of included: that header's
// v_perm helpers and inline assembly do not compile for the host, and this
// one has to (tests/kernel_emu).
#ifndef QF_DEV
#define QF_DEV __device__ __forceinline__
#endif

namespace qf {

// bytes [off, off + 4) of a buffer read through aligned dwords
QF_DEV uint32_t load_u32_unaligned(const uint8_t* base, uint64_t off) {
    const uint64_t a = off & ~3ull;
    const uint32_t sh = (uint32_t)(off & 3) * 8;
    const uint32_t lo = *reinterpret_cast<const uint32_t*>(base + a);
    if (sh == 0) return lo;
    const uint32_t hi = *reinterpret_cast<const uint32_t*>(base + a + 4);
    return __builtin_amdgcn_alignbit(hi, lo, sh);
}

// 16 bytes from slot byte o (any alignment) of a frame whose readable bytes end
// at slot byte `end`: one aligned 16-byte load, else aligned dwords joined with
// v_alignbit (which touch up to 3 bytes past o + 16, hence the 20).  The
// caller has checked can_copy16(o, end).
QF_DEV bool can_copy16(uint32_t o, uint32_t end) {
    return (o & 15) == 0 ? o + 16 <= end : o + 20 <= end;
}

QF_DEV uint4 load16(const uint8_t* slot, uint32_t o) {
    if ((o & 15) == 0) return *reinterpret_cast<const uint4*>(slot + o);
    uint4 v;
    v.x = load_u32_unaligned(slot, o);
    v.y = load_u32_unaligned(slot, o + 4);
    v.z = load_u32_unaligned(slot, o + 8);
    v.w = load_u32_unaligned(slot, o + 12);
    return v;
}

// What a frame's header says: its status, and for QF_OK the column of a
// systematic frame (k for a coded one), the payload's start from the slot's
// first byte and its length.
struct FrameHead {
    int32_t st;
    uint32_t idx, pay, plen;
};

// The header decision for the frame of flen bytes at byte foff of its slot:
// "0x01 | payload" or "0x00 | k (BE u16) | vector | payload".  Reads the frame's
// first byte, and bytes 1 and 2 of a frame of 3 bytes or more that is not
// systematic; *id only for a systematic frame.  pay16: the payload must start
// at a multiple of 16 in its slot to be read in place.
QF_DEV FrameHead frame_head(const uint8_t* slot, uint32_t flen, uint32_t foff, uint64_t frame_stride,
                            const uint64_t* id, uint32_t k, uint32_t L, bool pay16) {
    const uint8_t* fr = slot + foff;   // (read only once the frame is known to lie in its slot)
    int32_t st = QF_OK;
    uint32_t idx = 0xFFFF, pay = 0, plen = 0, off = 0;
    if (flen == 0 || (uint64_t)foff + flen > frame_stride) {
        st = QF_EINVAL;  // "Raw data is empty", or not inside its slot
    } else if (fr[0] == 1) {
        off = 1;
        idx = (uint32_t)(*id % k);  // decoder.rs:684
    } else if (flen < 3) {
        st = QF_ETOOSMALL;  // coefficient length missing (encoder.rs:33-38)
    } else {
        const uint32_t cl = ((uint32_t)fr[1] << 8) | fr[2];
        if (flen < 3 + cl) st = QF_ETOOSMALL;  // coefficients truncated
        else if (cl != k) st = QF_ERANGE;
        off = 3 + cl;
        idx = k;
    }
    if (st == QF_OK) {
        plen = flen - off;
        pay = foff + off;
        // longer than a row, or a payload that cannot be read in place
        if (plen > L || (pay16 && (pay & 15))) st = QF_EINVAL;
    }
    return FrameHead{st, idx, pay, plen};
}

// Bytes [c0, min(c0 + 16, k)) of an accepted row's coefficient vector to cd
// (c0 a multiple of 16), in two halves with vector_block below around them.
// wide: the block is whole and its destination aligned, so one 16-byte store.
QF_DEV bool wide_block(const uint8_t* cd, uint32_t c0, uint32_t k) {
    return c0 + 16 <= k && ((uintptr_t)(cd + c0) & 15) == 0;
}

// The unit vector of column idx < k (a systematic frame).
QF_DEV void unit_block(uint8_t* cd, uint32_t c0, uint32_t k, uint32_t idx, bool wide) {
    if (wide) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (idx >= c0 && idx < c0 + 16) {
            const uint32_t bit = 1u << (8 * (idx & 3));
            const uint32_t q = (idx - c0) >> 2;
            v.x = q == 0 ? bit : 0;
            v.y = q == 1 ? bit : 0;
            v.z = q == 2 ? bit : 0;
            v.w = q == 3 ? bit : 0;
        }
        *reinterpret_cast<uint4*>(cd + c0) = v;
    } else {
        const uint32_t cend = min(c0 + 16, k);
        for (uint32_t t = c0; t < cend; ++t) cd[t] = t == idx ? 1 : 0;
    }
}

// A coded frame's vector, which sits in front of the payload at bytes
// [pay - k, pay) of the slot.  `end` is the slot byte at which the frame's
// readable bytes end (pay, or pay + plen where the payload is read too):
// nothing at or after it is touched.
QF_DEV void vector_copy_block(uint8_t* cd, uint32_t c0, uint32_t k, const uint8_t* fslot, uint32_t pay, uint32_t end,
                              bool wide) {
    const uint32_t v0 = pay - k;
    if (wide && can_copy16(v0 + c0, end)) {
        *reinterpret_cast<uint4*>(cd + c0) = load16(fslot, v0 + c0);
    } else {
        const uint32_t cend = min(c0 + 16, k);
        for (uint32_t t = c0; t < cend; ++t) cd[t] = fslot[v0 + t];
    }
}

// Either half, by the frame's idx (idx < k: systematic).  k_parse_frames_coded
// writes these three lines out at its call instead (measured: DESIGN.md 3.16).
QF_DEV void vector_block(uint8_t* cd, uint32_t c0, uint32_t k, uint32_t idx, const uint8_t* fslot, uint32_t pay,
                         uint32_t end) {
    const bool wide = wide_block(cd, c0, k);
    if (idx < k) unit_block(cd, c0, k, idx, wide);
    else vector_copy_block(cd, c0, k, fslot, pay, end, wide);
}

// The exclusive prefix of `ok` over a 256-thread block (4 waves) and, in
// total, its sum.  wave_cnt: 4 words of LDS.  Every thread of the block calls
// it, and the block meets at a barrier before it calls it again.
QF_DEV uint32_t block_prefix4(bool ok, uint32_t* wave_cnt, uint32_t& total) {
    const uint64_t bal = __ballot(ok);
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t before = __popcll(bal & ((lane == 0) ? 0ull : (~0ull >> (64 - lane))));
    if (lane == 0) wave_cnt[w] = __popcll(bal);
    __syncthreads();
    uint32_t woff = 0;
    for (uint32_t q = 0; q < w; ++q) woff += wave_cnt[q];
    total = 0;
    for (uint32_t q = 0; q < 4; ++q) total += wave_cnt[q];
    return woff + before;
}

}  // namespace qf
