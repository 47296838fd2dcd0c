// qf_wire.hip -- wire framing on the device (encoder.rs:18-152), the step on
// either side of the codec kernels.
//
//   k_frame_batch   encode batch -> frames: source i "0x01 | payload",
//                   repair j "0x00 | k (BE u16) | C[j][0..k) | payload"
//   k_parse_frames  received frames -> decode-batch rows / row_index / n_rows
//   k_frame_rows          rows with index and vector -> frames in payload-aligned
//                         slots (any coefficient vector)
//   k_parse_frames_coded  frames at an offset in their slots -> rows / row_index /
//                         n_rows / row_coeffs / row_len, any coefficient vector
//   k_parse_frame_headers the same decisions from the headers alone: row_off /
//                         row_len instead of copied rows
//
// Payloads sit at byte offset 1 or 3 + k inside a frame, so the copy loops
// move 16-byte blocks assembled from aligned dwords with v_alignbit (one
// block per lane); the header bytes and the ragged tail go byte by byte.
// The loads, the header decision, the coefficient-vector block and the
// compaction prefix of the parsers are qf_wire_dev.h's, shared with
// k_poll_headers (qf_poll.hip); the argument structs are qf_kernels.h's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qf_fec.h"
#include "qf_kernels.h"
#include "qf_wire_dev.h"

namespace qf {

namespace {

QF_DEV uint8_t cauchy_coeff(const uint8_t* sexp, const uint8_t* slog, uint32_t i, uint32_t k, uint32_t j) {
    const uint32_t d = (i & 0xFF) ^ ((k + j) & 0xFF);  // decoder.rs:280-298 (k + r <= 256: d != 0)
    return sexp[255 - slog[d]];
}

// one lane per 16-byte block of a frame (frames are frame_stride apart)
__global__ void __launch_bounds__(256) k_frame_batch(FrameArgs a) {
    __shared__ uint8_t sexp[512];
    __shared__ uint8_t slog[256];
    for (uint32_t i = threadIdx.x; i < 768; i += blockDim.x) {
        if (i < 512) sexp[i] = a.explog[i];
        else slog[i - 512] = a.explog[i];
    }
    __syncthreads();
    const uint32_t n = a.k + a.r;
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < a.total_blocks;
         b += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t f = b / a.blocks_per_frame;
        const uint32_t blk = (uint32_t)(b - f * a.blocks_per_frame);
        const uint64_t g = f / n;
        const uint32_t i = (uint32_t)(f - g * n);
        const bool sys = i < a.k;
        const uint32_t j = sys ? 0 : i - a.k;
        const uint32_t off = sys ? 1 : 3 + a.k;  // payload offset in the frame
        const uint32_t flen = off + a.L;
        const uint8_t* pay = sys ? a.src + g * a.src_gen_stride + (uint64_t)i * a.src_row_stride
                                 : a.rep + g * a.rep_gen_stride + (uint64_t)j * a.rep_row_stride;
        uint8_t* fr = a.frames + f * a.frame_stride;
        const uint32_t t0 = blk * 16;
        if (t0 >= flen) continue;
        if (blk == 0 && a.frame_len) a.frame_len[f] = flen;
        if (t0 >= off && t0 + 20 <= flen) {
            uint4 v;
            v.x = load_u32_unaligned(pay, t0 - off);
            v.y = load_u32_unaligned(pay, t0 - off + 4);
            v.z = load_u32_unaligned(pay, t0 - off + 8);
            v.w = load_u32_unaligned(pay, t0 - off + 12);
            *reinterpret_cast<uint4*>(fr + t0) = v;
        } else {
            for (uint32_t t = t0; t < t0 + 16 && t < flen; ++t) {
                uint8_t v;
                if (t >= off) v = pay[t - off];
                else if (t == 0) v = sys ? 1 : 0;
                else if (t == 1) v = (uint8_t)(a.k >> 8);
                else if (t == 2) v = (uint8_t)(a.k & 0xFF);
                else v = cauchy_coeff(sexp, slog, t - 3, a.k, j);
                fr[t] = v;
            }
        }
    }
}

// one 256-thread block per generation
__global__ void __launch_bounds__(256) k_parse_frames(ParseArgs a) {
    __shared__ uint8_t sexp[512];
    __shared__ uint8_t slog[256];
    __shared__ uint32_t slot_of[1024];   // frame -> output slot (or ~0)
    __shared__ uint32_t off_of[1024];    // payload offset of the frame
    __shared__ uint32_t len_of[1024];    // payload length
    __shared__ uint32_t wave_cnt[4];
    const uint32_t g = blockIdx.x;
    for (uint32_t i = threadIdx.x; i < 768; i += blockDim.x) {
        if (i < 512) sexp[i] = a.explog[i];
        else slog[i - 512] = a.explog[i];
    }
    __syncthreads();
    const uint32_t nf = a.n_frames ? min(a.n_frames[g], a.max_rows) : a.max_rows;
    uint32_t base = 0;
    for (uint32_t s0 = 0; s0 < nf; s0 += blockDim.x) {
        const uint32_t s = s0 + threadIdx.x;
        int32_t st = QF_OK;
        uint32_t idx = 0xFFFF, off = 0, plen = 0;
        if (s < nf) {
            const uint64_t fi = (uint64_t)g * a.max_rows + s;
            const uint8_t* fr = a.frames + fi * a.frame_stride;
            const uint32_t flen = a.frame_len[fi];
            if (flen == 0 || flen > a.frame_stride) {
                st = QF_EINVAL;  // "Raw data is empty"
            } else if (fr[0] == 1) {
                off = 1;
                idx = (uint32_t)(a.ids[fi] % a.k);  // decoder.rs:684
            } else if (flen < 3) {
                st = QF_ETOOSMALL;  // coefficient length missing (encoder.rs:33-38)
            } else {
                const uint32_t cl = ((uint32_t)fr[1] << 8) | fr[2];
                if (flen < 3 + cl) st = QF_ETOOSMALL;  // coefficients truncated
                else if (cl != a.k) st = QF_ERANGE;
                else {
                    // the coefficient vector must be Cauchy row j < r: c_0 = inv(k + j)
                    const uint32_t c0 = fr[3];
                    uint32_t j = 0xFFFF;
                    if (c0) j = ((uint32_t)sexp[255 - slog[c0]] - a.k) & 0xFF;
                    if (j >= a.r) st = QF_ERANGE;
                    else {
                        for (uint32_t i = 1; i < a.k && st == QF_OK; ++i)
                            if (fr[3 + i] != cauchy_coeff(sexp, slog, i, a.k, j)) st = QF_ERANGE;
                    }
                    off = 3 + cl;
                    idx = a.k + j;
                }
            }
            if (st == QF_OK) {
                plen = flen - off;
                if (plen > a.L) st = QF_EINVAL;
            }
            a.frame_status[fi] = st;
        }
        const bool ok = s < nf && st == QF_OK;
        uint32_t total;
        const uint32_t slot = base + block_prefix4(ok, wave_cnt, total);
        if (s < nf && s < 1024) {
            slot_of[s] = ok ? slot : 0xFFFFFFFFu;
            off_of[s] = off;
            len_of[s] = plen;
        }
        if (ok) a.row_index[(uint64_t)g * a.max_rows + slot] = (uint16_t)idx;
        base += total;
        __syncthreads();
    }
    if (threadIdx.x == 0 && a.n_rows) a.n_rows[g] = base;
    __syncthreads();
    // payload copy: 16-byte blocks of every accepted row, zero beyond the payload
    const uint32_t bpr = (a.L + 15) / 16;
    const uint32_t nwork = min(nf, 1024u) * bpr;
    for (uint32_t w = threadIdx.x; w < nwork; w += blockDim.x) {
        const uint32_t s = w / bpr, blk = w - s * bpr;
        const uint32_t slot = slot_of[s];
        if (slot == 0xFFFFFFFFu) continue;
        const uint64_t fi = (uint64_t)g * a.max_rows + s;
        const uint8_t* src = a.frames + fi * a.frame_stride + off_of[s];
        uint8_t* dst = a.rows + g * a.rows_gen_stride + (uint64_t)slot * a.row_stride;
        const uint32_t t0 = blk * 16, plen = len_of[s];
        if (t0 + 20 <= plen) {
            const uint64_t o = (uint64_t)(src - a.frames);
            uint4 v;
            v.x = load_u32_unaligned(a.frames, o + t0);
            v.y = load_u32_unaligned(a.frames, o + t0 + 4);
            v.z = load_u32_unaligned(a.frames, o + t0 + 8);
            v.w = load_u32_unaligned(a.frames, o + t0 + 12);
            *reinterpret_cast<uint4*>(dst + t0) = v;
        } else {
            for (uint32_t t = t0; t < t0 + 16 && t < a.L; ++t) dst[t] = t < plen ? src[t] : 0;
        }
    }
}

// ---------------------------------------------------------------------------
// Coded rows that carry their coefficient vectors (relay and receiver of
// recoded traffic).  Payload-aligned slots: the payload of every frame sits at
// byte P = round_up(3 + k, 16) of its slot and the frame's header directly in
// front of it, so payload copies are aligned 16-byte loads and stores.
// ---------------------------------------------------------------------------

// one lane per 16-byte block of a slot: blocks [0, P/16) hold the header,
// the blocks behind them the payload (copy mode only)
__global__ void __launch_bounds__(256) k_frame_rows(FrameRowsArgs a) {
    __shared__ uint8_t sexp[512];
    __shared__ uint8_t slog[256];
    if (!a.row_coeffs) {
        for (uint32_t i = threadIdx.x; i < 768; i += blockDim.x) {
            if (i < 512) sexp[i] = a.explog[i];
            else slog[i - 512] = a.explog[i];
        }
    }
    __syncthreads();
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < a.total_blocks;
         b += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t f = b / a.blocks_per_frame;
        const uint32_t blk = (uint32_t)(b - f * a.blocks_per_frame);
        const uint64_t g = f / a.max_rows;
        const uint32_t s = (uint32_t)(f - g * a.max_rows);
        const uint32_t n = a.n_rows ? min(a.n_rows[g], a.max_rows) : a.max_rows;
        const uint32_t idx = a.row_index ? a.row_index[f] : a.k;
        const uint32_t rlen = a.row_len ? a.row_len[f] : a.L;
        const bool sys = idx < a.k;
        const bool valid = s < n && rlen <= a.L && (sys || a.row_coeffs || idx - a.k < a.r);
        const uint32_t foff = sys ? a.P - 1 : a.P - 3 - a.k;
        if (blk == 0) {
            a.frame_len[f] = valid ? a.P - foff + rlen : 0;
            if (a.frame_off) a.frame_off[f] = valid ? foff : 0;
        }
        if (!valid) continue;
        uint8_t* slot = a.frames + f * a.frame_stride;
        const uint32_t t0 = blk * 16;
        if (blk >= a.hdr_blocks) {
            // payload block: both sides 16-byte aligned
            const uint32_t p0 = t0 - a.P;
            if (p0 >= rlen) continue;
            const uint8_t* row = a.rows + g * a.rows_gen_stride + (uint64_t)s * a.row_stride;
            if (p0 + 16 <= rlen) {
                *reinterpret_cast<uint4*>(slot + t0) = *reinterpret_cast<const uint4*>(row + p0);
            } else {
                for (uint32_t t = p0; t < rlen; ++t) slot[a.P + t] = row[t];
            }
            continue;
        }
        if (t0 + 16 <= foff) continue;   // in front of the frame
        if (sys) {
            slot[foff] = 1;
            continue;
        }
        // header of a coded frame: 0x00 | k (BE u16) | vector
        const uint32_t v0 = foff + 3;    // slot byte of the vector
        const uint8_t* vec = a.row_coeffs ? a.row_coeffs + f * a.k : nullptr;
        if (vec && t0 >= v0 && ((uintptr_t)(vec + (t0 - v0)) & 15) == 0) {
            // P - v0 = k: the block ends inside the vector; 16 aligned bytes of it
            *reinterpret_cast<uint4*>(slot + t0) = *reinterpret_cast<const uint4*>(vec + (t0 - v0));
            continue;
        }
        for (uint32_t t = max(t0, foff); t < t0 + 16; ++t) {
            const uint32_t h = t - foff;
            uint8_t v;
            if (h == 0) v = 0;
            else if (h == 1) v = (uint8_t)(a.k >> 8);
            else if (h == 2) v = (uint8_t)(a.k & 0xFF);
            else v = vec ? vec[h - 3] : cauchy_coeff(sexp, slog, h - 3, a.k, idx - a.k);
            slot[t] = v;
        }
    }
}

// one 256-thread block per generation; k_parse_frames with any coefficient
// vector accepted and written out, and frames at an offset inside their slots
__global__ void __launch_bounds__(256) k_parse_frames_coded(ParseCodedArgs a) {
    __shared__ uint32_t slot_of[1024];   // frame -> output slot (or ~0)
    __shared__ uint32_t pay_of[1024];    // payload start, from the slot's first byte
    __shared__ uint32_t len_of[1024];    // payload length
    __shared__ uint16_t idx_of[1024];    // column of a systematic frame, k for a coded one
    __shared__ uint32_t wave_cnt[4];
    const uint32_t g = blockIdx.x;
    const uint32_t nf = a.n_frames ? min(a.n_frames[g], a.max_rows) : a.max_rows;
    uint32_t base = 0;
    for (uint32_t s0 = 0; s0 < nf; s0 += blockDim.x) {
        const uint32_t s = s0 + threadIdx.x;
        FrameHead h{QF_OK, 0xFFFF, 0, 0};
        if (s < nf) {
            const uint64_t fi = (uint64_t)g * a.max_rows + s;
            h = frame_head(a.frames + fi * a.frame_stride, a.frame_len[fi], a.frame_off ? a.frame_off[fi] : 0,
                           a.frame_stride, a.ids + fi, a.k, a.L, false);
            a.frame_status[fi] = h.st;
        }
        const bool ok = s < nf && h.st == QF_OK;
        uint32_t total;
        const uint32_t slot = base + block_prefix4(ok, wave_cnt, total);
        if (s < nf) {   // nf <= max_rows <= 1024
            slot_of[s] = ok ? slot : 0xFFFFFFFFu;
            pay_of[s] = h.pay;
            len_of[s] = h.plen;
            idx_of[s] = (uint16_t)h.idx;
        }
        if (ok) {
            const uint64_t o = (uint64_t)g * a.max_rows + slot;
            a.row_index[o] = (uint16_t)h.idx;
            if (a.row_len) a.row_len[o] = h.plen;
        }
        base += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) a.n_rows[g] = base;
    __syncthreads();
    // 16-byte blocks of every accepted row: the payload, zero beyond it, then
    // the coefficient vector (the unit vector of a systematic frame)
    const uint32_t bpr = (a.L + 15) / 16, cpr = (a.k + 15) / 16, upr = bpr + cpr;
    const uint32_t nwork = nf * upr;
    for (uint32_t w = threadIdx.x; w < nwork; w += blockDim.x) {
        const uint32_t s = w / upr, u = w - s * upr;
        const uint32_t slot = slot_of[s];
        if (slot == 0xFFFFFFFFu) continue;
        const uint64_t fi = (uint64_t)g * a.max_rows + s;
        const uint8_t* fslot = a.frames + fi * a.frame_stride;
        const uint32_t pay = pay_of[s], plen = len_of[s];
        if (u < bpr) {
            uint8_t* dst = a.rows + g * a.rows_gen_stride + (uint64_t)slot * a.row_stride;
            const uint32_t t0 = u * 16;
            if (t0 + 16 <= plen && can_copy16(pay + t0, pay + plen)) {
                *reinterpret_cast<uint4*>(dst + t0) = load16(fslot, pay + t0);
            } else if (t0 >= plen && t0 + 16 <= a.L) {
                *reinterpret_cast<uint4*>(dst + t0) = make_uint4(0, 0, 0, 0);
            } else {
                for (uint32_t t = t0; t < t0 + 16 && t < a.L; ++t) dst[t] = t < plen ? fslot[pay + t] : 0;
            }
            continue;
        }
        const uint32_t c0 = (u - bpr) * 16;
        uint8_t* cd = a.row_coeffs + ((uint64_t)g * a.max_rows + slot) * a.k;
        const uint32_t idx = idx_of[s];
        // the payload behind the vector is this kernel's to read as well
        const bool wide = wide_block(cd, c0, a.k);
        if (idx < a.k) unit_block(cd, c0, a.k, idx, wide);   // (vector_block, written out: see there)
        else vector_copy_block(cd, c0, a.k, fslot, pay, pay + plen, wide);
    }
}

// one 256-thread block per generation; the decisions of k_parse_frames_coded,
// the payloads left where they are: an accepted row is (row_off, row_len) into
// the generation's frame region, and must start at a multiple of 16 in its
// slot.  Reads the 3 header bytes and the k vector bytes of a frame only.
__global__ void __launch_bounds__(256) k_parse_frame_headers(ParseHeadersArgs a) {
    __shared__ uint32_t slot_of[1024];   // frame -> output slot (or ~0)
    __shared__ uint32_t pay_of[1024];    // payload start, from the slot's first byte
    __shared__ uint16_t idx_of[1024];    // column of a systematic frame, k for a coded one
    __shared__ uint32_t wave_cnt[4];
    const uint32_t g = blockIdx.x;
    const uint32_t nf = a.n_frames ? min(a.n_frames[g], a.max_rows) : a.max_rows;
    uint32_t base = 0;
    for (uint32_t s0 = 0; s0 < nf; s0 += blockDim.x) {
        const uint32_t s = s0 + threadIdx.x;
        FrameHead h{QF_OK, 0xFFFF, 0, 0};
        if (s < nf) {
            const uint64_t fi = (uint64_t)g * a.max_rows + s;
            h = frame_head(a.frames + fi * a.frame_stride, a.frame_len[fi], a.frame_off ? a.frame_off[fi] : 0,
                           a.frame_stride, a.ids + fi, a.k, a.L, true);
            a.frame_status[fi] = h.st;
        }
        const bool ok = s < nf && h.st == QF_OK;
        uint32_t total;
        const uint32_t slot = base + block_prefix4(ok, wave_cnt, total);
        if (s < nf) {   // nf <= max_rows <= 1024
            slot_of[s] = ok ? slot : 0xFFFFFFFFu;
            pay_of[s] = h.pay;
            idx_of[s] = (uint16_t)h.idx;
        }
        if (ok) {
            const uint64_t o = (uint64_t)g * a.max_rows + slot;
            a.row_index[o] = (uint16_t)h.idx;
            a.row_len[o] = h.plen;
            a.row_off[o] = (uint32_t)(s * a.frame_stride) + h.pay;   // max_rows * frame_stride <= 2^32
        }
        base += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) a.n_rows[g] = base;
    __syncthreads();
    // 16-byte blocks of every accepted row's coefficient vector (the unit
    // vector of a systematic frame)
    const uint32_t cpr = (a.k + 15) / 16;
    const uint32_t nwork = nf * cpr;
    for (uint32_t w = threadIdx.x; w < nwork; w += blockDim.x) {
        const uint32_t s = w / cpr, u = w - s * cpr;
        const uint32_t slot = slot_of[s];
        if (slot == 0xFFFFFFFFu) continue;
        const uint64_t fi = (uint64_t)g * a.max_rows + s;
        const uint8_t* fslot = a.frames + fi * a.frame_stride;
        const uint32_t pay = pay_of[s];
        // the readable bytes end with the vector (no payload byte is touched)
        vector_block(a.row_coeffs + ((uint64_t)g * a.max_rows + slot) * a.k, u * 16, a.k, idx_of[s], fslot, pay, pay);
    }
}

}  // namespace

hipError_t launch_parse_frame_headers(const ParseHeadersArgs& a, uint32_t G, hipStream_t st) {
    if (G == 0) return hipSuccess;
    hipLaunchKernelGGL(k_parse_frame_headers, dim3(G), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_frame_rows(const FrameRowsArgs& args, uint32_t G, int num_cus, hipStream_t st) {
    FrameRowsArgs a = args;
    a.P = qf_frame_payload_offset(a.k);
    a.hdr_blocks = a.P / 16;
    // rows == NULL selects in-place mode: qf_frame_rows_dev passes NULL for QF_FRAME_IN_PLACE and
    // refuses a NULL rows in copy mode
    a.blocks_per_frame = a.hdr_blocks + (a.rows ? (a.L + 15) / 16 : 0);
    a.total_blocks = (uint64_t)G * a.max_rows * a.blocks_per_frame;
    if (a.total_blocks == 0) return hipSuccess;
    uint64_t blocks = (a.total_blocks + 255) / 256;
    const uint64_t cap = (uint64_t)num_cus * 8;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(k_frame_rows, dim3((uint32_t)blocks), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_parse_frames_coded(const ParseCodedArgs& a, uint32_t G, hipStream_t st) {
    if (G == 0) return hipSuccess;
    hipLaunchKernelGGL(k_parse_frames_coded, dim3(G), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_frame_batch(const FrameArgs& args, uint32_t G, int num_cus, hipStream_t st) {
    FrameArgs a = args;
    a.blocks_per_frame = (uint32_t)((3 + a.k + a.L + 15) / 16);
    a.total_blocks = (uint64_t)G * (a.k + a.r) * a.blocks_per_frame;
    if (a.total_blocks == 0) return hipSuccess;
    uint64_t blocks = (a.total_blocks + 255) / 256;
    const uint64_t cap = (uint64_t)num_cus * 8;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(k_frame_batch, dim3((uint32_t)blocks), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_parse_frames(const ParseArgs& a, uint32_t G, hipStream_t st) {
    if (G == 0) return hipSuccess;
    hipLaunchKernelGGL(k_parse_frames, dim3(G), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace qf
