// qf_partial.hip -- the control kernel of qf_decode_partial_frames_dev
// (DESIGN.md 3.18): what the rows a generation holds determine, whether or not
// they reach rank k.
//
//  k_partial_prepare  k_decode_prepare<true> (qf_kernels.hip) with the square
//                     solve replaced by a reduced row echelon form.  One wave
//                     per generation.  A = the slots k_rank_filter flagged, S
//                     the sources with a systematic slot in A, E the other
//                     sources (ascending), c the coded slots of A.  The wave
//                     builds M = [A_E | A_S | I_c] (c rows, k + c columns) in
//                     LDS and reduces A_E scanning the columns left to right;
//                     a column with no pivot among the unused rows is free and
//                     is skipped (the square solve's QF_ERANK).  A row that is
//                     zero at every free column then reads
//                       x_pivot = (row of A_S) x_S + (row of I_c) y
//                     with y the coded rows' payloads: its pivot's source is
//                     determined.  The pivots go left to right and the rows
//                     are swapped into place, so the determined rows come out
//                     in ascending source order; a ballot prefix compacts them.
//                     The payload pass is k_combine_rows_at, unchanged: this
//                     kernel writes its pair records (qf_kernels.h,
//                     PrepareArgs), but only for the slots of A with a nonzero
//                     coefficient in some determined row.  At rank k no column
//                     is free, the operations are the square solve's, and every
//                     output equals qf_decode_frames_dev's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qf_kernels.h"

#define QF_DEV __device__ __forceinline__

namespace qf {

namespace {

struct PartLds {
    uint8_t* exp;        // 512
    uint8_t* log;        // 256
    uint32_t* first;     // 256: first flagged slot of systematic index
    uint16_t* sys_slot;  // 256: accepted slot of systematic i (0xFFFF none)
    uint16_t* col;       // 256: matrix column of source i
    uint16_t* rep_slot;  // 256: slot of coded row m
    uint16_t* emap;      // 256: the unknown sources E, ascending
    uint16_t* lf;        // 256: log of elimination factors (0xFFFF = zero)
    uint16_t* pivcol;    // 128: pivot column of row m
    uint16_t* drow;      // 128: matrix row of determined source d
    uint8_t* free_col;   // 256: 1 = column of A_E without a pivot
    uint16_t* slot_col;  // max_rows_pad: column of slot (0xFFFF = not in A)
    uint8_t* M;          // e_lds x (k + e_lds)
};

constexpr uint32_t kPartFixedLds = 768 + 4 * 256 + 2 * 256 * 5 + 2 * 128 * 2 + 256;

QF_DEV uint8_t pmul(const PartLds& L, uint32_t a, uint32_t b) {
    if (a == 0 || b == 0) return 0;
    return L.exp[(uint32_t)L.log[a] + (uint32_t)L.log[b]];
}

__global__ void __launch_bounds__(64) k_partial_prepare(PrepareArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const uint32_t g = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const uint32_t k = a.k, emax = a.e_max;
    PartLds L;
    {
        uint8_t* p = lds;
        L.exp = p; p += 512;
        L.log = p; p += 256;
        L.first = reinterpret_cast<uint32_t*>(p); p += 4 * 256;
        L.sys_slot = reinterpret_cast<uint16_t*>(p); p += 2 * 256;
        L.col = reinterpret_cast<uint16_t*>(p); p += 2 * 256;
        L.rep_slot = reinterpret_cast<uint16_t*>(p); p += 2 * 256;
        L.emap = reinterpret_cast<uint16_t*>(p); p += 2 * 256;
        L.lf = reinterpret_cast<uint16_t*>(p); p += 2 * 256;
        L.pivcol = reinterpret_cast<uint16_t*>(p); p += 2 * 128;
        L.drow = reinterpret_cast<uint16_t*>(p); p += 2 * 128;
        L.free_col = p; p += 256;
        L.slot_col = reinterpret_cast<uint16_t*>(p); p += 2 * a.max_rows_pad;
        L.M = p;
    }
    for (uint32_t i = lane; i < 768; i += 64) lds[i] = a.explog[i];
    for (uint32_t i = lane; i < 256; i += 64) {
        L.first[i] = 0xFFFFFFFFu;
        L.sys_slot[i] = 0xFFFF;
        L.free_col[i] = 1;
    }
    __syncthreads();
    const uint32_t n = a.n_rows ? min(a.n_rows[g], a.max_rows) : a.max_rows;
    const uint16_t* ridx = a.row_index + (uint64_t)g * a.max_rows;
    const uint8_t* acpt = a.accept + (uint64_t)g * a.max_rows;   // k_rank_filter's flags: the set A
    const uint32_t* ro = a.row_off + (uint64_t)g * a.max_rows;
    const uint32_t* rl = a.row_len + (uint64_t)g * a.max_rows;
    // the index and row rules of k_decode_prepare<true>, over every slot
    bool bad = false;
    for (uint32_t s = lane; s < n; s += 64) {
        const uint32_t idx = ridx[s];
        if (idx < k) {
            if (acpt[s]) atomicMin(&L.first[idx], s);
        } else if (idx - k >= a.rep_limit) bad = true;
        const uint32_t off = ro[s], len = rl[s];
        if (len > a.L || (off & 15) || (uint64_t)off + len > a.src_gen_stride) bad = true;
    }
    for (uint32_t s = lane; s < a.max_rows; s += 64) L.slot_col[s] = 0xFFFF;
    __syncthreads();
    int32_t status = __any(bad) ? -1 : 0;  // QF_EINVAL
    // The slots of A in arrival order (at most k: A is independent).
    uint32_t accepted = 0, nrep = 0, bound = 0;
    const uint64_t lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    for (uint32_t s0 = 0; s0 < n && accepted < k; s0 += 64) {
        const uint32_t s = s0 + lane;
        uint32_t idx = 0;
        bool cand = false;
        if (s < n && acpt[s]) {
            idx = ridx[s];
            cand = idx >= k ? (idx - k < a.rep_limit) : (L.first[idx] == s);
        }
        const uint64_t bc = __ballot(cand);
        const uint32_t pos = accepted + __popcll(bc & lt_mask);
        const bool acc = cand && pos < k;
        const bool isrep = acc && idx >= k;
        const uint64_t br = __ballot(isrep);
        const uint32_t rpos = nrep + __popcll(br & lt_mask);
        if (acc) {
            if (idx < k) L.sys_slot[idx] = (uint16_t)s;
            else if (rpos < 256) L.rep_slot[rpos] = (uint16_t)s;
        }
        const uint64_t ba = __ballot(acc);
        if (ba) bound = s0 + 64 - __builtin_clzll(ba);
        accepted += __popcll(ba);
        nrep += __popcll(br);
    }
    __syncthreads();
    const uint32_t c = nrep;                // coded rows of A
    const uint32_t nE = k - (accepted - c);  // unknown sources
    if (status == 0 && c > a.e_lds) status = -1;  // QF_EINVAL: the matrix rows held in LDS
    const uint32_t W = k + c;
    uint32_t nD = 0;
    if (status == 0 && c > 0) {
        // Unknown list (ascending source index) and column map.
        uint32_t ne = 0, np = 0;
        for (uint32_t i0 = 0; i0 < k; i0 += 64) {
            const uint32_t i = i0 + lane;
            const bool miss = i < k && L.sys_slot[i] == 0xFFFF;
            const bool pres = i < k && !miss;
            const uint64_t bm = __ballot(miss), bp = __ballot(pres);
            if (miss) {
                const uint32_t p = ne + __popcll(bm & lt_mask);
                L.emap[p] = (uint16_t)i;
                L.col[i] = (uint16_t)p;
            }
            if (pres) {
                const uint32_t p = np + __popcll(bp & lt_mask);
                L.col[i] = (uint16_t)(nE + p);
                L.slot_col[L.sys_slot[i]] = (uint16_t)(nE + p);
            }
            ne += __popcll(bm);
            np += __popcll(bp);
        }
        for (uint32_t m = lane; m < c; m += 64) L.slot_col[L.rep_slot[m]] = (uint16_t)(k + m);
        __syncthreads();
        // Build M = [A_E | A_S | I_c].
        bool erange = false;
        for (uint32_t m = 0; m < c; ++m) {
            const uint32_t s = L.rep_slot[m];
            const uint32_t j = ridx[s] - k;
            const uint8_t* rc = a.row_coeffs ? a.row_coeffs + ((uint64_t)g * a.max_rows + s) * k : nullptr;
            const uint32_t y = (k + j) & 0xFF;
            for (uint32_t i = lane; i < k; i += 64) {
                uint8_t v;
                if (rc) v = rc[i];
                else {
                    const uint32_t d = (i & 0xFF) ^ y;
                    if (d == 0) { erange = true; v = 0; }
                    else v = L.exp[255 - L.log[d]];
                }
                L.M[m * W + L.col[i]] = v;
            }
            for (uint32_t q = lane; q < c; q += 64) L.M[m * W + k + q] = (q == m) ? 1 : 0;
        }
        __syncthreads();
        if (__any(erange)) status = -2;  // QF_ERANGE
        // Reduced row echelon form of the first nE columns: rows [0, rr) hold
        // the pivots found so far, a column without one stays free.
        uint32_t rr = 0;
        for (uint32_t cc = 0; cc < nE && rr < c && status == 0; ++cc) {
            int32_t p = -1;
            for (uint32_t r0 = rr; r0 < c; r0 += 64) {
                const uint32_t row = r0 + lane;
                const uint64_t b = __ballot(row < c && L.M[row * W + cc] != 0);
                if (b) { p = (int32_t)(r0 + __builtin_ctzll(b)); break; }
            }
            if (p < 0) continue;   // free column
            if ((uint32_t)p != rr) {
                for (uint32_t col = lane; col < W; col += 64) {
                    const uint8_t t = L.M[rr * W + col];
                    L.M[rr * W + col] = L.M[p * W + col];
                    L.M[p * W + col] = t;
                }
                __syncthreads();
            }
            const uint8_t piv = L.M[rr * W + cc];
            const uint8_t inv = L.exp[255 - L.log[piv]];
            __syncthreads();
            for (uint32_t col = lane; col < W; col += 64) L.M[rr * W + col] = pmul(L, L.M[rr * W + col], inv);
            for (uint32_t m = lane; m < c; m += 64) {
                const uint8_t f = L.M[m * W + cc];
                L.lf[m] = (m == rr || f == 0) ? 0xFFFF : L.log[f];
            }
            if (lane == 0) {
                L.pivcol[rr] = (uint16_t)cc;
                L.free_col[cc] = 0;
            }
            __syncthreads();
            for (uint32_t col = lane; col < W; col += 64) {
                const uint8_t pv = L.M[rr * W + col];
                if (pv == 0) continue;
                const uint32_t lp = L.log[pv];
                for (uint32_t m = 0; m < c; ++m) {
                    const uint32_t lfm = L.lf[m];
                    if (lfm == 0xFFFF) continue;
                    L.M[m * W + col] ^= L.exp[lfm + lp];
                }
            }
            __syncthreads();
            ++rr;
        }
        // Determined rows: zero at every free column.  (c <= 128: two rounds.)
        if (status == 0) {
            for (uint32_t m0 = 0; m0 < rr; m0 += 64) {
                const uint32_t m = m0 + lane;
                bool det = m < rr;
                if (det)
                    for (uint32_t f = 0; f < nE; ++f)
                        if (L.free_col[f] && L.M[m * W + f] != 0) { det = false; break; }
                const uint64_t bd = __ballot(det);
                if (det) L.drow[nD + __popcll(bd & lt_mask)] = (uint16_t)m;
                nD += __popcll(bd);
            }
            __syncthreads();
        }
    }
    if (status == 0 && nD > emax) status = -1;  // QF_EINVAL: capacity min(k, r)
    if (status == 0 && accepted < k) status = -3;  // QF_ENOTREADY: the outputs describe what is known
    const bool known = status == 0 || status == -3;
    if (!known) nD = 0;
    // Pair records (PrepareArgs, qf_kernels.h) over the slots of A that some
    // determined row uses, in arrival order: recorded row t sits in pair t / 2.
    // Rows at and after the recorded count are zero records of length 0 at the
    // last recorded row's offset (0 when none), so that every lane of
    // k_combine_rows_at finds a readable unit.
    const uint32_t nrec = 2 * ((min(k, a.max_rows) + 1) / 2 + 1);
    const uint32_t nb = nD ? bound : 0;
    uint32_t at_bound = 0, last_slot = 0xFFFFFFFFu;
    uint32_t mn = 0xFFFFFFFFu;
    for (uint32_t s0 = 0; s0 < nb; s0 += 64) {
        const uint32_t s = s0 + lane;
        const uint32_t cl = s < nb ? L.slot_col[s] : 0xFFFF;
        bool used = false;
        if (cl != 0xFFFF)
            for (uint32_t d = 0; d < nD; ++d)
                if (L.M[(uint32_t)L.drow[d] * W + cl] != 0) { used = true; break; }
        const uint64_t bu = __ballot(used);
        if (used) {
            const uint32_t t = at_bound + __popcll(bu & lt_mask);
            const uint32_t off = ro[s], len = rl[s];
            mn = min(mn, len);
            for (uint32_t pass = 0; pass < a.passes; ++pass) {
                uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const uint32_t d = pass * 16 + q;
                    const uint32_t v = d < nD ? L.M[(uint32_t)L.drow[d] * W + cl] : 0u;
                    w[q >> 2] |= v << (8 * (q & 3));
                }
                uint8_t* pair = a.coef_out + ((uint64_t)pass * a.G + g) * a.coef_gen_stride +
                                (uint64_t)(t >> 1) * kPairRecBytes;
                reinterpret_cast<uint32_t*>(pair)[t & 1] = off;
                reinterpret_cast<uint32_t*>(pair)[2 + (t & 1)] = len;
                *reinterpret_cast<uint4*>(pair + 16 + (t & 1) * 16) = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
        if (bu) last_slot = s0 + 63 - __builtin_clzll(bu);
        at_bound += __popcll(bu);
    }
    const uint32_t last_off = last_slot != 0xFFFFFFFFu ? ro[last_slot] : 0;
    for (uint32_t t = at_bound + lane; t < nrec; t += 64) {
        for (uint32_t pass = 0; pass < a.passes; ++pass) {
            uint8_t* pair = a.coef_out + ((uint64_t)pass * a.G + g) * a.coef_gen_stride +
                            (uint64_t)(t >> 1) * kPairRecBytes;
            reinterpret_cast<uint32_t*>(pair)[t & 1] = last_off;
            reinterpret_cast<uint32_t*>(pair)[2 + (t & 1)] = 0;
            *reinterpret_cast<uint4*>(pair + 16 + (t & 1) * 16) = make_uint4(0, 0, 0, 0);
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mn = min(mn, (uint32_t)__shfl_xor(mn, o, 64));
    if (a.src_slot)
        for (uint32_t i = lane; i < k; i += 64)
            a.src_slot[(uint64_t)g * k + i] = known ? L.sys_slot[i] : (uint16_t)0xFFFF;
    for (uint32_t d = lane; d < nD; d += 64)
        a.rec_index[(uint64_t)g * emax + d] = L.emap[L.pivcol[L.drow[d]]];
    if (lane == 0) {
        a.min_len[g] = at_bound ? mn : 0;
        a.status[g] = status;
        a.n_out[g] = nD;
        a.bound[g] = at_bound;
    }
}

}  // namespace

size_t partial_prepare_lds_bytes(uint32_t k, uint32_t max_rows) {
    const uint32_t max_rows_pad = (max_rows + 7) & ~7u;
    const uint32_t rows = k < 128 ? k : 128;
    return kPartFixedLds + 2 * (size_t)max_rows_pad + (size_t)rows * (k + rows) + 16;
}

hipError_t launch_partial_prepare(const PrepareArgs& a, hipStream_t st) {
    const size_t lds = partial_prepare_lds_bytes(a.k, a.max_rows);
    static bool attr_done = false;
    if (!attr_done) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_partial_prepare),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
        attr_done = true;
    }
    if (a.G == 0) return hipSuccess;
    // rows by offset, flagged by k_rank_filter; the recorded rows must fit the records
    if (!a.accept || !a.row_off || !a.row_len || !a.min_len || !a.n_out || !a.bound || !a.status ||
        (a.e_max && !a.rec_index) || a.k == 0 || a.k > 256 || a.e_lds != (a.k < 128 ? a.k : 128) ||
        a.max_rows_pad < a.max_rows || (a.src_gen_stride & 15) || (a.coef_gen_stride & 15) ||
        a.coef_gen_stride < ((uint64_t)((a.k < a.max_rows ? a.k : a.max_rows) + 1) / 2 + 1) * kPairRecBytes ||
        lds > 160 * 1024)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_partial_prepare, dim3(a.G), dim3(64), lds, st, a);
    return hipGetLastError();
}

}  // namespace qf
