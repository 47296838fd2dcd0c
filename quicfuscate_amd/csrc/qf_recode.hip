// qf_recode.hip -- batched RLNC recoding for relay nodes (qf_recode_batch).
//
// A relay holds n rows of a generation (systematic, Cauchy repairs, or rows
// that carry explicit coefficient vectors) and emits m fresh linear
// combinations of them, each with its coefficient vector over the k sources:
//   out[g][j]        = XOR_s M[j][s] * rows[g][s]
//   out_coeffs[g][j] = XOR_s M[j][s] * v(s)
// The payload product is the decode's payload pass over 16-byte coefficient
// records (combine_payload of qf_api.hip: k_combine_slots, its split variant
// or the bit-sliced qf_combine_bs), ceil(m / 16) passes, so every input row is
// read from HBM once per pass.  New here is the control kernel that builds M,
// the records and the output vectors.
//
//  k_recode_prepare   one wave per generation: index validation and status,
//                     M from mix_dev or the splitmix64 stream of
//                     qf_fill_splitmix_dev, the records [pass][G][max_rows + 1],
//                     n_out = m, bound = n (0 when the status is not QF_OK, so
//                     the payload pass stores zero rows), and out_coeffs.
//                     Systematic slots hang on a per-column list in LDS and
//                     contribute M[j][s] to their column only; the k-wide
//                     products run over the compacted list of coded slots,
//                     lanes over columns, with the slots' vectors and the mix
//                     entries in log form in LDS (exp / log tables of d_explog).
//                     For qf_recode_frames_dev (qf_relay.hip) it also checks
//                     the rows' (offset, length) and writes their descriptors.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <mutex>
#include <string>

#include "qf_fec.h"
#include "qf_kernels.h"
#include "qf_internal.h"

namespace qf {

namespace {
constexpr uint32_t kNone16 = 0xFFFF;      // end of a column's slot list
constexpr uint32_t kLogZero = 255;        // log form of 0 (logs are 0..254)

__host__ __device__ inline uint32_t pad8(uint32_t x) { return (x + 7) & ~7u; }
__host__ __device__ inline uint32_t pad16(uint32_t x) { return (x + 15) & ~15u; }
}  // namespace

// LDS: exp[512] log[256] | head[256] u32 | next[mrp] u16 | cslot[mrp] u16 |
//      M[m][max_rows] | LM[m][mrp] | V[pad4(max_rows)][k]
size_t recode_prepare_lds_bytes(uint32_t k, uint32_t m, uint32_t max_rows) {
    const uint32_t mrp = pad8(max_rows);
    return 768 + 1024 + 4 * (size_t)mrp + pad16(m * max_rows) + (size_t)m * mrp +
           pad16(((max_rows + 3) & ~3u) * k);
}

__global__ void __launch_bounds__(64) k_recode_prepare(RecodePrepareArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const uint32_t g = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const uint32_t k = a.k, m = a.m, mr = a.max_rows, mrp = pad8(mr);
    uint8_t* const lexp = lds;
    uint8_t* const llog = lds + 512;
    uint32_t* const head = reinterpret_cast<uint32_t*>(lds + 768);
    uint16_t* const next = reinterpret_cast<uint16_t*>(lds + 768 + 1024);
    uint16_t* const cslot = next + mrp;
    uint8_t* const M = lds + 768 + 1024 + 4 * (size_t)mrp;
    uint8_t* const LM = M + pad16(m * mr);
    uint8_t* const V = LM + (size_t)m * mrp;

    for (uint32_t i = lane; i < 768; i += 64) lds[i] = a.explog[i];
    for (uint32_t i = lane; i < 256; i += 64) head[i] = 0xFFFFFFFFu;
    __syncthreads();

    const uint32_t n_raw = a.n_rows ? a.n_rows[g] : mr;
    int32_t status = n_raw == 0 ? QF_ENOTREADY : (n_raw > mr ? QF_EINVAL : QF_OK);
    uint32_t n = status == QF_OK ? n_raw : 0;
    const uint16_t* ridx = a.row_index + (uint64_t)g * mr;

    // Slot kinds: a systematic slot joins its column's list; coded slots
    // (index >= k) are compacted in slot order.
    uint32_t ncoded = 0;
    bool bad = false;
    const uint64_t lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    for (uint32_t s0 = 0; s0 < n; s0 += 64) {
        const uint32_t s = s0 + lane;
        const uint32_t idx = s < n ? ridx[s] : 0;
        const bool coded = s < n && idx >= k;
        if (coded && !a.row_coeffs && idx - k >= a.r) bad = true;
        if (a.row_off && s < n) {
            // a row given by (offset, length): whole 16-byte units inside the region
            const uint32_t off = a.row_off[(uint64_t)g * mr + s], len = a.row_len[(uint64_t)g * mr + s];
            if (len > a.L || (off & 15) || (uint64_t)off + len > a.src_gen_stride) bad = true;
        }
        if (s < n && idx < k) next[s] = (uint16_t)atomicExch(&head[idx], s);   // 0xFFFFFFFF -> kNone16
        const uint64_t bc = __ballot(coded);
        if (coded) cslot[ncoded + __popcll(bc & lt_mask)] = (uint16_t)s;
        ncoded += __popcll(bc);
    }
    __syncthreads();
    if (__any(bad)) {
        // a coded row without a coefficient vector (or a row that is not inside
        // its source region): the generation's outputs are zero
        status = QF_EINVAL;
        n = 0;
        ncoded = 0;
        for (uint32_t i = lane; i < 256; i += 64) head[i] = 0xFFFFFFFFu;
    }

    // Mix matrix, flat [j][s] with row stride max_rows: the bytes of mix_dev, or
    // bytes t0 .. t0 + m * max_rows of the splitmix64 stream (t0 = g * m * max_rows).
    const uint32_t total = m * mr;
    if (n) {
        if (a.mix) {
            const uint8_t* src = a.mix + (uint64_t)g * total;
            for (uint32_t t = lane; t < total; t += 64) M[t] = src[t];
        } else {
            const uint64_t t0 = (uint64_t)g * total, t1 = t0 + total;
            for (uint64_t w = t0 / 8 + lane; w * 8 < t1; w += 64) {
                const uint64_t v = splitmix64(a.seed + w);
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const uint64_t t = w * 8 + q;
                    if (t >= t0 && t < t1) M[t - t0] = (uint8_t)(v >> (8 * q));
                }
            }
        }
    }
    __syncthreads();

    // Coded slots: the vector of slot cslot[c] in log form, V[c][i], and the
    // mix column of that slot in log form, LM[j][c] (padded to 4 with zeros).
    const uint32_t nc4 = (ncoded + 3) & ~3u;
    for (uint32_t c = 0; c < ncoded; ++c) {
        const uint32_t s = cslot[c];
        if (a.row_coeffs) {
            const uint8_t* rc = a.row_coeffs + ((uint64_t)g * mr + s) * k;
            for (uint32_t i = lane; i < k; i += 64) {
                const uint32_t v = rc[i];
                V[c * k + i] = (uint8_t)(v ? llog[v] : kLogZero);
            }
        } else {
            // Cauchy row j = index - k: 1 / (i ^ (k + j)); k + j <= 255 and i < k, so never 1 / 0
            const uint32_t y = ridx[s];
            for (uint32_t i = lane; i < k; i += 64) {
                const uint32_t lg = llog[i ^ y];
                V[c * k + i] = (uint8_t)(lg ? 255 - lg : 0);
            }
        }
    }
    if (nc4) {
        for (uint32_t f = lane; f < m * nc4; f += 64) {
            const uint32_t j = f / nc4, c = f - j * nc4;
            uint32_t lm = kLogZero;
            if (c < ncoded) {
                const uint32_t v = M[j * mr + cslot[c]];
                if (v) lm = llog[v];
            }
            LM[j * mrp + c] = (uint8_t)lm;
        }
    }
    __syncthreads();

    // Coefficient records of the payload pass: slot s of pass p holds
    // M[16p .. 16p + 15][s]; slots >= n and the record at max_rows are zero.
    // (Rows by offset: the record of slot s sits in pair record s / 2, behind
    // the pair's 16 descriptor bytes, and the last pair is all zero slots.)
    const uint32_t nrec = a.row_off ? 2 * ((mr + 1) / 2 + 1) : mr + 1;
    for (uint32_t p = 0; p < a.passes; ++p) {
        uint8_t* out = a.coef_out + ((uint64_t)p * a.G + g) * a.coef_gen_stride;
        for (uint32_t s = lane; s < nrec; s += 64) {
            uint32_t w[4] = {0, 0, 0, 0};
            if (s < n) {
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const uint32_t j = p * 16 + q;
                    const uint32_t v = j < m ? M[j * mr + s] : 0u;
                    w[q >> 2] |= v << (8 * (q & 3));
                }
            }
            const uint64_t at = a.row_off ? (uint64_t)(s >> 1) * kPairRecBytes + 16 + (s & 1) * 16 : (uint64_t)s * 16;
            *reinterpret_cast<uint4*>(out + at) = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }

    // Row descriptors of the in-place payload pass (qf_relay.hip), in front of
    // each pair's records: offset and length of slot s, the offset of slot
    // n - 1 and length 0 at and after n, so a lane of k_combine_rows_at that
    // runs past its generation's rows finds a readable unit and a zero record.
    if (a.row_off) {
        const uint32_t* ro = a.row_off + (uint64_t)g * mr;
        const uint32_t* rl = a.row_len + (uint64_t)g * mr;
        const uint32_t last_off = n ? ro[n - 1] : 0;
        uint32_t mx = 0, mn = 0xFFFFFFFFu;
        for (uint32_t s = lane; s < nrec; s += 64) {
            uint32_t off = last_off, len = 0;
            if (s < n) {
                off = ro[s];
                len = rl[s];
                mx = max(mx, len);
                mn = min(mn, len);
            }
            for (uint32_t p = 0; p < a.passes; ++p) {
                uint32_t* pair = reinterpret_cast<uint32_t*>(a.coef_out + ((uint64_t)p * a.G + g) * a.coef_gen_stride +
                                                             (uint64_t)(s >> 1) * kPairRecBytes);
                pair[s & 1] = off;
                pair[2 + (s & 1)] = len;
            }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            mx = max(mx, (uint32_t)__shfl_xor(mx, o, 64));
            mn = min(mn, (uint32_t)__shfl_xor(mn, o, 64));
        }
        if (lane == 0) a.min_len[g] = n ? mn : 0;
        if (a.out_len)
            for (uint32_t j = lane; j < m; j += 64) a.out_len[(uint64_t)g * m + j] = mx;
    }

    // Output vectors, lanes over columns: the systematic slots of column i
    // add their mix entry; the coded slots add M[j][s] * v(s)[i].
    uint8_t* oc = a.out_coeffs + (uint64_t)g * m * k;
    for (uint32_t i = lane; i < k; i += 64) {
        const uint32_t h = head[i];
        for (uint32_t j = 0; j < m; ++j) {
            uint32_t acc = 0;
            for (uint32_t s = h; s < kNone16; s = next[s]) acc ^= M[j * mr + s];
            const uint8_t* lmj = LM + j * mrp;
            for (uint32_t c = 0; c < nc4; c += 4) {
                const uint32_t lm4 = *reinterpret_cast<const uint32_t*>(lmj + c);
                if (lm4 == 0xFFFFFFFFu) continue;   // four zero mix entries (wave-uniform)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const uint32_t lm = (lm4 >> (8 * q)) & 0xFF;
                    const uint32_t lv = V[(c + q) * k + i];
                    const uint32_t pr = lexp[lm + lv];
                    acc ^= (lm == kLogZero || lv == kLogZero) ? 0u : pr;
                }
            }
            oc[j * k + i] = (uint8_t)acc;
        }
    }
    if (lane == 0) {
        a.status[g] = status;
        a.n_out[g] = m;
        a.bound[g] = n;
    }
}

hipError_t launch_recode_prepare(const RecodePrepareArgs& a, hipStream_t st) {
    if (a.G == 0) return hipSuccess;
    if (a.k == 0 || a.k > 255 || a.m == 0 || a.m > 64 || a.max_rows == 0 || a.max_rows > 255 ||
        a.k + a.r > 256 || a.passes != (a.m + 15) / 16)
        return hipErrorInvalidValue;
    const uint64_t rec_bytes = a.row_off ? ((uint64_t)(a.max_rows + 1) / 2 + 1) * kPairRecBytes
                                         : ((uint64_t)a.max_rows + 1) * 16;
    if (a.coef_gen_stride < rec_bytes || (a.coef_gen_stride & 15) || (a.row_off && (!a.row_len || !a.min_len)))
        return hipErrorInvalidValue;
    const size_t lds = recode_prepare_lds_bytes(a.k, a.m, a.max_rows);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    static bool attr_done = false;
    if (!attr_done) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_recode_prepare),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
        attr_done = true;
    }
    hipLaunchKernelGGL(k_recode_prepare, dim3(a.G), dim3(64), lds, st, a);
    return hipGetLastError();
}

}  // namespace qf

extern "C" int qf_recode_batch(qf_ctx* ctx, const qf_recode_shape* sh, uint32_t G, const uint8_t* rows,
                               const uint16_t* row_index, const uint32_t* n_rows, const uint8_t* row_coeffs,
                               const uint8_t* mix, uint64_t seed, uint8_t* out, uint8_t* out_coeffs,
                               int32_t* status) {
    if (!ctx || !sh) return QF_EINVAL;
    const uint32_t k = sh->k, r = sh->r, L = sh->L, max_rows = sh->max_rows, m = sh->m;
    if (k == 0 || k > 255 || max_rows == 0 || max_rows > 255 || m == 0 || m > 64 || L == 0 || sh->flags != 0)
        return QF_EINVAL;
    if (sh->row_stride < L || sh->out_row_stride < L) return QF_EINVAL;
    if ((uint64_t)k + r > 256) return QF_ERANGE;
    if (G == 0) return QF_OK;
    if (!rows || !row_index || !out || !out_coeffs || !status) return QF_EINVAL;
    if (!aligned16(rows) || (sh->row_stride & 15) || (sh->rows_gen_stride & 15) || !aligned16(out) ||
        (sh->out_row_stride & 15) || (sh->out_gen_stride & 15))
        return QF_EINVAL;
    std::unique_lock<std::mutex> lk;
    int s = qf::ctx_lock(ctx, lk);
    if (s) return s;
    hipStream_t st = qf::ctx_stream(ctx);
    // workspace: records [pass][G][(max_rows + 1) * 16] | n_out[G] | bound[G]
    const uint32_t passes = (m + 15) / 16;
    const uint64_t coef_gen_stride = ((uint64_t)max_rows + 1) * 16;
    qf::WorkLayout wl;
    const size_t off_coef = wl.take((size_t)passes * G * coef_gen_stride);
    const size_t off_nout = wl.take((size_t)G * 4);
    const size_t off_bound = wl.take((size_t)G * 4);
    uint8_t* w = nullptr;
    s = qf::ctx_work(ctx, wl.size(), &w);
    if (s) return s;
    uint32_t* d_nout = reinterpret_cast<uint32_t*>(w + off_nout);
    uint32_t* d_bound = reinterpret_cast<uint32_t*>(w + off_bound);
    qf::RecodePrepareArgs pa{};
    pa.row_index = row_index;
    pa.n_rows = n_rows;
    pa.row_coeffs = row_coeffs;
    pa.mix = mix;
    pa.explog = qf::ctx_explog(ctx);
    pa.seed = seed;
    pa.coef_out = w + off_coef;
    pa.coef_gen_stride = coef_gen_stride;
    pa.n_out = d_nout;
    pa.bound = d_bound;
    pa.out_coeffs = out_coeffs;
    pa.status = status;
    pa.k = k;
    pa.r = r;
    pa.m = m;
    pa.max_rows = max_rows;
    pa.passes = passes;
    pa.G = G;
    QF_PROFILED(ctx, st, "k_recode_prepare", qf::launch_recode_prepare(pa, st));
    const uint32_t Lu = (L + 15) / 16;
    for (uint32_t p = 0; p < passes; ++p) {
        qf::CombineSlotsArgs a{};
        a.rows = rows;
        a.rows_gen_stride = sh->rows_gen_stride;
        a.row_stride = sh->row_stride;
        a.dst = out + (uint64_t)p * 16 * sh->out_row_stride;
        a.dst_gen_stride = sh->out_gen_stride;
        a.dst_row_stride = sh->out_row_stride;
        a.coef = pa.coef_out + (uint64_t)p * G * coef_gen_stride;
        a.coef_gen_stride = coef_gen_stride;
        a.n_out = d_nout;
        a.bound = d_bound;
        a.tab256 = qf::ctx_tab256(ctx);
        a.pass = p;
        a.L = L;
        a.Lu = Lu;
        a.zero_slot = max_rows;
        a.total_units = (uint64_t)G * Lu;
        std::string cname;   // the launch names the kernel it picked
        QF_PROFILED(ctx, st, cname, qf::ctx_combine_payload(ctx, a, st, &cname));
    }
    return QF_OK;
}
