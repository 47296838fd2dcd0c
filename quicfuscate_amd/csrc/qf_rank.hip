// qf_rank.hip -- the RLNC receive rule "a row is accepted iff it is
// innovative" (qf_rank_batch, qf_decode_innovative_batch, qf_gf256_rank and the
// decoder object's innovative mode).
//
// For generation g the slots are taken in arrival order; slot s has the vector
// v(s) over the k sources (unit vector of a systematic index, the explicit
// vector of row_coeffs, or the Cauchy row of its index) and is innovative iff
// v(s) is not in the GF(2^8) span of v(0) .. v(s-1).
//
//  k_rank_filter   one wave per generation, lanes over the k columns
//                  (ceil(k / 64) per lane).  The span held so far is kept as
//                    U  the set of unit columns (accepted systematic rows), and
//                    B  nb coded basis rows in reduced form: zero at every
//                       column of U, 1 at their own pivot column, zero at every
//                       other row's pivot column.
//                  Reducing by a unit row is clearing one coordinate, so a
//                  systematic slot costs no products unless its column is a
//                  coded pivot: a free column joins U (and is cleared in B); a
//                  column of U is a repeat; at the pivot of row b the rest of
//                  that row decides: nothing left means e_c is already
//                  spanned, otherwise c joins U and the rest of the row is
//                  re-pivoted.  A run of consecutive systematic slots that
//                  meets no pivot is taken by all lanes at once (first slot of
//                  a column by an LDS atomicMin).  A coded slot drops its U
//                  coordinates, takes its factors v[pivot(b)] (the reduced
//                  form makes them independent of each other), subtracts
//                  factor * B[b] for the nonzero ones, and joins B when
//                  something is left, after which its pivot column is cleared
//                  in the other rows.  Pivots prefer columns that no slot of
//                  the generation brings as a systematic row, so re-pivoting
//                  is rare.  B is stored column-major, four rows of a lane's
//                  column to the dword.  The products thus run over coded
//                  slots and coded basis rows only; the walk stops when the
//                  rank reaches k.
//                  Its second form (qf_rank_update_batch) restores U, B and
//                  piv from a per-generation rank state in HBM first and
//                  writes them back when the rank grew, so a generation
//                  fills over many calls.  Its third form
//                  (qf_rank_update_sel_batch) does so for the generations of
//                  a list only.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "gf256_tables.h"
#include "qf_fec.h"
#include "qf_kernels.h"
#include "qf_gf_dev.h"
#include "qf_internal.h"

namespace qf {

namespace {
constexpr uint32_t kColFree = 0, kColUnit = 1, kColCoded = 2;
constexpr uint32_t kLogZero = 255;   // log form of 0 (logs are 0..254)
// LDS, kc = k rounded up to 16: exp[512] log[256] | first[kc] u32 | colst[kc] |
//      pivrow[kc] | piv[kc] | lfac[kc] | stage[kc] | later[kc] (bytes) | Bt[k][kp]
// Bt is the basis transposed: the entries of column c for basis rows 0, 1, ..
// are the bytes at c * kp, so four rows of a lane's column are one dword.
// kp / 4 is odd, so the lanes' dwords fall into different banks.
__host__ __device__ inline uint32_t rank_kc(uint32_t k) { return (k + 15) & ~15u; }
__host__ __device__ inline uint32_t rank_hdr(uint32_t k) { return 768 + 10 * rank_kc(k); }

__host__ __device__ inline uint32_t rank_kp(uint32_t k) { return ((k + 7) & ~7u) + 4; }

struct RankLds {
    const uint8_t* exp;   // 512
    const uint8_t* log;   // 256
    uint8_t* colst;       // per column: free / unit row / pivot of a coded row
    uint8_t* pivrow;      // per coded pivot column: its basis row
    uint8_t* piv;         // per basis row: its pivot column
    uint8_t* lfac;        // per basis row: log of the current factor (kLogZero: none)
    uint8_t* stage;       // the incoming vector, for the factor gather
    uint8_t* later;       // per column: some slot of the generation is its systematic row
    uint32_t* first;      // per free column: first lane of the current run that brings it
    uint8_t* Bt;          // basis, column-major: entry (row b, column c) at c * kp + b
    uint32_t k, kp;
};

// lfac[b] = log(B[b][col]) for b < nb, b != skip; kLogZero there and up to the
// next multiple of 4.
QF_DEV void rank_factors_of_column(const RankLds& L, uint32_t lane, uint32_t nb, uint32_t col, uint32_t skip) {
    const uint32_t nb4 = (nb + 3) & ~3u;
    for (uint32_t b = lane; b < nb4; b += 64) {
        uint32_t f = 0;
        if (b < nb && b != skip) f = L.Bt[col * L.kp + b];
        L.lfac[b] = (uint8_t)(f ? L.log[f] : kLogZero);
    }
}

// Column c leaves the basis (it became a unit column): zero in every row.
QF_DEV void rank_clear_column(const RankLds& L, uint32_t lane, uint32_t nb, uint32_t c) {
    uint32_t* p = reinterpret_cast<uint32_t*>(L.Bt + c * L.kp);
    for (uint32_t d = lane; d < (nb + 3) / 4; d += 64) p[d] = 0;
}

// to_rows: B[b] ^= exp(lfac[b]) * x for every b < nb with a factor (lx: the log
// form of x); otherwise x ^= exp(lfac[b]) * B[b].  Four rows per step.
template <bool to_rows, int NQ>
QF_DEV void rank_products(const RankLds& L, uint32_t lane, uint32_t nb, uint32_t (&x)[NQ], const uint32_t (&lx)[NQ]) {
    const uint32_t nb4 = (nb + 3) & ~3u;
    for (uint32_t b0 = 0; b0 < nb4; b0 += 4) {
        // (the same word for every lane: kept scalar, so the skips below are branches)
        const uint32_t lf4 = __builtin_amdgcn_readfirstlane(*reinterpret_cast<const uint32_t*>(L.lfac + b0));
        if (lf4 == 0xFFFFFFFFu) continue;   // four rows without a factor
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const uint32_t col = lane + 64 * q;
            if (col >= L.k) continue;
            uint32_t* p = reinterpret_cast<uint32_t*>(L.Bt + col * L.kp + b0);
            uint32_t bw = *p;
            if (to_rows) {
                if (lx[q] == kLogZero) continue;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const uint32_t lf = (lf4 >> (8 * t)) & 0xFF;
                    if (lf != kLogZero) bw ^= (uint32_t)L.exp[lf + lx[q]] << (8 * t);
                }
                *p = bw;
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const uint32_t lf = (lf4 >> (8 * t)) & 0xFF;
                    const uint32_t bv = (bw >> (8 * t)) & 0xFF;
                    if (lf != kLogZero && bv) x[q] ^= L.exp[lf + L.log[bv]];
                }
            }
        }
    }
}

// The nonzero vector w (zero at every unit column and every pivot column)
// becomes basis row t, normalised at its pivot, that column cleared in the
// other rows.  Any nonzero column serves as the pivot; the first one that no
// slot of the generation brings as a systematic row (sysc: the lane's columns
// that some slot does) is taken where there is one, so that a systematic row
// arriving later does not land on a pivot and force the row to be re-pivoted.
template <int NQ>
QF_DEV void rank_insert(const RankLds& L, uint32_t lane, uint32_t nb, uint32_t t, uint32_t (&w)[NQ],
                        const uint32_t (&sysc)[NQ]) {
    __syncthreads();   // the caller's reads of lfac and Bt are done
    uint32_t pcol = 0, pv = 1;
    bool found = false;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const uint64_t bal = __ballot(w[q] != 0 && (pass == 1 || !sysc[q]));
            if (!found && bal) {
                const uint32_t l = (uint32_t)__builtin_ctzll(bal);
                pcol = 64 * q + l;
                pv = (uint32_t)__shfl((int)w[q], (int)l, 64);
                found = true;
            }
        }
    }
    const uint32_t linv = 255 - L.log[pv];
    uint32_t lw[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        lw[q] = kLogZero;
        if (w[q]) {
            const uint32_t l = L.log[w[q]] + linv;
            lw[q] = l >= 255 ? l - 255 : l;
            w[q] = L.exp[lw[q]];
        }
    }
    rank_factors_of_column(L, lane, nb, pcol, t);
    __syncthreads();
    rank_products<true, NQ>(L, lane, nb, w, lw);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const uint32_t col = lane + 64 * q;
        if (col < L.k) L.Bt[col * L.kp + t] = (uint8_t)w[q];
    }
    if (lane == 0) {
        L.piv[t] = (uint8_t)pcol;
        L.pivrow[pcol] = (uint8_t)t;
        L.colst[pcol] = (uint8_t)kColCoded;
    }
}
}  // namespace

size_t rank_filter_lds_bytes(uint32_t k) { return rank_hdr(k) + (size_t)k * rank_kp(k); }

// The rank state of one generation in HBM (qf_rank_update_batch): the span
// k_rank_filter holds in LDS, without what a call rebuilds.
//   0   magic, k, nu, nb (u32 each); sixteen zero bytes: nothing received
//   16  U as a bit per column, four u64 (column c: bit c % 64 of word c / 64)
//   48  piv[kc] bytes, the first nb valid
//   48 + kc  B, a dword per (row group d, column c) at (d * k + c) * 4: rows
//       4d .. 4d + 3 of column c, the dwords of Bt; consecutive lanes hold
//       consecutive columns, so a row group is one coalesced run.  The first
//       ceil(nb / 4) groups are valid.
// colst and pivrow follow from U and piv; first, lfac, stage and later are
// scratch of one call.
template <bool STATE, bool SEL = false> struct RankArgsOf { typedef RankFilterArgs type; };
template <> struct RankArgsOf<true, false> { typedef RankUpdateArgs type; };
template <> struct RankArgsOf<true, true> { typedef RankUpdateSelArgs type; };
constexpr uint32_t kStateMagic = 0x53524651u;   // "QFRS"
constexpr uint32_t kStateUnits = 16, kStatePiv = 48;
__host__ __device__ inline uint32_t rank_state_basis(uint32_t k) { return kStatePiv + rank_kc(k); }
__host__ __device__ inline uint32_t rank_state_size(uint32_t k) {
    return rank_state_basis(k) + ((((k + 3) & ~3u) * k + 15) & ~15u);
}

// NQ = ceil(k / 64) columns per lane.  STATE: the span is resumed from and
// written back to a.state (the arguments are RankUpdateArgs; timed as
// k_rank_update); without it every added block drops out and the code is the
// one-call filter's, instruction for instruction.  SEL (with STATE; the
// arguments are RankUpdateSelArgs, timed as k_rank_update_sel):
// the block is list entry g of a.G = n_max, its slots and outputs are indexed
// by g, and the state and the dense rank array by the listed generation gs,
// the only two places where that number is used.  Without SEL gs is g and the
// code is what it was.
template <int NQ, bool STATE, bool SEL = false>
__global__ void __launch_bounds__(64) k_rank_filter(typename RankArgsOf<STATE, SEL>::type a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const uint32_t g = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const uint32_t k = a.k, mr = a.max_rows;
    uint32_t gs = g;
    if constexpr (SEL) {
        uint32_t n_used = a.G;
        if (a.n_sel) n_used = min(*a.n_sel, n_used);
        // an unused entry's sel value is not looked at; nothing is read or
        // written through an invalid one
        const bool unused = g >= n_used;
        if (!unused) gs = a.sel[g];
        if (unused || gs >= a.G_src) {
            if (a.innovative)
                for (uint32_t s = lane; s < mr; s += 64) a.innovative[(uint64_t)g * mr + s] = 0;
            if (lane == 0) {
                if (a.rank) a.rank[g] = 0;
                if (a.status) a.status[g] = unused ? QF_OK : QF_EINVAL;
            }
            return;
        }
    }
    uint32_t nu0 = 0, nb0 = 0;   // what the state held; rank0 = nu0 + nb0
    uint32_t rank0 = 0;
    uint8_t* sg = nullptr;
    if constexpr (STATE) {
        // The header decides, before anything else is read: an idle generation
        // (no slot in this call) and an invalid state cost these 16 bytes.
        sg = a.state + (uint64_t)gs * rank_state_size(k);
        const uint4 h = *reinterpret_cast<const uint4*>(sg);
        const bool empty = (h.x | h.y | h.z | h.w) == 0;
        const bool valid = empty || (h.x == kStateMagic && h.y == k && h.z <= k && h.w <= k && h.z + h.w <= k);
        const uint32_t n_in = a.n_rows ? min(a.n_rows[g], mr) : mr;
        if (valid) {
            nu0 = h.z;
            nb0 = h.w;
            rank0 = nu0 + nb0;
        }
        if (!valid || n_in == 0) {
            if (a.innovative)
                for (uint32_t s = lane; s < mr; s += 64) a.innovative[(uint64_t)g * mr + s] = 0;
            if (lane == 0) {
                if (a.rank) a.rank[g] = rank0;
                if constexpr (SEL) {
                    if (a.rank_dense) a.rank_dense[gs] = rank0;
                }
                if (a.status) a.status[g] = valid ? QF_OK : QF_EINVAL;
            }
            return;
        }
    }
    RankLds L;
    L.exp = lds;
    L.log = lds + 512;
    const uint32_t kc = rank_kc(k);
    L.first = reinterpret_cast<uint32_t*>(lds + 768);
    L.colst = lds + 768 + 4 * kc;
    L.pivrow = L.colst + kc;
    L.piv = L.pivrow + kc;
    L.lfac = L.piv + kc;
    L.stage = L.lfac + kc;
    L.later = L.stage + kc;
    L.Bt = lds + rank_hdr(k);
    L.k = k;
    L.kp = rank_kp(k);

    for (uint32_t i = lane; i < 768; i += 64) lds[i] = a.explog[i];
    for (uint32_t i = lane; i < kc; i += 64) {
        L.colst[i] = (uint8_t)kColFree;
        L.later[i] = 0;
        L.first[i] = 0xFFFFFFFFu;
    }
    __syncthreads();

    uint32_t n = a.n_rows ? min(a.n_rows[g], mr) : mr;
    const uint16_t* ridx = a.row_index + (uint64_t)g * mr;
    uint8_t* inn = a.innovative ? a.innovative + (uint64_t)g * mr : nullptr;
    const uint32_t lim = a.row_coeffs ? 256u : a.r;
    bool bad = false;
    for (uint32_t s = lane; s < n; s += 64) {
        const uint32_t idx = ridx[s];
        if (idx < k) L.later[idx] = 1;
        else if (idx - k >= lim) bad = true;
    }
    __syncthreads();
    int32_t status = QF_OK;
    if (__any(bad)) {   // a coded row without a coefficient vector: rank 0, no flags
        status = QF_EINVAL;
        n = 0;
    }
    uint32_t sysc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) sysc[q] = lane + 64 * q < k ? L.later[lane + 64 * q] : 0u;
    const uint64_t lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));

    if constexpr (STATE) {
        // Restore U, piv and the nb rows of B into the layout above.  A full
        // span and a generation with a bad slot walk nothing and need none of it.
        if (n && rank0 < k && rank0) {
            const uint32_t ng = (nb0 + 3) / 4;
            // piv first, range-checked before any of it is used as an index
            bool badp = false;
            const uint32_t* sp = reinterpret_cast<const uint32_t*>(sg + kStatePiv);
            for (uint32_t d = lane; d < ng; d += 64) {
                const uint32_t p4 = sp[d];
#pragma unroll
                for (uint32_t t = 0; t < 4; ++t)
                    if (4 * d + t < nb0 && ((p4 >> (8 * t)) & 0xFF) >= k) badp = true;
                reinterpret_cast<uint32_t*>(L.piv)[d] = p4;
            }
            // U: as many columns below k as the header counts
            const uint64_t* su = reinterpret_cast<const uint64_t*>(sg + kStateUnits);
            uint32_t cnt_u = 0;
            bool unit[NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const uint64_t m = su[q];
                if (64u * (q + 1) > k && (m >> (k - 64u * q))) badp = true;   // a column at or above k
                unit[q] = (m >> lane) & 1;
                cnt_u += (uint32_t)__popcll(m);
            }
            for (int q = NQ; q < 4; ++q)
                if (su[q]) badp = true;
            if (__any(badp) || cnt_u != nu0) {
                status = QF_EINVAL;
                n = 0;
                nu0 = nb0 = rank0 = 0;
            } else {
#pragma unroll
                for (int q = 0; q < NQ; ++q)
                    if (unit[q]) L.colst[lane + 64 * q] = (uint8_t)kColUnit;
                __syncthreads();
                for (uint32_t b = lane; b < nb0; b += 64) {
                    const uint32_t c = L.piv[b];
                    L.colst[c] = (uint8_t)kColCoded;
                    L.pivrow[c] = (uint8_t)b;
                }
                const uint32_t* sb = reinterpret_cast<const uint32_t*>(sg + rank_state_basis(k));
                for (uint32_t d = 0; d < ng; ++d) {
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        const uint32_t col = lane + 64 * q;
                        if (col < k) reinterpret_cast<uint32_t*>(L.Bt + col * L.kp)[d] = sb[d * k + col];
                    }
                }
                __syncthreads();
            }
        }
    }

    uint32_t nu = nu0, nb = nb0;   // unit rows, coded basis rows; rank = nu + nb
    uint32_t s0 = 0;
    for (; s0 < n && nu + nb < k; s0 += 64) {
        const uint32_t cnt = min(64u, n - s0);
        const uint32_t my_idx = lane < cnt ? ridx[s0 + lane] : 0xFFFFu;
        // lanes whose slot is no systematic row (coded, or past the chunk's end)
        const uint64_t other = __ballot(my_idx >= k);
        uint32_t my_flag = 0;
        uint32_t j = 0;
        while (j < cnt && nu + nb < k) {
            const uint64_t other_from_j = other & (~0ull << j);
            const uint32_t jc = other_from_j ? (uint32_t)__builtin_ctzll(other_from_j) : 64u;
            if (jc > j) {
                // A run of systematic slots [j, jc), all lanes at once up to the
                // first one whose column is a coded pivot (jh): a free column
                // joins U at its first slot of the run (and leaves B), a column
                // of U is a repeat; no products.
                const bool in_run = lane >= j && lane < jc;
                const uint32_t st = in_run ? L.colst[my_idx] : kColUnit;
                const uint64_t hit = __ballot(in_run && st == kColCoded);
                const uint32_t jh = hit ? (uint32_t)__builtin_ctzll(hit) : jc;
                const bool cand = in_run && lane < jh && st == kColFree;
                if (cand) atomicMin(&L.first[my_idx], lane);
                __syncthreads();
                const bool fresh = cand && L.first[my_idx] == lane;
                const uint64_t fm = __ballot(fresh);
                const uint32_t room = k - (nu + nb);
                if (fresh && (uint32_t)__popcll(fm & lt_mask) < room) {
                    L.colst[my_idx] = (uint8_t)kColUnit;
                    uint32_t* p = reinterpret_cast<uint32_t*>(L.Bt + my_idx * L.kp);
                    for (uint32_t d = 0; d < (nb + 3) / 4; ++d) p[d] = 0;
                    my_flag = 1;
                }
                nu += min((uint32_t)__popcll(fm), room);
                __syncthreads();
                j = jh;
                if (jh == jc) continue;
                if (nu + nb >= k) break;
            }
            const uint32_t idx = (uint32_t)__builtin_amdgcn_readlane((int)my_idx, (int)j);
            bool take = false;
            if (idx < k) {
                // a systematic row at the pivot column of basis row t: e_idx - B[t] is
                // B[t] without its pivot; nothing left means e_idx is spanned already,
                // otherwise idx joins U and the rest of the row finds a new pivot
                const uint32_t t = L.pivrow[idx];
                uint32_t w[NQ];
                bool nz = false;
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const uint32_t col = lane + 64 * q;
                    w[q] = (col < k && col != idx) ? L.Bt[col * L.kp + t] : 0u;
                    nz |= w[q] != 0;
                }
                if (__any(nz)) {
                    __syncthreads();
                    rank_clear_column(L, lane, nb, idx);
                    if (lane == 0) L.colst[idx] = (uint8_t)kColUnit;
                    rank_insert<NQ>(L, lane, nb, t, w, sysc);
                    ++nu;
                    take = true;
                }
            } else {
                uint32_t v[NQ];
                const uint8_t* rc = a.row_coeffs ? a.row_coeffs + ((uint64_t)g * mr + s0 + j) * k : nullptr;
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const uint32_t col = lane + 64 * q;
                    uint32_t x = 0;
                    if (col < k) {
                        // Cauchy row index - k: 1 / (col ^ index); index <= 255 and col < k <= index
                        x = rc ? rc[col] : L.exp[255 - L.log[(col ^ idx) & 0xFF]];
                        if (L.colst[col] == kColUnit) x = 0;
                        L.stage[col] = (uint8_t)x;
                    }
                    v[q] = x;
                }
                __syncthreads();
                const uint32_t nb4 = (nb + 3) & ~3u;
                for (uint32_t b = lane; b < nb4; b += 64) {
                    const uint32_t f = b < nb ? L.stage[L.piv[b]] : 0u;
                    L.lfac[b] = (uint8_t)(f ? L.log[f] : kLogZero);
                }
                __syncthreads();
                uint32_t none[NQ];
#pragma unroll
                for (int q = 0; q < NQ; ++q) none[q] = 0;
                rank_products<false, NQ>(L, lane, nb, v, none);
                bool nz = false;
#pragma unroll
                for (int q = 0; q < NQ; ++q) nz |= v[q] != 0;
                if (__any(nz)) {
                    rank_insert<NQ>(L, lane, nb, nb, v, sysc);
                    ++nb;
                    take = true;
                }
            }
            __syncthreads();
            if (take && lane == j) my_flag = 1;
            ++j;
        }
        if (inn && s0 + lane < mr) inn[s0 + lane] = (uint8_t)my_flag;
    }
    if (inn)
        for (uint32_t s = s0 + lane; s < mr; s += 64) inn[s] = 0;
    if constexpr (STATE) {
        // The span changes exactly when the rank does: a call that brought
        // nothing new (and one that was ignored) leaves the state as it is.
        if (status == QF_OK && nu + nb != rank0) {
            __syncthreads();
            const uint32_t ng = (nb + 3) / 4;
            uint64_t* su = reinterpret_cast<uint64_t*>(sg + kStateUnits);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                uint64_t m = 0;
                if (q < NQ) m = __ballot(lane + 64 * q < k && L.colst[lane + 64 * q] == kColUnit);
                if (lane == 0) su[q] = m;
            }
            // (rows nb .. 4 ng - 1 of the last group were never written: zeros go out)
            const uint32_t tail = nb & 3 ? (1u << (8 * (nb & 3))) - 1 : 0xFFFFFFFFu;
            uint32_t* sp = reinterpret_cast<uint32_t*>(sg + kStatePiv);
            for (uint32_t d = lane; d < ng; d += 64)
                sp[d] = reinterpret_cast<const uint32_t*>(L.piv)[d] & (d + 1 == ng ? tail : 0xFFFFFFFFu);
            uint32_t* sb = reinterpret_cast<uint32_t*>(sg + rank_state_basis(k));
            for (uint32_t d = 0; d < ng; ++d) {
                const uint32_t keep = d + 1 == ng ? tail : 0xFFFFFFFFu;
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const uint32_t col = lane + 64 * q;
                    if (col < k) sb[d * k + col] = reinterpret_cast<const uint32_t*>(L.Bt + col * L.kp)[d] & keep;
                }
            }
            if (lane == 0) *reinterpret_cast<uint4*>(sg) = make_uint4(kStateMagic, k, nu, nb);
        }
    }
    if (lane == 0) {
        if (a.rank) a.rank[g] = nu + nb;
        if constexpr (SEL) {
            if (a.rank_dense) a.rank_dense[gs] = nu + nb;
        }
        if (a.status) a.status[g] = status;
    }
}

template <int NQ, class Args>
static hipError_t launch_rank_nq(void (*kern)(Args), const Args& a, size_t lds, hipStream_t st) {
    if (lds > 64 * 1024) {   // k near 256: above the default dynamic LDS limit
        static bool attr_done = false;   // (one per kernel: NQ and Args name it)
        if (!attr_done) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            if (e != hipSuccess) return e;
            attr_done = true;
        }
    }
    hipLaunchKernelGGL(kern, dim3(a.G), dim3(64), lds, st, a);
    return hipGetLastError();
}

template <int NQ>
static hipError_t launch_rank_filter_nq(const RankFilterArgs& a, size_t lds, hipStream_t st) {
    return launch_rank_nq<NQ, RankFilterArgs>(k_rank_filter<NQ, false>, a, lds, st);
}

hipError_t launch_rank_filter(const RankFilterArgs& a, hipStream_t st) {
    if (a.G == 0) return hipSuccess;
    if (a.k == 0 || a.k > 256 || a.max_rows == 0 || a.max_rows > 4096 || (!a.row_coeffs && a.r && a.k + a.r > 256))
        return hipErrorInvalidValue;
    const size_t lds = rank_filter_lds_bytes(a.k);
    switch ((a.k + 63) / 64) {
        case 1: return launch_rank_filter_nq<1>(a, lds, st);
        case 2: return launch_rank_filter_nq<2>(a, lds, st);
        case 3: return launch_rank_filter_nq<3>(a, lds, st);
        default: return launch_rank_filter_nq<4>(a, lds, st);
    }
}

size_t rank_state_bytes(uint32_t k) { return k >= 1 && k <= 256 ? rank_state_size(k) : 0; }

hipError_t launch_rank_update(const RankUpdateArgs& a, hipStream_t st) {
    if (a.G == 0) return hipSuccess;
    if (a.k == 0 || a.k > 256 || a.max_rows == 0 || a.max_rows > 4096 || !a.state ||
        (!a.row_coeffs && a.r && a.k + a.r > 256))
        return hipErrorInvalidValue;
    const size_t lds = rank_filter_lds_bytes(a.k);
    switch ((a.k + 63) / 64) {
        case 1: return launch_rank_nq<1, RankUpdateArgs>(k_rank_filter<1, true>, a, lds, st);
        case 2: return launch_rank_nq<2, RankUpdateArgs>(k_rank_filter<2, true>, a, lds, st);
        case 3: return launch_rank_nq<3, RankUpdateArgs>(k_rank_filter<3, true>, a, lds, st);
        default: return launch_rank_nq<4, RankUpdateArgs>(k_rank_filter<4, true>, a, lds, st);
    }
}

hipError_t launch_rank_update_sel(const RankUpdateSelArgs& a, hipStream_t st) {
    if (a.G == 0) return hipSuccess;
    if (a.k == 0 || a.k > 256 || a.max_rows == 0 || a.max_rows > 4096 || !a.state || !a.sel || a.G_src == 0 ||
        (!a.row_coeffs && a.r && a.k + a.r > 256))
        return hipErrorInvalidValue;
    const size_t lds = rank_filter_lds_bytes(a.k);
    switch ((a.k + 63) / 64) {
        case 1: return launch_rank_nq<1, RankUpdateSelArgs>(k_rank_filter<1, true, true>, a, lds, st);
        case 2: return launch_rank_nq<2, RankUpdateSelArgs>(k_rank_filter<2, true, true>, a, lds, st);
        case 3: return launch_rank_nq<3, RankUpdateSelArgs>(k_rank_filter<3, true, true>, a, lds, st);
        default: return launch_rank_nq<4, RankUpdateSelArgs>(k_rank_filter<4, true, true>, a, lds, st);
    }
}

hipError_t launch_rank(qf_ctx* ctx, const RowArrays& rows, uint32_t k, uint32_t r, uint32_t max_rows, uint32_t G,
                       uint8_t* state, uint8_t* innovative, uint32_t* rank, int32_t* status, hipStream_t st) {
    RankUpdateArgs fa{};
    fa.row_index = rows.index;
    fa.n_rows = rows.n_rows;
    fa.row_coeffs = rows.coeffs;
    fa.explog = ctx_explog(ctx);
    fa.innovative = innovative;
    fa.rank = rank;
    fa.status = status;
    fa.k = k;
    fa.r = r;
    fa.max_rows = max_rows;
    fa.G = G;
    fa.state = state;
    return state ? launch_rank_update(fa, st) : launch_rank_filter(fa, st);
}

void RankBasis::reset(uint32_t k) {
    k_ = k;
    rank_ = 0;
    rows_.assign((size_t)k * k, 0);
    has_.assign(k, 0);
}

bool RankBasis::add(uint8_t* v) {
    const Gf256& f = gf();
    const uint32_t k = k_;
    for (uint32_t c = 0; c < k; ++c) {
        const uint8_t x = v[c];
        if (!x) continue;
        if (!has_[c]) {
            // first nonzero left: the new pivot, normalised
            uint8_t inv = 1;
            f.inv(x, &inv);
            uint8_t* row = &rows_[(size_t)c * k];
            for (uint32_t i = c; i < k; ++i) row[i] = f.mul(v[i], inv);
            has_[c] = 1;
            ++rank_;
            return true;
        }
        const uint8_t* row = &rows_[(size_t)c * k];
        for (uint32_t i = c; i < k; ++i) v[i] ^= f.mul(x, row[i]);
    }
    return false;
}

}  // namespace qf

extern "C" int qf_gf256_rank(uint32_t k, uint32_t n, const uint8_t* vectors, uint8_t* innovative_out,
                             uint32_t* rank_out) {
    if (k == 0 || !rank_out || (n && !vectors)) return QF_EINVAL;
    qf::RankBasis basis;
    basis.reset(k);
    std::vector<uint8_t> v(k);
    for (uint32_t s = 0; s < n; ++s) {
        bool take = false;
        if (basis.rank() < k) {
            memcpy(v.data(), vectors + (size_t)s * k, k);
            take = basis.add(v.data());
        }
        if (innovative_out) innovative_out[s] = take ? 1 : 0;
    }
    *rank_out = basis.rank();
    return QF_OK;
}

// qf_rank_batch, and with `resume` qf_rank_update_batch from and into `state`.
static int rank_run(qf_ctx* ctx, const qf_rank_shape* sh, uint32_t G, const uint16_t* row_index,
                    const uint32_t* n_rows, const uint8_t* row_coeffs, bool resume, uint8_t* state,
                    uint8_t* innovative, uint32_t* rank, int32_t* status) {
    if (!ctx || !sh) return QF_EINVAL;
    const uint32_t k = sh->k, r = sh->r, max_rows = sh->max_rows;
    if (k == 0 || k > 256 || max_rows == 0 || max_rows > 4096 || sh->flags != 0) return QF_EINVAL;
    if (!row_coeffs && r && (uint64_t)k + r > 256) return QF_ERANGE;
    if (G == 0) return QF_OK;
    if (!row_index || !rank || !status) return QF_EINVAL;
    if (resume && (!state || !aligned16(state))) return QF_EINVAL;
    std::unique_lock<std::mutex> lk;
    int s = qf::ctx_lock(ctx, lk);
    if (s) return s;
    hipStream_t st = qf::ctx_stream(ctx);
    const qf::RowArrays rows{nullptr, nullptr, row_index, n_rows, row_coeffs};
    QF_PROFILED(ctx, st, resume ? "k_rank_update" : "k_rank_filter",
                qf::launch_rank(ctx, rows, k, r, max_rows, G, state, innovative, rank, status, st));
    return QF_OK;
}

extern "C" int qf_rank_batch(qf_ctx* ctx, const qf_rank_shape* sh, uint32_t G, const uint16_t* row_index,
                             const uint32_t* n_rows, const uint8_t* row_coeffs, uint8_t* innovative,
                             uint32_t* rank, int32_t* status) {
    return rank_run(ctx, sh, G, row_index, n_rows, row_coeffs, false, nullptr, innovative, rank, status);
}

extern "C" size_t qf_rank_state_bytes(uint32_t k) { return qf::rank_state_bytes(k); }

extern "C" int qf_rank_update_batch(qf_ctx* ctx, const qf_rank_shape* sh, uint32_t G, const uint16_t* row_index,
                                    const uint32_t* n_rows, const uint8_t* row_coeffs, uint8_t* state,
                                    uint8_t* innovative, uint32_t* rank, int32_t* status) {
    return rank_run(ctx, sh, G, row_index, n_rows, row_coeffs, true, state, innovative, rank, status);
}

extern "C" int qf_rank_update_sel_batch(qf_ctx* ctx, const qf_rank_shape* sh, const qf_gen_sel* sel,
                                        const uint16_t* row_index, const uint32_t* n_rows, const uint8_t* row_coeffs,
                                        uint8_t* state, uint8_t* innovative, uint32_t* rank_sel, uint32_t* rank,
                                        int32_t* status) {
    if (!ctx || !sh || !sel || !sel->sel_dev || sel->n_max == 0 || sel->G_src == 0) return QF_EINVAL;
    const uint32_t k = sh->k, r = sh->r, max_rows = sh->max_rows;
    if (k == 0 || k > 256 || max_rows == 0 || max_rows > 4096 || sh->flags != 0) return QF_EINVAL;
    if (!row_coeffs && r && (uint64_t)k + r > 256) return QF_ERANGE;
    if (!row_index || !status || !state || !aligned16(state)) return QF_EINVAL;
    std::unique_lock<std::mutex> lk;
    int s = qf::ctx_lock(ctx, lk);
    if (s) return s;
    hipStream_t st = qf::ctx_stream(ctx);
    qf::RankUpdateSelArgs fa{};
    fa.row_index = row_index;
    fa.n_rows = n_rows;
    fa.row_coeffs = row_coeffs;
    fa.explog = qf::ctx_explog(ctx);
    fa.innovative = innovative;
    fa.rank = rank_sel;
    fa.status = status;
    fa.k = k;
    fa.r = r;
    fa.max_rows = max_rows;
    fa.G = sel->n_max;
    fa.state = state;
    fa.sel = sel->sel_dev;
    fa.n_sel = sel->n_sel_dev;
    fa.rank_dense = rank;
    fa.G_src = sel->G_src;
    QF_PROFILED(ctx, st, "k_rank_update_sel", qf::launch_rank_update_sel(fa, st));
    return QF_OK;
}
