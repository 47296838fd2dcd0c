// qf_kernels.hip -- hand-written CDNA4 (gfx950) kernels for GF(2^8) RLNC.
//
// Arithmetic core: split-index table multiply on v_perm_b32 (see
// gf256_tables.h).  One v_perm performs four 8-entry byte lookups, so a
// product c*x of four packed bytes is three v_perm (bits 0-2, 3-5, 6-7); two
// source rows are folded per step so that six products accumulate with three
// v_bitop3_b32 (3-input XOR, truth table 0x96).  That is 4.5 VALU ops per
// dword-coefficient (1.125 per byte multiply-add), no MFMA, no LDS lookups in
// the inner loop for encode.  The selectors (x & 7, x>>3 & 7, x>>6 & 3) of a
// source dword are computed once and reused by all r repairs.
//
// Kernels
//  k_combine_uniform<R,V,TAIL>  encode: out[g][j] = sum_i C[j][i] * in[g][i]
//                               with one coefficient matrix for the batch;
//                               its split tables live in LDS, [i][j] order,
//                               read by broadcast ds_read with immediate
//                               offsets.  Lanes map flat over (generation,
//                               16-byte unit) so a 1200-B row costs no lane
//                               waste.  Persistent grid.
//  k_combine_slots<R,TAIL>      decode payload pass: per-generation
//                               coefficient records (one 16-byte record per
//                               received slot), value-indexed split tables in
//                               LDS.
//  k_decode_prepare             decode control: row acceptance
//                               (decoder.rs:678-701), erasure bookkeeping and
//                               Gauss-Jordan over [A_E | A_S | I] in LDS
//                               (decoder.rs:720-783, F4 fixed) producing the
//                               e x k recovery matrix; one wave per generation,
//                               ballot pivot search.
//  k_mul_slice                  element-wise a[i]*b[i] (gf_tables.rs:255-274).
//  k_fill_splitmix              synthetic payload generator.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "qf_kernels.h"
#include "qf_gf_dev.h"

namespace qf {

// The multiply-add, unit load / store and streaming-load helpers live in
// qf_gf_dev.h (shared with qf_relay.hip).  The counted waits of the asm loads:
template <int N>
QF_DEV void vm_wait2(v4u& a, v4u& b);
#define QF_VM_WAIT2(N)                                                           \
    template <>                                                                  \
    QF_DEV void vm_wait2<N>(v4u & a, v4u & b) {                                  \
        asm volatile("s_waitcnt vmcnt(" #N ")" : "+v"(a), "+v"(b)::"memory");   \
    }
QF_VM_WAIT2(0)
QF_VM_WAIT2(2)
QF_VM_WAIT2(4)
QF_VM_WAIT2(6)
QF_VM_WAIT2(8)
QF_VM_WAIT2(10)
QF_VM_WAIT2(12)
QF_VM_WAIT2(14)
QF_VM_WAIT2(16)
QF_VM_WAIT2(20)
QF_VM_WAIT2(24)

// ---------------------------------------------------------------------------
// Encode: one coefficient matrix for the whole batch.
// ---------------------------------------------------------------------------
template <int R, int V>
QF_DEV void fma_rows(uint4 (&acc)[R][V], const uint32_t* __restrict__ t, const uint4 (&xa)[V],
                     const uint4 (&xb)[V]) {
    Sel sa[V], sb[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        sa[v] = selectors(xa[v]);
        sb[v] = selectors(xb[v]);
    }
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const uint4 A = *reinterpret_cast<const uint4*>(t + j * 8);
        const uint32_t a2 = t[j * 8 + 4];
        const uint4 B = *reinterpret_cast<const uint4*>(t + R * 8 + j * 8);
        const uint32_t b2 = t[R * 8 + j * 8 + 4];
#pragma unroll
        for (int v = 0; v < V; ++v) fma_pair(acc[j][v], A, a2, sa[v], B, b2, sb[v]);
    }
}

template <int V>
QF_DEV void load_pair(uint4 (&xa)[V], uint4 (&xb)[V], const uint8_t* const (&sp)[V],
                      uint64_t offa, uint64_t offb, const uint32_t (&nbytes)[V]) {
#pragma unroll
    for (int v = 0; v < V; ++v) {
        xa[v] = load_unit(sp[v] + offa, nbytes[v]);
        xb[v] = load_unit(sp[v] + offb, nbytes[v]);
    }
}

template <int V>
QF_DEV void aload_pair(v4u (&xa)[V], v4u (&xb)[V], const uint8_t* const (&sp)[V], uint64_t offa,
                       uint64_t offb) {
#pragma unroll
    for (int v = 0; v < V; ++v) {
        aload16(xa[v], sp[v] + offa);
        aload16(xb[v], sp[v] + offb);
    }
}

template <int V>
QF_DEV void to_u4v(uint4 (&o)[V], const v4u (&x)[V]) {
#pragma unroll
    for (int v = 0; v < V; ++v) o[v] = to_u4(x[v]);
}

// One work item: V units per lane, all k rows, R outputs.
//
// Row pairs stream through a ring of PD+1 register buffers: the loads of
// pair p+PD are issued before pair p is computed, so 2*V*PD loads (PD pairs)
// stay in flight per wave while it computes.  Rows past k-1 are clamped to
// row k-1; their split tables are zero records (k_pad = round_up(k,
// 2*(PD+1))), so the clamped data contributes nothing and every load is
// unconditional.
template <int R, int V, int PD, bool TAIL>
QF_DEV void combine_uniform_item(const CombineUniformArgs& a, const uint32_t* __restrict__ tabs,
                                 const uint8_t* const (&sp)[V], uint8_t* const (&dp)[V],
                                 const uint32_t (&nbytes)[V]) {
    const uint64_t rs = a.src_row_stride;
    const uint32_t k = a.k;
    const uint32_t klast = k - 1;
    auto off = [&](uint32_t i) -> uint64_t { return (uint64_t)(i < klast ? i : klast) * rs; };
    uint4 acc[R][V];
#pragma unroll
    for (int j = 0; j < R; ++j)
#pragma unroll
        for (int v = 0; v < V; ++v) acc[j][v] = make_uint4(0, 0, 0, 0);

    if (TAIL) {
        // Partial units (rows shorter than a whole 16-byte unit): plain loads.
        uint4 xa[V], xb[V];
        for (uint32_t i = 0; i < k; i += 2) {
            load_pair<V>(xa, xb, sp, off(i), off(i + 1), nbytes);
            fma_rows<R, V>(acc, tabs + (size_t)i * R * 8, xa, xb);
        }
    } else {
        constexpr int NB = PD + 1;
        v4u ba[NB][V], bb[NB][V];
#pragma unroll
        for (int q = 0; q < PD; ++q) aload_pair<V>(ba[q], bb[q], sp, off(2 * q), off(2 * q + 1));
        for (uint32_t i = 0; i < k; i += 2 * NB) {
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                const int nbuf = (q + PD) % NB;
                aload_pair<V>(ba[nbuf], bb[nbuf], sp, off(i + 2 * (q + PD)), off(i + 2 * (q + PD) + 1));
#pragma unroll
                for (int v = 0; v < V; ++v) vm_wait2<2 * V * PD>(ba[q][v], bb[q][v]);
                uint4 xa[V], xb[V];
                to_u4v<V>(xa, ba[q]);
                to_u4v<V>(xb, bb[q]);
                fma_rows<R, V>(acc, tabs + (size_t)(i + 2 * q) * R * 8, xa, xb);
            }
        }
        // Drain the prefetches of the (unused) pairs past the end.
#pragma unroll
        for (int q = 0; q < NB; ++q)
#pragma unroll
            for (int v = 0; v < V; ++v) vm_wait2<0>(ba[q][v], bb[q][v]);
    }
    const uint32_t ra = a.r_active;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        if ((uint32_t)j < ra) {
#pragma unroll
            for (int v = 0; v < V; ++v) {
                if (TAIL) {
                    if (nbytes[v]) store_unit(dp[v] + (uint64_t)j * a.dst_row_stride, acc[j][v], nbytes[v]);
                } else {
                    store_unit(dp[v] + (uint64_t)j * a.dst_row_stride, acc[j][v], 16);
                }
            }
        }
    }
}

template <int R, int V, int PD>
__global__ void __launch_bounds__(256, (V == 1 && PD == 1 ? 3 : 2)) k_combine_uniform(CombineUniformArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_tabs[];
    {
        const uint32_t n4 = a.k_pad * R * 2;  // uint4 count (8 words per record)
        const uint4* g = reinterpret_cast<const uint4*>(a.tabs);
        uint4* l = reinterpret_cast<uint4*>(lds_tabs);
        for (uint32_t w = threadIdx.x; w < n4; w += blockDim.x) l[w] = g[w];
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wpb = blockDim.x >> 6;
    const uint32_t wave = blockIdx.x * wpb + (threadIdx.x >> 6);
    const uint32_t nwaves = gridDim.x * wpb;
    const uint32_t per_wave = 64u * V;
    for (uint64_t base = (uint64_t)wave * per_wave; base < a.total_units;
         base += (uint64_t)nwaves * per_wave) {
        const uint8_t* sp[V];
        uint8_t* dp[V];
        uint32_t nbytes[V];
        bool all_full = true;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const uint64_t f = base + (uint64_t)v * 64 + lane;
            sp[v] = a.src;
            dp[v] = a.dst;
            nbytes[v] = 0;
            if (f < a.total_units) {
                const uint64_t g = f / a.Lu;
                const uint32_t u = (uint32_t)(f - g * a.Lu);
                sp[v] = gen_base(a.src, g, a.src_gen_stride, a.src_offs) + (uint64_t)u * 16;
                dp[v] = gen_base(a.dst, g, a.dst_gen_stride, a.dst_offs) + (uint64_t)u * 16;
                const uint32_t rem = a.L - u * 16;
                nbytes[v] = rem < 16 ? rem : 16;
            }
            all_full = all_full && nbytes[v] == 16;
        }
        if (__all(all_full)) combine_uniform_item<R, V, PD, false>(a, lds_tabs, sp, dp, nbytes);
        else combine_uniform_item<R, V, PD, true>(a, lds_tabs, sp, dp, nbytes);
    }
}

// ---------------------------------------------------------------------------
// Decode payload pass: per-generation coefficient records over slots.
// ---------------------------------------------------------------------------

// Coefficient records: slot s of a lane's generation, or the all-zero record
// at index a.zero_slot for slots at/after the lane's bound.  Data rows past
// the bound are clamped to the last valid slot (multiplied by zero).
template <int R, int PD, bool TAIL>
QF_DEV void combine_slots_item(const CombineSlotsArgs& a, const uint32_t* __restrict__ tab256,
                               const uint8_t* rowp, uint8_t* outp, const uint8_t* coefp,
                               uint32_t nbytes, uint32_t e_lane, uint32_t bound_lane,
                               uint32_t smax) {
    const uint64_t rs = a.row_stride;
    const uint32_t zs = a.zero_slot;
    uint4 acc[R];
#pragma unroll
    for (int j = 0; j < R; ++j) acc[j] = make_uint4(0, 0, 0, 0);
    const uint32_t blast = bound_lane ? bound_lane - 1 : 0;
#define QF_ROW(s) (rowp + (uint64_t)((s) < blast ? (s) : blast) * rs)
#define QF_COEF(s) (coefp + (uint64_t)((s) < bound_lane ? (s) : zs) * 16)
    if (TAIL) {
        for (uint32_t s = 0; s < smax; s += 2) {
            const uint4 xa = load_unit(QF_ROW(s), nbytes);
            const uint4 xb = load_unit(QF_ROW(s + 1), nbytes);
            const uint4 ca = *reinterpret_cast<const uint4*>(QF_COEF(s));
            const uint4 cb = *reinterpret_cast<const uint4*>(QF_COEF(s + 1));
            fma_rows_slots<R>(acc, tab256, xa, xb, ca, cb);
        }
    } else {
        // Ring of PD+1 slot pairs as in combine_uniform_item: four loads per
        // pair (two rows, two coefficient records), PD pairs in flight.
        constexpr int NB = PD + 1;
        v4u pa[NB], pb[NB], qa[NB], qb[NB];
#pragma unroll
        for (int q = 0; q < PD; ++q) {
            aload16(pa[q], QF_ROW(2u * q));
            aload16(pb[q], QF_ROW(2u * q + 1));
            aload16(qa[q], QF_COEF(2u * q));
            aload16(qb[q], QF_COEF(2u * q + 1));
        }
        for (uint32_t s = 0; s < smax; s += 2 * NB) {
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                const int nb = (q + PD) % NB;
                const uint32_t sn = s + 2 * (q + PD);
                aload16(pa[nb], QF_ROW(sn));
                aload16(pb[nb], QF_ROW(sn + 1));
                aload16(qa[nb], QF_COEF(sn));
                aload16(qb[nb], QF_COEF(sn + 1));
                vm_wait2<4 * PD>(pa[q], pb[q]);
                vm_wait2<4 * PD>(qa[q], qb[q]);
                fma_rows_slots<R>(acc, tab256, to_u4(pa[q]), to_u4(pb[q]), to_u4(qa[q]), to_u4(qb[q]));
            }
        }
#pragma unroll
        for (int q = 0; q < NB; ++q) {
            vm_wait2<0>(pa[q], pb[q]);
            vm_wait2<0>(qa[q], qb[q]);
        }
    }
#undef QF_ROW
#undef QF_COEF
#pragma unroll
    for (int j = 0; j < R; ++j) {
        if ((uint32_t)j < e_lane) {
            if (TAIL) store_unit(outp + (uint64_t)j * a.dst_row_stride, acc[j], nbytes);
            else store_unit(outp + (uint64_t)j * a.dst_row_stride, acc[j], 16);
        }
    }
}

template <int R, int PD>
QF_DEV void combine_slots_dispatch(const CombineSlotsArgs& a, const uint32_t* tab256,
                                   const uint8_t* rowp, uint8_t* outp, const uint8_t* coefp,
                                   uint32_t nbytes, uint32_t e_lane, uint32_t bound_lane,
                                   uint32_t smax, bool full) {
    if (full) combine_slots_item<R, PD, false>(a, tab256, rowp, outp, coefp, nbytes, e_lane, bound_lane, smax);
    else combine_slots_item<R, PD, true>(a, tab256, rowp, outp, coefp, nbytes, e_lane, bound_lane, smax);
}

template <int PD>
__global__ void __launch_bounds__(256, (PD == 1 ? 3 : 2)) k_combine_slots(CombineSlotsArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t tab256[256 * 8];
    {
        const uint4* g = reinterpret_cast<const uint4*>(a.tab256);
        uint4* l = reinterpret_cast<uint4*>(tab256);
        for (uint32_t w = threadIdx.x; w < 512; w += blockDim.x) l[w] = g[w];
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wpb = blockDim.x >> 6;
    const uint32_t wave = blockIdx.x * wpb + (threadIdx.x >> 6);
    const uint32_t nwaves = gridDim.x * wpb;
    for (uint64_t base = (uint64_t)wave * 64; base < a.total_units; base += (uint64_t)nwaves * 64) {
        const uint64_t f = base + lane;
        const uint8_t* rowp = a.rows;
        uint8_t* outp = a.dst;
        const uint8_t* coefp = a.coef;
        uint32_t nbytes = 0, e_lane = 0, bound_lane = 0;
        if (f < a.total_units) {
            const uint64_t g = f / a.Lu;
            const uint32_t u = (uint32_t)(f - g * a.Lu);
            rowp = gen_base(a.rows, g, a.rows_gen_stride, a.rows_offs) + (uint64_t)u * 16;
            outp = gen_base(a.dst, g, a.dst_gen_stride, a.dst_offs) + (uint64_t)u * 16;
            coefp = a.coef + g * a.coef_gen_stride;
            const uint32_t rem = a.L - u * 16;
            nbytes = rem < 16 ? rem : 16;
            const uint32_t e = a.n_out[g];
            const uint32_t lo = a.pass * 16;
            e_lane = e > lo ? (e - lo < 16 ? e - lo : 16) : 0;
            bound_lane = e_lane ? a.bound[g] : 0;
        }
        const uint32_t jmax = wave_max_u32(e_lane);
        if (jmax == 0) continue;
        const uint32_t smax = wave_max_u32(bound_lane);
        const bool full = __all(nbytes == 16);
        // Output rows per wave pick the unrolled width (zero coefficients
        // beyond a generation's e make the extra rows harmless).
        if (jmax <= 4) combine_slots_dispatch<4, PD>(a, tab256, rowp, outp, coefp, nbytes, e_lane, bound_lane, smax, full);
        else if (jmax <= 8) combine_slots_dispatch<8, PD>(a, tab256, rowp, outp, coefp, nbytes, e_lane, bound_lane, smax, full);
        else if (jmax <= 12) combine_slots_dispatch<12, PD>(a, tab256, rowp, outp, coefp, nbytes, e_lane, bound_lane, smax, full);
        else if (jmax <= 13) combine_slots_dispatch<13, PD>(a, tab256, rowp, outp, coefp, nbytes, e_lane, bound_lane, smax, full);
        else if (jmax <= 14) combine_slots_dispatch<14, PD>(a, tab256, rowp, outp, coefp, nbytes, e_lane, bound_lane, smax, full);
        else combine_slots_dispatch<16, PD>(a, tab256, rowp, outp, coefp, nbytes, e_lane, bound_lane, smax, full);
    }
}

// Small batches (at most one 64-unit wave-item per CU): the four waves of a
// block share one wave-item and split its slot pairs (wave w takes pairs w,
// w + 4, ...; the next pair's rows and records load while the current one
// multiplies), the partial outputs of waves 1..3 meet wave 0's in LDS, and
// wave 0 stores.  Same arithmetic as combine_slots_item, so the same bytes.
template <int R>
QF_DEV void combine_slots_split_item(const CombineSlotsArgs& a, const uint32_t* __restrict__ tab256,
                                     const uint8_t* rowp, uint8_t* outp, const uint8_t* coefp, uint32_t nbytes,
                                     uint32_t e_lane, uint32_t bound_lane, uint32_t smax, uint32_t wave,
                                     uint4 (*part)[16][64]) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t rs = a.row_stride;
    const uint32_t zs = a.zero_slot;
    const uint32_t blast = bound_lane ? bound_lane - 1 : 0;
    uint4 acc[R];
#pragma unroll
    for (int j = 0; j < R; ++j) acc[j] = make_uint4(0, 0, 0, 0);
#define QF_ROW(s) (rowp + (uint64_t)((s) < blast ? (s) : blast) * rs)
#define QF_COEF(s) (coefp + (uint64_t)((s) < bound_lane ? (s) : zs) * 16)
    uint32_t s = 2 * wave;
    if (s < smax) {
        uint4 xa = load_unit(QF_ROW(s), nbytes), xb = load_unit(QF_ROW(s + 1), nbytes);
        uint4 ca = *reinterpret_cast<const uint4*>(QF_COEF(s)), cb = *reinterpret_cast<const uint4*>(QF_COEF(s + 1));
        for (; s < smax; s += 8) {
            uint4 nxa = xa, nxb = xb, nca = ca, ncb = cb;
            if (s + 8 < smax) {
                nxa = load_unit(QF_ROW(s + 8), nbytes);
                nxb = load_unit(QF_ROW(s + 9), nbytes);
                nca = *reinterpret_cast<const uint4*>(QF_COEF(s + 8));
                ncb = *reinterpret_cast<const uint4*>(QF_COEF(s + 9));
            }
            fma_rows_slots<R>(acc, tab256, xa, xb, ca, cb);
            xa = nxa;
            xb = nxb;
            ca = nca;
            cb = ncb;
        }
    }
#undef QF_ROW
#undef QF_COEF
    if (wave != 0) {
#pragma unroll
        for (int j = 0; j < R; ++j) part[wave - 1][j][lane] = acc[j];
    }
    __syncthreads();
    if (wave == 0) {
        for (int w = 0; w < 3; ++w) {
#pragma unroll
            for (int j = 0; j < R; ++j) {
                const uint4 p = part[w][j][lane];
                acc[j].x ^= p.x;
                acc[j].y ^= p.y;
                acc[j].z ^= p.z;
                acc[j].w ^= p.w;
            }
        }
#pragma unroll
        for (int j = 0; j < R; ++j)
            if ((uint32_t)j < e_lane) store_unit(outp + (uint64_t)j * a.dst_row_stride, acc[j], nbytes);
    }
    __syncthreads();   // part[] is rewritten by the next wave-item
}

__global__ void __launch_bounds__(256) k_combine_slots_split(CombineSlotsArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t tab256[256 * 8];
    __shared__ uint4 part[3][16][64];
    {
        const uint4* g = reinterpret_cast<const uint4*>(a.tab256);
        uint4* l = reinterpret_cast<uint4*>(tab256);
        for (uint32_t w = threadIdx.x; w < 512; w += blockDim.x) l[w] = g[w];
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // every wave of the block walks the same wave-items: the barriers match
    for (uint64_t base = (uint64_t)blockIdx.x * 64; base < a.total_units; base += (uint64_t)gridDim.x * 64) {
        const uint64_t f = base + lane;
        const uint8_t* rowp = a.rows;
        uint8_t* outp = a.dst;
        const uint8_t* coefp = a.coef;
        uint32_t nbytes = 0, e_lane = 0, bound_lane = 0;
        if (f < a.total_units) {
            const uint64_t g = f / a.Lu;
            const uint32_t u = (uint32_t)(f - g * a.Lu);
            rowp = gen_base(a.rows, g, a.rows_gen_stride, a.rows_offs) + (uint64_t)u * 16;
            outp = gen_base(a.dst, g, a.dst_gen_stride, a.dst_offs) + (uint64_t)u * 16;
            coefp = a.coef + g * a.coef_gen_stride;
            const uint32_t rem = a.L - u * 16;
            nbytes = rem < 16 ? rem : 16;
            const uint32_t e = a.n_out[g];
            const uint32_t lo = a.pass * 16;
            e_lane = e > lo ? (e - lo < 16 ? e - lo : 16) : 0;
            bound_lane = e_lane ? a.bound[g] : 0;
        }
        // the same lanes in every wave: jmax and smax are block-uniform
        const uint32_t jmax = wave_max_u32(e_lane);
        if (jmax == 0) continue;
        const uint32_t smax = wave_max_u32(bound_lane);
        if (jmax <= 4)
            combine_slots_split_item<4>(a, tab256, rowp, outp, coefp, nbytes, e_lane, bound_lane, smax, wave, part);
        else if (jmax <= 8)
            combine_slots_split_item<8>(a, tab256, rowp, outp, coefp, nbytes, e_lane, bound_lane, smax, wave, part);
        else
            combine_slots_split_item<16>(a, tab256, rowp, outp, coefp, nbytes, e_lane, bound_lane, smax, wave, part);
    }
}

// ---------------------------------------------------------------------------
// Decode control: one wave (64 lanes) per generation.
// ---------------------------------------------------------------------------
struct PrepLds {
    uint8_t* exp;     // 512
    uint8_t* log;     // 256
    uint32_t* first;  // k    : first slot of systematic index
    uint16_t* sys_slot;  // k : accepted slot of systematic i (0xFFFF none)
    uint16_t* col;    // k    : matrix column of source i
    uint16_t* rep_slot;  // e_max
    uint16_t* emap;   // e_max: erased source indices
    uint16_t* slot_col;  // max_rows: D column of slot (0xFFFF = unused)
    uint16_t* lf;     // e_max: log of elimination factors (0xFFFF = zero)
    uint8_t* M;       // e_max x W
};

QF_DEV uint8_t gmul(const PrepLds& L, uint32_t a, uint32_t b) {
    if (a == 0 || b == 0) return 0;
    return L.exp[(uint32_t)L.log[a] + (uint32_t)L.log[b]];
}

// AT (qf_decode_frames_dev): the rows are given by offset and length
// (PrepareArgs::row_off) and the records are the in-place payload pass's.
template <bool AT>
__global__ void __launch_bounds__(64) k_decode_prepare(PrepareArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const uint32_t g = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const uint32_t k = a.k, emax = a.e_max;
    PrepLds L;
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
        L.slot_col = reinterpret_cast<uint16_t*>(p); p += 2 * a.max_rows_pad;
        L.M = p;
    }
    for (uint32_t i = lane; i < 768; i += 64) lds[i] = a.explog[i];
    for (uint32_t i = lane; i < 256; i += 64) {
        L.first[i] = 0xFFFFFFFFu;
        L.sys_slot[i] = 0xFFFF;
    }
    __syncthreads();
    const uint32_t n = a.n_rows ? min(a.n_rows[g], a.max_rows) : a.max_rows;
    const uint16_t* ridx = a.row_index + (uint64_t)g * a.max_rows;
    // accept flags of k_rank_filter (qf_decode_innovative_batch): a slot
    // without its flag is no candidate; index validity covers every slot
    const uint8_t* acpt = a.accept ? a.accept + (uint64_t)g * a.max_rows : nullptr;
    bool bad = false;
    for (uint32_t s = lane; s < n; s += 64) {
        const uint32_t idx = ridx[s];
        if (idx < k) {
            if (!acpt || acpt[s]) atomicMin(&L.first[idx], s);
        } else if (idx - k >= a.rep_limit) bad = true;
        if (AT) {
            // a row given by (offset, length): whole 16-byte units inside the
            // region, whether the slot is accepted or not (k_recode_prepare's rule)
            const uint32_t off = a.row_off[(uint64_t)g * a.max_rows + s], len = a.row_len[(uint64_t)g * a.max_rows + s];
            if (len > a.L || (off & 15) || (uint64_t)off + len > a.src_gen_stride) bad = true;
        }
    }
    for (uint32_t s = lane; s < a.max_rows; s += 64) L.slot_col[s] = 0xFFFF;
    __syncthreads();
    int32_t status = 0;
    if (__any(bad)) status = -1;  // QF_EINVAL
    // Acceptance scan (first k candidate rows win).
    uint32_t accepted = 0, nrep = 0, bound = 0;
    const uint64_t lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    for (uint32_t s0 = 0; s0 < n && accepted < k; s0 += 64) {
        const uint32_t s = s0 + lane;
        uint32_t idx = 0;
        bool cand = false;
        if (s < n) {
            idx = ridx[s];
            cand = idx >= k ? (idx - k < a.rep_limit) : (L.first[idx] == s);
            if (acpt && !acpt[s]) cand = false;
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
    const uint32_t e = nrep;
    if (status == 0 && accepted < k) status = -3;  // QF_ENOTREADY
    // The matrix is built for up to e_lds rows so that duplicated repair rows
    // (which the reference accepts, decoder.rs:694-697) report a singular
    // matrix exactly like the reference; only a full-rank system with more
    // erasures than the output capacity min(k, r) is a shape error.
    if (status == 0 && e > a.e_lds) status = -1;
    uint32_t W = k + e;
    if (status == 0 && e > 0) {
        // Erased list (ascending source index) and column map.
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
                L.col[i] = (uint16_t)(e + p);
                L.slot_col[L.sys_slot[i]] = (uint16_t)(e + p);
            }
            ne += __popcll(bm);
            np += __popcll(bp);
        }
        for (uint32_t m = lane; m < e; m += 64) L.slot_col[L.rep_slot[m]] = (uint16_t)(k + m);
        __syncthreads();
        // Build M = [A_E | A_S | I_e].
        bool erange = false;
        for (uint32_t m = 0; m < e; ++m) {
            const uint32_t s = L.rep_slot[m];
            const uint32_t j = ridx[s] - k;
            const uint8_t* rc = a.row_coeffs ? a.row_coeffs + ((uint64_t)g * a.max_rows + s) * k : nullptr;
            const uint32_t y = (k + j) & 0xFF;
            for (uint32_t i = lane; i < k; i += 64) {
                uint8_t c;
                if (rc) c = rc[i];
                else {
                    const uint32_t d = (i & 0xFF) ^ y;
                    if (d == 0) { erange = true; c = 0; }
                    else c = L.exp[255 - L.log[d]];
                }
                L.M[m * W + L.col[i]] = c;
            }
            for (uint32_t q = lane; q < e; q += 64) L.M[m * W + k + q] = (q == m) ? 1 : 0;
        }
        __syncthreads();
        if (__any(erange)) status = -2;  // QF_ERANGE
        // Gauss-Jordan on the first e columns.
        for (uint32_t c = 0; c < e && status == 0; ++c) {
            int32_t p = -1;
            for (uint32_t r0 = c; r0 < e; r0 += 64) {
                const uint32_t rr = r0 + lane;
                const uint64_t b = __ballot(rr < e && L.M[rr * W + c] != 0);
                if (b) { p = (int32_t)(r0 + __builtin_ctzll(b)); break; }
            }
            if (p < 0) { status = -4; break; }  // QF_ERANK
            if ((uint32_t)p != c) {
                for (uint32_t col = lane; col < W; col += 64) {
                    const uint8_t t = L.M[c * W + col];
                    L.M[c * W + col] = L.M[p * W + col];
                    L.M[p * W + col] = t;
                }
                __syncthreads();
            }
            const uint8_t piv = L.M[c * W + c];
            const uint8_t inv = L.exp[255 - L.log[piv]];
            __syncthreads();
            for (uint32_t col = lane; col < W; col += 64) L.M[c * W + col] = gmul(L, L.M[c * W + col], inv);
            for (uint32_t m = lane; m < e; m += 64) {
                const uint8_t f = L.M[m * W + c];
                L.lf[m] = (m == c || f == 0) ? 0xFFFF : L.log[f];
            }
            __syncthreads();
            for (uint32_t col = lane; col < W; col += 64) {
                const uint8_t pv = L.M[c * W + col];
                if (pv == 0) continue;
                const uint32_t lp = L.log[pv];
                for (uint32_t m = 0; m < e; ++m) {
                    const uint32_t lfm = L.lf[m];
                    if (lfm == 0xFFFF) continue;
                    L.M[m * W + col] ^= L.exp[lfm + lp];
                }
            }
            __syncthreads();
        }
    }
    if (status == 0 && e > emax) status = -1;  // QF_EINVAL: capacity min(k, r)
    // Outputs.  Record layout per (pass, generation): max_rows slot records
    // of 16 coefficient bytes, then one all-zero record (slot max_rows) that
    // the payload pass reads for slots past a lane's bound.
    if (!AT && lane < a.passes) {
        uint8_t* out = a.coef_out + ((uint64_t)lane * a.G + g) * a.coef_gen_stride;
        *reinterpret_cast<uint4*>(out + (uint64_t)a.max_rows * 16) = make_uint4(0, 0, 0, 0);
    }
    // Rows by offset: 48-byte pair records over the accepted slots only, in
    // arrival order (slot_col marks them once the matrix is built): accepted
    // row t sits in pair t / 2, its offset and length in the pair's first 16
    // bytes and its record behind them.  Rows at and after the accepted count
    // are zero records of length 0 at the last accepted row's offset, also
    // for a generation with nothing to recover, so every lane of
    // k_combine_rows_at finds a readable unit.
    uint32_t at_bound = 0;
    if (AT) {
        const uint32_t* ro = a.row_off + (uint64_t)g * a.max_rows;
        const uint32_t* rl = a.row_len + (uint64_t)g * a.max_rows;
        const uint32_t nrec = 2 * ((min(k, a.max_rows) + 1) / 2 + 1);
        const uint32_t nb = (status == 0 && e > 0) ? bound : 0;
        const uint32_t last_off = nb ? ro[nb - 1] : 0;   // slot bound - 1 is accepted
        uint32_t mn = 0xFFFFFFFFu;
        for (uint32_t s0 = 0; s0 < nb; s0 += 64) {
            const uint32_t s = s0 + lane;
            const uint32_t cl = s < nb ? L.slot_col[s] : 0xFFFF;
            const uint64_t ba = __ballot(cl != 0xFFFF);
            if (cl != 0xFFFF) {
                const uint32_t t = at_bound + __popcll(ba & lt_mask);
                const uint32_t off = ro[s], len = rl[s];
                mn = min(mn, len);
                for (uint32_t pass = 0; pass < a.passes; ++pass) {
                    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const uint32_t m = pass * 16 + q;
                        const uint32_t v = m < e ? L.M[m * W + cl] : 0u;
                        w[q >> 2] |= v << (8 * (q & 3));
                    }
                    uint8_t* pair = a.coef_out + ((uint64_t)pass * a.G + g) * a.coef_gen_stride +
                                    (uint64_t)(t >> 1) * kPairRecBytes;
                    reinterpret_cast<uint32_t*>(pair)[t & 1] = off;
                    reinterpret_cast<uint32_t*>(pair)[2 + (t & 1)] = len;
                    *reinterpret_cast<uint4*>(pair + 16 + (t & 1) * 16) = make_uint4(w[0], w[1], w[2], w[3]);
                }
            }
            at_bound += __popcll(ba);
        }
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
        if (lane == 0) a.min_len[g] = at_bound ? mn : 0;
        if (a.src_slot)
            for (uint32_t i = lane; i < k; i += 64)
                a.src_slot[(uint64_t)g * k + i] = status == 0 ? L.sys_slot[i] : (uint16_t)0xFFFF;
        if (status == 0 && e > 0)
            for (uint32_t m = lane; m < e; m += 64) a.rec_index[(uint64_t)g * emax + m] = L.emap[m];
    } else if (status == 0 && e > 0) {
        for (uint32_t pass = 0; pass < a.passes; ++pass) {
            uint8_t* out = a.coef_out + ((uint64_t)pass * a.G + g) * a.coef_gen_stride;
            for (uint32_t s = lane; s < bound; s += 64) {
                const uint32_t cl = L.slot_col[s];
                uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const uint32_t m = pass * 16 + q;
                    uint32_t v = 0;
                    if (cl != 0xFFFF && m < e) v = L.M[m * W + cl];
                    w[q >> 2] |= v << (8 * (q & 3));
                }
                *reinterpret_cast<uint4*>(out + (uint64_t)s * 16) = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
        for (uint32_t m = lane; m < e; m += 64) a.rec_index[(uint64_t)g * emax + m] = L.emap[m];
    }
    if (lane == 0) {
        a.status[g] = status;
        a.n_out[g] = status == 0 ? e : 0;
        a.bound[g] = AT ? at_bound : (status == 0 ? bound : 0);
    }
}

// ---------------------------------------------------------------------------
// Decode control, Cauchy code: one wave per generation.
//
// Acceptance is k_decode_prepare's (first k candidate rows in arrival order;
// a source counts once, at its first slot; decoder.rs:678-701).  With the
// accepted repairs J (arrival order) and the erased sources E (ascending),
// the syndromes s_J = C[J, E] x_E come from the syndrome kernel and
// x_E = D s_J with D = C[J, E]^-1 in closed form (Cauchy matrix,
// X_a = k + J[a], Y_b = E[b]):
//   D[b][a] = A_a B_b / ((X_a + Y_b) E_a F_b),
//   A_a = prod_t (X_a + Y_t), B_b = prod_t (X_t + Y_b),
//   E_a = prod_{t != a} (X_a + X_t), F_b = prod_{t != b} (Y_b + Y_t).
// A square Cauchy matrix is nonsingular, so the only singular systems are
// repeated repair indices (identical rows), reported as QF_ERANK exactly as
// Gauss-Jordan does.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_decode_prepare_cauchy(PrepareCauchyArgs a) {
    __shared__ uint8_t sexp[512];
    __shared__ uint8_t slog[256];
    __shared__ uint32_t first[256];
    __shared__ uint8_t sys_slot[256];
    __shared__ uint8_t rep_slot[256];   // by repair index j
    __shared__ uint32_t rep_cnt[256];
    __shared__ uint8_t J[256], Eidx[256];
    __shared__ uint32_t lA[256], lB[256], lE[256], lF[256];
    // D = C[J,E]^-1 by repair index: row j holds D[b][.] for outputs b < 64
    // (r <= 64, e <= 64), written out as 16-output pass records
    __shared__ __attribute__((aligned(16))) uint8_t rec[65 * 64];
    const uint32_t g = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const uint32_t k = a.k, r = a.r;
    for (uint32_t i = lane; i < 768; i += 64) {
        if (i < 512) sexp[i] = a.explog[i];
        else slog[i - 512] = a.explog[i];
    }
    for (uint32_t i = lane; i < 256; i += 64) {
        first[i] = 0xFFFFFFFFu;
        sys_slot[i] = 0xFF;
        rep_slot[i] = 0xFF;
        rep_cnt[i] = 0;
    }
    for (uint32_t i = lane; i < 65 * 64; i += 64) rec[i] = 0;
    __syncthreads();
    const uint32_t n = a.n_rows ? min(a.n_rows[g], a.max_rows) : a.max_rows;
    const uint16_t* ridx = a.row_index + (uint64_t)g * a.max_rows;
    bool bad = false;
    for (uint32_t s = lane; s < n; s += 64) {
        const uint32_t idx = ridx[s];
        if (idx < k) atomicMin(&first[idx], s);
        else if (idx - k >= r) bad = true;
    }
    __syncthreads();
    int32_t status = __any(bad) ? -1 : 0;  // QF_EINVAL
    uint32_t accepted = 0, nrep = 0, bound = 0;
    const uint64_t lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    for (uint32_t s0 = 0; s0 < n && accepted < k; s0 += 64) {
        const uint32_t s = s0 + lane;
        uint32_t idx = 0;
        bool cand = false;
        if (s < n) {
            idx = ridx[s];
            cand = idx >= k ? (idx - k < r) : (first[idx] == s);
        }
        const uint64_t bc = __ballot(cand);
        const uint32_t pos = accepted + __popcll(bc & lt_mask);
        const bool acc = cand && pos < k;
        const bool isrep = acc && idx >= k;
        const uint64_t br = __ballot(isrep);
        const uint32_t rpos = nrep + __popcll(br & lt_mask);
        if (acc) {
            if (idx < k) {
                sys_slot[idx] = (uint8_t)s;
            } else {
                const uint32_t j = idx - k;
                J[rpos] = (uint8_t)j;
                rep_slot[j] = (uint8_t)s;
                atomicAdd(&rep_cnt[j], 1u);
                bound = max(bound, j + 1);
            }
        }
        accepted += __popcll(__ballot(acc));
        nrep += __popcll(br);
    }
    // wave max of the highest accepted repair index
    for (int off = 32; off >= 1; off >>= 1) bound = max(bound, (uint32_t)__shfl_xor((int)bound, off, 64));
    __syncthreads();
    const uint32_t e = nrep;
    if (status == 0 && accepted < k) status = -3;  // QF_ENOTREADY
    bool dup = false;
    for (uint32_t j = lane; j < r; j += 64) dup |= rep_cnt[j] > 1;
    if (status == 0 && __any(dup)) status = -4;    // QF_ERANK: repeated repair rows
    if (status == 0 && e > 0) {
        uint32_t ne = 0;
        for (uint32_t i0 = 0; i0 < k; i0 += 64) {
            const uint32_t i = i0 + lane;
            const bool miss = i < k && sys_slot[i] == 0xFF;
            const uint64_t bm = __ballot(miss);
            if (miss) Eidx[ne + __popcll(bm & lt_mask)] = (uint8_t)i;
            ne += __popcll(bm);
        }
        __syncthreads();
        for (uint32_t q = lane; q < e; q += 64) {
            const uint32_t X = (k + J[q]) & 0xFF, Y = Eidx[q];
            uint32_t sa = 0, sb = 0, se = 0, sf = 0;
            for (uint32_t t = 0; t < e; ++t) {
                const uint32_t Xt = (k + J[t]) & 0xFF, Yt = Eidx[t];
                sa += slog[X ^ Yt];
                sb += slog[Xt ^ Y];
                if (t != q) {
                    se += slog[X ^ Xt];
                    sf += slog[Y ^ Yt];
                }
            }
            lA[q] = sa % 255;
            lB[q] = sb % 255;
            lE[q] = se % 255;
            lF[q] = sf % 255;
        }
        __syncthreads();
        for (uint32_t t = lane; t < e * e; t += 64) {
            const uint32_t b = t / e, q = t - b * e;
            const uint32_t X = (k + J[q]) & 0xFF, Y = Eidx[b];
            const uint32_t num = lA[q] + lB[b];
            const uint32_t den = slog[X ^ Y] + lE[q] + lF[b];  // < 3 * 255
            const uint32_t l = (num + 3 * 255 - den) % 255;
            rec[J[q] * 64 + b] = sexp[l];
        }
        __syncthreads();
    }
    const bool ok = status == 0;
    // stage-B records, one set per pass of 16 outputs (pass-major over the
    // batch): slot j < r = syndrome of repair j, slot r = zero
    const uint32_t passes = (a.e_max + 15) / 16;
    for (uint32_t p = 0; p < passes; ++p) {
        uint8_t* co = a.coef_out + ((uint64_t)p * a.G + g) * (r + 1) * 16;
        for (uint32_t j = lane; j <= r; j += 64) {
            uint4 v = make_uint4(0, 0, 0, 0);
            if (ok && j < r) v = *reinterpret_cast<const uint4*>(rec + j * 64 + 16 * p);
            *reinterpret_cast<uint4*>(co + j * 16) = v;
        }
    }
    // slot map for the syndrome kernel (all absent when the generation fails)
    uint8_t* sm = a.smap + (uint64_t)g * a.map_stride;
    for (uint32_t q = lane; q < a.map_stride; q += 64) {
        uint8_t v = 0xFF;
        if (ok) {
            if (q < k) v = sys_slot[q];
            else if (q < k + r) v = rep_slot[q - k];
        }
        sm[q] = v;
    }
    if (ok)
        for (uint32_t b = lane; b < e; b += 64) a.rec_index[(uint64_t)g * a.e_max + b] = Eidx[b];
    if (lane == 0) {
        a.status[g] = status;
        a.n_out[g] = ok ? e : 0;
        a.bound[g] = ok ? bound : 0;
    }
}

// ---------------------------------------------------------------------------
// Decode control of the fused decode: one wave per generation, kPrepWaves
// generations per workgroup sharing the log/exp tables.  Acceptance exactly
// as k_decode_prepare_cauchy (decoder.rs:678-701: first k rows win,
// duplicate systematic rows ignored); then the packed LU record of C[J, E]
// in closed form (bs_codegen._lu_solve_and_store has the layout), the slot
// map, rec_index, n_out and status.  Only wave-local synchronisation after
// the shared tables are loaded.
// ---------------------------------------------------------------------------
constexpr uint32_t kPrepWaves = 4;

QF_DEV void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

struct PrepWave {
    uint32_t first[256];     // first slot of systematic index i (0xFFFFFFFF none)
    uint32_t rep_cnt[16];
    uint8_t sys_slot[256];   // accepted slot of source i (0xFF none)
    uint8_t rep_slot[16];    // accepted slot of repair j
    uint8_t Js[16], rank[16], Eidx[16];
    uint8_t LU[16][16];
    int16_t PP[2][16][17];   // log prefix sums of the closed-form LU
};

__global__ void __launch_bounds__(64 * kPrepWaves) k_decode_prepare_lu(PrepareCauchyArgs a) {
    __shared__ uint8_t sexp[512];
    __shared__ uint8_t slog[256];
    __shared__ PrepWave pw[kPrepWaves];
    for (uint32_t i = threadIdx.x; i < 768; i += blockDim.x) {
        if (i < 512) sexp[i] = a.explog[i];
        else slog[i - 512] = a.explog[i];
    }
    __syncthreads();  // the only block-wide barrier
    const uint32_t w = threadIdx.x >> 6;
    const uint32_t lane = threadIdx.x & 63;
    PrepWave& P = pw[w];
    const uint32_t k = a.k, r = a.r;
    // persistent: each wave takes generations blockIdx*4 + w, + gridDim*4, ...
    for (uint32_t g = blockIdx.x * kPrepWaves + w; g < a.G; g += gridDim.x * kPrepWaves) {
    // the row indices of this generation stay in registers (max_rows <= 255:
    // four slots per lane)
    const uint32_t n = a.n_rows ? min(a.n_rows[g], a.max_rows) : a.max_rows;
    uint32_t idxs[4] = {0xFFFF, 0xFFFF, 0xFFFF, 0xFFFF};
    {
        const uint16_t* ridx = a.row_index + (uint64_t)g * a.max_rows;
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q)
            if (lane + 64 * q < n) idxs[q] = ridx[lane + 64 * q];
    }
    for (uint32_t i = lane; i < 256; i += 64) {
        P.first[i] = 0xFFFFFFFFu;
        P.sys_slot[i] = 0xFF;
    }
    if (lane < 16) {
        P.rep_slot[lane] = 0xFF;
        P.rep_cnt[lane] = 0;
        P.rank[lane] = 0xFF;
        P.Js[lane] = 0;
        P.Eidx[lane] = 0;
    }
    wave_sync();
    bool bad = false;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
        const uint32_t s = lane + 64 * q, idx = idxs[q];
        if (s < n) {
            if (idx < k) atomicMin(&P.first[idx], s);
            else if (idx - k >= r) bad = true;
        }
    }
    wave_sync();
    int32_t status = __any(bad) ? -1 : 0;  // QF_EINVAL
    uint32_t accepted = 0, nrep = 0;
    const uint64_t lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
        const uint32_t s = lane + 64 * q, idx = idxs[q];
        const bool cand = s < n && (idx >= k ? (idx - k < r) : (P.first[idx] == s));
        const uint64_t bc = __ballot(cand);
        const uint32_t pos = accepted + __popcll(bc & lt_mask);
        const bool acc = cand && pos < k;
        const bool isrep = acc && idx >= k;
        if (acc) {
            if (idx < k) {
                P.sys_slot[idx] = (uint8_t)s;
            } else {
                P.rep_slot[idx - k] = (uint8_t)s;
                atomicAdd(&P.rep_cnt[idx - k], 1u);
            }
        }
        accepted += __popcll(__ballot(acc));
        nrep += __popcll(__ballot(isrep));
    }
    wave_sync();
    const uint32_t e = nrep;
    if (status == 0 && accepted < k) status = -3;  // QF_ENOTREADY
    const bool dup = lane < r && P.rep_cnt[lane] > 1;
    if (status == 0 && __any(dup)) status = -4;    // QF_ERANK: repeated repair rows
    const bool ok = status == 0;
    if (ok && e > 0) {
        uint32_t ne = 0;
        for (uint32_t i0 = 0; i0 < k; i0 += 64) {
            const uint32_t i = i0 + lane;
            const bool miss = i < k && P.sys_slot[i] == 0xFF;
            const uint64_t bm = __ballot(miss);
            if (miss) P.Eidx[ne + __popcll(bm & lt_mask)] = (uint8_t)i;
            ne += __popcll(bm);
        }
        const bool accj = lane < r && P.rep_slot[lane] != 0xFF;
        const uint64_t bj = __ballot(accj);
        if (accj) {
            const uint32_t p = __popcll(bj & lt_mask);
            P.Js[p] = (uint8_t)lane;
            P.rank[lane] = (uint8_t)p;
        }
        wave_sync();
        // closed-form LU of A[b][c] = 1 / (x_b + y_c) (formulas at
        // k_decode_prepare_cauchy) through prefix sums of logs:
        //   P1[a][m] = sum_{q<m} log(x_a + x_q) - log(x_a + y_q)
        //   P2[a][m] = sum_{q<m} log(y_a + x_q) - log(y_a + y_q)
        //   L  (i > j): log(x_j + y_j) - log(x_i + y_j) + P1[i][j] - P1[j][j]
        //   U  (i = j): log(x_i + y_i) + P2[i][i] - P1[i][i]
        //   U' (i < j): log(x_i + y_i) - log(x_i + y_j) + P2[i][i] - P2[j][i]
        // (the q = a term, log 0, only enters prefixes past a, never read)
        uint32_t X[16], Y[16];
#pragma unroll
        for (uint32_t q = 0; q < 16; ++q) {
            X[q] = (k + P.Js[q]) & 0xFF;
            Y[q] = P.Eidx[q];
        }
        const uint32_t Xl = (k + P.Js[lane & 15]) & 0xFF, Yl = P.Eidx[lane & 15];
        {
            // lanes 0-15: P1 rows, 16-31: P2 rows, one prefix step per q
            const uint32_t which = (lane >> 4) & 1, ra = lane & 15;
            const uint32_t v = which ? Yl : Xl;
            int32_t acc = 0;
            if (lane < 32) P.PP[which][ra][0] = 0;
#pragma unroll
            for (uint32_t q = 0; q < 16; ++q) {
                if (q >= e) break;  // wave-uniform
                acc += (int32_t)slog[v ^ X[q]] - (int32_t)slog[v ^ Y[q]];
                if (lane < 32) P.PP[which][ra][q + 1] = (int16_t)acc;
            }
        }
        wave_sync();
#pragma unroll
        for (uint32_t pass = 0; pass < 4; ++pass) {
            const uint32_t t = lane + 64 * pass, i = t >> 4, j = t & 15;
            // x_i, y_i, x_j, y_j by lane permutes (lane q & 15 holds X[q], Y[q]);
            // taken with every lane active
            const uint32_t xi = __shfl(Xl, (int)i), yi = __shfl(Yl, (int)i);
            const uint32_t xj = __shfl(Xl, (int)j), yj = __shfl(Yl, (int)j);
            if (i >= e || j >= e) continue;
            const bool lo_ = i > j, di = i == j;
            const uint32_t u = lo_ ? (xj ^ yj) : (xi ^ yi);
            const int32_t t1 = lo_ ? P.PP[0][i][j] : P.PP[1][i][i];
            const int32_t t2 = lo_ ? P.PP[0][j][j] : (di ? P.PP[0][i][i] : P.PP[1][j][i]);
            const int32_t l0 = (int32_t)slog[u] - (di ? 0 : (int32_t)slog[xi ^ yj]) + t1 - t2;
            const uint32_t l = (uint32_t)(l0 + 64 * 255) % 255u;  // |t1 - t2| < 32 * 255
            P.LU[i][j] = sexp[l];
        }
        wave_sync();
    }
    // record: 16 columns x 16 bytes, then 16 rank bytes = 68 dwords, one
    // dword per lane (column u = d / 4, bytes t = 4 (d % 4) .. + 3): the
    // lookups of a lane are independent, so they overlap
    uint8_t* lo = a.lu_out + (uint64_t)g * a.lu_stride;
    for (uint32_t d = lane; d < 68; d += 64) {
        const uint32_t u = d >> 2, q = d & 3;
        const uint32_t ru = u < 16 ? P.rank[u] : 0xFF;
        uint32_t v = 0;
#pragma unroll
        for (uint32_t b = 0; b < 4; ++b) {
            const uint32_t t = 4 * q + b;
            const uint32_t rt = P.rank[t];
            uint32_t x;
            if (u == 16) x = ok ? rt : 0xFF;
            else x = (ok && rt != 0xFF && ru != 0xFF) ? P.LU[rt][ru] : 0;
            v |= x << (8 * b);
        }
        *reinterpret_cast<uint32_t*>(lo + 4 * d) = v;
    }
    uint8_t* sm = a.smap + (uint64_t)g * a.map_stride;
    for (uint32_t q = lane; q < a.map_stride; q += 64) {
        uint8_t v = 0xFF;
        if (ok) {
            if (q < k) v = P.sys_slot[q];
            else if (q < k + r) v = P.rep_slot[q - k];
        }
        sm[q] = v;
    }
    if (ok)
        for (uint32_t b = lane; b < e; b += 64) a.rec_index[(uint64_t)g * a.e_max + b] = P.Eidx[b];
    if (lane == 0) {
        a.status[g] = status;
        a.n_out[g] = ok ? e : 0;
    }
    wave_sync();  // P is rewritten for the next generation
    }
}

// ---------------------------------------------------------------------------
// The same decode control with one generation per LANE (k_decode_prepare_lu
// runs one per wave): a generation's acceptance is a scalar walk over its row
// indices, its closed-form LU ~3 e^2 table lookups, so a lane does it with
// the wave's other 63 generations in lockstep instead of 64 lanes sharing one
// through ballots, LDS atomics and wave barriers (~15x fewer wave
// instructions per generation).  The record and slot map of the block's
// generations are staged in LDS ([word][lane]: a lane's bytes land at
// data-dependent offsets) and written out coalesced; outputs are byte-equal
// to k_decode_prepare_lu's (tests/test_gpu_decode.py compares the two).
// ---------------------------------------------------------------------------
constexpr uint32_t kPrepLanes = 128;      // generations per block
constexpr uint32_t kPrepRecWords = 68;    // 272-B record
constexpr uint32_t kPrepMapWords = 64;    // slot map <= 256 B
constexpr uint32_t kPrepMaskWords = 8;    // accepted-source bits, k <= 256
// 768 B of tables + 72 KB of staging: fits gfx950's 160 KB LDS per CU (the
// library is built for gfx950 only, build_lib.ARCH)
static_assert(768 + 4 * (kPrepRecWords + kPrepMapWords + kPrepMaskWords) * kPrepLanes <= 160 * 1024,
              "k_decode_prepare_lu_lanes LDS exceeds the gfx950 CU");

__global__ void __launch_bounds__(kPrepLanes) k_decode_prepare_lu_lanes(PrepareCauchyArgs a) {
    __shared__ uint8_t sexp[512];
    __shared__ uint8_t slog[256];
    __shared__ __attribute__((aligned(16))) uint32_t srec[kPrepRecWords * kPrepLanes];
    __shared__ __attribute__((aligned(16))) uint32_t smp[kPrepMapWords * kPrepLanes];
    __shared__ __attribute__((aligned(16))) uint32_t sam[kPrepMaskWords * kPrepLanes];
    for (uint32_t i = threadIdx.x; i < 768; i += blockDim.x) {
        if (i < 512) sexp[i] = a.explog[i];
        else slog[i - 512] = a.explog[i];
    }
    const uint32_t tid = threadIdx.x, k = a.k, r = a.r;
    const uint32_t mw = a.map_stride / 4;
    uint8_t* rec8 = reinterpret_cast<uint8_t*>(srec);
    uint8_t* map8 = reinterpret_cast<uint8_t*>(smp);
    auto rec_b = [&](uint32_t byte) -> uint8_t& { return rec8[((byte >> 2) * kPrepLanes + tid) * 4 + (byte & 3)]; };
    auto map_b = [&](uint32_t byte) -> uint8_t& { return map8[((byte >> 2) * kPrepLanes + tid) * 4 + (byte & 3)]; };
    for (uint64_t g0 = (uint64_t)blockIdx.x * kPrepLanes; g0 < a.G; g0 += (uint64_t)gridDim.x * kPrepLanes) {
        __syncthreads();   // the tables (first pass) / the previous pass's copy-out
        const uint64_t g = g0 + tid;
        const bool live = g < a.G;
        // record: LU columns zero, rank bytes absent; map all absent (the
        // block fills them together, 16 bytes per write)
        {
            uint4* r4 = reinterpret_cast<uint4*>(srec);
            const uint32_t zero4 = 64 * kPrepLanes / 4, all4 = kPrepRecWords * kPrepLanes / 4;
            for (uint32_t i = tid; i < all4; i += kPrepLanes)
                r4[i] = i < zero4 ? make_uint4(0, 0, 0, 0) : make_uint4(~0u, ~0u, ~0u, ~0u);
            uint4* m4 = reinterpret_cast<uint4*>(smp);
            for (uint32_t i = tid; i < mw * kPrepLanes / 4; i += kPrepLanes) m4[i] = make_uint4(~0u, ~0u, ~0u, ~0u);
            uint4* a4 = reinterpret_cast<uint4*>(sam);
            for (uint32_t i = tid; i < kPrepMaskWords * kPrepLanes / 4; i += kPrepLanes) a4[i] = make_uint4(0, 0, 0, 0);
        }
        __syncthreads();
        int32_t status = 0;
        uint32_t e = 0;
        if (live) {
            // decoder.rs:679-699: rows in arrival order, the first k
            // candidates accepted; a systematic row only at its index's first
            // arrival, every valid repair row a candidate (a repeated one:
            // ERANK); any index >= k + r: EINVAL
            const uint32_t n = a.n_rows ? min(a.n_rows[g], a.max_rows) : a.max_rows;
            const uint16_t* ridx = a.row_index + g * a.max_rows;
            uint32_t accepted = 0, rep = 0;
            uint64_t acc64 = 0;
            bool bad = false, dup = false;
            auto step = [&](uint32_t s, uint32_t x) {
                if (k <= 64) {   // branch-free: the accepted-source bits in a register pair, one predicated store
                    const bool isrep = x >= k;
                    const uint32_t j = x - k;
                    const bool vrep = isrep && j < r;
                    bad |= isrep && !vrep;
                    const bool open = accepted < k;
                    const uint64_t bit = isrep ? 0ull : 1ull << (x & 63);
                    const bool sys_take = !isrep && open && !(acc64 & bit);
                    const bool rep_take = vrep && open;
                    acc64 |= sys_take ? bit : 0ull;
                    dup |= rep_take && ((rep >> (j & 31)) & 1u);
                    rep |= rep_take ? 1u << (j & 31) : 0u;
                    const bool take = sys_take || rep_take;
                    if (take) map_b(isrep ? k + j : x) = (uint8_t)s;
                    accepted += take ? 1u : 0u;
                    return;
                }
                if (x >= k) {
                    const uint32_t j = x - k;
                    if (j >= r) {
                        bad = true;
                        return;
                    }
                    if (accepted < k) {
                        dup |= (rep >> j) & 1u;
                        rep |= 1u << j;
                        map_b(k + j) = (uint8_t)s;
                        ++accepted;
                    }
                } else if (accepted < k) {
                    uint32_t& m = sam[(x >> 5) * kPrepLanes + tid];
                    const uint32_t bit = 1u << (x & 31);
                    if (!(m & bit)) {
                        m |= bit;
                        map_b(x) = (uint8_t)s;
                        ++accepted;
                    }
                }
            };
            // the row indices in chunks of 32, the next chunk's loads in
            // flight while this one is walked (one memory latency per chunk
            // instead of one per 8 rows)
            constexpr uint32_t kChunk = 32;
            uint32_t cur[kChunk], nxt[kChunk];
#pragma unroll
            for (uint32_t q = 0; q < kChunk; ++q) cur[q] = q < n ? ridx[q] : 0xFFFFu;
            for (uint32_t s0 = 0; s0 < n; s0 += kChunk) {
                const bool more = s0 + kChunk < n;
#pragma unroll
                for (uint32_t q = 0; q < kChunk; ++q) nxt[q] = more && s0 + kChunk + q < n ? ridx[s0 + kChunk + q] : 0xFFFFu;
#pragma unroll
                for (uint32_t q = 0; q < kChunk; ++q)
                    if (s0 + q < n) step(s0 + q, cur[q]);
#pragma unroll
                for (uint32_t q = 0; q < kChunk; ++q) cur[q] = nxt[q];
            }
            if (k <= 64) {
                sam[tid] = (uint32_t)acc64;
                sam[kPrepLanes + tid] = (uint32_t)(acc64 >> 32);
            }
            status = bad ? -1 : accepted < k ? -3 : dup ? -4 : 0;
            e = __popc(rep);
            if (status != 0) {
                for (uint32_t w = 0; w < mw; ++w) smp[w * kPrepLanes + tid] = 0xFFFFFFFFu;
            } else if (e > 0) {
                // J ascending (x = k + j), E = the erased sources ascending (y)
                uint32_t X[16], Y[16], J[16];
                {
                    uint32_t m = rep;
#pragma unroll
                    for (uint32_t q = 0; q < 16; ++q) {
                        J[q] = m ? (uint32_t)__builtin_ctz(m) : 0u;
                        X[q] = (k + J[q]) & 0xFF;
                        m &= m - 1;
                    }
                    uint32_t cw = 0, cm = ~sam[tid] & (k >= 32 ? 0xFFFFFFFFu : ((1u << k) - 1));
#pragma unroll
                    for (uint32_t q = 0; q < 16; ++q) {
                        while (cm == 0 && cw + 1 < (k + 31) / 32) {
                            ++cw;
                            const uint32_t lim = k - 32 * cw;
                            cm = ~sam[cw * kPrepLanes + tid] & (lim >= 32 ? 0xFFFFFFFFu : ((1u << lim) - 1));
                        }
                        Y[q] = cm ? 32 * cw + (uint32_t)__builtin_ctz(cm) : 0u;
                        cm &= cm - 1;
                    }
                }
#pragma unroll
                for (uint32_t q = 0; q < 16; ++q)
                    if (q < e) a.rec_index[g * a.e_max + q] = (uint16_t)Y[q];
                // closed-form LU of C[J, E] (as k_decode_prepare_lu): with
                //   P0[a][m] = sum_{q<m} log(x_a + x_q) - log(x_a + y_q),
                //   P1[a][m] = sum_{q<m} log(y_a + x_q) - log(y_a + y_q),
                //   L  (i > j): log(x_j + y_j) - log(x_i + y_j) + P0[i][j] - P0[j][j]
                //   U  (i = j): log(x_i + y_i) + P1[i][i] - P0[i][i]
                //   U' (i < j): log(x_i + y_i) - log(x_i + y_j) + P1[i][i] - P1[j][i]
                // row a of L and column a of U' come with the prefixes of row a
                int32_t S[16], D0[16], D1[16];
#pragma unroll
                for (uint32_t q = 0; q < 16; ++q) S[q] = slog[X[q] ^ Y[q]];
                auto put = [&](uint32_t i, uint32_t j, int32_t l0) {   // LU[i][j] -> column J[j], byte J[i]
                    const uint32_t l = (uint32_t)(l0 + 64 * 255) % 255u;
                    rec_b(16 * J[j] + J[i]) = sexp[l];
                };
                // (static trip counts, guarded by e: the loops unroll fully,
                // so X, Y, J, S, D0 and D1 stay in registers)
#pragma unroll
                for (uint32_t p = 0; p < 16; ++p) {
                    if (p < e) {
                        int32_t pp0 = 0, pp1 = 0;
#pragma unroll
                        for (uint32_t q = 0; q < p; ++q) {
                            const int32_t xx = slog[X[p] ^ X[q]], xy = slog[X[p] ^ Y[q]];
                            const int32_t yx = slog[Y[p] ^ X[q]], yy = slog[Y[p] ^ Y[q]];
                            put(p, q, S[q] - xy + pp0 - D0[q]);   // L[p][q]
                            put(q, p, S[q] - yx + D1[q] - pp1);   // U'[q][p]: log(x_q + y_p) = yx
                            pp0 += xx - xy;
                            pp1 += yx - yy;
                        }
                        D0[p] = pp0;
                        D1[p] = pp1;
                        put(p, p, S[p] + pp1 - pp0);
                    }
                }
#pragma unroll
                for (uint32_t q = 0; q < 16; ++q)
                    if (q < e) rec_b(256 + J[q]) = (uint8_t)q;   // rank of repair J[q]
            }
            a.status[g] = status;
            a.n_out[g] = status == 0 ? e : 0;
        }
        __syncthreads();
        // copy-out: the block's records and slot maps, contiguous runs
        const uint32_t ng = (uint32_t)min<uint64_t>(kPrepLanes, a.G - g0);
        if ((a.lu_stride & 3) == 0)
            for (uint32_t d = tid; d < ng * kPrepRecWords; d += kPrepLanes) {
                const uint32_t gl = d / kPrepRecWords, w = d - gl * kPrepRecWords;
                *reinterpret_cast<uint32_t*>(a.lu_out + (g0 + gl) * a.lu_stride + 4 * w) = srec[w * kPrepLanes + gl];
            }
        for (uint32_t d = tid; d < ng * mw; d += kPrepLanes) {
            const uint32_t gl = d / mw, w = d - gl * mw;
            *reinterpret_cast<uint32_t*>(a.smap + (g0 + gl) * a.map_stride + 4 * w) = smp[w * kPrepLanes + gl];
        }
    }
}

// ---------------------------------------------------------------------------
// Element-wise slice multiply and synthetic fill.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_mul_slice(const uint8_t* __restrict__ a,
                                                   const uint8_t* __restrict__ b,
                                                   uint8_t* __restrict__ out, uint64_t n,
                                                   const uint8_t* __restrict__ explog) {
    __shared__ uint8_t sexp[512];
    __shared__ uint8_t slog[256];
    for (uint32_t i = threadIdx.x; i < 768; i += blockDim.x) {
        if (i < 512) sexp[i] = explog[i];
        else slog[i - 512] = explog[i];
    }
    __syncthreads();
    const uint64_t nvec = n / 16;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < nvec; w += stride) {
        const uint4 va = reinterpret_cast<const uint4*>(a)[w];
        const uint4 vb = reinterpret_cast<const uint4*>(b)[w];
        uint4 r;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint32_t x = comp(va, c), y = comp(vb, c);
            uint32_t o = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t xa = (x >> (8 * q)) & 0xFF, yb = (y >> (8 * q)) & 0xFF;
                const uint32_t p = (xa && yb) ? sexp[(uint32_t)slog[xa] + slog[yb]] : 0u;
                o |= p << (8 * q);
            }
            set_comp(r, c, o);
        }
        reinterpret_cast<uint4*>(out)[w] = r;
    }
    // tail bytes
    const uint64_t t0 = nvec * 16;
    for (uint64_t t = t0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride) {
        const uint32_t xa = a[t], yb = b[t];
        out[t] = (xa && yb) ? sexp[(uint32_t)slog[xa] + slog[yb]] : 0;
    }
}

// Large slices: the whole 64 KiB product table T[a * 256 + b] in LDS (built
// per block from exp/log), one LDS byte read per product and no branches;
// index pairs are formed two at a time with v_perm.  Persistent grid.
__global__ void __launch_bounds__(1024) k_mul_slice_tab(const uint8_t* __restrict__ a,
                                                        const uint8_t* __restrict__ b,
                                                        uint8_t* __restrict__ out, uint64_t n,
                                                        const uint8_t* __restrict__ explog) {
    __shared__ uint8_t sexp[512];
    __shared__ uint8_t slog[256];
    __shared__ __attribute__((aligned(16))) uint8_t tab[65536];
    for (uint32_t i = threadIdx.x; i < 768; i += blockDim.x) {
        if (i < 512) sexp[i] = explog[i];
        else slog[i - 512] = explog[i];
    }
    __syncthreads();
    for (uint32_t w = threadIdx.x; w < 65536 / 4; w += blockDim.x) {
        uint32_t v = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t t = 4 * w + q, xa = t >> 8, yb = t & 0xFF;
            const uint32_t p = (xa && yb) ? sexp[(uint32_t)slog[xa] + slog[yb]] : 0u;
            v |= p << (8 * q);
        }
        reinterpret_cast<uint32_t*>(tab)[w] = v;
    }
    __syncthreads();
    const uint64_t nvec = n / 16;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < nvec; w += stride) {
        const uint4 va = reinterpret_cast<const uint4*>(a)[w];
        const uint4 vb = reinterpret_cast<const uint4*>(b)[w];
        uint4 r;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint32_t x = comp(va, c), y = comp(vb, c);
            // indices (a_q << 8 | b_q) for bytes 0,1 and 2,3 of the dword
            const uint32_t i01 = vperm(x, y, 0x05010400u);  // bytes: b0 a0 b1 a1
            const uint32_t i23 = vperm(x, y, 0x07030602u);  // bytes: b2 a2 b3 a3
            const uint32_t p0 = tab[i01 & 0xFFFF], p1 = tab[i01 >> 16];
            const uint32_t p2 = tab[i23 & 0xFFFF], p3 = tab[i23 >> 16];
            set_comp(r, c, p0 | (p1 << 8) | (p2 << 16) | (p3 << 24));
        }
        reinterpret_cast<uint4*>(out)[w] = r;
    }
    const uint64_t t0 = nvec * 16;
    for (uint64_t t = t0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride)
        out[t] = tab[(uint32_t)a[t] << 8 | b[t]];
}

// (splitmix64: qf_kernels.h, shared with k_recode_prepare)
__global__ void __launch_bounds__(256) k_fill_splitmix(uint8_t* __restrict__ dst, uint64_t n,
                                                       uint64_t seed, uint64_t word_offset) {
    const uint64_t nw = n / 8;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const bool aligned = (reinterpret_cast<uintptr_t>(dst) & 7) == 0;
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < nw; w += stride) {
        const uint64_t v = splitmix64(seed + word_offset + w);
        if (aligned) {
            reinterpret_cast<uint64_t*>(dst)[w] = v;
        } else {
            for (int q = 0; q < 8; ++q) dst[w * 8 + q] = (uint8_t)(v >> (8 * q));
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && nw * 8 < n) {
        const uint64_t v = splitmix64(seed + word_offset + nw);
        for (uint64_t t = nw * 8; t < n; ++t) dst[t] = (uint8_t)(v >> (8 * (t - nw * 8)));
    }
}

// ---------------------------------------------------------------------------
// Launch wrappers (host).
// ---------------------------------------------------------------------------
template <int R, int V, int PD>
static hipError_t launch_uniform_rvp(const CombineUniformArgs& a, int num_cus, hipStream_t st) {
    const size_t lds = (size_t)a.k_pad * R * 32;
    auto kern = k_combine_uniform<R, V, PD>;
    static bool attr_done = false;
    if (!attr_done) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
        attr_done = true;
    }
    int occ = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kern, 256, lds);
    if (e != hipSuccess) return e;
    if (occ < 1) return hipErrorInvalidConfiguration;
    const uint64_t waves = (a.total_units + 64 * V - 1) / (64 * V);
    uint64_t blocks = (waves + 3) / 4;
    const uint64_t cap = (uint64_t)num_cus * occ;
    if (blocks > cap) blocks = cap;
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(kern, dim3((uint32_t)blocks), dim3(256), lds, st, a);
    return hipGetLastError();
}

template <int V, int PD>
static hipError_t launch_uniform_vp(const CombineUniformArgs& a, int R, int num_cus, hipStream_t st) {
    switch (R) {
        case 1: return launch_uniform_rvp<1, V, PD>(a, num_cus, st);
        case 2: return launch_uniform_rvp<2, V, PD>(a, num_cus, st);
        case 4: return launch_uniform_rvp<4, V, PD>(a, num_cus, st);
        case 8: return launch_uniform_rvp<8, V, PD>(a, num_cus, st);
        // 16 outputs x 2 units do not fit 256 VGPRs without spilling the
        // in-flight buffers: R = 16 always runs one unit per lane.
        case 16: return launch_uniform_rvp<16, 1, PD>(a, num_cus, st);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_combine_uniform(const CombineUniformArgs& a, int R, int V, int PD, int num_cus,
                                  hipStream_t st) {
    if (V == 2) {
        if (PD == 1) return launch_uniform_vp<2, 1>(a, R, num_cus, st);
        if (PD == 2) return launch_uniform_vp<2, 2>(a, R, num_cus, st);
    } else {
        if (PD == 1) return launch_uniform_vp<1, 1>(a, R, num_cus, st);
        if (PD == 2) return launch_uniform_vp<1, 2>(a, R, num_cus, st);
        if (PD == 3) return launch_uniform_vp<1, 3>(a, R, num_cus, st);
    }
    return hipErrorInvalidValue;
}

template <int PD>
static hipError_t launch_slots_p(const CombineSlotsArgs& a, int num_cus, hipStream_t st) {
    auto kern = k_combine_slots<PD>;
    int occ = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kern, 256, 0);
    if (e != hipSuccess) return e;
    if (occ < 1) occ = 1;
    const uint64_t waves = (a.total_units + 63) / 64;
    uint64_t blocks = (waves + 3) / 4;
    const uint64_t cap = (uint64_t)num_cus * occ;
    if (blocks > cap) blocks = cap;
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(kern, dim3((uint32_t)blocks), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_combine_slots(const CombineSlotsArgs& a, int PD, int num_cus, hipStream_t st, bool split_ok) {
    // at most one 64-unit wave-item per CU: the slot-split kernel, unless
    // the context's QF_OPT_COMBINE_SPLIT is 0 (split_ok)
    const uint64_t items = (a.total_units + 63) / 64;
    if (split_ok && num_cus > 0 && items <= (uint64_t)num_cus) {
        if (items == 0) return hipSuccess;
        hipLaunchKernelGGL(k_combine_slots_split, dim3((uint32_t)items), dim3(256), 0, st, a);
        return hipGetLastError();
    }
    if (PD == 1) return launch_slots_p<1>(a, num_cus, st);
    if (PD == 2) return launch_slots_p<2>(a, num_cus, st);
    if (PD == 3) return launch_slots_p<3>(a, num_cus, st);
    return hipErrorInvalidValue;
}

size_t prepare_lds_bytes(uint32_t k, uint32_t e_max, uint32_t max_rows) {
    const uint32_t max_rows_pad = (max_rows + 7) & ~7u;
    return 768 + 4 * 256 + 2 * 256 * 5 + 2 * (size_t)max_rows_pad + (size_t)e_max * (k + e_max) + 16;
}

hipError_t launch_decode_prepare(const PrepareArgs& a, hipStream_t st) {
    const size_t lds = prepare_lds_bytes(a.k, a.e_lds, a.max_rows);
    static bool attr_done = false;
    if (!attr_done) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_decode_prepare<false>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e == hipSuccess)
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_decode_prepare<true>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
        attr_done = true;
    }
    if (a.G == 0) return hipSuccess;
    if (a.row_off) {
        // rows by offset: pair records, and the accepted rows must fit them
        if (!a.row_len || !a.min_len || (a.src_gen_stride & 15) || (a.coef_gen_stride & 15) ||
            a.coef_gen_stride < ((uint64_t)((a.k < a.max_rows ? a.k : a.max_rows) + 1) / 2 + 1) * kPairRecBytes)
            return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_decode_prepare<true>, dim3(a.G), dim3(64), lds, st, a);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(k_decode_prepare<false>, dim3(a.G), dim3(64), lds, st, a);
    return hipGetLastError();
}

// Syndromes through the encode kernels (codes with more repairs than a
// syndrome kernel holds): the accepted systematic rows of each generation in
// source order, erased sources zero (k_gather_sources); the bit-sliced encode
// of that gives C x' = C[., S] x_S; XOR the accepted repair rows in
// (k_xor_repairs): s_J = p_J ^ C[J, S] x_S.
__global__ void __launch_bounds__(256) k_gather_sources(GatherArgs a) {
    const uint64_t total = (uint64_t)a.G * a.k * a.Lu;
    for (uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; f < total;
         f += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t t = f / a.Lu;
        const uint32_t u = (uint32_t)(f - t * a.Lu);
        const uint64_t g = t / a.k;
        const uint32_t i = (uint32_t)(t - g * a.k);
        const uint32_t slot = a.smap[g * a.map_stride + i];
        uint4 v = make_uint4(0, 0, 0, 0);
        if (slot != 0xFF)
            v = *reinterpret_cast<const uint4*>(gen_base(a.rows, g, a.rows_gen_stride, a.rows_offs) +
                                                slot * a.row_stride + 16ull * u);
        *reinterpret_cast<uint4*>(a.out + g * a.out_gen_stride + i * a.out_row_stride + 16ull * u) = v;
    }
}

__global__ void __launch_bounds__(256) k_xor_repairs(GatherArgs a) {
    const uint64_t total = (uint64_t)a.G * a.r * a.Lu;
    for (uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; f < total;
         f += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t t = f / a.Lu;
        const uint32_t u = (uint32_t)(f - t * a.Lu);
        const uint64_t g = t / a.r;
        const uint32_t j = (uint32_t)(t - g * a.r);
        const uint32_t slot = a.smap[g * a.map_stride + a.k + j];
        if (slot == 0xFF) continue;
        const uint4 p = *reinterpret_cast<const uint4*>(gen_base(a.rows, g, a.rows_gen_stride, a.rows_offs) +
                                                        slot * a.row_stride + 16ull * u);
        uint4* s = reinterpret_cast<uint4*>(a.out + g * a.out_gen_stride + j * a.out_row_stride + 16ull * u);
        uint4 v = *s;
        v.x ^= p.x;
        v.y ^= p.y;
        v.z ^= p.z;
        v.w ^= p.w;
        *s = v;
    }
}

hipError_t launch_gather_sources(const GatherArgs& a, int num_cus, hipStream_t st) {
    const uint64_t total = (uint64_t)a.G * a.k * a.Lu;
    if (!total) return hipSuccess;
    const uint64_t blocks = std::min<uint64_t>((total + 255) / 256, (uint64_t)num_cus * 16);
    hipLaunchKernelGGL(k_gather_sources, dim3((uint32_t)blocks), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_xor_repairs(const GatherArgs& a, int num_cus, hipStream_t st) {
    const uint64_t total = (uint64_t)a.G * a.r * a.Lu;
    if (!total) return hipSuccess;
    const uint64_t blocks = std::min<uint64_t>((total + 255) / 256, (uint64_t)num_cus * 16);
    hipLaunchKernelGGL(k_xor_repairs, dim3((uint32_t)blocks), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_decode_prepare_cauchy(const PrepareCauchyArgs& a, hipStream_t st) {
    if (a.G == 0) return hipSuccess;
    // fused decode records: r <= 16; stage-B records: r <= 64 (e <= 64)
    if (a.r > (a.lu_out ? 16u : 64u) || a.e_max > 64 || a.k + a.r > 256 || a.max_rows > 255 ||
        a.map_stride < a.k + a.r)
        return hipErrorInvalidValue;
    if (a.lu_out) {
        // one generation per wave (a persistent grid measured slower: the
        // kernel is LDS/VALU-issue-bound per CU, not launch-bound)
        uint32_t blocks = (a.G + kPrepWaves - 1) / kPrepWaves;
        // a capped persistent grid when the pass runs beside other work
        // (split-phase decode): fewer CUs taken from the concurrent kernel
        if (a.grid_cap && blocks > a.grid_cap) blocks = a.grid_cap;
        if (a.lanes && a.G >= 2048 && a.map_stride <= 4 * kPrepMapWords && a.lu_stride % 4 == 0 &&
            a.lu_stride >= 4 * kPrepRecWords) {
            // one generation per lane (the same grid cap, in 128-generation
            // blocks); small batches keep a wave per generation: a lane's
            // walk is serial, so one generation alone finishes sooner on 64
            // lanes (the per-packet decode)
            uint32_t lb = (a.G + kPrepLanes - 1) / kPrepLanes;
            if (a.grid_cap && lb > a.grid_cap) lb = a.grid_cap;
            hipLaunchKernelGGL(k_decode_prepare_lu_lanes, dim3(lb), dim3(kPrepLanes), 0, st, a);
        } else {
            hipLaunchKernelGGL(k_decode_prepare_lu, dim3(blocks), dim3(64 * kPrepWaves), 0, st, a);
        }
    } else {
        hipLaunchKernelGGL(k_decode_prepare_cauchy, dim3(a.G), dim3(64), 0, st, a);
    }
    return hipGetLastError();
}

hipError_t launch_mul_slice(const uint8_t* a, const uint8_t* b, uint8_t* out, uint64_t n,
                            const uint8_t* explog, int num_cus, hipStream_t st) {
    uint64_t blocks = (n / 16 + 255) / 256;
    if (blocks < 1) blocks = 1;
    const uint64_t cap = (uint64_t)num_cus * 8;
    if (blocks > cap) blocks = cap;
    // from 16 MiB the table kernel (one LDS read per product) wins; below, the
    // 64 KiB per-block table build is not amortised
    if (n >= (16u << 20)) {
        hipLaunchKernelGGL(k_mul_slice_tab, dim3((uint32_t)num_cus), dim3(1024), 0, st, a, b, out, n, explog);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(k_mul_slice, dim3((uint32_t)blocks), dim3(256), 0, st, a, b, out, n, explog);
    return hipGetLastError();
}

hipError_t launch_fill_splitmix(uint8_t* dst, uint64_t n, uint64_t seed, uint64_t word_offset,
                                int num_cus, hipStream_t st) {
    uint64_t blocks = (n / 8 + 255) / 256;
    if (blocks < 1) blocks = 1;
    const uint64_t cap = (uint64_t)num_cus * 8;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(k_fill_splitmix, dim3((uint32_t)blocks), dim3(256), 0, st, dst, n, seed,
                       word_offset);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Small-batch encode: the bit-sliced kernels run one wave per 128 units, so a
// single 1 KiB window (AdaptiveFec::on_send -> generate_repair_packet,
// adaptive.rs:546-562, decoder.rs:172-275) was one wave doing all k rows x r
// repairs (60 us per pass at k = 128).  Here a block takes one (generation,
// repair, 64 units) tile, its four waves split the k rows, and a lane sums
// its quarter with split-table products (v_perm, records of gf256_tables.h in
// LDS); the loop is memory-latency-bound at this size, so each batch of 8
// rows has all its loads in flight before its products.
// ---------------------------------------------------------------------------
// system-scope 16-byte store into host-coherent memory (fused send)
QF_DEV void store_sys16(uint8_t* p, const uint4& v) {
    v4u x = {v.x, v.y, v.z, v.w};
    // (s_nop: the store's data VGPRs are not rewritten in the next cycle)
    asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" : : "v"(p), "v"(x) : "memory");
}

__global__ void __launch_bounds__(256) k_encode_small(EncodeSmallArgs a) {
    // tile = (generation g, repair j, 64 consecutive units); the block's four
    // waves take a quarter of the k rows each (batches of 8 rows whose loads
    // are all in flight before the products), then reduce through LDS
    __shared__ __attribute__((aligned(16))) uint32_t tab[256 * 8];
    __shared__ uint4 part[3][64];
    {
        const uint4* g = reinterpret_cast<const uint4*>(a.tab256);
        uint4* l = reinterpret_cast<uint4*>(tab);
        for (uint32_t w = threadIdx.x; w < 256 * 2; w += blockDim.x) l[w] = g[w];
    }
    __syncthreads();
    const uint8_t* tb = reinterpret_cast<const uint8_t*>(tab);
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t ut = (a.Lu + 63) / 64;                     // unit tiles per row
    const uint64_t tiles = (uint64_t)a.G * a.r * ut;
    const uint32_t kc = ((a.k + 3) / 4 + 7) & ~7u;            // rows per wave (multiple of 8)
    const uint32_t i0 = wv * kc, i1 = min(a.k, i0 + kc);
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t gj = t / ut;
        const uint32_t u = (uint32_t)(t - gj * ut) * 64 + lane;
        const uint64_t g = gj / a.r;
        const uint32_t j = (uint32_t)(gj - g * a.r);
        uint32_t L = a.L, rot = a.rot;
        uint64_t srs = a.src_row_stride, rrs = a.rep_row_stride;
        const uint8_t* sbase;
        uint8_t* rbase;
        if (a.wins) {   // one ring window per generation (send batches)
            const RingWin w = a.wins[g];
            L = w.L;
            rot = w.rot;
            srs = w.src_row_stride;
            rrs = w.rep_row_stride;
            sbase = a.src + w.src_off;
            rbase = a.rep + w.rep_off;
        } else {
            sbase = gen_base(a.src, g, a.src_gen_stride, a.src_offs);
            rbase = gen_base(a.rep, g, a.rep_gen_stride, a.rep_offs);
        }
        const bool act = 16 * u < L;
        const uint32_t nb = act ? min(16u, L - 16 * u) : 0u;
        const uint8_t* sp = sbase + 16ull * (act ? u : 0);
        const uint8_t* cp = a.coef + (uint64_t)j * a.k;
        uint4 acc = make_uint4(0, 0, 0, 0);
        for (uint32_t ib = i0; ib < i1; ib += 8) {
            uint4 x[8];
            uint32_t c[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const uint32_t i = ib + q;
                const bool ok = act && i < i1;
                const uint32_t row = i + rot >= a.k ? i + rot - a.k : i + rot;
                x[q] = ok ? load_unit(sp + (uint64_t)row * srs, nb) : make_uint4(0, 0, 0, 0);
                c[q] = (i < i1) ? ((uint32_t)cp[i] << 5) : 0u;    // record 0: zero products
            }
#pragma unroll
            for (int q = 0; q < 8; q += 2) {
                const uint4 A = *reinterpret_cast<const uint4*>(tb + c[q]);
                const uint32_t a2 = *reinterpret_cast<const uint32_t*>(tb + c[q] + 16);
                const uint4 B = *reinterpret_cast<const uint4*>(tb + c[q + 1]);
                const uint32_t b2 = *reinterpret_cast<const uint32_t*>(tb + c[q + 1] + 16);
                fma_pair(acc, A, a2, selectors(x[q]), B, b2, selectors(x[q + 1]));
            }
        }
        if (wv > 0) part[wv - 1][lane] = acc;
        __syncthreads();
        if (wv == 0 && act) {
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const uint4 p = part[q][lane];
                acc.x ^= p.x;
                acc.y ^= p.y;
                acc.z ^= p.z;
                acc.w ^= p.w;
            }
            store_unit(rbase + (uint64_t)j * rrs + 16ull * u, acc, nb);
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// Fused per-packet send (AdaptiveFec::on_send -> emit_repairs for one
// connection, adaptive.rs:519-562): the packet that completes the window
// travels in the kernel arguments (SEND_PKT_UNITS 16-byte units), block 0 puts
// it into its ring slot, and the repairs go straight to a host-coherent
// buffer -- one launch instead of copy + encode + copy.  A block = (repair j,
// 64 units); its four waves split the rows and issue all their loads (up to
// 16 at a time) together with the split-table copy, then sum, reduce through
// LDS and store with system-scope stores.
// ---------------------------------------------------------------------------
struct SendWinArgs {
    EncodeSmallArgs a;
    uint4 pkt[SEND_PKT_UNITS];
};

__global__ void __launch_bounds__(256) k_send_window(SendWinArgs p) {
    const EncodeSmallArgs& a = p.a;
    __shared__ __attribute__((aligned(16))) uint32_t tab[256 * 8];
    __shared__ uint4 part[3][64];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t ut = (a.Lu + 63) / 64;
    const uint32_t t = blockIdx.x;   // one tile per block
    const uint32_t j = t / ut, u = (t - j * ut) * 64 + lane;
    const bool act = 16 * u < a.L;
    const uint32_t kc = (a.k + 3) / 4, i0 = min(a.k, wv * kc), i1 = min(a.k, i0 + kc);
    const uint8_t* sp = a.src + 16ull * (act ? u : 0);
    const uint8_t* cp = a.coef + (uint64_t)j * a.k;
    // split tables: global loads now, into LDS after the row loads are issued
    const uint4* gt = reinterpret_cast<const uint4*>(a.tab256);
    const uint4 t0 = gt[threadIdx.x], t1 = gt[threadIdx.x + 256];
    uint4 acc = make_uint4(0, 0, 0, 0);
    bool tab_ready = false;
    for (uint32_t ib = i0; ib < i1; ib += 16) {
        uint4 x[16];
        uint32_t c[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const uint32_t i = ib + q;
            const bool ok = act && i < i1;
            const uint32_t row = i + a.rot >= a.k ? i + a.rot - a.k : i + a.rot;
            if (i == a.k - 1)   // the new packet (window position k - 1)
                x[q] = ok ? p.pkt[u] : make_uint4(0, 0, 0, 0);
            else
                x[q] = ok ? *reinterpret_cast<const uint4*>(sp + (uint64_t)row * a.src_row_stride)
                          : make_uint4(0, 0, 0, 0);
            c[q] = (i < i1) ? ((uint32_t)cp[i] << 5) : 0u;   // record 0: zero products
        }
        if (!tab_ready) {
            reinterpret_cast<uint4*>(tab)[threadIdx.x] = t0;
            reinterpret_cast<uint4*>(tab)[threadIdx.x + 256] = t1;
            __syncthreads();
            tab_ready = true;
        }
        const uint8_t* tb = reinterpret_cast<const uint8_t*>(tab);
#pragma unroll
        for (int q = 0; q < 16; q += 2) {
            const uint4 A = *reinterpret_cast<const uint4*>(tb + c[q]);
            const uint32_t a2 = *reinterpret_cast<const uint32_t*>(tb + c[q] + 16);
            const uint4 B = *reinterpret_cast<const uint4*>(tb + c[q + 1]);
            const uint32_t b2 = *reinterpret_cast<const uint32_t*>(tb + c[q + 1] + 16);
            fma_pair(acc, A, a2, selectors(x[q]), B, b2, selectors(x[q + 1]));
        }
    }
    // every wave passes one table barrier (waves without rows too; the
    // condition is wave-uniform)
    if (!tab_ready) {
        reinterpret_cast<uint4*>(tab)[threadIdx.x] = t0;
        reinterpret_cast<uint4*>(tab)[threadIdx.x + 256] = t1;
        __syncthreads();
    }
    if (wv > 0) part[wv - 1][lane] = acc;
    __syncthreads();
    if (wv == 0 && act) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const uint4 pp = part[q][lane];
            acc.x ^= pp.x;
            acc.y ^= pp.y;
            acc.z ^= pp.z;
            acc.w ^= pp.w;
        }
        store_sys16(a.rep + (uint64_t)j * a.rep_row_stride + 16ull * u, acc);   // rows >= 16 Lu bytes
    }
    if (blockIdx.x == 0)   // the new packet into its ring slot
        for (uint32_t v = threadIdx.x; v < a.fresh_units; v += blockDim.x)
            *reinterpret_cast<uint4*>(a.fresh_dst + 16ull * v) = p.pkt[v];
}

hipError_t launch_send_window(const EncodeSmallArgs& a, const uint8_t* pkt, uint32_t pkt_bytes, hipStream_t st) {
    if (!a.fresh_dst || a.G != 1 || a.k == 0 || a.r == 0 || a.Lu == 0 || a.fresh_units > SEND_PKT_UNITS ||
        a.Lu > a.fresh_units || pkt_bytes > 16u * a.fresh_units)
        return hipErrorInvalidValue;
    SendWinArgs p;
    p.a = a;
    memset(p.pkt, 0, 16u * a.fresh_units);
    if (pkt_bytes) memcpy(p.pkt, pkt, pkt_bytes);
    const uint32_t blocks = a.r * ((a.Lu + 63) / 64);
    hipLaunchKernelGGL(k_send_window, dim3(blocks), dim3(256), 0, st, p);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Send batches (qf_adaptive_on_send_batch): many windows, each with its own
// ring rotation and length.  k_encode_small gives a tile one repair, so a
// window's ring is read r times; here a tile = (window, 64 units, RC
// repairs): each source unit is loaded once per tile and feeds RC
// accumulators.  The block's four waves split the k rows, the coefficient
// bytes are wave-uniform (scalar loads), their split-table records LDS
// broadcasts.  Ring rows are zero padded to their 16-byte stride, so every
// active lane loads whole units; only the store is cut at L.
// ---------------------------------------------------------------------------
template <int RC>
__global__ void __launch_bounds__(256) k_encode_windows(EncodeSmallArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t tab[256 * 8];
    __shared__ uint4 part[3][RC][64];
    {
        const uint4* g = reinterpret_cast<const uint4*>(a.tab256);
        uint4* l = reinterpret_cast<uint4*>(tab);
        for (uint32_t w = threadIdx.x; w < 256 * 2; w += blockDim.x) l[w] = g[w];
    }
    __syncthreads();
    const uint8_t* tb = reinterpret_cast<const uint8_t*>(tab);
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t ut = (a.Lu + 63) / 64, nj = (a.r + RC - 1) / RC;
    const uint64_t tiles = (uint64_t)a.G * ut * nj;
    const uint32_t kc = ((a.k + 3) / 4 + 1) & ~1u;   // rows per wave (even)
    const uint32_t i0 = min(a.k, wv * kc), i1 = min(a.k, i0 + kc);
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t g = t / ((uint64_t)ut * nj);
        const uint32_t rem = (uint32_t)(t - g * ut * nj);
        const uint32_t jc = rem / ut, u = (rem - jc * ut) * 64 + lane;
        const RingWin w = a.wins[g];
        const bool act = 16 * u < w.L;
        const uint8_t* sp = a.src + w.src_off + 16ull * u;
        const uint8_t* cp = a.coef + (uint64_t)jc * RC * a.k;
        const uint32_t jn = min((uint32_t)RC, a.r - jc * RC);
        uint4 acc[RC];
#pragma unroll
        for (int j = 0; j < RC; ++j) acc[j] = make_uint4(0, 0, 0, 0);
        for (uint32_t i = i0; i < i1; i += 2) {
            const bool two = i + 1 < i1;
            const uint32_t ra = i + w.rot >= a.k ? i + w.rot - a.k : i + w.rot;
            const uint32_t rb = ra + 1 == a.k ? 0 : ra + 1;
            uint4 xa = make_uint4(0, 0, 0, 0), xb = make_uint4(0, 0, 0, 0);
            if (act) {
                xa = *reinterpret_cast<const uint4*>(sp + (uint64_t)ra * w.src_row_stride);
                if (two) xb = *reinterpret_cast<const uint4*>(sp + (uint64_t)rb * w.src_row_stride);
            }
            const Sel sa = selectors(xa), sb = selectors(xb);
#pragma unroll
            for (int j = 0; j < RC; ++j) {
                // rows past the chunk's repairs / the wave's rows: record 0 (zero products)
                const uint32_t ca = (uint32_t)j < jn ? (uint32_t)cp[(uint64_t)j * a.k + i] << 5 : 0u;
                const uint32_t cb = ((uint32_t)j < jn && two) ? (uint32_t)cp[(uint64_t)j * a.k + i + 1] << 5 : 0u;
                const uint4 A = *reinterpret_cast<const uint4*>(tb + ca);
                const uint32_t a2 = *reinterpret_cast<const uint32_t*>(tb + ca + 16);
                const uint4 B = *reinterpret_cast<const uint4*>(tb + cb);
                const uint32_t b2 = *reinterpret_cast<const uint32_t*>(tb + cb + 16);
                fma_pair(acc[j], A, a2, sa, B, b2, sb);
            }
        }
        if (wv > 0) {
#pragma unroll
            for (int j = 0; j < RC; ++j) part[wv - 1][j][lane] = acc[j];
        }
        __syncthreads();
        if (wv == 0 && act) {
            const uint32_t nb = min(16u, w.L - 16 * u);
            uint8_t* dp = a.rep + w.rep_off + 16ull * u;
#pragma unroll
            for (int j = 0; j < RC; ++j) {
                if ((uint32_t)j >= jn) continue;
                uint4 v = acc[j];
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const uint4 p = part[q][j][lane];
                    v.x ^= p.x;
                    v.y ^= p.y;
                    v.z ^= p.z;
                    v.w ^= p.w;
                }
                store_unit(dp + (uint64_t)(jc * RC + j) * w.rep_row_stride, v, nb);
            }
        }
        __syncthreads();
    }
}

hipError_t launch_encode_windows(const EncodeSmallArgs& a, int num_cus, hipStream_t st) {
    if (!a.wins || a.k == 0 || a.r == 0 || a.G == 0 || a.Lu == 0) return hipSuccess;
    // at most 8 accumulators per lane (more spill); r split into equal chunks
    const uint32_t ut = (a.Lu + 63) / 64, chunks = (a.r + 7) / 8, per = (a.r + chunks - 1) / chunks;
    const int RC = per <= 2 ? 2 : per <= 3 ? 3 : per <= 4 ? 4 : per <= 5 ? 5 : per <= 6 ? 6 : 8;
    const uint64_t tiles = (uint64_t)a.G * ut * ((a.r + RC - 1) / RC);
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(tiles, (uint64_t)num_cus * 8);
    switch (RC) {
        case 2: hipLaunchKernelGGL(k_encode_windows<2>, dim3(blocks), dim3(256), 0, st, a); break;
        case 3: hipLaunchKernelGGL(k_encode_windows<3>, dim3(blocks), dim3(256), 0, st, a); break;
        case 4: hipLaunchKernelGGL(k_encode_windows<4>, dim3(blocks), dim3(256), 0, st, a); break;
        case 5: hipLaunchKernelGGL(k_encode_windows<5>, dim3(blocks), dim3(256), 0, st, a); break;
        case 6: hipLaunchKernelGGL(k_encode_windows<6>, dim3(blocks), dim3(256), 0, st, a); break;
        default: hipLaunchKernelGGL(k_encode_windows<8>, dim3(blocks), dim3(256), 0, st, a); break;
    }
    return hipGetLastError();
}

// send batches: block m copies packet m into its ring slot(s), zero padded
__global__ void __launch_bounds__(128) k_ring_scatter(const uint8_t* stage, const RingSlot* slots, uint32_t M) {
    for (uint32_t m = blockIdx.x; m < M; m += gridDim.x) {
        const RingSlot s = slots[m];
        const uint32_t have = (s.len + 15) / 16, units = s.stride / 16;
        for (uint32_t v = threadIdx.x; v < units; v += blockDim.x) {
            const uint4 x = v < have ? *reinterpret_cast<const uint4*>(stage + s.src_off + 16ull * v)
                                     : make_uint4(0, 0, 0, 0);
            *reinterpret_cast<uint4*>(s.dst + 16ull * v) = x;
            if (s.dst2) *reinterpret_cast<uint4*>(s.dst2 + 16ull * v) = x;
        }
    }
}

hipError_t launch_ring_scatter(const uint8_t* stage, const RingSlot* slots, uint32_t M, hipStream_t st) {
    if (!M) return hipSuccess;
    hipLaunchKernelGGL(k_ring_scatter, dim3(std::min<uint32_t>(M, 4096)), dim3(128), 0, st, stage, slots, M);
    return hipGetLastError();
}

hipError_t launch_encode_small(const EncodeSmallArgs& a, int num_cus, hipStream_t st) {
    const uint64_t tiles = (uint64_t)a.G * a.r * ((a.Lu + 63) / 64);
    if (!tiles || a.k == 0) return hipSuccess;
    const uint64_t blocks = std::min<uint64_t>(tiles, (uint64_t)num_cus * 8);
    hipLaunchKernelGGL(k_encode_small, dim3((uint32_t)blocks), dim3(256), 0, st, a);
    return hipGetLastError();
}

// --- heterogeneous decode batches: metadata gather / scatter -----------------
__global__ void __launch_bounds__(256) k_desc_gather_index(DescIndexArgs a) {
    const uint64_t total = (uint64_t)a.G * a.max_rows;
    for (uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; f < total;
         f += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t g = f / a.max_rows;
        const uint32_t s = (uint32_t)(f - g * a.max_rows);
        a.out[f] = s < a.n_rows[g] ? a.row_index[a.ri_off[g] + s] : (uint16_t)0;
    }
}

__global__ void __launch_bounds__(256) k_desc_scatter_out(DescOutArgs a) {
    const uint32_t w = a.emax + 1;
    const uint64_t total = (uint64_t)a.G * w;
    for (uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; f < total;
         f += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t g = f / w;
        const uint32_t m = (uint32_t)(f - g * w);
        if (m < a.emax) {
            a.rec_index[a.rec_index_off[g] + m] = a.rec_index_ws[g * a.emax + m];
        } else {
            a.n_rec[a.desc_id[g]] = a.n_rec_ws[g];
            a.status[a.desc_id[g]] = a.status_ws[g];
        }
    }
}

hipError_t launch_desc_gather_index(const DescIndexArgs& a, hipStream_t st) {
    const uint64_t total = (uint64_t)a.G * a.max_rows;
    if (!total) return hipSuccess;
    const uint64_t blocks = std::min<uint64_t>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(k_desc_gather_index, dim3((uint32_t)blocks), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_desc_scatter_out(const DescOutArgs& a, hipStream_t st) {
    const uint64_t total = (uint64_t)a.G * (a.emax + 1);
    if (!total) return hipSuccess;
    const uint64_t blocks = std::min<uint64_t>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(k_desc_scatter_out, dim3((uint32_t)blocks), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace qf
