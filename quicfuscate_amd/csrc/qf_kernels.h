// qf_kernels.h -- kernel argument blocks and launch wrappers (internal).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qf {

// Encode / uniform combination:
//   dst[g][j] = XOR_i C[j][i] * src[g][i]   for j < r_active, i < k
// tabs: k_pad * R records of 8 dwords, record (i, j) at (i*R + j)*8, zero
// records for i >= k.  Lanes map over units f = g*Lu + u (16 bytes each).
struct CombineUniformArgs {
    const uint8_t* src;
    uint64_t src_gen_stride;
    uint64_t src_row_stride;
    uint8_t* dst;
    uint64_t dst_gen_stride;
    uint64_t dst_row_stride;
    const uint32_t* tabs;
    uint32_t k;
    uint32_t k_pad;
    uint32_t r_active;
    uint32_t L;
    uint32_t Lu;
    uint32_t pad0;
    uint64_t total_units;
    // generation offset tables (nullptr: g * gen_stride), the heterogeneous
    // batch API: generation g starts at src + src_offs[g] / dst + dst_offs[g]
    const uint64_t* src_offs = nullptr;
    const uint64_t* dst_offs = nullptr;
};

// Decode payload pass (one 16-output pass):
//   dst[g][j] = XOR_s coef[g][s][j] * rows[g][s]   for j < n_out[g]-16*pass
// coef: 16 coefficient bytes per slot, slot s of generation g at
// coef + g*coef_gen_stride + s*16.  Slots >= bound[g] are not read.
struct CombineSlotsArgs {
    const uint8_t* rows;
    uint64_t rows_gen_stride;
    uint64_t row_stride;
    uint8_t* dst;
    uint64_t dst_gen_stride;
    uint64_t dst_row_stride;
    const uint8_t* coef;
    uint64_t coef_gen_stride;
    const uint32_t* n_out;
    const uint32_t* bound;
    const uint32_t* tab256;
    uint32_t pass;
    uint32_t L;
    uint32_t Lu;
    uint32_t zero_slot;  // index of an all-zero coefficient record
    uint64_t total_units;
    const uint64_t* rows_offs = nullptr;  // generation offset tables (nullptr: strided)
    const uint64_t* dst_offs = nullptr;
};

struct PrepareArgs {
    const uint16_t* row_index;
    const uint32_t* n_rows;
    const uint8_t* row_coeffs;
    const uint8_t* explog;  // exp[512] then log[256]
    uint8_t* coef_out;      // [pass][G][coef_gen_stride]
    uint64_t coef_gen_stride;
    uint32_t* n_out;
    uint32_t* bound;
    uint16_t* rec_index;    // [G][e_max]
    int32_t* status;
    uint32_t k;
    uint32_t e_max;   // output capacity min(k, r)
    uint32_t rep_limit;  // repair index j = row_index - k must be < rep_limit
    uint32_t e_lds;   // matrix rows held in LDS, min(k, 128)
    uint32_t max_rows;
    uint32_t max_rows_pad;
    uint32_t passes;
    uint32_t G;
    // qf_decode_innovative_batch: [G][max_rows] accept flags of k_rank_filter;
    // a slot is a candidate only if its byte is set (nullptr: every slot)
    const uint8_t* accept = nullptr;
    // qf_decode_frames_dev (qf_relay.hip): row s of generation g is row_len
    // bytes at row_off from the generation's source region (nullptr: strided
    // rows, and none of the fields below is used).  A row among the n slots
    // with row_len > L, row_off % 16 != 0 or row_off + row_len >
    // src_gen_stride makes the generation QF_EINVAL.  coef_out then holds the
    // 48-byte pair records of RecodePrepareArgs, compacted to the accepted
    // slots in arrival order, (min(k, max_rows) + 1) / 2 + 1 of them per
    // generation and pass: rows at and after the accepted count have a zero
    // record, length 0 and the offset of the last accepted row (0 when none),
    // and a generation that is not QF_OK or has nothing to recover counts as
    // having accepted none.  bound receives the accepted count and min_len the
    // shortest row_len among the accepted rows (both 0 for such a generation).
    // src_slot (nullable, [G][k]): the accepted slot of each source's
    // systematic row, 0xFFFF for an erased source or a generation not QF_OK.
    const uint32_t* row_off = nullptr;   // [G][max_rows]
    const uint32_t* row_len = nullptr;   // [G][max_rows]
    uint32_t* min_len = nullptr;         // [G]
    uint16_t* src_slot = nullptr;
    uint64_t src_gen_stride = 0;
    uint32_t L = 0;
};

// Decode control for the reference's Cauchy code (no row_coeffs): row
// acceptance as k_decode_prepare, then the closed-form inverse of the square
// Cauchy submatrix C[J, E] (no elimination).  Outputs the slot map of the
// syndrome kernel and the stage-B coefficient records (slot j = syndrome of
// repair j, record r all zero).
struct PrepareCauchyArgs {
    const uint16_t* row_index;
    const uint32_t* n_rows;
    const uint8_t* explog;
    uint8_t* coef_out;      // [pass][G][(r + 1) * 16], passes of 16 outputs (e_max <= 64)
    uint8_t* smap;          // [G][map_stride]: k source slots, r repair slots, 0xFF absent
    uint32_t* n_out;
    uint32_t* bound;
    uint16_t* rec_index;    // [G][e_max]
    int32_t* status;
    uint32_t k, r;
    uint32_t e_max;
    uint32_t max_rows;      // <= 255
    uint32_t map_stride;
    uint32_t G;
    // fused decode (qf_cauchy_dec_*): when lu_out != nullptr the kernel
    // writes the packed LU record of C[J, E] per generation (lu_stride bytes,
    // layout bs_codegen._lu_solve_and_store) instead of coef_out / bound
    uint8_t* lu_out;
    uint32_t lu_stride;
    uint32_t grid_cap;   // k_decode_prepare_lu: max blocks (0 = one generation per wave)
    uint32_t lanes;      // 1: k_decode_prepare_lu_lanes (one generation per lane)
};
hipError_t launch_decode_prepare_cauchy(const PrepareCauchyArgs& a, hipStream_t st);

// Syndromes of codes without a syndrome kernel: gather the accepted sources
// (zero rows for erased ones) in source order, encode them with the
// bit-sliced encode kernels, XOR the accepted repair rows in.  Rows are read
// in whole 16-B units (Lu = ceil(L / 16)).
struct GatherArgs {
    const uint8_t* rows;   // received rows
    uint64_t rows_gen_stride, row_stride;
    const uint8_t* smap;   // [G][map_stride]: k source slots, r repair slots
    uint32_t map_stride;
    uint8_t* out;          // gather: sources [G][k]; xor: syndromes [G][r]
    uint64_t out_gen_stride, out_row_stride;
    uint32_t k, r, Lu, G;
    const uint64_t* rows_offs = nullptr;  // generation offset table of the received rows (nullptr: strided)
};
hipError_t launch_gather_sources(const GatherArgs& a, int num_cus, hipStream_t st);
hipError_t launch_xor_repairs(const GatherArgs& a, int num_cus, hipStream_t st);

// PD: prefetch depth in row pairs (V=1: 1..3, V=2: 1..2); k_pad must be a
// multiple of 2*(PD+1).
hipError_t launch_combine_uniform(const CombineUniformArgs& a, int R, int V, int PD, int num_cus,
                                  hipStream_t st);
hipError_t launch_combine_slots(const CombineSlotsArgs& a, int PD, int num_cus, hipStream_t st,
                                bool split_ok = true);
hipError_t launch_decode_prepare(const PrepareArgs& a, hipStream_t st);
size_t prepare_lds_bytes(uint32_t k, uint32_t e_max, uint32_t max_rows);
// qf_decode_partial_frames_dev (k_partial_prepare, qf_partial.hip; DESIGN.md
// 3.18): PrepareArgs with accept and the row_off group required.  The set A is
// the flagged slots; status is QF_OK at rank k and QF_ENOTREADY below it, and
// for both n_out / rec_index are the sources outside S that A determines,
// src_slot the slots of S.  The pair records, bound and min_len are as
// described there with "recorded" in the place of "accepted": only the slots of
// A with a nonzero coefficient in some determined source are recorded, and a
// generation with no determined source, or of another status, records none.
hipError_t launch_partial_prepare(const PrepareArgs& a, hipStream_t st);
size_t partial_prepare_lds_bytes(uint32_t k, uint32_t max_rows);
// qf_deliver_frames_dev / qf_deliver_frames_sel_dev (qf_deliver.hip; DESIGN.md
// 3.19).  The blocks of k_deliver_prepare are the G entries; with sel the
// source side (row_off, row_len, delivered, and the record's offset into src)
// is indexed by the listed generation sel[j] < G_src and everything else by
// the list position.  One 16-byte record per delivered packet, compacted in
// ascending source order at rec + j * k:
//   {offset low, offset high | kDeliverFromRec, length, source index}
// the offset from src (from rec_rows with kDeliverFromRec), and cnt[j] records
// (0 for an entry that delivers nothing).
constexpr uint32_t kDeliverFromRec = 0x80000000u;
constexpr uint32_t kDeliverPrepareLds = 256 * 4 + 256 * 2;
constexpr uint32_t kDeliverGroupsPerCu = 16;   // the copy's grid bound: workgroups per CU
struct DeliverPrepareArgs {
    const uint32_t* row_off;      // [G_src][max_rows]
    const uint32_t* row_len;
    const uint16_t* rec_index;    // [G][e_max]
    const uint32_t* n_rec;        // [G]
    const int32_t* dec_status;    // [G]
    const uint16_t* src_slot;     // [G][k]
    const uint64_t* ids;          // [G] or nullptr
    uint64_t* delivered;          // [G_src][5] or nullptr
    uint32_t* out_len;            // [G][k]
    uint8_t* out_state;           // [G][k]
    uint32_t* n_out;              // [G]
    uint32_t* n_known;            // [G] or nullptr
    int32_t* status;              // [G]
    uint4* rec;                   // [G][k]
    uint32_t* cnt;                // [G]
    uint64_t src_gen_stride, rec_row_stride, rec_gen_stride;
    uint32_t k, e_max, L, max_rows, G;
    const uint32_t* sel = nullptr;
    const uint32_t* n_sel = nullptr;   // nullptr: G
    uint32_t G_src = 0;
};
// The copy: wave w of the launch takes the quads q = w, w + n_waves, ... below
// n_quads = G * kq, quad q being records 4 (q % kq) .. + 3 of entry q / kq
// (kq = ceil(k / 4)).  round_up(length, 16) bytes per record, the bytes at and
// after the length zero, to out + j * out_gen_stride + source * out_row_stride.
struct DeliverRowsArgs {
    const uint8_t* src;
    const uint8_t* rec_rows;
    uint8_t* out;
    const uint4* rec;
    const uint32_t* cnt;
    uint64_t out_row_stride, out_gen_stride;
    uint32_t k, kq, n_quads, n_waves;
};
hipError_t launch_deliver_prepare(const DeliverPrepareArgs& a, hipStream_t st);
// grid_cap: the most workgroups (of four waves) to launch; the rest is strided
hipError_t launch_deliver_rows(DeliverRowsArgs a, uint32_t G, uint32_t grid_cap, hipStream_t st);
// qf_emit_frames_sel_dev (qf_emit.hip).  k_emit_count leaves
// every entry's wanted frame count in want and its status so far in
// entry_status, each block's sum in sums and the queue's base in head[0];
// k_emit_place derives every entry's position from them, writes the per-entry
// and per-frame outputs, the emitted frame count in head[1] and one 16-byte
// record per emitted frame, in queue order from the base:
//   {list position, row, row length, row index (k for a coded row)}
constexpr uint32_t kEmitPerBlock = 64;                 // entries of a block (one wave, one entry per lane)
constexpr uint32_t kEmitGroupsPerCu = 16;              // the copy's grid bound: workgroups per CU
struct EmitPlanArgs {
    const uint32_t* sel;          // [n_max]
    const uint32_t* n_sel;        // nullptr: n_max
    const uint16_t* row_index;    // [n_max][max_rows] or nullptr: every row coded
    const uint32_t* n_rows;       // [n_max] or nullptr: max_rows
    const uint32_t* row_len;      // [n_max][max_rows] or nullptr: L
    const int32_t* in_status;     // [n_max] or nullptr
    const uint64_t* ids;          // [n_max]
    const uint32_t* rank;         // [G_src] or nullptr, with sent
    uint32_t* sent;               // [G_src] or nullptr
    uint32_t* frame_len;          // [N_max]
    uint32_t* frame_off;
    uint64_t* frame_id;
    uint64_t* frame_pkt;
    uint32_t* n_frames;
    uint32_t* n_left;             // nullable
    uint32_t* entry_first;        // [n_max]
    uint32_t* entry_count;
    int32_t* entry_status;
    uint32_t* want;               // workspace [n_max]
    uint32_t* sums;               // workspace [blocks]
    uint32_t* head;               // workspace [2]: base, emitted
    uint4* rec;                   // workspace [min(n_max * max_rows, N_max)]
    uint32_t n_max, G_src, k, L, max_rows, N_max, P, append, has_coeffs, blocks;
};
// The copy: wave w takes the quads q = w, w + n_waves, ... of the head[1]
// records, quad q being records 4q .. 4q + 3, frames head[0] + 4q .. of the queue.
struct EmitFramesArgs {
    const uint8_t* rows;
    const uint8_t* row_coeffs;    // nullptr: no coded row among the records
    uint8_t* frames;
    const uint4* rec;
    const uint32_t* head;
    uint64_t row_stride, rows_gen_stride, frame_stride;
    uint32_t k, P, max_rows, n_waves;
};
hipError_t launch_emit_count(const EmitPlanArgs& a, hipStream_t st);
hipError_t launch_emit_place(const EmitPlanArgs& a, hipStream_t st);   // after launch_emit_count, same stream
// max_frames: the most frames the plan can have emitted; grid_cap as above
hipError_t launch_emit_frames(EmitFramesArgs a, uint64_t max_frames, uint32_t grid_cap, hipStream_t st);
// qf_rank_report_sel_dev and qf_credit_update_dev (qf_credit.hip; DESIGN.md
// 3.21).  A report is one 16-byte record {id lo, id hi, rank, 0}, a slot's
// feedback state one {owner lo, owner hi, peer, 0} with owner the id + 1.
struct ReportSelArgs {
    const uint32_t* sel;          // [n_max]
    const uint32_t* n_sel;        // nullptr: n_max
    const uint64_t* win;          // [G_src]
    const uint32_t* rank;         // [G_src]
    const uint32_t* head;         // with append: a copy of *n_reports from before the launch
    uint4* reports;               // [N_max]
    uint32_t* n_reports;
    uint32_t* n_left;             // nullable
    uint32_t n_max, G_src, k, N_max, append;
};
struct CreditArgs {
    const uint64_t* win;          // [G]
    const uint32_t* rank;         // [G]
    const uint32_t* sent;         // [G]
    const uint4* reports;         // [N_max], nullptr with N_max 0
    const uint32_t* n_reports;    // nullptr: N_max
    uint32_t* fresh;              // workspace [G], zeroed: the call's largest reported rank + 1 per slot
    uint4* state;                 // [G]
    uint32_t* credit;             // [G]
    int32_t* report_status;       // [N_max], nullable
    uint32_t G, N_max, k, num, den, cap;
};
hipError_t launch_report_sel(const ReportSelArgs& a, hipStream_t st);
hipError_t launch_credit_reports(const CreditArgs& a, hipStream_t st);   // after fresh is zeroed; N_max >= 1
hipError_t launch_credit_apply(const CreditArgs& a, hipStream_t st);     // after launch_credit_reports, same stream
// qf_frame_reports_dev, qf_parse_report_frames_dev and qf_report_closed_dev
// (qf_fbwire.hip).  A feedback packet is 0x02 | c (BE u16) | c
// entries of {id BE u64, rank BE u16}; per = (max_len - 3) / 10 entries at most.
constexpr uint32_t kFbPerBlock = 64;                   // records / packets of a block (one wave, one per lane)
constexpr uint32_t kFbRecordBlocks = 1u << 20;         // k_fbr_records' grid bound: the rest is strided
struct FbPackArgs {
    const uint4* reports;         // [N_max]
    const uint32_t* n_reports;    // nullptr: N_max
    uint8_t* pkts;                // [F_max] slots of stride bytes
    uint32_t* pkt_len;            // [F_max]
    uint32_t* n_pkts;
    uint32_t* n_left;             // nullable
    uint32_t* n_skipped;          // nullable
    uint32_t* sums;               // workspace [blocks]: the sendable records of each block
    uint64_t stride;
    uint32_t N_max, k, per, F_max, blocks;
};
hipError_t launch_fbw_count(const FbPackArgs& a, hipStream_t st);
hipError_t launch_fbw_pack(const FbPackArgs& a, hipStream_t st);        // after launch_fbw_count, same stream
struct FbParseArgs {
    const uint8_t* pkts;          // [F_max] slots of stride bytes
    const uint32_t* pkt_len;      // [F_max]
    const uint32_t* n_pkts;       // nullptr: F_max
    const uint32_t* head;         // with append: a copy of *n_reports from before the launches
    uint4* reports;               // [N_max]
    uint32_t* n_reports;
    uint32_t* n_left;             // nullable
    int32_t* pkt_status;          // [F_max], nullable
    uint32_t* pkt_first;          // [F_max], nullable
    uint32_t* pkt_count;          // [F_max], nullable
    uint32_t* cnt;                // workspace [F_max]: the entries of a QF_OK packet, else 0
    uint32_t* first;              // workspace [F_max]: min(where the packet's records begin, N_max)
    uint32_t* sums;               // workspace [blocks]
    uint64_t stride;
    uint32_t F_max, N_max, max_len, per, append, blocks;
    uint32_t chunks;              // ceil(per / 64): the waves of one packet in k_fbr_records
    uint32_t rec_blocks;          // derived by launch_fbr_records: its grid
};
uint32_t fb_parse_blocks(uint32_t F_max);
hipError_t launch_fbr_count(const FbParseArgs& a, hipStream_t st);
hipError_t launch_fbr_place(const FbParseArgs& a, hipStream_t st);      // after launch_fbr_count, same stream
hipError_t launch_fbr_records(FbParseArgs a, hipStream_t st);           // after launch_fbr_place, same stream
struct ClosedMarkArgs {
    const uint64_t* frame_id;     // [F_max]
    const int32_t* frame_status;  // [F_max]
    const uint32_t* n_frames;     // nullptr: F_max
    const uint64_t* win;          // [G_src]
    uint32_t* flags;              // workspace [G_src], zeroed: 1 for a marked slot
    uint32_t F_max, G_src;
};
hipError_t launch_closed_mark(const ClosedMarkArgs& a, hipStream_t st);
hipError_t launch_mul_slice(const uint8_t* a, const uint8_t* b, uint8_t* out, uint64_t n,
                            const uint8_t* explog, int num_cus, hipStream_t st);
hipError_t launch_fill_splitmix(uint8_t* dst, uint64_t n, uint64_t seed, uint64_t word_offset,
                                int num_cus, hipStream_t st);
// The generator of qf_fill_splitmix_dev: byte t of a region is byte (t & 7),
// little endian, of splitmix64(seed + word_offset + t / 8).  Shared by
// k_fill_splitmix and the seeded mix of k_recode_prepare (qf_recode.hip).
__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// Recode control (qf_recode_batch, qf_recode.hip): one wave per generation
// builds the m x n mix matrix (explicit or seeded), the payload pass's
// coefficient records [pass][G][(max_rows + 1) * 16] (record max_rows all
// zero), n_out = m, bound = n (0 for a generation whose status is not QF_OK),
// and the recoded coefficient vectors out_coeffs[g][j][0..k).
struct RecodePrepareArgs {
    const uint16_t* row_index;   // [G][max_rows]
    const uint32_t* n_rows;      // [G] or nullptr (= max_rows)
    const uint8_t* row_coeffs;   // [G][max_rows][k] or nullptr (Cauchy rows of (k, r))
    const uint8_t* mix;          // [G][m][max_rows] or nullptr (seeded)
    const uint8_t* explog;       // exp[512] then log[256]
    uint64_t seed;
    uint8_t* coef_out;
    uint64_t coef_gen_stride;
    uint32_t* n_out;
    uint32_t* bound;
    uint8_t* out_coeffs;         // [G][m][k]
    int32_t* status;
    uint32_t k, r, m, max_rows, passes, G;
    // qf_recode_frames_dev (qf_relay.hip): row s of generation g is row_len
    // bytes at row_off from the generation's source region (nullptr: the
    // strided rows of qf_recode_batch, and none of the fields below is used).
    // A row with row_len > L, row_off % 16 != 0 or row_off + row_len >
    // src_gen_stride makes the generation QF_EINVAL.  coef_out then holds
    // 48-byte pair records, (max_rows + 1) / 2 + 1 of them per generation and
    // pass: pair t = {off[2t], off[2t+1], len[2t], len[2t+1]} (u32), then the
    // coefficient records of slots 2t and 2t + 1.  Slots at and after n have
    // a zero record, offset row_off[n - 1] (0 when n == 0) and length 0.
    // min_len receives the shortest and out_len (nullable, [G][m]) the longest
    // row_len of the n rows, both 0 when the status is not QF_OK.
    const uint32_t* row_off = nullptr;   // [G][max_rows]
    const uint32_t* row_len = nullptr;   // [G][max_rows]
    uint32_t* min_len = nullptr;         // [G]
    uint32_t* out_len = nullptr;
    uint64_t src_gen_stride = 0;
    uint32_t L = 0;
};
size_t recode_prepare_lds_bytes(uint32_t k, uint32_t m, uint32_t max_rows);
hipError_t launch_recode_prepare(const RecodePrepareArgs& a, hipStream_t st);

// Recode payload pass over rows read where they lie (qf_recode_frames_dev,
// k_combine_rows_at in qf_relay.hip): one 16-output pass
//   dst[g][j] = XOR_s coef[g][s][j] * row(g, s)   for j < n_out
// with row(g, s) the len bytes at src + g*src_gen_stride + off, zero beyond
// them.  coef: this pass's 48-byte pair records ({off, off, len, len} and two
// coefficient records) and min_len as RecodePrepareArgs describes them.
constexpr uint32_t kPairRecBytes = 48;
struct CombineRowsAtArgs {
    const uint8_t* src;
    uint64_t src_gen_stride;
    uint8_t* dst;
    uint64_t dst_gen_stride;
    uint64_t dst_row_stride;
    const uint8_t* coef;
    uint64_t coef_gen_stride;
    const uint32_t* bound;
    const uint32_t* min_len;
    const uint32_t* tab256;
    uint32_t n_out;      // output rows of this pass, 1..16
    uint32_t L;
    uint32_t Lu;
    uint32_t max_rows;
    uint64_t total_units;
    // qf_decode_frames_dev: generation g writes clamp(n_out_gen[g] - 16 * pass,
    // 0, 16) rows in this pass, and a generation without a row in it is not
    // read (nullptr: n_out rows for every generation, the recoder's pass)
    const uint32_t* n_out_gen = nullptr;
    uint32_t pass = 0;
};
// The calls over a list (qf_decode_frames_sel_dev, qf_recode_frames_sel_dev;
// DESIGN.md 3.15): generation g of the batch reads the source region of
// generation gen_map[g]; everything else stays indexed by g.  Needs n_out_gen.
// Its own argument type, so the dense calls' kernels keep their arguments.
struct CombineRowsAtMapArgs : CombineRowsAtArgs {
    const uint32_t* gen_map;
};
hipError_t launch_combine_rows_at(const CombineRowsAtArgs& a, int num_cus, hipStream_t st,
                                  const uint32_t* gen_map = nullptr);

// The batch a list stands for (k_sel_gather, qf_select.hip): one wave per list
// entry j < n_max copies the first min(n_rows, max_rows) slots of generation
// sel[j]'s row_off / row_len / row_index and vectors to entry j of the compact
// arrays, with n_rows[j] the generation's and gen_map[j] = sel[j].  An entry at
// or above min(*n_sel, n_max) gets n_rows 0, gen_map 0 and n_out 0 and is not
// read; an entry >= G_src gets gen_map 0 and one slot of index 0xFFFF, length 0
// with n_rows = invalid_n_rows, which the control kernels answer with QF_EINVAL
// (k_rank_filter / k_decode_prepare for the index with invalid_n_rows = 1,
// k_recode_prepare for invalid_n_rows > max_rows).
struct SelGatherArgs {
    const uint32_t* sel;
    const uint32_t* n_sel;       // nullptr: n_max
    const uint32_t* row_off;     // [G_src][max_rows]
    const uint32_t* row_len;
    const uint16_t* row_index;
    const uint32_t* n_rows;      // [G_src] or nullptr (= max_rows)
    const uint8_t* row_coeffs;   // [G_src][max_rows][k]
    uint32_t* c_row_off;         // [n_max][max_rows]
    uint32_t* c_row_len;
    uint16_t* c_row_index;
    uint32_t* c_n_rows;          // [n_max]
    uint8_t* c_row_coeffs;       // [n_max][max_rows][k]
    uint32_t* gen_map;           // [n_max]
    uint32_t* n_out;             // [n_max] or nullptr: n_out_listed for a listed entry, 0 for an unused one
    uint32_t n_max, G_src, k, max_rows, invalid_n_rows, n_out_listed;
};
hipError_t launch_sel_gather(const SelGatherArgs& a, hipStream_t st);

// Innovative-row filter (qf_rank_batch, qf_decode_innovative_batch;
// qf_rank.hip): one wave per generation walks the slots in arrival order and
// flags the rows that raise the rank (k <= 256, max_rows <= 4096; without
// row_coeffs k + r <= 256).  An invalid generation gets rank 0 and no flags.
struct RankFilterArgs {
    const uint16_t* row_index;   // [G][max_rows]
    const uint32_t* n_rows;      // [G] or nullptr (= max_rows)
    const uint8_t* row_coeffs;   // [G][max_rows][k] or nullptr (Cauchy rows of (k, r))
    const uint8_t* explog;       // exp[512] then log[256]
    uint8_t* innovative;         // [G][max_rows] or nullptr
    uint32_t* rank;              // [G] or nullptr
    int32_t* status;             // [G] or nullptr
    uint32_t k, r, max_rows, G;
};
size_t rank_filter_lds_bytes(uint32_t k);
hipError_t launch_rank_filter(const RankFilterArgs& a, hipStream_t st);

// The same walk resumed from and written back to a per-generation rank state
// (qf_rank_update_batch): generation g's rank_state_bytes(k) bytes at state +
// g * rank_state_bytes(k), all zero for "nothing received".
struct RankUpdateArgs : RankFilterArgs {
    uint8_t* state;
};
size_t rank_state_bytes(uint32_t k);   // 0 for k outside 1..256
hipError_t launch_rank_update(const RankUpdateArgs& a, hipStream_t st);

// The resumed walk over a list (qf_rank_update_sel_batch): G
// is the list's n_max, the slots and the outputs are indexed by the list
// position j, state by the listed generation sel[j] < G_src, and rank_dense
// (nullable) receives rank_dense[sel[j]] of the listed entries only.  Its own
// argument type, so the dense calls' kernels keep their arguments.
struct RankUpdateSelArgs : RankUpdateArgs {
    const uint32_t* sel;
    const uint32_t* n_sel;       // nullptr: G
    uint32_t* rank_dense;        // [G_src] or nullptr
    uint32_t G_src;
};
hipError_t launch_rank_update_sel(const RankUpdateSelArgs& a, hipStream_t st);

// One encoder window of a multi-connection send batch: the window's ring at
// src + src_off (position i in slot (rot + i) % k), its repairs at
// rep + rep_off, rows rep_row_stride apart.
struct RingWin {
    uint64_t src_off, rep_off;
    uint32_t rot, L, src_row_stride, rep_row_stride;
};

// Small-batch encode (the per-packet send path: one or a few windows).
// repair[g][j] = sum_i coef[j*k + i] * src[g][i] over L bytes; lanes over
// (generation, repair, 16-B unit), units fastest.
struct EncodeSmallArgs {
    const uint8_t* src;
    uint64_t src_gen_stride, src_row_stride;
    uint8_t* rep;
    uint64_t rep_gen_stride, rep_row_stride;
    const uint8_t* coef;     // r x k device bytes
    const uint32_t* tab256;  // split-table records (8 dwords) of every coefficient
    uint32_t k, r, L, Lu, G;
    uint32_t rot;            // window row i is source row (i + rot) % k (a ring; 0: plain)
    const uint64_t* src_offs = nullptr;  // generation offset tables (nullptr: strided)
    const uint64_t* rep_offs = nullptr;
    // per-window records (nullptr: the scalar fields above); L / Lu above are
    // then the class maxima that size the tile grid
    const RingWin* wins = nullptr;
    // fused per-packet send (k_send_window): the ring slot of the new packet
    // and its 16-byte units (the packet itself travels in the arguments)
    uint8_t* fresh_dst = nullptr;
    uint32_t fresh_units = 0;
};

// Source packets of a send batch into their encoders' ring slots: bytes
// [0, len) from the staged copy at stage + src_off (zero padded to 16 bytes
// by the host), zeros to the slot's stride; dst2 (nullable) is the slot's
// twin in a double ring.
struct RingSlot {
    uint64_t src_off;
    uint8_t* dst;
    uint8_t* dst2;
    uint32_t len, stride;
};
hipError_t launch_ring_scatter(const uint8_t* stage, const RingSlot* slots, uint32_t M, hipStream_t st);

// Heterogeneous decode batches (qf_decode_batch_desc): a class's row indices
// gathered from the caller's arrays into [G][max_rows] (zero past n_rows)...
struct DescIndexArgs {
    const uint16_t* row_index;  // caller's row-index array
    const uint64_t* ri_off;     // [G] element offset of each generation's indices
    const uint32_t* n_rows;     // [G]
    uint16_t* out;              // [G][max_rows]
    uint32_t max_rows, G;
};
hipError_t launch_desc_gather_index(const DescIndexArgs& a, hipStream_t st);
// ... and its outputs scattered back: recovered indices to the caller's
// offsets, counts and statuses to the descriptors' positions
struct DescOutArgs {
    const uint16_t* rec_index_ws;  // [G][emax]
    const uint32_t* n_rec_ws;
    const int32_t* status_ws;
    const uint64_t* rec_index_off;  // [G]
    const uint32_t* desc_id;        // [G]
    uint16_t* rec_index;
    uint32_t* n_rec;
    int32_t* status;
    uint32_t emax, G;
};
hipError_t launch_desc_scatter_out(const DescOutArgs& a, hipStream_t st);

// base of generation g: base + offs[g] with an offset table, else base + g * stride
template <typename T>
__host__ __device__ inline T* gen_base(T* base, uint64_t g, uint64_t stride, const uint64_t* offs) {
    return base + (offs ? offs[g] : g * stride);
}
// Fused per-packet send: the new packet (pkt_bytes <= 16 fresh_units, in the
// kernel arguments) is window position k - 1 and goes into the ring slot
// a.fresh_dst; repairs to a.rep (host-coherent, whole 16-byte units).
constexpr uint32_t SEND_PKT_UNITS = 224;   // 3,584 bytes: with the arguments under 4 KiB
hipError_t launch_send_window(const EncodeSmallArgs& a, const uint8_t* pkt, uint32_t pkt_bytes, hipStream_t st);
hipError_t launch_encode_small(const EncodeSmallArgs& a, int num_cus, hipStream_t st);
// The same over per-window records (a.wins != nullptr), all repairs of a
// 64-unit tile per block (send batches of many windows).
hipError_t launch_encode_windows(const EncodeSmallArgs& a, int num_cus, hipStream_t st);

// Wire framing (qf_wire.hip).  The callers fill the fields by name; the
// launchers derive the grid and the fields marked "derived" from them and G,
// and launch nothing for an empty batch.
// k_frame_batch: an encode batch's sources and Cauchy repairs -> frames.
struct FrameArgs {
    const uint8_t* src;
    const uint8_t* rep;
    uint64_t src_row_stride, src_gen_stride, rep_row_stride, rep_gen_stride;
    uint8_t* frames;
    uint64_t frame_stride;
    uint32_t* frame_len;
    const uint8_t* explog;
    uint32_t k, r, L;
    uint32_t blocks_per_frame;  // derived: ceil((3 + k + L) / 16)
    uint64_t total_blocks;      // derived
};
hipError_t launch_frame_batch(const FrameArgs& a, uint32_t G, int num_cus, hipStream_t st);

// k_parse_frames: received frames of the Cauchy code -> decode-batch rows.
struct ParseArgs {
    const uint8_t* frames;
    uint64_t frame_stride;
    const uint32_t* frame_len;
    const uint64_t* ids;
    const uint32_t* n_frames;
    uint8_t* rows;
    uint64_t row_stride, rows_gen_stride;
    uint16_t* row_index;
    uint32_t* n_rows;
    int32_t* frame_status;
    const uint8_t* explog;
    uint32_t k, r, L, max_rows;
};
hipError_t launch_parse_frames(const ParseArgs& a, uint32_t G, hipStream_t st);

// k_frame_rows: rows with index and vector -> frames in payload-aligned slots.
struct FrameRowsArgs {
    const uint8_t* rows;        // NULL in place
    const uint16_t* row_index;  // NULL: every row coded
    const uint32_t* n_rows;     // NULL: max_rows
    const uint8_t* row_coeffs;  // NULL: Cauchy rows of (k, r)
    const uint32_t* row_len;    // NULL: L
    uint8_t* frames;
    uint32_t* frame_len;
    uint32_t* frame_off;        // may be NULL
    const uint8_t* explog;
    uint64_t row_stride, rows_gen_stride, frame_stride;
    uint32_t k, r, L, max_rows;
    uint32_t P;                 // derived: qf_frame_payload_offset(k)
    uint32_t hdr_blocks;        // derived: P / 16
    uint32_t blocks_per_frame;  // derived: hdr_blocks (+ ceil(L / 16) in copy mode)
    uint64_t total_blocks;      // derived
};
hipError_t launch_frame_rows(const FrameRowsArgs& a, uint32_t G, int num_cus, hipStream_t st);

// k_parse_frames_coded: frames at an offset in their slots -> rows, any vector.
struct ParseCodedArgs {
    const uint8_t* frames;
    uint64_t frame_stride;
    const uint32_t* frame_len;
    const uint32_t* frame_off;  // NULL: 0
    const uint64_t* ids;
    const uint32_t* n_frames;
    uint8_t* rows;
    uint64_t row_stride, rows_gen_stride;
    uint16_t* row_index;
    uint32_t* n_rows;
    uint8_t* row_coeffs;
    uint32_t* row_len;          // may be NULL
    int32_t* frame_status;
    uint32_t k, L, max_rows;
};
hipError_t launch_parse_frames_coded(const ParseCodedArgs& a, uint32_t G, hipStream_t st);

// k_parse_frame_headers: the same decisions, the payloads left where they are.
struct ParseHeadersArgs {
    const uint8_t* frames;
    uint64_t frame_stride;
    const uint32_t* frame_len;
    const uint32_t* frame_off;  // NULL: 0
    const uint64_t* ids;
    const uint32_t* n_frames;
    uint16_t* row_index;
    uint32_t* n_rows;
    uint8_t* row_coeffs;
    uint32_t* row_len;
    uint32_t* row_off;
    int32_t* frame_status;
    uint32_t k, L, max_rows;
};
hipError_t launch_parse_frame_headers(const ParseHeadersArgs& a, uint32_t G, hipStream_t st);

}  // namespace qf
