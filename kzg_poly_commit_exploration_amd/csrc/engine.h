// engine.h -- internal interface between the C-ABI (api.hip) and the kernel translation units.
// Not installed; the public boundary is include/kzg_mi355x.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace kzg {

// One affine SRS / table point in HBM: x as 13 signed radix-2^30 digits in words 0..12, y in words 16..28
// (field30.hip.h: Montgomery R' = 2^390, magnitude < 0.62 p), all zero = infinity: a 128-byte record, so that every
// random gather of the accumulation kernel touches exactly one 128-byte line.  Table layout:
// level-major, T[j * n + i] = 2^(level_bits*j) * SRS[i]  (j < W), so level 0 is the SRS itself.
constexpr size_t kAffineBytes = 128;
constexpr size_t kAffineU4 = kAffineBytes / 16;  // record stride in uint4 units
// One XYZZ accumulator in HBM: X, Y, ZZ, ZZZ as four groups of 13 signed radix-2^30 digits (field30.hip.h,
// Montgomery R' = 2^390, lazily reduced), each group padded to 16 words: 256 bytes, all zero = infinity.
constexpr size_t kXyzzBytes = 256;
constexpr size_t kXyzzU4 = kXyzzBytes / 16;      // record stride in uint4 units
constexpr size_t kXyzzWords64 = kXyzzBytes / 8;  // record stride in u64 units (host side)

// Two scalar recodings share every kernel after the digit loop:
//   kRecodeWindows  aligned signed windows of c bits: W = ceil(255/c) digits per scalar, one table level per
//                   window (level_bits = c), digit magnitude 1 .. 2^(c-1) -> 2^(c-1) buckets of weight b+1.
//   kRecodeNaf      width-c non-adjacent form: digits are odd, |d| < 2^(c-1), at most one per c consecutive
//                   bits and on average one per c+1 bits (vs one per c-1 for the same bucket count with
//                   windows: ~11 % fewer mixed additions), but a digit can start at ANY bit, so the table
//                   carries one level per scalar bit (W = 255, level_bits = 1): 255 x n x 128 B, 34 GB at
//                   2^20 points, which the 288 GB of HBM3E hold easily.  2^(c-2) buckets of weight 2b+1.
//                   Opt-in (KZG_MSM_RECODE=naf): bit-exact, but on MI355X the fewer additions are eaten by
//                   address-translation misses of the gathers over the larger table (msm_sort.hip).
enum : uint32_t { kRecodeWindows = 0, kRecodeNaf = 1 };
struct MsmConfig {
    uint32_t recode;      // kRecodeWindows | kRecodeNaf
    uint32_t c;           // digit width in bits
    uint32_t W;           // table levels
    uint32_t level_bits;  // doublings between consecutive table levels
    uint32_t nb;          // buckets per polynomial (power of two)
    uint32_t max_digits;  // bound on the non-zero digits of one scalar
};

// table_budget_bytes: what the table may occupy (the NAF recoding is refused when its table does not fit)
MsmConfig choose_msm_config(size_t n_points, size_t table_budget_bytes);

// Segment length of the bucket accumulation for M sorted references on `lanes` lanes (msm_accum.hip): computed
// on the device from the actual M, so that scalars with many zero digits still fill every lane.
// shortest segment: 8 references, or 4 for tiny jobs (up to kTinyRefs references: latency-bound, every dependent
// addition counts; measured at degree 1000: 0.77 -> 0.67 ms, while at 16384 terms the extra partials cost 2x)
constexpr uint32_t kTinyRefs = 65536;
__host__ __device__ inline uint32_t accumulate_min_seg(uint64_t refs) { return refs <= kTinyRefs ? 4u : 8u; }
__host__ __device__ inline uint32_t accumulate_seg_len(uint32_t M, uint32_t lanes) {
    uint32_t L = (M + lanes - 1) / lanes;
    const uint32_t lo = accumulate_min_seg(M);
    return L < lo ? lo : L;
}

// ---- msm_kernels.hip --------------------------------------------------------------------
constexpr size_t kHeavyHeaderBytes = 1024;  // zeroed per job: long-bucket counters (line 0), phase counters of the one-launch paths (own lines)
// scalar recoding + two-level LDS counting sort of `batch` polynomials of n terms at once (polynomial p
// at d_scalars + p * stride scalars; its buckets are [p * nb, (p+1) * nb)): fills
// d_offs[0 .. batch*nb] (last = number of references) and d_sorted (bucket-major table references,
// index | sign << 31).  d_cnt: sort_count_entries(max_batch, cfg) u32; d_ws: sort_workspace_words() u32;
// d_pairs: batch * n * max_digits u64; d_recoded: batch * n * 32 bytes (the folded scalars between the two recoding passes;
// not touched by the one-workgroup sort of small inputs).  batch <= sort_max_batch(cfg).
uint32_t sort_count_entries(uint32_t max_batch, MsmConfig cfg);
uint32_t sort_max_batch(MsmConfig cfg);
uint32_t sort_workspace_words();
uint32_t sort_workspace_zero_words();  // leading words of d_ws that must be zero when the workspace is first used (the sort keeps them so)
// d_header: kHeavyHeaderBytes that the job wants zeroed before its next kernel; returns true when the sort did that
// itself (it does whenever it launches anything), false when the caller has to memset them (n == 0).
bool launch_bucket_sort(hipStream_t s, const uint32_t* d_scalars, int scalars_are_mont, uint32_t n, uint32_t batch,
                        uint64_t stride, uint32_t table_stride, MsmConfig cfg, uint32_t* d_cnt,
                        uint32_t* d_ws, uint64_t* d_pairs, uint32_t* d_recoded, uint32_t* d_offs, uint32_t* d_sorted,
                        uint32_t* d_header);
// bucket accumulation (dominant kernel): one lane per segment of L sorted references
constexpr uint32_t kMaxAccumLanes = 262144 + 64;  // bound on accumulate_lanes()
// lanes (= segments) for at most max_refs references; a multiple of the workgroup size
// alone: no other job is in flight on the context (the light kernels of other slots need no room)
uint32_t accumulate_lanes(uint64_t max_refs, bool alone = false);
// d_pair_scratch: accumulate_pair_scratch_bytes(max_refs) of scratch for the affine front end (prefix products of the
// shared inversions), or null to run plain mixed additions; max_refs bounds the references of this launch
size_t accumulate_pair_scratch_bytes(uint64_t max_refs);
void launch_bucket_accumulate(hipStream_t s, const void* d_table, const uint32_t* d_sorted, const uint32_t* d_offs,
                              uint32_t nb, uint32_t lanes, void* d_buckets /* complete buckets only: the rest by the finalisation */,
                              void* d_part_a, void* d_part_b, uint32_t lds_reserve_bytes, void* d_pair_scratch,
                              uint64_t max_refs, void* d_clock = nullptr /* kAccumClockOffset into the job's zeroed header, or null */);
// the accumulation kernel's own start / end stamps: two u64 in the job header (zeroed by the sort), copied next to the
// reference count by the finalisation (d_refs_out[2..5])
constexpr size_t kAccumClockOffset = 768;  // bytes into d_heavy_ws (words 192..195 of the header: unused by the counters)
// adds the head / tail partials of buckets that span several segments (serial for short runs, three passes of
// 64-wide trees for long ones) and writes empty buckets as infinity: every bucket is written once per job, the array is
// never cleared.  d_heavy_ws: heavy_workspace_bytes() of scratch whose first kHeavyHeaderBytes (the counters) are zero
// (launch_bucket_sort does that) -- ahead of time, so that nothing sits between the end of the accumulation and this
// launch (a fill kernel there lets the next slot's accumulation take the chip first: +0.9 ms)
size_t heavy_workspace_bytes();
// group: quads per bucket (finalize_group_size(nb); 1 = one quad per bucket, the throughput form).
void launch_bucket_finalize(hipStream_t s, const uint32_t* d_offs, uint32_t nb, uint32_t lanes, const void* d_part_a,
                            const void* d_part_b, void* d_buckets, void* d_heavy_ws,
                            uint32_t* d_refs_out /* receives the number of references, may be null */, uint32_t group = 1);
uint32_t finalize_group_size(uint32_t nb);
// Small jobs (at most kTinyRefs references, one polynomial): accumulation, finalisation, long-bucket trees and both
// reduction stages in ONE launch (msm_finalize.hip: k_small_msm).  The first kHeavyHeaderBytes of d_heavy_ws must be zero.
// lds_bytes: small_msm_lds_bytes() once hipFuncAttributeMaxDynamicSharedMemorySize has been raised for
// small_msm_kernel(), otherwise at most 64 KiB.
struct TreeSumDesc;
uint32_t small_msm_lds_bytes();
const void* small_msm_kernel();
void launch_small_msm(hipStream_t s, const void* d_table, const uint32_t* d_sorted, const uint32_t* d_offs, uint32_t nb,
                      uint32_t lanes, uint64_t max_refs, void* d_buckets, void* d_part_a, void* d_part_b, void* d_heavy_ws,
                      uint32_t* d_refs_out, const TreeSumDesc* stage1 /* 2 */, const TreeSumDesc* stage2 /* 4 */,
                      uint32_t lds_bytes);
// out[g] = sum_{q<len} in[g*gstride + q*estride], XYZZ records: log-depth tree per group;
// up to four independent jobs per launch
// group g reads in[(g / inner) * ostride + (g % inner) * gstride + q * estride], q < len
struct TreeSumDesc {
    const void* in;
    void* out;
    uint32_t groups, len;
    uint64_t gstride, estride;
    uint32_t inner;    // groups per outer block (= groups when there is no batch dimension)
    uint64_t ostride;  // record stride between outer blocks
};
void launch_tree_sums(hipStream_t s, const TreeSumDesc* descs, uint32_t count, bool dense = false, bool alone = true);
// stage2 reads what stage1 wrote.  One launch when both stages fit the chip at once (d_sync: two zeroed words, e.g.
// words 4 and 5 of d_heavy_ws), otherwise two launches.
void launch_tree_sums_two_stage(hipStream_t s, const TreeSumDesc* stage1, uint32_t count1, const TreeSumDesc* stage2,
                                uint32_t count2, uint32_t* d_sync, bool alone);

// ---- srs_kernels.hip --------------------------------------------------------------------
// blst_p1 Jacobian (host layout, strided) already copied to d_jac (n x 144 B contiguous) -> affine
void launch_jacobian_to_affine(hipStream_t s, const void* d_jac, uint32_t n, void* d_affine_out,
                               void* d_prefix_tmp);
// table level j from level j-1:  T[j][i] = 2^c * T[j-1][i]
void launch_table_window(hipStream_t s, const void* d_prev_affine, uint32_t n, uint32_t c,
                         void* d_xyzz_tmp, void* d_prefix_tmp, void* d_next_affine);
// fixed-base trusted setup: out[i] = [s^(first+i)] G1, affine
void launch_srs_generate(hipStream_t s, const uint32_t* secret_raw8 /* 256-bit LE integer */, uint64_t first, uint32_t n,
                         void* d_gtable, void* d_xyzz_tmp, void* d_prefix_tmp, void* d_affine_out);
size_t srs_gtable_bytes();
// ---- srs_io.hip ------------------------------------------------------------------------
// n x 96-byte affine points (x, y as blst_fp; (0, 0) = infinity) -> table level 0
void launch_affine96_to_table(hipStream_t s, const void* d_affine96, uint32_t n, void* d_table);
// n x 48-byte compressed points (ZCash encoding) -> table level 0; *d_status (pre-set to 0xffffffff) receives
// index + 1 of the first malformed point
void launch_uncompress(hipStream_t s, const void* d_compressed, uint32_t n, void* d_table, uint32_t* d_status);

// ---- wire_kernels.hip: inputs decoded from their wire bytes (wire30.hip.h; 16-byte aligned arrays) ----------------------
// n compressed points (48 bytes each; point d_src[i] when d_src is given) -> affine table records at d_records + i *
// stride_bytes (a multiple of 16, >= 128), infinity for a point that does not decode; *d_err (pre-set to 0xffffffff)
// receives the least source index that did not decode
void launch_wire_g1(hipStream_t s, const void* d_in48, const uint32_t* d_src, uint32_t n, void* d_records, uint32_t stride_bytes,
                    uint32_t* d_err);
// n big-endian scalars (32 bytes each) -> blst_fr images; bit_reversed: value i of every row of 2^log_row values goes to
// position brp_(log_row)(i) of its row (n a multiple of the row length); *d_err: the least input index not below r
void launch_wire_fr(hipStream_t s, const void* d_in32, uint32_t n, uint32_t log_row, bool bit_reversed, void* d_out, uint32_t* d_err);

// ---- blob_kernels.hip: outputs encoded into their wire bytes (wire_enc30.hip.h; 16-byte aligned arrays) -----------------
// n affine table records -> 48-byte compressed points; bit_reversed: record j of every row of 2^log_row records goes to
// slot brp_(log_row)(j) of its row (n a multiple of the row length)
void launch_enc_g1(hipStream_t s, const void* d_affine, uint32_t n, uint32_t log_row, bool bit_reversed, void* d_out48);
// n blst_fr images -> 32 big-endian bytes each; bit_reversed: value i of cell j (cells of 2^log_row values, 2^log_cells cells
// per polynomial) goes to position brp(i) of cell brp(j) of its polynomial; *d_err (pre-set to 0xffffffff) receives the least
// source index whose image is not below r
void launch_enc_fr(hipStream_t s, const void* d_in, uint32_t n, uint32_t log_row, uint32_t log_cells, bool bit_reversed, void* d_out32,
                   uint32_t* d_err);
// d_out[b] (pre-set to 0) = 1 + the index of the highest non-zero coefficient of polynomial b (n coefficients at d_coeffs +
// 32 b stride bytes), 0 for the zero polynomial; scale: every coefficient is multiplied by it in place first (multiplier form)
struct Fr30;
void launch_poly_trim(hipStream_t s, void* d_coeffs, uint32_t n, uint64_t stride, uint32_t batch, const Fr30* scale, uint32_t* d_out);

// ---- msm_accum.hip (table format) ---------------------------------------------------------
// native table entries -> blst_p1 (Z = Montgomery one / all zero for infinity)
void launch_affine_to_p1(hipStream_t s, const void* d_affine, uint32_t n, void* d_p1_out);

// ---- ntt_kernels.hip: NTT over the subgroup of 2^k-th roots of unity, natural order in and out, x 2^256 form ----------
struct Fr30;
constexpr uint32_t kNttMaxLog = 22;        // largest domain (the largest SRS)
constexpr uint32_t kNttTableLen = 2048;    // entries of each twiddle table (lo: w^i, hi: w^(2048 i), w = w_(2^22))
constexpr uint32_t kNttTileLog = 11;       // values per workgroup tile (nine LDS digit planes: 72 KiB)
constexpr uint32_t kNttTile = 1u << kNttTileLog;
constexpr uint32_t kNttMaxRadixLog = 9;    // radix of a pass when there are several (tile = 2^(11 - m) runs of 2^m values)
struct NttPlan {
    uint32_t passes;
    uint32_t m[3];  // log radix of each pass
};
NttPlan ntt_plan(uint32_t log_n);
// raises the dynamic-LDS limit of the pass kernel on the current device; false when refused
bool ntt_prepare_device();
// d_tw: the direction's lo[2048] then hi[2048] tables (Fr30, multiplier form); last_c: the multiplier of the last pass in
// the same form (1, or 1/n for the inverse).  Pass i < passes - 1 writes d_buf_a (i even) or d_buf_b (i odd), the last
// pass writes d_out.  No intermediate may alias the buffer its pass reads; d_in == d_out only for a single pass.
void launch_ntt(hipStream_t s, const uint32_t* d_in, uint32_t* d_out, uint32_t log_n, const void* d_tw, const Fr30& last_c,
                uint32_t* d_buf_a, uint32_t* d_buf_b);

// ---- ntt_batch_kernels.hip: the same transform over `batch` columns, one launch per pass of ntt_plan for the whole batch ----
// raises the dynamic-LDS limit of the batched pass kernel on the current device; false when refused
bool ntt_batch_prepare_device();
// Column b is read at d_in + 8 b in_stride words and written at d_out + 8 b out_stride words (strides in values, >= 2^log_n);
// the intermediates use stride 2^log_n: d_buf_a and d_buf_b hold batch * 2^log_n values each when there is more than one pass
// (pass i < passes - 1 writes d_buf_a for even i, d_buf_b for odd i).  d_tw, last_c: as for launch_ntt.  d_in == d_out with equal
// strides is allowed (no intermediate is either of them); batch <= 65535 (a grid dimension), batch == 0 launches nothing.
void launch_ntt_batch(hipStream_t s, const uint32_t* d_in, uint64_t in_stride, uint32_t* d_out, uint64_t out_stride, uint32_t log_n,
                      uint32_t batch, const void* d_tw, const Fr30& last_c, uint32_t* d_buf_a, uint32_t* d_buf_b);

// ---- cell_kernels.hip: quotients of P by X^l - w_N^(j l) for the cells j of a domain of N = 2^log_n points, l = 2^log_l ----
// cells [first_cell, first_cell + cells): q of cell first_cell + p at d_q + 8 p stride words, nq values each (nq = n' - l,
// d_coeffs holds at least nq + l coefficients); d_tw: the context's forward NTT twiddles; d_agg: cells_agg_words() words
uint32_t cells_chunk_log(uint32_t nq, uint32_t log_l);
uint64_t cells_agg_words(uint32_t nq, uint32_t log_l, uint32_t cells);
void launch_cell_quotients(hipStream_t s, const uint32_t* d_coeffs, uint32_t nq, uint32_t log_n, uint32_t log_l,
                           uint32_t first_cell, uint32_t cells, const void* d_tw, uint32_t* d_agg, uint32_t* d_q,
                           uint64_t stride);
// out[j l + i] = evals[j + (N / l) i] (N values)
void launch_cells_gather(hipStream_t s, const uint32_t* d_evals, uint32_t* d_out, uint32_t log_n, uint32_t log_l);

// ---- fk20_kernels.hip: G1 DFTs and the FK20 proofs of all cells ----------------------------------
// A twiddle w split as w = k1 + k2 lambda (lambda = z^2 - 1, k1, k2 < 2^128 as plain integers, little-endian u64)
struct Glv {
    uint64_t k1[2], k2[2];
};
// comb tables of the SRS side: entry (j, d - 1) = d 16^j B, j < 64 windows of 4 bits, d = 1..8 (signed digits)
constexpr uint32_t kFk20CombWindows = 64;
constexpr uint32_t kFk20CombDigits = 8;
constexpr uint32_t kFk20CombEntries = kFk20CombWindows * kFk20CombDigits;
// `batch` DFTs of 2^log_len XYZZ records (vector b at d_in + b 2^log_len records), natural order in and out, unnormalised
// (no 1/len); the stages ping-pong through d_a, d_b (neither may alias d_in); returns the buffer holding the result (d_in
// when log_len = 0).  d_tw: w_(2^log_tw)^e for e < 2^log_tw, log_tw >= log_len.
const void* launch_g1_dft(hipStream_t s, const void* d_in, void* d_a, void* d_b, uint32_t log_len, uint64_t batch,
                          const Glv* d_tw, uint32_t log_tw, bool inverse);
void launch_g1_scale(hipStream_t s, void* d_io, uint64_t n, const Glv& k);
// S_r[v] (r < l, v < L; out[r L + v]) from the table's level 0: SRS[v l + r] for v < L/2 inside the SRS, else infinity
void launch_fk20_srs_gather(hipStream_t s, const void* d_table, uint64_t srs_n, uint32_t log_L, uint32_t log_l, void* d_out);
// bases [first, first + count) in (i, r) order (base i l + r is d_bases[r L + i]) -> d_tmp: kFk20CombEntries XYZZ records
// per base (normalise them for the table)
void launch_fk20_comb(hipStream_t s, const void* d_bases, uint32_t log_L, uint32_t log_l, uint64_t first, uint32_t count,
                      void* d_tmp);
// R_r of `batch` polynomials (n coefficients each, contiguous) and their forward Fr DFTs of 2^log_L values, times inv_L
// (multiplier form), as plain integers: returns d_a or d_b
const uint32_t* launch_fk20_fr_side(hipStream_t s, const uint32_t* d_coeffs, uint32_t n, uint32_t m, uint32_t log_L,
                                    uint32_t log_l, uint64_t batch, const void* d_tw, const Fr30& inv_L, uint32_t* d_a,
                                    uint32_t* d_b);
// d_out[b L + i] = sum_r [A_(b,r)[i]] B_r[i] for i in [i0, i0 + ci) over the comb tables d_tab of bases
// [i0 l, (i0 + ci) l); d_part: batch ci l XYZZ records (unused for l = 1)
void launch_fk20_pointwise(hipStream_t s, const uint32_t* d_scal, const void* d_tab, uint32_t log_L, uint32_t log_l,
                           uint32_t i0, uint32_t ci, uint64_t batch, void* d_part, void* d_out);
// H[b M + d] = conv[b L + m - 1 - d] (d <= m - 2), infinity up to M = 2^log_M
void launch_fk20_select(hipStream_t s, const void* d_conv, uint32_t log_L, uint32_t m, uint32_t log_M, uint64_t batch, void* d_H);
// native affine table records -> XYZZ records
void launch_affine_to_xyzz(hipStream_t s, const void* d_affine, uint64_t n, void* d_out);
// srs_kernels.hip: XYZZ records -> native affine records (one inversion per 32 points; d_prefix: 64 B per point)
void launch_xyzz_to_affine(hipStream_t s, const void* d_xyzz, uint32_t n, void* d_out, void* d_prefix);
// `batch` Fr DFTs of 2^log_len canonical values each (vector b at d_in + 8 b 2^log_len words), natural order in and out,
// unnormalised; d_tw: one direction's lo / hi twiddle tables (the inverse ones give the inverse DFT without 1/len).  The
// stages (k_fr_stage) alternate between d_a and d_b, never writing the buffer they read; returns the buffer holding the result
// (d_in when log_len = 0).
const uint32_t* launch_fr_dft(hipStream_t s, const uint32_t* d_in, uint32_t* d_a, uint32_t* d_b, uint32_t log_len, uint64_t batch,
                              const void* d_tw);

// ---- recover_kernels.hip: all coefficients of a batch of polynomials from part of their cells --------
// Domain of N = 2^log_n points, cells of l = 2^log_l, M = N / l.  Stored multipliers are canonical 8 x u32 of the "x 2^270"
// form.  The vanishing evaluations: d_z[p] = Z'(w_M^p) for p < M and 1 / Z'(g^l w_M^(p - M)) for M <= p < 2M, Z' over the
// n_missing cells in d_missing; gl = g^l (multiplier form); d_part: recover_vanish_parts(n_missing) 2M x 8 words.
uint32_t recover_vanish_parts(uint32_t n_missing);
void launch_recover_vanishing(hipStream_t s, const uint32_t* d_missing, uint32_t n_missing, const void* d_tw, uint32_t log_n,
                              uint32_t log_l, const Fr30& gl, uint32_t* d_part, uint32_t* d_z);
// d_out[b N + j + M i] = cells[(b k + d_pos[j]) l + i] d_zrecv[j], 0 where d_pos[j] < 0
void launch_recover_scatter(hipStream_t s, const uint32_t* d_cells, const int32_t* d_pos, const uint32_t* d_zrecv, uint32_t k,
                            uint32_t log_n, uint32_t log_l, uint64_t batch, uint32_t* d_out);
// in place, value i of every vector times g^i c; d_gtab: the g^i tables (lo / hi as the NTT twiddles)
void launch_recover_twist(hipStream_t s, uint32_t* d_io, uint32_t log_n, uint64_t batch, const void* d_gtab, const Fr30& c);
// in place, value e of every vector times d_zinv[e mod M]
void launch_recover_divide(hipStream_t s, uint32_t* d_io, uint32_t log_n, uint32_t log_l, uint64_t batch, const uint32_t* d_zinv);
// P_i = v_i g^-i c: i < n to d_coef[b n + i]; pad: P padded to N in place; a non-zero P_i with i >= n sets d_flags[b]
void launch_recover_untwist(hipStream_t s, uint32_t* d_io, uint32_t log_n, uint32_t n, uint64_t batch, const void* d_ginv,
                            const Fr30& c, uint32_t* d_coef, bool pad, uint32_t* d_flags);
// d_out[b N + j l + i] = d_in[b N + j + M i]
void launch_recover_gather(hipStream_t s, const uint32_t* d_in, uint32_t* d_out, uint32_t log_n, uint32_t log_l, uint64_t batch);

// ---- verify_kernels.hip: one random-linear-combination check of many cell proofs ------------------
// lane t < lanes: P = d_rec[d_src ? d_src[t] : t] (affine records); lanes below n_check are checked to lie on the curve
// (else atomicMin(d_err[0], index)) and in G1 (else atomicMin(d_err[1], index)); [d_glv[t]] P (XYZZ) to d_out_a[t] for
// t < split, d_out_b[t - split] otherwise
void launch_vc_ladder(hipStream_t s, const void* d_rec, const uint32_t* d_src, const Glv* d_glv, uint32_t lanes, uint32_t n_check,
                      uint32_t split, void* d_out_a, void* d_out_b, uint32_t* d_err);
// d_out[d] = [w_M^(d_ids[d])] d_T[d], the power read from split twiddles d_tw[d_ids[d] << shift]
void launch_vc_cell_scale(hipStream_t s, const void* d_T, const uint32_t* d_ids, uint32_t D, const Glv* d_tw, uint32_t shift,
                          void* d_out);
// one level of a segmented sum: d_out[g] = sum of the XYZZ records d_in[d_starts[g] .. d_starts[g + 1])
void launch_vc_g1_sum(hipStream_t s, const void* d_in, const uint32_t* d_starts, uint32_t groups, void* d_out);
// the same over rows of 2^log_l canonical Fr values; with d_rho, row q is d_in's row d_order[q] times d_rho[q] (multiplier form)
void launch_vc_fr_sum(hipStream_t s, const uint32_t* d_in, const uint32_t* d_order, const Fr30* d_rho, const uint32_t* d_starts,
                      uint32_t groups, uint32_t log_l, uint32_t* d_out);
// in place, value i of row d times w_N^-(d_ids[d] i) inv_l; d_itw: the inverse NTT twiddles
void launch_vc_fr_twist(hipStream_t s, uint32_t* d_io, const uint32_t* d_ids, uint32_t D, const void* d_itw, uint32_t log_n,
                        uint32_t log_l, const Fr30& inv_l);

// ---- circuit_verify_kernels.hip: the second stage of the batch verifier of circuit proofs -------------
// lane (k, j), k < count, j < 4: [d_s[4 k + j]] X, X = d_D[k], d_E[k], d_F[k], d_F[k] (XYZZ records).  Products 0 .. 2 go to
// d_p0[3 k + j], product 3 to d_p1[k]
void launch_cvb_stage2(hipStream_t st, const void* d_D, const void* d_E, const void* d_F, const Glv* d_s, uint32_t count, void* d_p0,
                       void* d_p1);

// The Fr side.  d_consts (Fr30, multiplier form): 2^14, w, 1 + w, 1 / n, w^64, then the t shifts.  All inputs are canonical blst_fr
// images on the device: d_chal 5 per proof (beta, gamma, alpha, zeta, v), d_evals 2 t per proof, d_rho one per proof, d_pub proof
// k's n_public values at d_pub + 8 k stride.
enum : uint32_t { kCvbK284 = 0, kCvbW, kCvbW1, kCvbInvN, kCvbW64, kCvbShifts };  // (2^14 x 2^270 = 2^284 takes an image into the form)
// d_out[k] = PI(zeta_k), multiplier form
void launch_cvb_public(hipStream_t st, const uint32_t* d_pub, uint32_t n_public, uint64_t stride, const uint32_t* d_chal,
                       const Fr30* d_consts, uint32_t lg_n, uint32_t count, Fr30* d_out);
// per proof k: the split scalars d_glv[k (t + e) + i] (i < t + e), d_glv[o_e + k], d_s2[4 k + j], and the row of 2 (2 t + 3 + g)
// plain integers at d_rows + 8 (k << log_l); d_pim: launch_cvb_public's output or null, d_exps: g x t bytes or null; d_lin: 4 Fr30
// per proof between the two launches (k_cvb_lin, k_cvb_scalars)
void launch_cvb_scalars(hipStream_t st, const uint32_t* d_chal, const uint32_t* d_evals, const uint32_t* d_rho, const Fr30* d_pim,
                        const Fr30* d_consts, const uint8_t* d_exps, uint32_t count, uint32_t t, uint32_t e, uint32_t g, uint32_t lg_n,
                        Fr30* d_lin, Glv* d_glv, uint64_t o_e, Glv* d_s2, uint32_t* d_rows, uint32_t log_l);
// d_out[j] = the split of the plain canonical integer d_sums[j], j < n
void launch_cvb_key_split(hipStream_t st, const uint32_t* d_sums, uint32_t n, Glv* d_out);

// ---- srs_update_kernels.hip: a powers-of-tau contribution and the per-point checks of a setup --------
// d_out_xyzz[i] = [tau^(first + i) mod r] d_level0[i] (affine records in, XYZZ out, infinity stays); tau_raw8: the
// 256-bit little-endian integer, any value below 2^256 (the kernel-argument copy lives as long as k_srs_points' secret)
void launch_srs_update(hipStream_t s, const uint32_t* tau_raw8, uint64_t first, uint32_t n, const void* d_level0, void* d_out_xyzz);
// d_err[0] (pre-set to 0xffffffff) = least index at infinity, d_err[1] = least index off the curve or outside G1
void launch_srs_check(hipStream_t s, const void* d_level0, uint32_t n, uint32_t* d_err);

// ---- bary_kernels.hip: barycentric evaluation of polynomials in evaluation form --------------------
constexpr uint32_t kBaryThreads = 256;       // lanes of a workgroup of the partial kernel
constexpr uint32_t kBaryRun = 4;             // indices per lane
constexpr uint32_t kBaryTile = kBaryThreads * kBaryRun;  // indices per workgroup: one Fr inversion each
constexpr uint32_t kBaryPartialWords = 12;   // a tile's record: nine digits of its sum, the index where z = w^i, padding
inline uint32_t bary_tiles(uint32_t log_n) { return (uint32_t)((((uint64_t)1 << log_n) + kBaryTile - 1) / kBaryTile); }
// d_out[b] = P_b(z_b) (canonical blst_fr) for polynomial b given by its 2^log_n values at d_evals + 8 b 2^log_n; d_zs: the
// points in multiplier form; d_tw: the forward NTT twiddles; inv_n: 1 / n in multiplier form; d_partial: batch x
// bary_tiles(log_n) records of kBaryPartialWords words
void launch_bary(hipStream_t s, const uint32_t* d_evals, uint32_t log_n, uint32_t batch, const Fr30* d_zs, const void* d_tw,
                 const Fr30& inv_n, uint32_t* d_partial, uint32_t* d_out);

// ---- lagrange_kernels.hip: the quotient of an opening taken on the values ---------------------------
constexpr uint32_t kLagTile = 1024;          // indices per workgroup: one Fr inversion each
constexpr uint32_t kLagPartialWords = 24;    // a tile's record: nine digits of each of its two sums, the index where z = w^i, a flag
inline uint32_t lagrange_tiles(uint32_t log_n) { return (uint32_t)((((uint64_t)1 << log_n) + kLagTile - 1) / kLagTile); }
// d_q[i] = (y - f_i) / (z - w^i) (2^log_n canonical values; the entry with w^i = z from the others) for P given by its 2^log_n
// values at d_evals; z, inv_n = 1 / n in multiplier form, y as the digits of its blst_fr image; d_tw: the context's four NTT
// twiddle tables (forward lo, hi, inverse lo, hi); d_partial: lagrange_tiles(log_n) records of kLagPartialWords words; d_flags:
// the job's 64 flag words, zero at launch: [0] = some value differs from f_0, [8..15] = P(z), [16..23] = f_0.
// d_q may not alias d_evals.
void launch_lagrange_quotient(hipStream_t s, const uint32_t* d_evals, uint32_t log_n, const Fr30& z, const Fr30& y, const Fr30& inv_n,
                              const void* d_tw, uint32_t* d_q, uint32_t* d_partial, uint32_t* d_flags);

// ---- grand_product_kernels.hip: z_0 = 1, z_(i+1) = z_i A_i / B_i with one inversion per call ----------
constexpr uint32_t kGpTile = 1024;           // consecutive indices per workgroup: 256 lanes x a run of 4
constexpr uint32_t kGpCarryThreads = 256;    // lanes of the carry kernel's one workgroup: <= 16 consecutive tiles each
constexpr uint32_t kGpPartialWords = 24;     // a tile's record: the digits of its product of A, then of B, the least index with B_i = 0
constexpr uint32_t kGpMaxColumns = 16;       // KZG_GP_MAX_COLUMNS
constexpr uint32_t kGpNone = 0xffffffffu;    // "no zero denominator"
inline uint32_t gp_tiles(size_t n) { return (uint32_t)((n + kGpTile - 1) / kGpTile); }
// The arguments both forms share.  d_z: n canonical blst_fr, may alias no input; d_partial: gp_tiles(n) records of
// kGpPartialWords words; d_flags: 16 words the carry kernel writes: [0] = the least i with B_i = 0 or kGpNone, [8..15] = z_n.
// scale: 2^(14 t) in multiplier form (takes a product of t images into multiplier form); img_one: the digits of the image of one.
struct GpOut {
    uint32_t* d_z;
    uint32_t* d_partial;
    uint32_t* d_flags;
};
// A_i = prod_j nums[i + j stride], B_i = prod_j dens[i + j stride] (t columns of n blst_fr each, stride in blst_fr)
void launch_grand_product(hipStream_t s, const uint32_t* d_nums, const uint32_t* d_dens, uint32_t n, uint32_t t, size_t stride,
                          const Fr30& scale, const Fr30& img_one, const GpOut& out);
// A_i = prod_j (f_j[i] + bk[j] w^i + gamma), B_i = prod_j (f_j[i] + beta sigma_j[i] + gamma) over the 2^log_n-domain.  bk: the t
// products beta k_j and gamma as the digits of their blst_fr images, beta in multiplier form; d_tw: the forward NTT twiddles.
void launch_permutation_product(hipStream_t s, const uint32_t* d_wires, const uint32_t* d_sigmas, uint32_t log_n, uint32_t t,
                                size_t stride, const Fr30* bk, const Fr30& beta, const Fr30& gamma, const void* d_tw,
                                const Fr30& scale, const Fr30& img_one, const GpOut& out);

// ---- lookup_kernels.hip: phi_0 = 0, phi_(i+1) = phi_i + sum_j a_j[i] / b_j[i] with one inversion per call, a batch inverse, and
// the multiplicities of a lookup through a hash table ----------------------------------------------------
constexpr uint32_t kLuTile = 512;            // consecutive rows per workgroup: 256 lanes x a run of 2
constexpr uint32_t kLuCarryThreads = 256;    // lanes of the carry kernel's one workgroup: <= 32 consecutive tiles each
constexpr uint32_t kLuMaxColumns = 16;       // KZG_LOGUP_MAX_COLUMNS
constexpr uint32_t kLuNone = 0xffffffffu;    // "no zero denominator", "no missing value", an empty slot of the hash table
// a tile's record, in words: the digits of its product of D, the least row with D_i = 0, the digits of W_T, of c_T (carry kernel),
// and base_T as 8 canonical limbs (carry kernel; 16-byte aligned)
constexpr uint32_t kLuRecD = 0, kLuRecHit = 9, kLuRecW = 10, kLuRecC = 20, kLuRecBase = 32, kLuPartialWords = 40;
inline uint32_t lu_tiles(size_t n) { return (uint32_t)((n + kLuTile - 1) / kLuTile); }
// d_phi: n canonical blst_fr, may alias no input; d_partial: lu_tiles(n) records of kLuPartialWords words; d_flags: 16 words the
// carry kernel writes: [0] = the least row with a zero denominator or kLuNone, [8..15] = phi_n.
// scale: 2^(14 t) in multiplier form (t: the columns per side, k + 1 in the lookup form, 1 for the batch inverse); img_one: the
// digits of the image of one.
struct LuOut {
    uint32_t* d_phi;
    uint32_t* d_partial;
    uint32_t* d_flags;
};
// t columns per side of n blst_fr each, stride in blst_fr; d_nums null: every numerator is one
void launch_logderivative_sum(hipStream_t s, const uint32_t* d_nums, const uint32_t* d_dens, uint32_t n, uint32_t t, size_t stride,
                              const Fr30& scale, const Fr30& img_one, const LuOut& out);
// sum_j 1 / (beta + f_j[i]) - m_i / (beta + T_i) over k lookup columns; beta as the digits of its image
void launch_lookup_sum(hipStream_t s, const uint32_t* d_lookups, uint32_t n, uint32_t k, size_t stride, const uint32_t* d_table,
                       const uint32_t* d_mult, const Fr30& beta, const Fr30& scale, const Fr30& img_one, const LuOut& out);
// out.d_phi[i] = 1 / vals[i]; flags as above ([8..15] is written and means nothing)
void launch_batch_inverse(hipStream_t s, const uint32_t* d_vals, uint32_t n, const Fr30& scale, const Fr30& img_one, const LuOut& out);
// The hash table of one call: 2^log_cap slots (set to kLuNone by the caller, on the stream), n_table counts (set to zero), two
// flag words (set to kLuNone): [0] the least lookup row holding a value in no table row, [1] the least table row whose walk hit
// the loop bound.  count_img: 2^256 in multiplier form.  d_out_rows may be null.  d_flags: >= 2 words, takes the two flag words.
struct LuHash {
    uint32_t* d_slots;
    uint32_t log_cap;
    uint32_t* d_counts;
    uint32_t* d_words;
};
void launch_lookup_multiplicities(hipStream_t s, const uint32_t* d_table, uint32_t n_table, const uint32_t* d_lookups, uint32_t n,
                                  uint32_t k, size_t stride, const LuHash& h, const Fr30& count_img, uint32_t* d_out_mult,
                                  uint32_t* d_out_rows, uint32_t* d_flags);

// ---- quotient_kernels.hip: the quotient of a permutation argument on the coset g H_N, g = 7 ------------
constexpr uint32_t kPqTile = 256;            // coset points per workgroup of k_pq_constraints: one per lane
constexpr uint32_t kPqMaxColumns = 7;        // KZG_PQ_MAX_COLUMNS: t + 1 <= rot <= 8
constexpr uint32_t kPqMaxLogExt = 3;         // KZG_PQ_MAX_LOG_EXT
// what k_pq_constraints reads: N = 2^log_N values per column on the coset (column j of the wires / sigmas at + 8 j stride words),
// d_gate null for G = 0, d_zinv: rot stored multipliers (canonical 8 x u32 of the x 2^270 form), 1 / Z_H(x_i) by i mod rot
struct PqColumns {
    const uint32_t *d_wires, *d_sigmas, *d_z, *d_l0, *d_gate, *d_zinv;
};
// its scalars: beta in multiplier form; gamma, one and the t products beta k_j g as the digits of their blst_fr images;
// alpha1 = alpha 2^(14 t) and alpha2 = alpha^2 2^14 in multiplier form (they take the products of images back to images)
struct PqScalars {
    const Fr30 *beta, *gamma, *one, *alpha1, *alpha2;
    const Fr30* bkg;  // t of them
};
// d_out[i] = Num(x_i) / Z_H(x_i), canonical, i < N; rot = N / n; d_out may alias no input; d_tw: the forward NTT twiddles
void launch_pq_constraints(hipStream_t s, const PqColumns& cols, uint32_t log_N, uint32_t rot, uint32_t t, size_t stride,
                           const PqScalars& sc, const void* d_tw, uint32_t* d_out);
// d_out[b N + i] = d_in[b stride + i] g^i c for i < len, 0 for len <= i < N (b < batch); d_in null: every input value is `fill`
// (digits of an image); d_gtab: the g^i tables; c in multiplier form.  d_out may not alias d_in.
void launch_pq_pad_twist(hipStream_t s, const uint32_t* d_in, size_t stride, uint32_t len, const Fr30& fill, uint32_t log_N,
                         uint64_t batch, const void* d_gtab, const Fr30& c, uint32_t* d_out);

// ---- circuit_kernels.hip: the quotient of a circuit with a resident key, the arithmetic gate built in ---
// what k_ck_constraints reads: N values per column on the coset, all blst_fr images.  The wires are the call's (column j at
// + 8 j stride words); q_lin and sigmas are the circuit's (column j at + 8 j N words); d_pi and d_gate may be null
struct CkColumns {
    const uint32_t *d_wires, *d_q_lin, *d_sigmas, *d_q_mul, *d_q_const, *d_z, *d_l0, *d_pi, *d_gate, *d_zinv;
};
// d_out[i] = Num(x_i) / Z_H(x_i) with the gate sum_j q_j f_j + q_M f_0 f_1 + q_C + PI + G' in Num, canonical, i < N; t >= 2;
// k14: 2^14 in multiplier form; the rest as launch_pq_constraints
void launch_ck_constraints(hipStream_t s, const CkColumns& cols, uint32_t log_N, uint32_t rot, uint32_t t, size_t stride,
                           const PqScalars& sc, const Fr30& k14, const void* d_tw, uint32_t* d_out);

// ---- lookup_circuit_kernels.hip: the lookup argument of a circuit whose key holds a table ---------------
// the scalars of both kernels: theta^j (j < c) in multiplier form; beta as the digits of its image; k14 = 2^14, ak14 = alpha 2^14
// and a3 = alpha^3 in multiplier form (k_lk_fold reads theta and k14 alone)
struct LkScalars {
    const Fr30 *theta, *beta, *k14, *ak14, *a3;
};
// d_out_f[i] = q_K[i] sum_j theta^j f_j[i], d_out_t[i] = sum_j theta^j tab_j[i], canonical, i < n: the first c wire columns
// (column j at + 8 j stride words), the c table columns (column j at + 8 j n words) and q_K, n blst_fr images each; 1 <= c <=
// kPqMaxColumns; the outputs overlap no input and not each other
void launch_lk_fold(hipStream_t s, const uint32_t* d_wires, size_t stride, const uint32_t* d_table, const uint32_t* d_qk, uint32_t n,
                    uint32_t c, const LkScalars& sc, uint32_t* d_out_f, uint32_t* d_out_t);
// what k_lk_constraints reads: N = 2^log_N values per column on the coset, all blst_fr images.  The wires are the call's (column j
// at + 8 j stride words), the table columns the circuit's (column j at + 8 j N words)
struct LkColumns {
    const uint32_t *d_wires, *d_table, *d_qk, *d_l0, *d_mult, *d_phi;
};
// d_out[i] = G'(x_i) = alpha^3 Lk1 + alpha^4 Lk2, canonical, i < N; rot = N / n; d_out may alias no input
void launch_lk_constraints(hipStream_t s, const LkColumns& cols, uint32_t log_N, uint32_t rot, uint32_t c, size_t stride,
                           const LkScalars& sc, uint32_t* d_out);

// ---- custom_gate_kernels.hip: the selector x wire-monomial terms of a custom circuit on the coset ---------
constexpr uint32_t kCgMaxTerms = 8;  // KZG_CIRCUIT_MAX_CUSTOM
// d_out[i] = G'(x_i) = sum_{s<g} qx_s[i] prod_{j<t} f_j[i]^exps[s t + j], canonical, i < N: the t wire columns on the coset (column j
// at + 8 j stride words), the g resident selector columns (column s at + 8 s N words), all blst_fr images; exps: g t bytes in 0..7,
// every row with a sum >= 1; k14: 2^14 in multiplier form.  1 <= t <= kPqMaxColumns, 1 <= g <= kCgMaxTerms; d_out aliases no input
void launch_cg_gate(hipStream_t s, const uint32_t* d_wires, size_t stride, const uint32_t* d_qx, uint32_t N, uint32_t t, uint32_t g,
                    const uint8_t* exps, const Fr30& k14, uint32_t* d_out);

// ---- custom_next_kernels.hip: the terms of a next-row circuit on the coset -------------------------------
// d_out[i] = G'(x_i) = sum_{s<g} qx_s[i] prod_{j<t} f_j[i]^exps[s t + j] f_j[(i + e) mod N]^exps_next[s t + j], canonical, i < N:
// launch_cg_gate's arguments, the second matrix (g t bytes in 0..7, every row sum of both matrices together >= 1) and e = N / n,
// 1 <= e < N, the distance on the coset of the domain's next row
void launch_cgn_gate(hipStream_t s, const uint32_t* d_wires, size_t stride, const uint32_t* d_qx, uint32_t N, uint32_t e, uint32_t t,
                     uint32_t g, const uint8_t* exps, const uint8_t* exps_next, const Fr30& k14, uint32_t* d_out);

// ---- combine_kernels.hip: F = sum gamma^i P_i and the values P_i(z) in one pass -------------------
constexpr uint32_t kCombineThreads = 256;     // lanes of a workgroup
constexpr uint32_t kCombineTile = 2048;       // consecutive indices per workgroup: lane l takes l + 256 m, m < 8
constexpr uint32_t kCombinePartialWords = 12; // a (polynomial, tile) record: nine digits, padded to 3 x 16 bytes
constexpr uint32_t kCombineMax = 256;         // polynomials per combination (KZG_MAX_COMBINE)
// the multipliers of one call, Fr30 records in multiplier form (x 2^270), prepared on the host:
constexpr uint32_t kCombineTabPa = 0;         // z^(16 e), e < 16
constexpr uint32_t kCombineTabPb = 16;        // z^e
constexpr uint32_t kCombineTabZ256 = 32;      // z^256
constexpr uint32_t kCombineTabWa = 33;        // W^(16 e), W = z^2048
constexpr uint32_t kCombineTabWb = 49;        // W^e
constexpr uint32_t kCombineTabW256 = 65;      // W^256
constexpr uint32_t kCombineTabGamma = 66;     // gamma^i, i < kCombineMax
constexpr uint32_t kCombineTabLen = kCombineTabGamma + kCombineMax;
inline uint32_t combine_tiles(uint32_t n) { return (uint32_t)(((uint64_t)n + kCombineTile - 1) / kCombineTile); }
// Polynomials first .. first + t of a combination (polynomial first + i: n coefficients at d_coeffs + 8 i stride words):
// d_f[j] (n canonical values) = (carry ? d_f[j] : 0) + sum_i gamma^(first + i) c_(i,j); d_ys[8 i ..] = P_(first + i)(z),
// canonical.  d_partial: t x combine_tiles(n) records of kCombinePartialWords words.  n >= 1, t <= kCombineMax.
void launch_combine_eval(hipStream_t s, const uint32_t* d_coeffs, uint32_t n, uint32_t t, uint64_t stride, const Fr30* d_tab,
                         uint32_t first, bool carry, uint32_t* d_f, uint32_t* d_partial, uint32_t* d_ys);
// Openings at several point sets: one pass per distinct point p.  d_tab: the 66 powers of p in the
// layout above; d_mult[j]: the multiplier gamma^i w_(g(i),p) of polynomial j of the pass, which sits at
// d_coeffs + 8 (d_sel[j] - sel_base) stride words.  d_g[k] (n canonical values) = (carry ? d_g[k] : 0) + sum_j mult_j c_(j,k);
// d_ys[8 j ..] = P_sel[j](p).  d_partial as above.
constexpr uint32_t kSetsMax = 8;          // point sets per call (KZG_MAX_SETS)
constexpr uint32_t kSetsMaxPoints = 16;   // distinct points over all sets (KZG_MAX_SET_POINTS)
constexpr uint32_t kSetsMaxValues = kCombineMax * kSetsMaxPoints;  // values of one call: sum_i |S_g(i)| <= 4096
void launch_sets_combine(hipStream_t s, const uint32_t* d_coeffs, uint32_t n, uint32_t t, uint64_t stride, const Fr30* d_tab,
                         const Fr30* d_mult, const uint32_t* d_sel, uint32_t sel_base, bool carry, uint32_t* d_g, uint32_t* d_partial,
                         uint32_t* d_ys);

// ---- linearise_kernels.hip: a weighted sum of columns in different buffers -------------------------
// d_out[i] (n canonical values) = sum_{k < ncols} mult_k C_k[i], plus konst at i = 0; d_y[0..8) = d_out(z), canonical, for the z
// whose 66 powers are at d_tab (the layout above).  Column k is the n blst_fr images at d_cols[k].coeffs, which d_out does not
// overlap; its multiplier is canonical, in the x 2^270 form (fr30_arg_from_mont256).  d_partial: combine_tiles(n) records of
// kCombinePartialWords words.  n >= 1, 1 <= ncols <= kLinMaxColumns.
constexpr uint32_t kLinMaxColumns = 32;
struct LinColumn {
    const uint32_t* coeffs;
    int32_t mult[9];  // the digits of an Fr30
    uint32_t pad;
};
static_assert(sizeof(LinColumn) == 48, "the device reads the records the host wrote");
struct LinConst {
    uint32_t l[8];  // a canonical blst_fr
};
void launch_lin_combine(hipStream_t s, const LinColumn* d_cols, uint32_t ncols, uint32_t n, const Fr30* d_tab, const LinConst& konst,
                        uint32_t* d_out, uint32_t* d_partial, uint32_t* d_y);

// ---- blind_kernels.hip: the blinders of a circuit proof in coefficient form -------------------------
// k columns of n canonical coefficients (column c at d_cols + 8 c stride words); d_lo, d_hi: nb <= kBlindLow canonical values
// per column (column c at + 8 c nb words).  Column c < k_hi: coefficient i < nb loses d_lo[c][i], index n + i receives d_hi[c][i]
// (less d_lo[c][n + i] where n + i < nb) and [n + nb, stride) is zeroed, stride >= n + nb.  A column from k_hi on only loses d_lo
// below n.  The blinders overlap no column.
constexpr uint32_t kBlindLow = 3;          // a blinder has at most three coefficients
constexpr uint32_t kBlindMaxColumns = 16;  // per-proof columns of the last round: t wires, z, e - 1 chunks of T
void launch_blind_patch(hipStream_t s, uint32_t* d_cols, uint32_t n, uint64_t k, uint64_t stride, const uint32_t* d_lo,
                        const uint32_t* d_hi, uint32_t nb, uint64_t k_hi);
// What the blinders add to a sum of launch_lin_combine: d_out holds n + ntail values, [0, n) written by that launch, d_y its value
// at z.  Column k contributes mult_k tail_k[i] at index n + i (i < tail_len <= ntail) and - mult_k low_k[i] at index i < kBlindLow
// (low null: nothing); [n, n + ntail) is written in full, d_y becomes d_out(z) over all n + ntail values.  d_pw: ntail + kBlindLow
// multipliers, z^(n + j) for j < ntail, then z^i.  kBlindLow <= ntail, ncols <= kBlindMaxColumns; tails, lows and d_out are
// canonical blst_fr images that do not overlap; multipliers canonical, x 2^270.
struct BlindColumn {
    const uint32_t* tail;
    const uint32_t* low;
    int32_t mult[9];  // the digits of an Fr30
    uint32_t tail_len;
};
static_assert(sizeof(BlindColumn) == 56, "the device reads the records the host wrote");
void launch_blind_tail(hipStream_t s, const BlindColumn* d_cols, uint32_t ncols, uint32_t n, uint32_t ntail, const Fr30* d_pw,
                       uint32_t* d_out, uint32_t* d_y);

// ---- multilinear_kernels.hip: folds, values and F of a multilinear opening ------------------------------
constexpr uint32_t kMlMaxVars = 22;      // KZG_ML_MAX_VARS
constexpr uint32_t kMlThreads = 256;     // lanes of a workgroup
constexpr uint32_t kMlTile = 2048;       // consecutive values of the source level per workgroup of k_ml_fold
constexpr uint32_t kMlLevels = 11;       // levels one launch of k_ml_fold writes: log2 of the tile
// up to 22 multipliers (u_i, or gamma^i) as the digits of Fr30 records in multiplier form, passed to the kernels by value
struct MlMultipliers {
    int32_t m[kMlMaxVars][9];
};
// The pyramid of f (n = 2^ell canonical values at d_evals): levels f_1 .. f_ell, n - 1 canonical values at d_pyr, level i at
// offset n - (n >> (i - 1)).  One launch for ell <= 11, two above.  d_pyr overlaps no input.
void launch_ml_fold(hipStream_t s, const uint32_t* d_evals, uint32_t ell, const MlMultipliers& us, uint32_t* d_pyr);
// d_ys[8 (3 i + p) ..] = f_i(r), f_i(-r), f_i(r^2) for i < ell, canonical.  d_tab: the 66 powers of r in launch_combine_eval's
// layout, then the 66 powers of r^2; d_partial: 3 ell combine_tiles(n) records of kCombinePartialWords words.
void launch_ml_eval(hipStream_t s, const uint32_t* d_evals, const uint32_t* d_pyr, uint32_t ell, const Fr30* d_tab,
                    uint32_t* d_partial, uint32_t* d_ys);
// d_f[j] = sum_{i < ell, j < n >> i} gam_i f_i[j] (gam_0 is not read: it is one), n canonical values; d_f overlaps no input
void launch_ml_combine(hipStream_t s, const uint32_t* d_evals, const uint32_t* d_pyr, uint32_t ell, const MlMultipliers& gam,
                       uint32_t* d_f);

// ---- multi.hip: a context spanning several devices (SRS-range slices, RCCL exchange of the partials) ------------
}  // namespace kzg
#include <string>
struct kzg_ctx;
namespace kzg {
// ---- api.hip: single-device pieces the multi-device context drives (never exported) ------------------------------
// A kid of a range-split context returns its partial sums UN-normalised (Jacobian X*ZZ, Y*ZZZ, ZZ of the XYZZ total:
// two products instead of an inversion); the parent normalises once after the K-1 additions.
void ctx_set_raw_partials(kzg_ctx* ctx, bool raw);
// A kid of a multi-device context gives up its SRS (multi.hip: its slice is empty now, or a sibling's slice was refused):
// kzg_srs_len(ctx) is 0 afterwards and every call that needs an SRS answers KZG_ERR_NO_SRS
int ctx_drop_srs(kzg_ctx* ctx);
// Host-pointer batches on ONE device: polynomial i (i < count) is the caller's polynomial first + i * step, its n
// coefficients at coeffs + (first + i * step) * stride_coeffs blst_fr values, its result at out_p1s + 18 * (first + i *
// step) (and statuses[first + i * step]).  Sub-batches flow through the context's stream slots so that the upload of
// one overlaps the kernels of the previous ones.
int ctx_commit_batch_host(kzg_ctx* ctx, const uint64_t* coeffs, size_t n, size_t stride_coeffs, size_t first, size_t step,
                          size_t count, uint64_t* out_p1s);
int ctx_open_batch_host(kzg_ctx* ctx, const uint64_t* coeffs, size_t n, size_t stride_coeffs, size_t first, size_t step,
                        size_t count, const uint64_t* zs, const uint64_t* ys, uint64_t* out_p1s, int* statuses);
// One device's share of a range-sharded opening (multi.hip): the slice is uploaded ONCE.  begin: slice -> the slot's
// staging buffer, H = sum_i slice[i] z^i (the quotient scan without output); finish: the carry becomes coefficient
// `len` of the staged slice, which is opened at z with claimed value `start`.  The slot stays reserved in between;
// ctx_open_slice_abort releases it when the recurrence on the host refuses the opening.
int ctx_open_slice_begin(kzg_ctx* ctx, const uint64_t* slice, size_t len, const uint64_t z[4], uint64_t out_h[4], int* slot_out);
int ctx_open_slice_finish(kzg_ctx* ctx, int slot, size_t len, const uint64_t carry[4], const uint64_t z[4],
                          const uint64_t start[4], uint64_t out_p1[18]);
void ctx_open_slice_abort(kzg_ctx* ctx, int slot);

struct MultiState;
enum : uint32_t { kMultiRange = 0, kMultiReplicate = 1 };
int multi_create(const int* devices, int ndev, uint32_t mode, MultiState** out, std::string& err);
void multi_destroy(MultiState* m);
size_t multi_srs_len(const MultiState* m);
int multi_num_devices(const MultiState* m);
uint64_t multi_rccl_exchanges(const MultiState* m);
kzg_ctx* multi_kid(MultiState* m, int g);
const char* multi_last_error(const MultiState* m);
int multi_srs_generate(MultiState* m, const uint8_t secret_be[32], uint64_t first, size_t n);
int multi_srs_load(MultiState* m, const void* first_g1, size_t stride, size_t n);
int multi_srs_load_affine(MultiState* m, const void* affine_xy, size_t n);
int multi_srs_load_compressed(MultiState* m, const uint8_t* compressed, size_t n, size_t* bad_index);
int multi_srs_read(MultiState* m, size_t index, size_t count, uint64_t* out_p1);
int multi_commit(MultiState* m, const void* scalars, int is_mont, size_t n, uint64_t out_p1[18]);
int multi_open(MultiState* m, const uint64_t* coeffs, size_t n, const uint64_t z[4], const uint64_t y[4], uint64_t out_p1[18]);
int multi_commit_batch(MultiState* m, const uint64_t* coeffs, size_t n, size_t batch, size_t stride_coeffs, uint64_t* out_p1s);
int multi_open_batch(MultiState* m, const uint64_t* coeffs, size_t n, size_t batch, size_t stride_coeffs, const uint64_t* zs,
                     const uint64_t* ys, uint64_t* out_p1s, int* statuses);
int multi_open_points(MultiState* m, const uint64_t* coeffs, size_t n, const uint64_t* zs, const uint64_t* ys, size_t k,
                      uint64_t out_p1[18]);
int multi_open_combined(MultiState* m, const uint64_t* coeffs, size_t n, size_t t, size_t stride, const uint64_t z[4],
                        const uint64_t gamma[4], uint64_t* out_ys, uint64_t out_p1[18]);
int multi_open_sets(MultiState* m, const uint64_t* coeffs, size_t n, size_t t, size_t stride, const uint32_t* set_of,
                    const uint32_t* set_len, size_t nsets, const uint64_t* zs, const uint64_t gamma[4], uint64_t* out_ys,
                    uint64_t out_p1[18]);
int multi_set_max_batch(MultiState* m, size_t max_batch);
uint32_t multi_mode(const MultiState* m);

// ---- poly_kernels.hip -------------------------------------------------------------------
struct PolyScratch {
    uint32_t* d_chunk;   // per-thread chunk values / carries (Fr)
    uint32_t* d_block;   // per-block aggregates (Fr)
    uint32_t* d_flags;   // the job's flag words, zero at launch: [0] = any non-zero coefficient with index >= 1, [16..23] receive c[0]
    uint32_t* d_result;  // P(z) (8 words)
};
// raises the dynamic-LDS limit of the scan kernels on the current device (kzg_ctx_create); false when refused
bool poly_prepare_device();
size_t poly_chunk_words(uint32_t n);
size_t poly_block_words(uint32_t n);
// suffix Horner scan S[i] = sum_{k>=i} c[k] z^(k-i):  q[i-1] = S[i] (i >= 1) when d_q != nullptr,
// P(z) = S[0] to scratch.d_result; flags as above.  z in Montgomery form (8 words, host copy).
// n <= 4096: one launch that also fills the slot's 64 flag words completely (P(z) at +8, c[0] at +16, flag at +0,
// zeros elsewhere); returns false (nothing enqueued) for larger n.
bool launch_quotient_single(hipStream_t s, const uint32_t* d_coeffs, uint32_t n, const uint32_t z_mont[8], uint32_t* d_q,
                            uint32_t* d_small);
void launch_quotient(hipStream_t s, const uint32_t* d_coeffs, uint32_t n, const uint32_t z_mont[8],
                     uint32_t* d_q, PolyScratch scratch);
// Several roots at once (KZG multiproofs): q = sum_i w_i Q_i with Q_i the single-root quotient at z_i and
// w_i = 1 / prod_{j != i} (z_i - z_j); P(z_i) is written to d_vals[8 i .. 8 i + 8) (canonical blst_fr image).
// The per-root multipliers live in device memory: points_fill_roots writes k records of points_root_bytes() each into
// host memory (z_i, w_i in Montgomery form, 4 x u64 each), the caller copies them to d_roots.  d_block:
// k * poly_block_words(n) words.  q[0 .. nq) is written when d_q != nullptr and nq > 0 (nq <= n - 1).
bool points_prepare_device();
size_t points_root_bytes();
void points_fill_roots(void* h_roots, const uint64_t* zs_mont, const uint64_t* ws_mont, uint32_t k, uint32_t n);
void launch_quotient_points(hipStream_t s, const uint32_t* d_coeffs, uint32_t n, const void* d_roots, uint32_t k, uint32_t* d_q,
                            uint32_t nq, uint32_t* d_block, uint32_t* d_vals);
// A source polynomial per root (openings at several point sets): h = sum_r Q(G_r, z_r) with G_r the n
// canonical values at d_g + 8 r n words and the roots as above (the weights are not read: they are inside the G_r already).
// h[0 .. n - 1) is written to d_q (nothing for n < 2); k <= kSetsMaxPoints; d_block: k * poly_block_words(n) words; d_vals:
// 8 k words the block stage may write.
bool sets_prepare_device();
void launch_quotient_sets(hipStream_t s, const uint32_t* d_g, uint32_t n, const void* d_roots, uint32_t k, uint32_t* d_q,
                          uint32_t* d_block, uint32_t* d_vals);

// ---- blobproof_kernels.hip ---------------------------------------
// The quotients of `batch` polynomials of n <= kBlobProofMaxN coefficients (polynomial b at d_coeffs + 8 b stride words), each at
// its own point, in one launch: q_b (n - 1 canonical values) to d_q + 8 b (n - 1) words (d_q may be null: values only), and
// polynomial b's 32 flag words to d_flags + 32 b, written in full -- [0] = any non-zero coefficient with index >= 1, [8..15] =
// P_b(z_b), [16..23] = c_0, zero elsewhere.  d_z: batch x kBlobProofZWords words, the first nine the digits of z_b * 2^270
// (fr30_arg_from_mont256).  Returns false (nothing enqueued) for n = 0 or n above the limit.
constexpr uint32_t kBlobProofMaxN = 4096;
constexpr uint32_t kBlobProofZWords = 12;
bool launch_blobproof_quotients(hipStream_t s, const uint32_t* d_coeffs, uint32_t n, uint64_t stride, uint32_t batch,
                                const uint32_t* d_z, uint32_t* d_q, uint32_t* d_flags);

}  // namespace kzg
