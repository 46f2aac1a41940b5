// lookup_kernels.hip -- the running sum of a log-derivative (LogUp) lookup argument, a batch inverse, and the multiplicities of a
// lookup found through a hash table on the device (kzg_logderivative_sum, kzg_lookup_sum, kzg_lookup_commit, kzg_batch_inverse,
// kzg_lookup_multiplicities).
//
// t numerator columns a_j and t denominator columns b_j of n values each:
//
//     phi_0 = 0,   phi_(i+1) = phi_i + sum_j a_j[i] / b_j[i]   (i < n),   last = phi_n
//
// Per row the fractions are added with a running pair, (N, D) <- (N b_j + a_j D, D b_j), so that N_i / D_i is the row's sum, and
//     1 / D_i = (prod_{k<i} D_k) (prod_{k>i} D_k) / (prod_{all k} D_k)                       -- ONE inversion for the whole call.
// Inside a tile T of kLuTile consecutive rows, with the tile-local exclusive prefix P_i and exclusive suffix S_i of D:
//     w_i = N_i P_i S_i,   c_T = (prod of D over the tiles before T) (prod of D over the tiles after T) / D_total,
//     s_i = sum_{k<i, k in T} w_k,   W_T = sum_{k in T} w_k,   base_T = sum_{T' < T} c_T' W_T',   phi_i = base_T + c_T s_i.
// The lookup form (k lookup columns f_j, a table column T, its multiplicities m, a challenge beta) never stores its columns:
//     a_j = 1, b_j[i] = beta + f_j[i]  (j < k);    a_k[i] = -m_i, b_k[i] = beta + T_i.
//
// Kernels of the sums:
//   k_lu_tile, k_lu_tile_lookup, k_lu_tile_inv   one body over three element steps (three kernels, so that the general form
//                    carries neither the lookup form's arguments nor its element step, and the batch inverse neither numerators
//                    nor the additive scan).  grid = tiles of kLuTile consecutive rows, 256 lanes; lane l owns the run of 2
//                    CONSECUTIVE rows tile + 2 l + k.  It forms N_i and D_i, scans the run products of D over the lanes in LDS
//                    (inclusive prefix and inclusive suffix, digit planes, double buffered), forms u_i = P_i S_i and
//                    w_i = N_i u_i, scans w_0 + w_1 additively over the lanes in the same planes and stores s_i (the batch
//                    inverse: u_i) into the output.  Record of the tile: the product of its D, W_T, the least row with D_i = 0.
//   k_lu_carry       one workgroup of kLuCarryThreads lanes; lane l owns the <= 32 consecutive tiles [l run, (l + 1) run).
//                    The two product scans over the lanes, lane 0 inverts the product of every D -- its own scan result, in
//                    its own registers: the call's only fr30_inv --, each lane walks its tiles forwards (prefix of D) and
//                    backwards (suffix of D) leaving c_T, sums its c_T W_T, the lanes scan those sums additively, and a last
//                    walk leaves base_T as a canonical residue.  Writes last and the least row with a zero denominator.
//   k_lu_finish      phi_i = s_i c_T + base_T in place, streaming, lane l of tile T takes T + 256 j + l.
//
// Forms (fr30.hip.h; fr30_mul(a, b) = a b / 2^270).  An IMAGE is x 2^256 (what the ABI holds), a MULTIPLIER x 2^270.
// image x multiplier = image, multiplier x multiplier = multiplier, image x image = x y 2^242: neither.
//   a_j[i], b_j[i]   images: loaded; in the lookup form beta + f, beta + T are sums of two images, 1 is the image of one (an
//                    argument) and -m_i the digit-wise negation of the loaded image.  With nums == NULL every a_j is that
//                    same image of one: the arithmetic is the one of explicit columns of ones, so the outputs are equal.
//   (N, D)           start as (a_0, b_0): X 2^256.  A step takes X 2^e to X 2^(e - 14) in BOTH (N b + a D and D b are sums and
//                    products of one value of each kind), so N_i and D_i carry the same power: X 2^(270 - 14 t) after t columns.
//   N_i, D_i         that x `scale`, scale = 2^(270 + 14 t) prepared by the host: X 2^270, MULTIPLIERS.  Rows past n stand in
//                    as D = 2^270 (fr30_const_one270, the neutral element) and N = 0.
//   u_i, w_i, s_i, W_T, the D records   products and sums of multipliers: MULTIPLIERS (s_i and u_i stored as canonical residues).
//   1 / D_total      fr30_inv of a multiplier is a multiplier; one product with img_one makes it the IMAGE of 1 / D_total.
//   c_T              (multiplier x that image) x multiplier: an IMAGE.   c_T W_T, base_T, last: IMAGES.
//   phi_i            s_i c_T + base_T = multiplier x image + image: an IMAGE, stored canonical.  phi_0 = 0 c_0 + 0: the image of
//                    zero, limb for limb.
//   counts           a count c < 2^26 is the digit vector {c, 0, ..}; x the multiplier form of 2^256 (count_img, from the host)
//                    it is the IMAGE of c.
//
// Bounds.  A loaded value is canonical, [0, r), in carry-normalised digits (fr30_from_limbs: digits 0..7 within
// [-2^29 - 4, 2^29 + 4]).  A product returns |v| <= 0.5001 r + |a b| / 2^270 with digits 0..7 in [-2^29, 2^29); r / 2^270 < 2^-15.
//   beta + f         one carry pass over two normalised values (fr30_add): [0, 2 r), normalised digits, top digit < 2 x 0x73ee.
//                    An operand of products ONLY; never tested for zero, never stored.  The same for -m_i in (-r, 0].
//   N b + a D        fr30_add of two products: |v| <= 1.0002 r + 2 x (2 r x 2 r) / 2^270 < 1.001 r, normalised digits; an operand
//                    of the next step's product and of the product with `scale` only.
//   D_i              a product (with `scale`), |v| <= 0.5001 r + r / 2^13: inside the (-r, 2 r) that fr30_to_limbs canonicalises.
//                    The zero test is made HERE, on the canonical residue of a product, never on a raw sum; D_i is zero exactly
//                    when one b_j[i] is (the field has no zero divisors).
//   every product scan, P_i, S_i, u_i, w_i, the D records, c_T   products of products: |v| <= 0.5001 r + r / 2^14.
//   the tile's additive scan   every step is a fr30_add (one carry pass over the raw sum of two normalised values): digits 0..7 stay
//                    normalised, the top digit -- value / 2^240, never reduced -- grows.  At most kLuTile = 512 terms of
//                    magnitude <= 0.5002 r: |sum| <= 256.2 r < 2^263 (r < 0.453 x 2^256), top digit below 256.2 x 0x73ee + 1
//                    < 2^23.  Such a sum is an operand of ONE product, fr30_sum_reduce (x the multiplier form of
//                    one): the product columns stay below 9 x 2^30 x 2^30 < 2^63, and the result is
//                    |v| <= 0.5001 r + 256.2 r x 0.5 r / 2^270 < 0.505 r, which fr30_to_limbs takes (s_i) or the record holds (W_T).
//   the carry kernel's sums    a lane sums <= 32 products c_T W_T (|each| <= 0.506 r: W_T is below 0.505 r): <= 16.2 r, reduced by
//                    fr30_sum_reduce to <= 0.5003 r before the lanes' scan; 256 of those: <= 128.1 r; plus the <= 16.2 r of the
//                    lane's own walk: |base| <= 144.3 r < 2^263, top digit < 2^23.  base_T and last go through fr30_sum_reduce
//                    (<= 0.503 r) and fr30_to_limbs: base_T is stored CANONICAL, [0, r), so that
//   phi_i            = s_i c_T (a product of a canonical value, |v| <= 0.5001 r + r / 2^15) + base_T in [0, r) lies in
//                    (-0.51 r, 1.51 r), inside what fr30_to_limbs canonicalises; the raw sum's digits stay below 2^30 + 4.
//   Nothing outside (-r, 2 r) goes through fr30_to_limbs.
//
// Multiplicities (kzg_lookup_multiplicities).  An open-addressing table of 2^log_cap uint32 slots, each empty (kLuNone) or the
// index of a table row; the key is the row's 32 bytes as given, compared limb for limb; the home slot is a hash of all eight
// limbs (images of small or structured values differ in few bits).
//   k_lu_build       one lane per table row r: from the home slot, atomicCAS(empty -> r); on an occupied slot the lane reads the
//                    value of the row the slot names (the table is read-only); equal -> atomicMin(slot, r) and stop; else the
//                    next slot.  A slot never becomes empty again and never changes its value, so every distinct value ends in
//                    exactly one slot, holding its least row, whatever the arrival order.
//   k_lu_probe       one lane per looked-up value: the same walk read-only.  A hit adds one to the row's count -- the lanes of a
//                    wave that hit the same row are combined first, one atomicAdd per distinct row of the wave (padding rows
//                    all look up one value) -- and goes to out_rows; an empty slot, or the loop bound, is a miss: atomicMin of the
//                    row i on a flag word.
//   k_lu_counts      the uint32 counts as images; hands the two flag words to the host.
// No lane waits for another: no spinning, no lock.  Every walk is bounded by the capacity and leaves through a flag word when
// the bound is hit; a capacity >= n_table guarantees the build a free or equal slot inside that bound.  Only atomicCAS, atomicMin
// and atomicAdd on global memory are used.  Every index read from a slot is a row some lane of k_lu_build stored: below n_table.
#include <hip/hip_runtime.h>

#include "engine.h"
#include "fr30.hip.h"
#include "fr30_lanes.hip.h"

namespace kzg {

namespace {

constexpr uint32_t kLuThreads = 256;
constexpr uint32_t kLuRun = 2;
static_assert(kLuThreads * kLuRun == kLuTile, "tile shape");
static_assert(kLuCarryThreads == kLuThreads, "both scans run over 256 lanes");
static_assert(((1u << kNttMaxLog) + kLuTile - 1) / kLuTile <= 32 * kLuCarryThreads, "a lane of the carry kernel owns <= 32 tiles");
static_assert(kLuRecW + kR9 <= kLuRecC && kLuRecC + kR9 <= kLuRecBase && kLuRecBase + 8 <= kLuPartialWords && kLuRecBase % 4 == 0 &&
                  kLuPartialWords % 4 == 0,
              "record layout");

__device__ __forceinline__ Fr30 lu_neg(const Fr30& a) {
    Fr30 v;
#pragma unroll
    for (int k = 0; k < kR9; k++) v.d[k] = -a.d[k];
    return v;
}

// digit planes of 256 values in LDS
using LuPlane = Fr30Plane<kLuThreads>;
// The additive scan over the 256 lanes: on return pl[cur] holds the sums of a over lanes [0, t] and a is the lane's own entry.
// Every lane has left the planes' earlier contents behind (the caller's barrier).  Each step is one carry pass over two
// normalised values; the top digit grows with the sum (the header's bound).
__device__ __forceinline__ uint32_t lu_scan_add(LuPlane (&pl)[2], uint32_t t, Fr30& a) {
    uint32_t cur = 0;
#pragma unroll 1
    for (uint32_t o = 1; o < kLuThreads; o <<= 1) {
        plane_put(pl[cur], t, a);
        __syncthreads();
        if (t >= o) a = fr30_add(plane_get(pl[cur], t - o), a);
        cur ^= 1;
    }
    plane_put(pl[cur], t, a);
    __syncthreads();
    return cur;
}

// what the three forms read
struct LuColumns {  // t columns each, column j at + 8 j stride words; nums null: every numerator is one
    const uint32_t* nums;
    const uint32_t* dens;
    Fr30 one;  // the digits of the image of one
};
struct LuLookup {  // k = t - 1 lookup columns, the table column and its multiplicities
    const uint32_t* lookups;
    const uint32_t* table;
    const uint32_t* mult;
    Fr30 beta;  // image
    Fr30 one;
};
struct LuValues {
    const uint32_t* vals;
};

// N_i and D_i before the product with `scale`: X 2^(270 - 14 t)
__device__ __forceinline__ void lu_element(const LuColumns& in, uint32_t i, uint32_t t, size_t stride, Fr30& nn, Fr30& dd) {
    const uint32_t* pb = in.dens + 8 * (size_t)i;
    const uint32_t* pa = in.nums ? in.nums + 8 * (size_t)i : nullptr;
    dd = fr30_load(pb);
    nn = pa ? fr30_load(pa) : in.one;
#pragma unroll 1
    for (uint32_t j = 1; j < t; j++) {
        pb += 8 * stride;
        if (pa) pa += 8 * stride;
        const Fr30 b = fr30_load(pb);
        const Fr30 a = pa ? fr30_load(pa) : in.one;
        nn = fr30_add(fr30_mul(nn, b), fr30_mul(a, dd));  // < 1.001 r: an operand only
        dd = fr30_mul(dd, b);
    }
}
__device__ __forceinline__ void lu_element(const LuLookup& in, uint32_t i, uint32_t t, size_t stride, Fr30& nn, Fr30& dd) {
    const uint32_t* pf = in.lookups + 8 * (size_t)i;
    dd = fr30_add(fr30_load(pf), in.beta);  // [0, 2 r): an operand only
    nn = in.one;
#pragma unroll 1
    for (uint32_t j = 1; j + 1 < t; j++) {
        pf += 8 * stride;
        const Fr30 b = fr30_add(fr30_load(pf), in.beta);
        nn = fr30_add(fr30_mul(nn, b), fr30_mul(in.one, dd));
        dd = fr30_mul(dd, b);
    }
    const Fr30 b = fr30_add(fr30_load(in.table + 8 * (size_t)i), in.beta);
    const Fr30 a = lu_neg(fr30_load(in.mult + 8 * (size_t)i));  // (-r, 0]
    nn = fr30_add(fr30_mul(nn, b), fr30_mul(a, dd));
    dd = fr30_mul(dd, b);
}
__device__ __forceinline__ void lu_element(const LuValues& in, uint32_t i, uint32_t, size_t, Fr30& nn, Fr30& dd) {
    dd = fr30_load(in.vals + 8 * (size_t)i);
    nn = dd;  // not used
}

// N_i and D_i of one row as multipliers; 0 and the neutral element past n; *hit takes the row when D_i = 0
template <bool kSum, class In>
__device__ __forceinline__ void lu_row(const In& in, uint32_t i, uint32_t n, uint32_t t_cols, size_t stride, const Fr30& scale,
                                       const Fr30& one, Fr30& nn, Fr30& dd, uint32_t* hit) {
    nn = fr30_zero();
    dd = one;
    if (i < n) {
        lu_element(in, i, t_cols, stride, nn, dd);
        dd = fr30_mul(dd, scale);
        if constexpr (kSum) nn = fr30_mul(nn, scale);
        if (fr30_is_zero(dd)) atomicMin(hit, i);
    }
}

template <bool kSum, class In>
__device__ __forceinline__ void lu_tile_body(const In& in, uint32_t n, uint32_t t_cols, size_t stride, const Fr30& scale,
                                             uint32_t* __restrict__ out, uint32_t* __restrict__ partial) {
    __shared__ LuPlane pre[2], suf[2];
    __shared__ uint32_t hit_s;
    const uint32_t t = threadIdx.x, tile = blockIdx.x;
    const uint32_t base = tile * kLuTile + t * kLuRun;
    const Fr30 one = fr30_const_one270();
    if (t == 0) hit_s = kLuNone;
    __syncthreads();
    // (two calls, not a loop over an array: the element step's own loop is not unrolled, and the values stay in registers)
    Fr30 nn[kLuRun], dd[kLuRun];
    lu_row<kSum>(in, base, n, t_cols, stride, scale, one, nn[0], dd[0], &hit_s);
    lu_row<kSum>(in, base + 1, n, t_cols, stride, scale, one, nn[1], dd[1], &hit_s);
    Fr30 mp = fr30_mul(dd[0], dd[1]), ms = mp;
    const uint32_t cur = fr30_scan_products(pre, suf, t, mp, ms);
    uint32_t* rec = partial + (size_t)tile * kLuPartialWords;
    if (t == kLuThreads - 1) fr30_put_digits(rec + kLuRecD, mp);
    if (t == 0) rec[kLuRecHit] = hit_s;
    // u_i = (D over the tile's rows before i) x (D over the tile's rows after i)
    const Fr30 pl = t > 0 ? plane_get(pre[cur], t - 1) : one;
    const Fr30 sl = t + 1 < kLuThreads ? plane_get(suf[cur], t + 1) : one;
    const Fr30 u0 = fr30_mul(pl, fr30_mul(dd[1], sl)), u1 = fr30_mul(fr30_mul(pl, dd[0]), sl);
    if constexpr (!kSum) {
        if (base < n) fr30_store(out + 8 * (size_t)base, u0);
        if (base + 1 < n) fr30_store(out + 8 * (size_t)(base + 1), u1);
        if (t == 0) fr30_put_digits(rec + kLuRecW, fr30_zero());
    } else {
        const Fr30 w0 = fr30_mul(nn[0], u0), w1 = fr30_mul(nn[1], u1);
        Fr30 a = fr30_add(w0, w1);
        __syncthreads();  // every lane has read its pl and sl: the planes are free for the additive scan
        const uint32_t c2 = lu_scan_add(pre, t, a);
        const Fr30 e = t > 0 ? plane_get(pre[c2], t - 1) : fr30_zero();
        if (base < n) fr30_store(out + 8 * (size_t)base, fr30_sum_reduce(e));
        if (base + 1 < n) fr30_store(out + 8 * (size_t)(base + 1), fr30_sum_reduce(fr30_add(e, w0)));
        if (t == kLuThreads - 1) fr30_put_digits(rec + kLuRecW, fr30_sum_reduce(a));
    }
}

__global__ void __launch_bounds__(kLuThreads) k_lu_tile(LuColumns in, uint32_t n, uint32_t t_cols, size_t stride, Fr30 scale,
                                                        uint32_t* __restrict__ out, uint32_t* __restrict__ partial) {
    lu_tile_body<true>(in, n, t_cols, stride, scale, out, partial);
}
__global__ void __launch_bounds__(kLuThreads) k_lu_tile_lookup(LuLookup in, uint32_t n, uint32_t t_cols, size_t stride, Fr30 scale,
                                                               uint32_t* __restrict__ out, uint32_t* __restrict__ partial) {
    lu_tile_body<true>(in, n, t_cols, stride, scale, out, partial);
}
__global__ void __launch_bounds__(kLuThreads) k_lu_tile_inv(LuValues in, uint32_t n, Fr30 scale, uint32_t* __restrict__ out,
                                                            uint32_t* __restrict__ partial) {
    lu_tile_body<false>(in, n, 1, 0, scale, out, partial);
}

__global__ void __launch_bounds__(kLuCarryThreads) k_lu_carry(uint32_t tiles, Fr30 img_one, uint32_t* __restrict__ partial,
                                                              uint32_t* __restrict__ flags) {
    __shared__ LuPlane pre[2], suf[2];
    __shared__ int32_t inv_s[kR9];
    __shared__ int32_t arg_s[kR9];  // img_one for lane 0: read back into vector registers, not held in scalar ones
    __shared__ uint32_t hit_s;
    const uint32_t t = threadIdx.x;
    const uint32_t run = (tiles + kLuCarryThreads - 1) / kLuCarryThreads;
    const uint32_t first = min(t * run, tiles), end = min(first + run, tiles);
    const Fr30 one = fr30_const_one270();
    if (t == 0) {
        hit_s = kLuNone;
#pragma unroll
        for (int k = 0; k < kR9; k++) arg_s[k] = img_one.d[k];
    }
    __syncthreads();
    Fr30 mp = one;
    uint32_t hit = kLuNone;
#pragma unroll 1
    for (uint32_t k = first; k < end; k++) {
        const uint32_t* rec = partial + (size_t)k * kLuPartialWords;
        mp = fr30_mul(mp, fr30_digits(rec + kLuRecD));
        hit = min(hit, rec[kLuRecHit]);
    }
    if (hit != kLuNone) atomicMin(&hit_s, hit);
    Fr30 ms = mp;
    const uint32_t cur = fr30_scan_products(pre, suf, t, mp, ms);  // ms of lane 0: every D
    if (t == 0) {
        // the product of every D is zero exactly when some D_i is: fr30_inv(0) = 0 and the call only reports
        Fr30 io;
#pragma unroll
        for (int k = 0; k < kR9; k++) io.d[k] = arg_s[k];
        const Fr30 inv = fr30_mul(fr30_inv(ms), io);  // the image of 1 / D_total
#pragma unroll
        for (int k = 0; k < kR9; k++) inv_s[k] = inv.d[k];
        flags[0] = hit_s;
    }
    __syncthreads();
    Fr30 p;
#pragma unroll
    for (int k = 0; k < kR9; k++) p.d[k] = inv_s[k];
    if (t > 0) p = fr30_mul(plane_get(pre[cur], t - 1), p);  // (D over the tiles of the lanes before) / D_total: an image
    Fr30 s = t + 1 < kLuCarryThreads ? plane_get(suf[cur], t + 1) : one;
    // forwards: the tile's c takes preD_k / D_total
#pragma unroll 1
    for (uint32_t k = first; k < end; k++) {
        uint32_t* rec = partial + (size_t)k * kLuPartialWords;
        fr30_put_digits(rec + kLuRecC, p);
        p = fr30_mul(p, fr30_digits(rec + kLuRecD));
    }
    // backwards: ... times sufD_k, the product of D over the tiles after k: c_T.  The lane's sum of c_T W_T on the way.
    Fr30 tot = fr30_zero();
#pragma unroll 1
    for (uint32_t k = end; k > first; k--) {
        uint32_t* rec = partial + (size_t)(k - 1) * kLuPartialWords;
        const Fr30 c = fr30_mul(fr30_digits(rec + kLuRecC), s);
        fr30_put_digits(rec + kLuRecC, c);
        tot = fr30_add(tot, fr30_mul(c, fr30_digits(rec + kLuRecW)));
        s = fr30_mul(s, fr30_digits(rec + kLuRecD));
    }
    tot = fr30_sum_reduce(tot);
    __syncthreads();  // every lane has read its prefix and suffix: the planes are free for the additive scan
    const uint32_t c2 = lu_scan_add(pre, t, tot);
    if (t == kLuCarryThreads - 1) fr30_store(flags + 8, fr30_sum_reduce(tot));  // last = phi_n
    // forwards again: base_T, canonical
    Fr30 b = t > 0 ? plane_get(pre[c2], t - 1) : fr30_zero();
#pragma unroll 1
    for (uint32_t k = first; k < end; k++) {
        uint32_t* rec = partial + (size_t)k * kLuPartialWords;
        fr30_store(rec + kLuRecBase, fr30_sum_reduce(b));
        b = fr30_add(b, fr30_mul(fr30_digits(rec + kLuRecC), fr30_digits(rec + kLuRecW)));
    }
}

__global__ void __launch_bounds__(kLuThreads) k_lu_finish(uint32_t n, const uint32_t* __restrict__ partial, uint32_t* __restrict__ phi) {
    const uint32_t tile = blockIdx.x;
    const uint32_t* rec = partial + (size_t)tile * kLuPartialWords;
    const Fr30 c = fr30_digits(rec + kLuRecC);
    const Fr30 b = fr30_load(rec + kLuRecBase);
#pragma unroll
    for (uint32_t j = 0; j < kLuRun; j++) {
        const uint32_t i = tile * kLuTile + j * kLuThreads + threadIdx.x;
        if (i < n) {
            uint32_t* p = phi + 8 * (size_t)i;
            fr30_store(p, fr30_add_raw(fr30_mul(fr30_load(p), c), b));
        }
    }
}

// ---- multiplicities ------------------------------------------------------------------------------------------------------------
struct LuKey {
    uint32_t w[8];
};
__device__ __forceinline__ LuKey lu_key(const uint32_t* __restrict__ p) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
    const uint4 a = q[0], b = q[1];
    return LuKey{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}};
}
__device__ __forceinline__ bool lu_same(const LuKey& a, const LuKey& b) {
    uint32_t d = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) d |= a.w[k] ^ b.w[k];
    return d == 0;
}
__device__ __forceinline__ uint32_t lu_rotl(uint32_t v, int s) { return (v << s) | (v >> (32 - s)); }
// the 32-bit MurmurHash3 over the eight limbs: every limb passes through two multiplications and the final avalanche
__device__ __forceinline__ uint32_t lu_hash(const LuKey& key) {
    uint32_t h = 0x9747b28cu;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        uint32_t v = key.w[k] * 0xcc9e2d51u;
        v = lu_rotl(v, 15) * 0x1b873593u;
        h = lu_rotl(h ^ v, 13) * 5u + 0xe6546b64u;
    }
    h ^= 32u;
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}

__global__ void __launch_bounds__(kLuThreads) k_lu_build(const uint32_t* __restrict__ table, uint32_t n_table, uint32_t* slots,
                                                         uint32_t log_cap, uint32_t* words) {
    const uint32_t r = blockIdx.x * kLuThreads + threadIdx.x;
    if (r >= n_table) return;
    const LuKey key = lu_key(table + 8 * (size_t)r);
    const uint32_t mask = (1u << log_cap) - 1u;
    uint32_t pos = lu_hash(key) & mask;
#pragma unroll 1
    for (uint32_t step = 0; step <= mask; step++) {
        const uint32_t prev = atomicCAS(&slots[pos], kLuNone, r);
        if (prev == kLuNone) return;
        if (lu_same(lu_key(table + 8 * (size_t)prev), key)) {  // prev < n_table: a row some lane stored
            atomicMin(&slots[pos], r);
            return;
        }
        pos = (pos + 1) & mask;
    }
    atomicMin(&words[1], r);  // the bound: not reached with 2^log_cap >= n_table
}

__global__ void __launch_bounds__(kLuThreads) k_lu_probe(const uint32_t* __restrict__ table, const uint32_t* __restrict__ lookups,
                                                         uint32_t n, uint32_t total, size_t stride, const uint32_t* __restrict__ slots,
                                                         uint32_t log_cap, uint32_t* counts, uint32_t* __restrict__ out_rows,
                                                         uint32_t* words) {
    const uint32_t idx = blockIdx.x * kLuThreads + threadIdx.x;
    uint32_t row = kLuNone;
    if (idx < total) {
        const uint32_t j = idx / n, i = idx - j * n;
        const LuKey key = lu_key(lookups + 8 * ((size_t)j * stride + i));
        const uint32_t mask = (1u << log_cap) - 1u;
        uint32_t pos = lu_hash(key) & mask;
#pragma unroll 1
        for (uint32_t step = 0; step <= mask; step++) {
            const uint32_t s = slots[pos];
            if (s == kLuNone) break;
            if (lu_same(lu_key(table + 8 * (size_t)s), key)) {
                row = s;
                break;
            }
            pos = (pos + 1) & mask;
        }
        if (row == kLuNone) atomicMin(&words[0], i);  // an empty slot or the bound: the value is in no row
        if (out_rows) out_rows[idx] = row;
    }
    // One atomicAdd per distinct row of the wave.  The loop is uniform over the wave (every lane of the workgroup is here, `todo`
    // is the same in all of them): the first lane still pending names a row, the lanes that hit it are counted and leave together.
    bool pending = row != kLuNone;
    uint64_t todo = __ballot(pending);
    while (todo) {
        const int src = __ffsll((unsigned long long)todo) - 1;
        const uint32_t lead = (uint32_t)__shfl((int)row, src);
        const bool mine = pending && row == lead;
        const uint64_t m = __ballot(mine);  // holds lane src at least
        if (__lane_id() == (uint32_t)src) atomicAdd(&counts[lead], (uint32_t)__popcll(m));
        if (mine) pending = false;
        todo &= ~m;
    }
}

__global__ void __launch_bounds__(kLuThreads) k_lu_counts(const uint32_t* __restrict__ counts, uint32_t n_table, Fr30 count_img,
                                                          uint32_t* __restrict__ out_mult, const uint32_t* __restrict__ words,
                                                          uint32_t* __restrict__ flags) {
    const uint32_t r = blockIdx.x * kLuThreads + threadIdx.x;
    if (r == 0) {
        flags[0] = words[0];
        flags[1] = words[1];
    }
    if (r < n_table) fr30_store(out_mult + 8 * (size_t)r, fr30_mul(fr30_small((int32_t)counts[r]), count_img));  // count < 2^26
}

void lu_finish(hipStream_t s, uint32_t n, uint32_t tiles, const Fr30& img_one, const LuOut& out) {
    hipLaunchKernelGGL(k_lu_carry, dim3(1), dim3(kLuCarryThreads), 0, s, tiles, img_one, out.d_partial, out.d_flags);
    hipLaunchKernelGGL(k_lu_finish, dim3(tiles), dim3(kLuThreads), 0, s, n, (const uint32_t*)out.d_partial, out.d_phi);
}

}  // namespace

void launch_logderivative_sum(hipStream_t s, const uint32_t* d_nums, const uint32_t* d_dens, uint32_t n, uint32_t t, size_t stride,
                              const Fr30& scale, const Fr30& img_one, const LuOut& out) {
    const uint32_t tiles = lu_tiles(n);
    hipLaunchKernelGGL(k_lu_tile, dim3(tiles), dim3(kLuThreads), 0, s, LuColumns{d_nums, d_dens, img_one}, n, t, stride, scale, out.d_phi,
                       out.d_partial);
    lu_finish(s, n, tiles, img_one, out);
}

void launch_lookup_sum(hipStream_t s, const uint32_t* d_lookups, uint32_t n, uint32_t k, size_t stride, const uint32_t* d_table,
                       const uint32_t* d_mult, const Fr30& beta, const Fr30& scale, const Fr30& img_one, const LuOut& out) {
    const uint32_t tiles = lu_tiles(n);
    hipLaunchKernelGGL(k_lu_tile_lookup, dim3(tiles), dim3(kLuThreads), 0, s, LuLookup{d_lookups, d_table, d_mult, beta, img_one}, n, k + 1,
                       stride, scale, out.d_phi, out.d_partial);
    lu_finish(s, n, tiles, img_one, out);
}

void launch_batch_inverse(hipStream_t s, const uint32_t* d_vals, uint32_t n, const Fr30& scale, const Fr30& img_one, const LuOut& out) {
    const uint32_t tiles = lu_tiles(n);
    hipLaunchKernelGGL(k_lu_tile_inv, dim3(tiles), dim3(kLuThreads), 0, s, LuValues{d_vals}, n, scale, out.d_phi, out.d_partial);
    lu_finish(s, n, tiles, img_one, out);
}

void launch_lookup_multiplicities(hipStream_t s, const uint32_t* d_table, uint32_t n_table, const uint32_t* d_lookups, uint32_t n,
                                  uint32_t k, size_t stride, const LuHash& h, const Fr30& count_img, uint32_t* d_out_mult,
                                  uint32_t* d_out_rows, uint32_t* d_flags) {
    const uint32_t total = k * n;
    hipLaunchKernelGGL(k_lu_build, dim3((n_table + kLuThreads - 1) / kLuThreads), dim3(kLuThreads), 0, s, d_table, n_table, h.d_slots,
                       h.log_cap, h.d_words);
    hipLaunchKernelGGL(k_lu_probe, dim3((total + kLuThreads - 1) / kLuThreads), dim3(kLuThreads), 0, s, d_table, d_lookups, n, total, stride,
                       (const uint32_t*)h.d_slots, h.log_cap, h.d_counts, d_out_rows, h.d_words);
    hipLaunchKernelGGL(k_lu_counts, dim3((n_table + kLuThreads - 1) / kLuThreads), dim3(kLuThreads), 0, s, (const uint32_t*)h.d_counts,
                       n_table, count_img, d_out_mult, (const uint32_t*)h.d_words, d_flags);
}

}  // namespace kzg
