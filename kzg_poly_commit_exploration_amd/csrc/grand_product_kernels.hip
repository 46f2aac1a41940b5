// grand_product_kernels.hip -- the running product of a permutation argument (kzg_grand_product, kzg_permutation_product,
// kzg_permutation_commit).
//
// t numerator columns a_j and t denominator columns b_j of n values each; A_i = prod_j a_j[i], B_i = prod_j b_j[i]:
//
//     z_0 = 1,   z_(i+1) = z_i A_i / B_i   (i < n),   last = z_n
//     z_i = (prod_{k < i} A_k) (prod_{k >= i} B_k) (prod_{all k} B_k)^-1            -- ONE inversion for the whole call
//
// The permutation form (n = 2^k, w = w_n) never stores the columns: from the wire values f_j and the permutation columns s_j
//     a_j[i] = f_j[i] + (beta k_j) w^i + gamma,        b_j[i] = f_j[i] + beta s_j[i] + gamma.
//
// Kernels:
//   k_gp_tile, k_gp_tile_perm   one body over the general and the permutation form's element step (two kernels, so that the
//                    general form carries neither the 18 Fr30 arguments nor the twiddle lookup).
//                    grid = tiles of kGpTile consecutive indices, 256 lanes; lane l owns the run of 4 CONSECUTIVE indices
//                    tile + 4 l + k (the scans are ordered, unlike k_lagrange_partial's strided runs).  It forms A_i and B_i,
//                    the inclusive prefix products of A and the inclusive suffix products of B inside the run and from them
//                    v_i = (A of the run below i) x (B of the run from i on) -- the only four values a lane keeps --, scans the
//                    run totals over the lanes in LDS (inclusive prefix of A, inclusive suffix of B, digit planes, double
//                    buffered) and stores u_i = v_i x (A of the lanes before) x (B of the lanes after) = (prod of A over the
//                    tile's indices below i) x (prod of B over the tile's indices from i on) into z.  Record of the tile: the
//                    product of its A, of its B, the least i with B_i = 0.
//   k_gp_carry       one workgroup of kGpCarryThreads lanes; lane l owns the <= 16 consecutive tiles [l run, (l + 1) run).
//                    Products of its tiles' records, the same two scans over the lanes, lane 0 inverts the product of every
//                    B -- the call's only fr30_inv -- and each lane walks its tiles forwards (prefix of A) and backwards
//                    (suffix of B), leaving c_T = preA_T sufB_T / B_total in the place of the tile's A record.  Writes
//                    last = A_total / B_total and the least index with a zero denominator (kGpNone when there is none).
//   k_gp_scale       z_i = u_i c_T in place, streaming, lane l of tile T takes T + 256 j + l.
// The last pass re-reads u rather than the 2 t columns: (2 t + 3) x 32 bytes per index against (4 t + 1) x 32.
//
// Forms (fr30.hip.h; fr30_mul(a, b) = a b / 2^270).  An IMAGE is x 2^256 (what the ABI holds), a MULTIPLIER x 2^270.
// image x multiplier = image, multiplier x multiplier = multiplier, image x image = x y 2^242: neither.
//   a_j[i], b_j[i]   images: loaded, or in the permutation form a sum of images -- f_j[i] and gamma are images, (beta k_j) is
//                    prepared by the host as an image and w^i is a multiplier (the twiddle tables), beta is a multiplier and
//                    s_j[i] an image.
//   prod of t images by t - 1 products: X 2^(256 t - 270 (t - 1)) = X 2^(270 - 14 t).
//   A_i, B_i         that product x `scale`, scale = 2^(270 + 14 t) prepared by the host: X 2^270, MULTIPLIERS.
//   every scan product, the run / lane / tile prefixes and suffixes, the tile records, u_i: multiplier x multiplier = MULTIPLIERS
//                    (u_i is stored as the canonical residue of its multiplier form).  The neutral element is 2^270
//                    (fr30_const_one270), which also stands in for the indices past n.
//   1 / B_total      fr30_inv of a multiplier is a multiplier; one product with img_one = 2^256 (the digits of the image of
//                    one) makes it the IMAGE of 1 / B_total.
//   c_T, last        (multiplier x that image) x multiplier = IMAGES.
//   z_i = u_i c_T    multiplier x image = IMAGE, stored canonical.  z_0 = B_total / B_total is exactly the image of one.
//
// Bounds.  A loaded value is canonical, [0, r), in carry-normalised digits (fr30_from_limbs).  A product returns
// |v| <= 0.5001 r + |a b| / 2^270 with digits 0..7 in [-2^29, 2^29).  In the permutation form f + gamma is one carry pass over
// two normalised values, [0, 2 r); adding one product (raw digits below 2^30 + 4, inside what fr30_norm takes) gives
// a_j, b_j in (-0.51 r, 2.51 r) in normalised digits with a top digit below 2.51 x 0x73ee: operands of products ONLY, whose
// excess |a b| / 2^270 <= 6.4 r^2 / 2^270 < r / 2^12.  They are never tested for zero and never stored: the zero test is made
// on B_i AFTER the product with `scale` -- a product, inside the (-r, 2 r) that fr30_to_limbs canonicalises -- which is zero
// exactly when one b_j[i] is (the field has no zero divisors).  So the sum is "folded" by the product that follows it and needs
// no fr30_sum_reduce.  Everything downstream is a product of products: |v| <= 0.5001 r + r / 2^14, stored through
// fr30_to_limbs (u_i, z_i, last) or as digits (the records, c_T).
#include <hip/hip_runtime.h>

#include "engine.h"
#include "fr30.hip.h"
#include "fr30_lanes.hip.h"

namespace kzg {

namespace {

constexpr uint32_t kGpThreads = 256;
constexpr uint32_t kGpRun = 4;
static_assert(kGpThreads * kGpRun == kGpTile, "tile shape");
static_assert(kGpCarryThreads == kGpThreads, "both scans run over 256 lanes");
static_assert(((1u << kNttMaxLog) + kGpTile - 1) / kGpTile <= 16 * kGpCarryThreads, "a lane of the carry kernel owns <= 16 tiles");

using GpPlane = Fr30Plane<kGpThreads>;

// what the two forms read
struct GpColumns {  // t columns each, column j at + 8 j stride words
    const uint32_t* nums;
    const uint32_t* dens;
};
struct GpPerm {
    const uint32_t* wires;
    const uint32_t* sigmas;
    const Fr30* tw;
    uint32_t log_n;
    Fr30 beta;                // multiplier
    Fr30 gamma;               // image
    Fr30 bk[kGpMaxColumns];   // beta k_j, images
};

// A_i and B_i before the product with `scale`: X 2^(270 - 14 t)
__device__ __forceinline__ void gp_element(const GpColumns& in, uint32_t i, uint32_t t, size_t stride, Fr30& a, Fr30& b) {
    const uint32_t* pa = in.nums + 8 * (size_t)i;
    const uint32_t* pb = in.dens + 8 * (size_t)i;
    a = fr30_load(pa);
    b = fr30_load(pb);
#pragma unroll 1
    for (uint32_t j = 1; j < t; j++) {
        pa += 8 * stride;
        pb += 8 * stride;
        a = fr30_mul(a, fr30_load(pa));
        b = fr30_mul(b, fr30_load(pb));
    }
}
__device__ __forceinline__ void gp_element(const GpPerm& in, uint32_t i, uint32_t t, size_t stride, Fr30& a, Fr30& b) {
    const uint32_t* pf = in.wires + 8 * (size_t)i;
    const uint32_t* ps = in.sigmas + 8 * (size_t)i;
    const Fr30 w = fr30_root(in.tw, i, in.log_n);
#pragma unroll 1
    for (uint32_t j = 0; j < t; j++) {
        const Fr30 fg = fr30_add(fr30_load(pf), in.gamma);                          // [0, 2 r)
        const Fr30 aj = fr30_add(fg, fr30_mul(in.bk[j], w));                      // (-0.51 r, 2.51 r): an operand only
        const Fr30 bj = fr30_add(fg, fr30_mul(fr30_load(ps), in.beta));
        a = j ? fr30_mul(a, aj) : aj;
        b = j ? fr30_mul(b, bj) : bj;
        pf += 8 * stride;
        ps += 8 * stride;
    }
}

// The walks over a lane's run, unrolled by recursion over the index so that the running products stay in registers.
// index K: pa[K] = A_0 .. A_K and sb[K] = B_K; one for both past n; *hit takes the index when B_K = 0
template <int K, class In>
__device__ __forceinline__ void gp_forward(Fr30 (&pa)[kGpRun], Fr30 (&sb)[kGpRun], const In& in, uint32_t base, uint32_t n,
                                           uint32_t t_cols, size_t stride, const Fr30& scale, const Fr30& one, uint32_t* hit) {
    const uint32_t i = base + (uint32_t)K;
    Fr30 a = one, b = one;
    if (i < n) {
        gp_element(in, i, t_cols, stride, a, b);
        a = fr30_mul(a, scale);
        b = fr30_mul(b, scale);
        if (fr30_is_zero(b)) atomicMin(hit, i);
    }
    if constexpr (K == 0) pa[0] = a;
    else pa[K] = fr30_mul(pa[K - 1], a);
    sb[K] = b;
    if constexpr (K + 1 < (int)kGpRun) gp_forward<K + 1>(pa, sb, in, base, n, t_cols, stride, scale, one, hit);
}
// sb[K] = B_K .. B_3
template <int K>
__device__ __forceinline__ void gp_suffix(Fr30 (&sb)[kGpRun]) {
    sb[K] = fr30_mul(sb[K], sb[K + 1]);
    if constexpr (K > 0) gp_suffix<K - 1>(sb);
}
// sb[K] = (A_0 .. A_(K-1)) x (B_K .. B_3), the part of u_i that the run knows; sb[0] stays
template <int K>
__device__ __forceinline__ void gp_local(const Fr30 (&pa)[kGpRun], Fr30 (&sb)[kGpRun]) {
    sb[K] = fr30_mul(pa[K - 1], sb[K]);
    if constexpr (K + 1 < (int)kGpRun) gp_local<K + 1>(pa, sb);
}
// u_i = v[K] x m, m = (A over the lanes before) x (B over the lanes after)
template <int K>
__device__ __forceinline__ void gp_emit(const Fr30 (&v)[kGpRun], const Fr30& m, uint32_t* __restrict__ z, uint32_t base, uint32_t n) {
    const uint32_t i = base + (uint32_t)K;
    if (i < n) fr30_store(z + 8 * (size_t)i, fr30_mul(v[K], m));
    if constexpr (K + 1 < (int)kGpRun) gp_emit<K + 1>(v, m, z, base, n);
}

template <class In>
__device__ __forceinline__ void gp_tile_body(const In& in, uint32_t n, uint32_t t_cols, size_t stride, const Fr30& scale,
                                             uint32_t* __restrict__ z, uint32_t* __restrict__ partial) {
    __shared__ GpPlane pre[2], suf[2];
    __shared__ uint32_t hit_s;
    const uint32_t t = threadIdx.x, tile = blockIdx.x;
    const uint32_t base = tile * kGpTile + t * kGpRun;
    const Fr30 one = fr30_const_one270();
    if (t == 0) hit_s = kGpNone;
    __syncthreads();
    // pa[k] = A_0 .. A_k, sb[k] = B_k .. B_3 of the run; the run totals go to the scans and only the four
    // v_k = (A_0 .. A_(k-1)) (B_k .. B_3) stay in registers across them
    Fr30 pa[kGpRun], sb[kGpRun];
    gp_forward<0>(pa, sb, in, base, n, t_cols, stride, scale, one, &hit_s);
    gp_suffix<(int)kGpRun - 2>(sb);
    Fr30 mp = pa[kGpRun - 1], ms = sb[0];
    gp_local<1>(pa, sb);
    const uint32_t cur = fr30_scan_products(pre, suf, t, mp, ms);
    uint32_t* rec = partial + (size_t)tile * kGpPartialWords;
    if (t == kGpThreads - 1) fr30_put_digits(rec, mp);
    if (t == 0) {
        fr30_put_digits(rec + kR9, ms);
        rec[2 * kR9] = hit_s;
    }
    // u_i = v_k x (A over the lanes before this one) x (B over the lanes after it)
    Fr30 m = t > 0 ? plane_get(pre[cur], t - 1) : one;
    if (t + 1 < kGpThreads) m = fr30_mul(m, plane_get(suf[cur], t + 1));
    gp_emit<0>(sb, m, z, base, n);
}

__global__ void __launch_bounds__(kGpThreads) k_gp_tile(GpColumns in, uint32_t n, uint32_t t_cols, size_t stride, Fr30 scale,
                                                        uint32_t* __restrict__ z, uint32_t* __restrict__ partial) {
    gp_tile_body(in, n, t_cols, stride, scale, z, partial);
}
__global__ void __launch_bounds__(kGpThreads) k_gp_tile_perm(GpPerm in, uint32_t n, uint32_t t_cols, size_t stride, Fr30 scale,
                                                             uint32_t* __restrict__ z, uint32_t* __restrict__ partial) {
    gp_tile_body(in, n, t_cols, stride, scale, z, partial);
}

__global__ void __launch_bounds__(kGpCarryThreads) k_gp_carry(uint32_t tiles, Fr30 img_one, uint32_t* __restrict__ partial,
                                                              uint32_t* __restrict__ flags) {
    __shared__ GpPlane pre[2], suf[2];
    __shared__ int32_t inv_s[kR9];
    __shared__ int32_t arg_s[kR9];  // img_one for lane 0: read back into vector registers, not held in scalar ones
    __shared__ uint32_t hit_s;
    const uint32_t t = threadIdx.x;
    const uint32_t run = (tiles + kGpCarryThreads - 1) / kGpCarryThreads;
    const uint32_t first = min(t * run, tiles), end = min(first + run, tiles);
    const Fr30 one = fr30_const_one270();
    if (t == 0) {
        hit_s = kGpNone;
#pragma unroll
        for (int k = 0; k < kR9; k++) arg_s[k] = img_one.d[k];
    }
    __syncthreads();
    Fr30 a = one, b = one;
    uint32_t hit = kGpNone;
#pragma unroll 1
    for (uint32_t k = first; k < end; k++) {
        const uint32_t* rec = partial + (size_t)k * kGpPartialWords;
        a = fr30_mul(a, fr30_digits(rec));
        b = fr30_mul(b, fr30_digits(rec + kR9));
        hit = min(hit, rec[2 * kR9]);
    }
    if (hit != kGpNone) atomicMin(&hit_s, hit);
    const uint32_t cur = fr30_scan_products(pre, suf, t, a, b);  // a of lane 255: every A; b of lane 0: every B
    if (t == 0) {
        // the product of every B is zero exactly when some B_i is: fr30_inv(0) = 0 and the call only reports
        Fr30 io;
#pragma unroll
        for (int k = 0; k < kR9; k++) io.d[k] = arg_s[k];
        const Fr30 inv = fr30_mul(fr30_inv(b), io);  // the image of 1 / B_total
#pragma unroll
        for (int k = 0; k < kR9; k++) inv_s[k] = inv.d[k];
        flags[0] = hit_s;
    }
    __syncthreads();
    Fr30 p;
#pragma unroll
    for (int k = 0; k < kR9; k++) p.d[k] = inv_s[k];
    if (t == kGpCarryThreads - 1) fr30_store(flags + 8, fr30_mul(a, p));  // last = A_total / B_total
    if (t > 0) p = fr30_mul(plane_get(pre[cur], t - 1), p);  // (A over the tiles of the lanes before) / B_total: an image
    // forwards: the A record of tile k becomes preA_k / B_total
#pragma unroll 1
    for (uint32_t k = first; k < end; k++) {
        uint32_t* rec = partial + (size_t)k * kGpPartialWords;
        const Fr30 ak = fr30_digits(rec);
        fr30_put_digits(rec, p);
        p = fr30_mul(p, ak);
    }
    // backwards: ... times sufB_k, the product of B over the tiles after k
    Fr30 s = t + 1 < kGpCarryThreads ? plane_get(suf[cur], t + 1) : one;
#pragma unroll 1
    for (uint32_t k = end; k > first; k--) {
        uint32_t* rec = partial + (size_t)(k - 1) * kGpPartialWords;
        fr30_put_digits(rec, fr30_mul(fr30_digits(rec), s));
        s = fr30_mul(s, fr30_digits(rec + kR9));
    }
}

__global__ void __launch_bounds__(kGpThreads) k_gp_scale(uint32_t n, const uint32_t* __restrict__ partial, uint32_t* __restrict__ z) {
    const uint32_t tile = blockIdx.x;
    const Fr30 c = fr30_digits(partial + (size_t)tile * kGpPartialWords);
#pragma unroll
    for (uint32_t j = 0; j < kGpRun; j++) {
        const uint32_t i = tile * kGpTile + j * kGpThreads + threadIdx.x;
        if (i < n) {
            uint32_t* p = z + 8 * (size_t)i;
            fr30_store(p, fr30_mul(fr30_load(p), c));
        }
    }
}

void gp_finish(hipStream_t s, uint32_t n, uint32_t tiles, const Fr30& img_one, const GpOut& out) {
    hipLaunchKernelGGL(k_gp_carry, dim3(1), dim3(kGpCarryThreads), 0, s, tiles, img_one, out.d_partial, out.d_flags);
    hipLaunchKernelGGL(k_gp_scale, dim3(tiles), dim3(kGpThreads), 0, s, n, (const uint32_t*)out.d_partial, out.d_z);
}

}  // namespace

void launch_grand_product(hipStream_t s, const uint32_t* d_nums, const uint32_t* d_dens, uint32_t n, uint32_t t, size_t stride,
                          const Fr30& scale, const Fr30& img_one, const GpOut& out) {
    const uint32_t tiles = gp_tiles(n);
    hipLaunchKernelGGL(k_gp_tile, dim3(tiles), dim3(kGpThreads), 0, s, GpColumns{d_nums, d_dens}, n, t, stride, scale, out.d_z,
                       out.d_partial);
    gp_finish(s, n, tiles, img_one, out);
}

void launch_permutation_product(hipStream_t s, const uint32_t* d_wires, const uint32_t* d_sigmas, uint32_t log_n, uint32_t t,
                                size_t stride, const Fr30* bk, const Fr30& beta, const Fr30& gamma, const void* d_tw,
                                const Fr30& scale, const Fr30& img_one, const GpOut& out) {
    const uint32_t n = 1u << log_n, tiles = gp_tiles(n);
    GpPerm in{};
    in.wires = d_wires;
    in.sigmas = d_sigmas;
    in.tw = (const Fr30*)d_tw;
    in.log_n = log_n;
    in.beta = beta;
    in.gamma = gamma;
    for (uint32_t j = 0; j < t && j < kGpMaxColumns; j++) in.bk[j] = bk[j];
    hipLaunchKernelGGL(k_gp_tile_perm, dim3(tiles), dim3(kGpThreads), 0, s, in, n, t, stride, scale, out.d_z, out.d_partial);
    gp_finish(s, n, tiles, img_one, out);
}

}  // namespace kzg
