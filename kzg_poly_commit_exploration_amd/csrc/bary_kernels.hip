// bary_kernels.hip -- barycentric evaluation of many polynomials held in evaluation form (kzg_evaluate_evaluations_batch,
// kzg_verify_evaluations_batch).
//
//     P(z) = (z^n - 1) / n * sum_i f_i w^i / (z - w^i),       P(w^j) = f_j when z lies in the domain
//
// for P given by its n = 2^k values f_i = P(w^i) over the domain of w = w_n, natural order, one z per polynomial.
//
// Kernels:
//   k_bary_partial  grid = (tiles per polynomial) x batch, a tile = kBaryTile consecutive indices.  Lane t takes the kBaryRun
//                   indices tile + j 256 + t (so that a wave reads consecutive values), forms d_i = z - w^i (w^i = lo x hi
//                   from the context's NTT twiddle tables, as ntt_kernels.hip reads them) and the running products of its
//                   run.  The run totals of the 256 lanes go through an inclusive product scan from both ends in LDS
//                   (eight steps of two products); lane 0 inverts the tile's product with fr30_inv -- ONE inversion per
//                   workgroup -- and every lane gets the inverse of its own run's product as
//                   inv(tile) x (product of the runs before it) x (product of the runs after it), then walks its run
//                   backwards (Montgomery's trick) and accumulates f_i w^i / d_i.  The d_i are formed again on the way back
//                   (one product) instead of being kept.  kBaryRun is 4: with 8 the kernel needs 263 VGPRs.
//                   d_i = 0 (z is the domain point w^i) would poison the shared product: the lane puts one in its place
//                   and records i.  The test is made on the canonical residue (fr30_to_limbs), not on the digits: the
//                   signed-digit form is redundant and a lazy difference may hold r for zero.
//                   Output per tile: the partial sum (nine digits, a product: |v| <= 0.5001 r) and the recorded index.
//   k_bary_finish   one workgroup of 64 lanes per polynomial: adds the tile partials, multiplies by (z^n - 1) / n (z^n by k
//                   squarings, 1 / n from the host in multiplier form), or copies f_j when an index was recorded; stores
//                   the canonical blst_fr.
//
// Forms (fr30.hip.h): values and results are blst_fr images (x 2^256); z, the twiddles, 1 / n and everything inverted carry
// 2^270, so a product of one of each kind stays an image and a product of two multipliers stays a multiplier.
// Bounds: a product returns |v| <= 0.5001 r; d = z - w^i with z canonical lies in (-0.51 r, 1.51 r), inside what
// fr30_to_limbs canonicalises; sums are carry-normalised digit-wise (fr30_add) and stay below 2^266 for the 4 terms of a
// run, the 256 lanes of a tile and the <= 4096 tiles of a polynomial, each level brought back below r by one product with
// the multiplier form of one before it is stored.
#include <hip/hip_runtime.h>

#include "engine.h"
#include "fr30.hip.h"
#include "fr30_lanes.hip.h"

namespace kzg {

namespace {

constexpr uint32_t kBaryFinishThreads = 64;
constexpr uint32_t kBaryNone = 0xffffffffu;

// digit planes of 256 values in LDS
using BaryPlane = Fr30Plane<kBaryThreads>;

// The two walks over a lane's run, unrolled by recursion over the index so that the running products stay in registers
// (the compiler leaves a loop of this size rolled, and an indexed array would live in scratch).
// forward, index J: p[J] = d_0 .. d_J with d = z - w^i, or one where the index is past n or d = 0 (then *hit takes i)
template <int J>
__device__ __forceinline__ void bary_forward(Fr30 (&p)[kBaryRun], const Fr30& z, const Fr30& one, const Fr30* __restrict__ tw,
                                             uint32_t base, uint32_t n, uint32_t log_n, uint32_t* hit) {
    const uint32_t i = base + (uint32_t)J * kBaryThreads;
    Fr30 d = one;
    if (i < n) {
        d = fr30_sub(z, fr30_root(tw, i, log_n));
        if (fr30_is_zero(d)) {
            atomicMin(hit, i);
            d = one;
        }
    }
    if constexpr (J == 0) p[0] = d;
    else p[J] = fr30_mul(p[J - 1], d);
    if constexpr (J + 1 < (int)kBaryRun) bary_forward<J + 1>(p, z, one, tw, base, n, log_n, hit);
}
// backward, index J: inv = 1 / (d_0 .. d_J) on entry; 1 / d_J = inv x (d_0 .. d_(J-1)), then inv x d_J drops d_J
template <int J>
__device__ __forceinline__ void bary_backward(const Fr30 (&p)[kBaryRun], Fr30& inv, Fr30& acc, const Fr30& z, const Fr30& one,
                                              const Fr30* __restrict__ tw, const uint32_t* __restrict__ f, uint32_t base,
                                              uint32_t n, uint32_t log_n) {
    const uint32_t i = base + (uint32_t)J * kBaryThreads;
    if (i < n) {
        const Fr30 w = fr30_root(tw, i, log_n);
        Fr30 d = fr30_sub(z, w);
        const bool zero = fr30_is_zero(d);
        if (zero) d = one;
        Fr30 dinv = inv;
        if constexpr (J > 0) {
            dinv = fr30_mul(inv, p[J - 1]);
            inv = fr30_mul(inv, d);
        }
        if (!zero) acc = fr30_add(acc, fr30_mul(fr30_mul(fr30_load(f + 8 * (size_t)i), w), dinv));
    }
    if constexpr (J > 0) bary_backward<J - 1>(p, inv, acc, z, one, tw, f, base, n, log_n);
}

// evals: polynomial b at evals + 8 n b (compact); zs[b]: the point in multiplier form; partial: kBaryPartialWords words per
// (b, tile): nine digits, then the least index i of the tile with z = w^i (kBaryNone when there is none)
__global__ void __launch_bounds__(kBaryThreads) k_bary_partial(const uint32_t* __restrict__ evals, uint32_t log_n, uint32_t tiles,
                                                               const Fr30* __restrict__ zs, const Fr30* __restrict__ tw,
                                                               uint32_t* __restrict__ partial) {
    __shared__ BaryPlane pre[2], suf[2];
    __shared__ int32_t inv_s[kR9];
    __shared__ uint32_t hit_s;
    const uint32_t t = threadIdx.x, tile = blockIdx.x % tiles, b = blockIdx.x / tiles;
    const uint32_t n = 1u << log_n, base = tile * kBaryTile + t;
    const uint32_t* f = evals + 8 * ((size_t)b << log_n);
    const Fr30 z = fr30_table(zs, b);
    const Fr30 one = fr30_const_one270();
    if (t == 0) hit_s = kBaryNone;
    __syncthreads();
    // forward: the running products of the run
    Fr30 p[kBaryRun];
    bary_forward<0>(p, z, one, tw, base, n, log_n, &hit_s);
    // products of the runs of lanes [0, t] and of lanes [t, 255]
    Fr30 mp = p[kBaryRun - 1], ms = mp;
    uint32_t cur = 0;
#pragma unroll 1
    for (uint32_t o = 1; o < kBaryThreads; o <<= 1) {
        plane_put(pre[cur], t, mp);
        plane_put(suf[cur], t, ms);
        __syncthreads();
        if (t >= o) mp = fr30_mul(plane_get(pre[cur], t - o), mp);
        if (t + o < kBaryThreads) ms = fr30_mul(ms, plane_get(suf[cur], t + o));
        cur ^= 1;
    }
    plane_put(pre[cur], t, mp);
    plane_put(suf[cur], t, ms);
    if (t == 0) {  // ms of lane 0 is the product of the whole tile
        const Fr30 inv = fr30_inv(ms);
#pragma unroll
        for (int k = 0; k < kR9; k++) inv_s[k] = inv.d[k];
    }
    __syncthreads();
    Fr30 inv;
#pragma unroll
    for (int k = 0; k < kR9; k++) inv.d[k] = inv_s[k];
    if (t > 0) inv = fr30_mul(inv, plane_get(pre[cur], t - 1));
    if (t + 1 < kBaryThreads) inv = fr30_mul(inv, plane_get(suf[cur], t + 1));
    // backwards: inv = 1 / (d_0 .. d_j); 1 / d_j = inv x (d_0 .. d_(j-1)), then inv x d_j drops d_j
    Fr30 acc = fr30_zero();
    bary_backward<(int)kBaryRun - 1>(p, inv, acc, z, one, tw, f, base, n, log_n);
    acc = fr30_mul(acc, one);
    // the tile's sum: a tree over the lanes in LDS (the scans are done with their planes)
    __syncthreads();
    BaryPlane& red = pre[0];
    plane_put(red, t, acc);
    __syncthreads();
#pragma unroll 1
    for (uint32_t o = kBaryThreads / 2; o > 0; o >>= 1) {
        if (t < o) {
            acc = fr30_add(acc, plane_get(red, t + o));
            plane_put(red, t, acc);
        }
        __syncthreads();
    }
    if (t == 0) {
        acc = fr30_mul(acc, one);
        uint32_t* out = partial + (size_t)blockIdx.x * kBaryPartialWords;
        fr30_put_digits(out, acc);
        out[kR9] = hit_s;
    }
}

// out[b] = P_b(z_b), canonical blst_fr
__global__ void __launch_bounds__(kBaryFinishThreads) k_bary_finish(const uint32_t* __restrict__ evals, uint32_t log_n,
                                                                    uint32_t tiles, const Fr30* __restrict__ zs, Fr30 inv_n,
                                                                    const uint32_t* __restrict__ partial,
                                                                    uint32_t* __restrict__ out) {
    __shared__ int32_t red[kR9][kBaryFinishThreads];
    __shared__ uint32_t hit_s;
    const uint32_t t = threadIdx.x, b = blockIdx.x;
    if (t == 0) hit_s = kBaryNone;
    __syncthreads();
    Fr30 acc = fr30_zero();
    uint32_t hit = kBaryNone;
#pragma unroll 1
    for (uint32_t q = t; q < tiles; q += kBaryFinishThreads) {
        const uint32_t* rec = partial + ((size_t)b * tiles + q) * kBaryPartialWords;
        acc = fr30_add(acc, fr30_digits(rec));
        hit = min(hit, rec[kR9]);
    }
    if (hit != kBaryNone) atomicMin(&hit_s, hit);
#pragma unroll
    for (int k = 0; k < kR9; k++) red[k][t] = acc.d[k];
    __syncthreads();
    if (t != 0) return;
    uint4* o = reinterpret_cast<uint4*>(out + 8 * (size_t)b);
    const uint32_t* f = evals + 8 * ((size_t)b << log_n);
    if (hit_s != kBaryNone) {
        const uint4* src = reinterpret_cast<const uint4*>(f + 8 * (size_t)hit_s);
        o[0] = src[0];
        o[1] = src[1];
        return;
    }
#pragma unroll 1
    for (uint32_t q = 1; q < kBaryFinishThreads; q++) {
        Fr30 v;
#pragma unroll
        for (int k = 0; k < kR9; k++) v.d[k] = red[k][q];
        acc = fr30_add(acc, v);
    }
    const Fr30 one = fr30_const_one270();
    Fr30 zn = fr30_table(zs, b);
#pragma unroll 1
    for (uint32_t q = 0; q < log_n; q++) zn = fr30_mul(zn, zn);
    const Fr30 factor = fr30_mul(fr30_sub(zn, one), inv_n);
    const Fr30 y = fr30_mul(fr30_mul(acc, one), factor);
    uint32_t l[8];
    fr30_to_limbs(y, l);
    o[0] = make_uint4(l[0], l[1], l[2], l[3]);
    o[1] = make_uint4(l[4], l[5], l[6], l[7]);
}

}  // namespace

void launch_bary(hipStream_t s, const uint32_t* d_evals, uint32_t log_n, uint32_t batch, const Fr30* d_zs, const void* d_tw,
                 const Fr30& inv_n, uint32_t* d_partial, uint32_t* d_out) {
    if (!batch) return;
    const uint32_t tiles = bary_tiles(log_n);
    hipLaunchKernelGGL(k_bary_partial, dim3(tiles * batch), dim3(kBaryThreads), 0, s, d_evals, log_n, tiles, d_zs,
                       (const Fr30*)d_tw, d_partial);
    hipLaunchKernelGGL(k_bary_finish, dim3(batch), dim3(kBaryFinishThreads), 0, s, d_evals, log_n, tiles, d_zs, inv_n,
                       (const uint32_t*)d_partial, d_out);
}

}  // namespace kzg
