// lagrange_kernels.hip -- the quotient of an opening taken directly on the values (kzg_open_lagrange, kzg_quotient_lagrange;
// DESIGN.md section 4.18).
//
// P is given by its n = 2^k values f_i = P(w^i) over the domain of w = w_n, natural order.  With y = P(z):
//
//     q_i = (y - f_i) / (z - w^i)                     for w^i != z        (the values of (P - y) / (X - z) on the domain)
//     q_m = -sum_{i != m} q_i w^(i - m)               when z = w^m        (the quotient has degree <= n - 2: its top
//                                                                          interpolation coefficient (1/n) sum q_i w^i is 0)
//     P(z) = (z^n - 1) / n * sum_i f_i w^i / (z - w^i),   P(w^m) = f_m    (the barycentric formula, as bary_kernels.hip)
//
// Kernels:
//   k_lagrange_partial  grid = tiles, a tile = kLagTile consecutive indices, modelled on k_bary_partial: lane t takes the kLagRun
//                       indices tile + j 256 + t, forms d_i = z - w^i from the context's NTT twiddle tables and the running
//                       products of its run; the run totals go through the two-sided product scan in LDS; lane 0 inverts the
//                       tile's product -- ONE fr30_inv per workgroup -- and every lane walks its run backwards (Montgomery's
//                       trick), forming the d_i again.  On the way back a lane writes q_i (canonical), accumulates the
//                       barycentric term f_i w^i / d_i and the in-domain term q_i w^i, and notes any f_i != f_0.
//                       d_i = 0 (z = w^i) would poison the shared product: the lane puts one in its place, records i, writes
//                       zero for q_i and leaves the index out of both sums.  Zero tests are made on the canonical residue
//                       (fr30_to_limbs), never on the redundant digits.
//                       Output per tile: both sums (nine digits each), the recorded index, the "not constant" flag.
//   k_lagrange_finish   one workgroup of 64 lanes: adds the tile partials; forms P(z) = (z^n - 1) / n x sum, or copies f_m when
//                       an index m was recorded and then stores q_m = -(sum q_i w^i) w^(-m); writes the flag words the host
//                       reads in the slot's mapped `small` buffer, in the layout of the coefficient route: [0] = some f_i differs
//                       from f_0 (the polynomial is not constant), [8..15] = P(z), [16..23] = f_0 (the constant's value).  The
//                       host compares P(z) with the claimed y (KZG_ERR_REMAINDER), as it does for the coefficient route; when
//                       the claim is wrong the q_i are the values of no polynomial of degree n - 2 and are never used.
//
// Forms (fr30.hip.h): f_i, y, q_i and both sums are blst_fr images (x 2^256); z, the twiddles, 1 / n and everything inverted
// carry 2^270, so a product of one of each kind stays an image and a product of two multipliers stays a multiplier.
// Bounds: a product returns |v| <= 0.5001 r.  d = z - w^i with z canonical and w^i a product lies in (-0.51 r, 1.51 r), inside
// what fr30_to_limbs canonicalises.  y - f_i with both canonical lies in (-r, r): carry-normalised digits, an operand of a
// product only.  f_i - f_0 likewise lies in (-r, r), which fr30_to_limbs canonicalises.  q_i is a product: |v| <= 0.5001 r when
// it is stored.  Each of the two sums adds products digit-wise with a carry pass per term (fr30_add): the 4 terms of a run
// stay below 2.01 r, the run sums are brought back below 0.5001 r + r / 2^13 by one product with the multiplier form of one
// before the tile's tree, the 256 lanes of a tile stay below 129 r < 2^263, brought back the same way before the tile's record
// is stored, and the <= 4096 tiles of a polynomial stay below 2100 r < 2^267 in the finish kernel (top digit below 2^27),
// brought back by the same product before the sum is used.
#include <hip/hip_runtime.h>

#include "engine.h"
#include "fr30.hip.h"
#include "fr30_lanes.hip.h"

namespace kzg {

namespace {

constexpr uint32_t kLagThreads = 256;
constexpr uint32_t kLagRun = 4;
static_assert(kLagThreads * kLagRun == kLagTile, "tile shape");
constexpr uint32_t kLagFinishThreads = 64;
constexpr uint32_t kLagNone = 0xffffffffu;

// digit planes of 256 values in LDS
using LagPlane = Fr30Plane<kLagThreads>;

// what a lane carries on the way back
struct LagAcc {
    Fr30 bary;  // sum f_i w^i / d_i
    Fr30 dom;   // sum q_i w^i
    uint32_t differs;
};

// The two walks over a lane's run, unrolled by recursion over the index so that the running products stay in registers.
// forward, index J: p[J] = d_0 .. d_J with d = z - w^i, or one where the index is past n or d = 0 (then *hit takes i)
template <int J>
__device__ __forceinline__ void lag_forward(Fr30 (&p)[kLagRun], const Fr30& z, const Fr30& one, const Fr30* __restrict__ tw,
                                            uint32_t base, uint32_t n, uint32_t log_n, uint32_t* hit) {
    const uint32_t i = base + (uint32_t)J * kLagThreads;
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
    if constexpr (J + 1 < (int)kLagRun) lag_forward<J + 1>(p, z, one, tw, base, n, log_n, hit);
}
// backward, index J: inv = 1 / (d_0 .. d_J) on entry; 1 / d_J = inv x (d_0 .. d_(J-1)), then inv x d_J drops d_J
template <int J>
__device__ __forceinline__ void lag_backward(const Fr30 (&p)[kLagRun], Fr30& inv, LagAcc& acc, const Fr30& z, const Fr30& y,
                                             const Fr30& f0, const Fr30& one, const Fr30* __restrict__ tw,
                                             const uint32_t* __restrict__ f, uint32_t* __restrict__ q, uint32_t base, uint32_t n,
                                             uint32_t log_n) {
    const uint32_t i = base + (uint32_t)J * kLagThreads;
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
        const Fr30 fi = fr30_load(f + 8 * (size_t)i);
        if (!fr30_is_zero(fr30_sub(fi, f0))) acc.differs = 1u;  // (-r, r): canonicalised by the test
        Fr30 qi = fr30_zero();
        if (!zero) {
            qi = fr30_mul(fr30_sub(y, fi), dinv);  // (y - f_i) in (-r, r) x a multiplier: an image, |v| <= 0.5001 r
            acc.bary = fr30_add(acc.bary, fr30_mul(fr30_mul(fi, w), dinv));
            acc.dom = fr30_add(acc.dom, fr30_mul(qi, w));
        }
        fr30_store(q + 8 * (size_t)i, qi);
    }
    if constexpr (J > 0) lag_backward<J - 1>(p, inv, acc, z, y, f0, one, tw, f, q, base, n, log_n);
}

// partial: kLagPartialWords words per tile: the digits of sum f_i w^i / d_i at [0..9), of sum q_i w^i at [9..18), then the least
// index i of the tile with z = w^i (kLagNone when there is none) and whether some f_i of the tile differs from f_0
__global__ void __launch_bounds__(kLagThreads) k_lagrange_partial(const uint32_t* __restrict__ f, uint32_t log_n, Fr30 z, Fr30 y,
                                                                  const Fr30* __restrict__ tw, uint32_t* __restrict__ q,
                                                                  uint32_t* __restrict__ partial) {
    __shared__ LagPlane pre[2], suf[2];
    __shared__ int32_t inv_s[kR9];
    __shared__ uint32_t hit_s, differs_s;
    const uint32_t t = threadIdx.x, tile = blockIdx.x;
    const uint32_t n = 1u << log_n, base = tile * kLagTile + t;
    const Fr30 one = fr30_const_one270();
    if (t == 0) {
        hit_s = kLagNone;
        differs_s = 0;
    }
    __syncthreads();
    // forward: the running products of the run
    Fr30 p[kLagRun];
    lag_forward<0>(p, z, one, tw, base, n, log_n, &hit_s);
    // products of the runs of lanes [0, t] and of lanes [t, 255]
    Fr30 mp = p[kLagRun - 1], ms = mp;
    uint32_t cur = 0;
#pragma unroll 1
    for (uint32_t o = 1; o < kLagThreads; o <<= 1) {
        plane_put(pre[cur], t, mp);
        plane_put(suf[cur], t, ms);
        __syncthreads();
        if (t >= o) mp = fr30_mul(plane_get(pre[cur], t - o), mp);
        if (t + o < kLagThreads) ms = fr30_mul(ms, plane_get(suf[cur], t + o));
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
    if (t + 1 < kLagThreads) inv = fr30_mul(inv, plane_get(suf[cur], t + 1));
    // backwards: the quotient values and both sums of the run (4 products each: below 2.01 r)
    LagAcc acc;
    acc.bary = fr30_zero();
    acc.dom = fr30_zero();
    acc.differs = 0;
    const Fr30 f0 = fr30_load(f);
    lag_backward<(int)kLagRun - 1>(p, inv, acc, z, y, f0, one, tw, f, q, base, n, log_n);
    if (acc.differs) differs_s = 1u;  // (every writer stores the same 1)
    acc.bary = fr30_mul(acc.bary, one);  // the run sums back below 0.5001 r + r / 2^13
    acc.dom = fr30_mul(acc.dom, one);
    // the tile's sums: trees over the lanes in LDS (the scans are done with their planes); 256 terms: below 129 r
    __syncthreads();
    LagPlane &red_b = pre[0], &red_d = suf[0];
    plane_put(red_b, t, acc.bary);
    plane_put(red_d, t, acc.dom);
    __syncthreads();
#pragma unroll 1
    for (uint32_t o = kLagThreads / 2; o > 0; o >>= 1) {
        if (t < o) {
            acc.bary = fr30_add(acc.bary, plane_get(red_b, t + o));
            acc.dom = fr30_add(acc.dom, plane_get(red_d, t + o));
            plane_put(red_b, t, acc.bary);
            plane_put(red_d, t, acc.dom);
        }
        __syncthreads();
    }
    if (t == 0) {
        acc.bary = fr30_mul(acc.bary, one);  // the tile's sums back below 0.5001 r + r / 2^7
        acc.dom = fr30_mul(acc.dom, one);
        uint32_t* out = partial + (size_t)tile * kLagPartialWords;
#pragma unroll
        for (int k = 0; k < kR9; k++) {
            out[k] = (uint32_t)acc.bary.d[k];
            out[kR9 + k] = (uint32_t)acc.dom.d[k];
        }
        out[2 * kR9] = hit_s;
        out[2 * kR9 + 1] = differs_s;
    }
}

// tw: the context's four twiddle tables (forward lo, hi, inverse lo, hi); flags: the 64 flag words of the job (zero at launch)
__global__ void __launch_bounds__(kLagFinishThreads) k_lagrange_finish(const uint32_t* __restrict__ f, uint32_t log_n,
                                                                       uint32_t tiles, Fr30 z, Fr30 inv_n,
                                                                       const Fr30* __restrict__ tw,
                                                                       const uint32_t* __restrict__ partial,
                                                                       uint32_t* __restrict__ q, uint32_t* __restrict__ flags) {
    __shared__ int32_t red_b[kR9][kLagFinishThreads], red_d[kR9][kLagFinishThreads];
    __shared__ uint32_t hit_s, differs_s;
    __shared__ int32_t arg_s[2][kR9];  // z and 1 / n for lane 0's tail: read back into vector registers, not held in scalar ones
    const uint32_t t = threadIdx.x;
    if (t == 0) {
        hit_s = kLagNone;
        differs_s = 0;
#pragma unroll
        for (int j = 0; j < kR9; j++) {
            arg_s[0][j] = z.d[j];
            arg_s[1][j] = inv_n.d[j];
        }
    }
    __syncthreads();
    // <= 4096 tile records of magnitude below 0.51 r each: below 2100 r over all lanes
    Fr30 bary = fr30_zero(), dom = fr30_zero();
    uint32_t hit = kLagNone, differs = 0;
#pragma unroll 1
    for (uint32_t k = t; k < tiles; k += kLagFinishThreads) {
        const uint32_t* rec = partial + (size_t)k * kLagPartialWords;
        bary = fr30_add(bary, fr30_digits(rec));
        dom = fr30_add(dom, fr30_digits(rec + kR9));
        hit = min(hit, rec[2 * kR9]);
        differs |= rec[2 * kR9 + 1];
    }
    if (hit != kLagNone) atomicMin(&hit_s, hit);
    if (differs) differs_s = 1u;
#pragma unroll
    for (int j = 0; j < kR9; j++) {
        red_b[j][t] = bary.d[j];
        red_d[j][t] = dom.d[j];
    }
    __syncthreads();
    if (t != 0) return;
#pragma unroll 1
    for (uint32_t k = 1; k < kLagFinishThreads; k++) {
        Fr30 vb, vd;
#pragma unroll
        for (int j = 0; j < kR9; j++) {
            vb.d[j] = red_b[j][k];
            vd.d[j] = red_d[j][k];
        }
        bary = fr30_add(bary, vb);
        dom = fr30_add(dom, vd);
    }
    const Fr30 one = fr30_const_one270();
    const uint4* f4 = reinterpret_cast<const uint4*>(f);
    uint4* fl4 = reinterpret_cast<uint4*>(flags);
    fl4[4] = f4[0];  // [16..23] = f_0
    fl4[5] = f4[1];
    const uint32_t m = hit_s;
    if (m != kLagNone) {
        // z = w^m: P(z) = f_m, and q_m = -(sum_{i != m} q_i w^i) w^-m
        fl4[2] = f4[2 * (size_t)m];
        fl4[3] = f4[2 * (size_t)m + 1];
        const Fr30 wi = fr30_root(tw + 2 * kNttTableLen, m, log_n);  // w^-m
        const Fr30 qm = fr30_mul(fr30_mul(dom, one), wi);           // the sum back below 0.51 r, then an image again
        fr30_store(q + 8 * (size_t)m, fr30_sub(fr30_zero(), qm));  // m < n: only indices below n are recorded
    } else {
        Fr30 zn, in;
#pragma unroll
        for (int j = 0; j < kR9; j++) {
            zn.d[j] = arg_s[0][j];
            in.d[j] = arg_s[1][j];
        }
#pragma unroll 1
        for (uint32_t k = 0; k < log_n; k++) zn = fr30_mul(zn, zn);
        const Fr30 factor = fr30_mul(fr30_sub(zn, one), in);
        fr30_store(flags + 8, fr30_mul(fr30_mul(bary, one), factor));  // [8..15] = P(z)
    }
    flags[0] = differs_s;
}

}  // namespace

void launch_lagrange_quotient(hipStream_t s, const uint32_t* d_evals, uint32_t log_n, const Fr30& z, const Fr30& y, const Fr30& inv_n,
                              const void* d_tw, uint32_t* d_q, uint32_t* d_partial, uint32_t* d_flags) {
    const uint32_t tiles = lagrange_tiles(log_n);
    hipLaunchKernelGGL(k_lagrange_partial, dim3(tiles), dim3(kLagThreads), 0, s, d_evals, log_n, z, y, (const Fr30*)d_tw, d_q,
                       d_partial);
    hipLaunchKernelGGL(k_lagrange_finish, dim3(1), dim3(kLagFinishThreads), 0, s, d_evals, log_n, tiles, z, inv_n,
                       (const Fr30*)d_tw, (const uint32_t*)d_partial, d_q, d_flags);
}

}  // namespace kzg
