// srs_update_kernels.hip -- a powers-of-tau contribution to the resident SRS and the device half of its verification
// (kzg_srs_update, kzg_srs_verify).
//
// A contribution multiplies point i of the SRS by tau^(first + i): one variable-base scalar multiplication per point with a
// per-point exponent.  Nothing of it goes through the host: a lane derives its own power (square-and-multiply over the 64-bit
// exponent, as k_srs_points does for the setup), makes it canonical, splits it as k1 + k2 lambda and runs the joint ladder of
// verify_kernels.hip / fk20_kernels.hip on the point it reads from table level 0.
//
// Kernels:
//   k_srs_update  lane per point: out[i] = [tau^(first + i) mod r] level0[i] as an XYZZ record (infinity stays infinity); the
//                 caller normalises the records and rebuilds the window tables from them
//   k_srs_check   lane per point: err[0] = least index at infinity, err[1] = least index that is off the curve or outside
//                 the subgroup of order r (Scott, ePrint 2021/1130: [z^2] P == (beta^2 x, -y); k_vc_ladder's check without
//                 the weight round)
//
// Bounds.  Fr: the secret arrives as a raw integer below 2^256; fr30_mul returns |v| <= 0.5001 r whatever it is given, so
// every power stays there, and the last product (by the digit 1) feeds fr30_to_limbs, which takes (-r, 2r) to [0, r).  The
// split: k < r = lambda^2 + lambda + 1, so k div lambda <= lambda + 1 < 2^128 and k mod lambda < lambda < 2^128; 128 joint steps.
// G1: the group law of g1_30.hip.h on normalised table records (|x|, |y| < 0.62 p) and on its own outputs (section 4.2).
#define KZG_G1_30_INLINE_DBL
#define KZG_G1_30_NO_SB
#include <hip/hip_runtime.h>

#include "engine.h"
#include "fr30.hip.h"
#include "g1_30.hip.h"

namespace kzg {

namespace {

// verify_kernels.hip's GLV ladder, restated here (it lives in an anonymous namespace of its translation unit):
// beta * 2^390 mod p, balanced radix-2^30 digits: the cube root of unity with (beta x, y) = [z^2 - 1](x, y) on G1
// (the same digits as fk20_kernels.hip and verify_kernels.hip, tests/test_srs_ceremony.py compares them)
__device__ __forceinline__ Fq fq_beta() {
    constexpr int32_t B[13] = {0x1c907181, -0x3421b7a, -0x19a8b3c1, -0xcdb8a13, 0x1c3ebc1c, -0x611979c, 0x16ffa857,
                               -0x13cb6601, 0x550bd17, 0x14cbac30, 0x17d18c86, -0x1ea6a609, 0x9c6d5};
    Fq r;
#pragma unroll
    for (int i = 0; i < kQ; i++) r.d[i] = B[i];
    return r;
}

__device__ __forceinline__ bool glv_bit(const Glv& k, int part, int bit) {
    const uint64_t w = part ? k.k2[bit >> 6] : k.k1[bit >> 6];
    return (w >> (bit & 63)) & 1;
}

// [k1 + k2 lambda] p, joint double-and-add over the 128 bits of k1 and k2
__device__ __forceinline__ XYZZ30 g1_mul_glv(const XYZZ30& p, const Glv& k) {
    XYZZ30 acc = xyzz30_inf();
    const uint64_t hi = k.k1[1] | k.k2[1], lo = k.k1[0] | k.k2[0];
    if (!(hi | lo) || xyzz30_is_inf(p)) return acc;
    const int top = hi ? 127 - __clzll(hi) : 63 - __clzll(lo);
    const Fq phix = fq_mul(p.X, fq_beta());  // phi(p) = (beta X, Y, ZZ, ZZZ)
    XYZZ30 both = p;
    {
        XYZZ30 q = p;
        q.X = phix;
        xyzz30_add(both, q);
    }
#pragma unroll 1
    for (int bit = top; bit >= 0; bit--) {
        xyzz30_dbl_body(acc);
        const uint32_t sel = (uint32_t)glv_bit(k, 0, bit) | ((uint32_t)glv_bit(k, 1, bit) << 1);
        if (sel) {
            XYZZ30 t;
#pragma unroll
            for (int i = 0; i < kQ; i++) {
                t.X.d[i] = sel == 1 ? p.X.d[i] : (sel == 2 ? phix.d[i] : both.X.d[i]);
                t.Y.d[i] = sel == 3 ? both.Y.d[i] : p.Y.d[i];
                t.ZZ.d[i] = sel == 3 ? both.ZZ.d[i] : p.ZZ.d[i];
                t.ZZZ.d[i] = sel == 3 ? both.ZZZ.d[i] : p.ZZZ.d[i];
            }
            xyzz30_add(acc, t);
        }
    }
    return acc;
}

constexpr uint32_t kSuThreads = 64;
constexpr uint64_t kBlsZAbs = 0xd201000000010000ULL;  // |z|, z = -0xd201000000010000
// lambda = z^2 - 1 (api.hip's kGlvLambda): r = lambda^2 + lambda + 1
constexpr uint64_t kLambdaHi = 0xac45a4010001a402ULL, kLambdaLo = 0x00000000ffffffffULL;

// the canonical scalar k (8 x u32, below r) as k1 + k2 lambda, k1 = k mod lambda, k2 = k div lambda: the host's glv_split,
// a restoring division bit by bit.  The dividend is shifted out of its own registers, so that nothing is indexed by the loop.
__device__ __forceinline__ Glv glv_split_device(const uint32_t l[8]) {
    uint64_t v0 = l[0] | ((uint64_t)l[1] << 32), v1 = l[2] | ((uint64_t)l[3] << 32), v2 = l[4] | ((uint64_t)l[5] << 32),
             v3 = l[6] | ((uint64_t)l[7] << 32);
    uint64_t r0 = 0, r1 = 0, q0 = 0, q1 = 0;
#pragma unroll 1
    for (int bit = 0; bit < 256; bit++) {
        const bool over = (r1 >> 63) != 0;  // the remainder shifted left passes 2^128: it is above lambda then
        r1 = (r1 << 1) | (r0 >> 63);
        r0 = (r0 << 1) | (v3 >> 63);
        v3 = (v3 << 1) | (v2 >> 63);
        v2 = (v2 << 1) | (v1 >> 63);
        v1 = (v1 << 1) | (v0 >> 63);
        v0 <<= 1;
        q1 = (q1 << 1) | (q0 >> 63);
        q0 <<= 1;
        if (over || r1 > kLambdaHi || (r1 == kLambdaHi && r0 >= kLambdaLo)) {
            const uint64_t borrow = r0 < kLambdaLo ? 1 : 0;
            r0 -= kLambdaLo;
            r1 = r1 - kLambdaHi - borrow;
            q0 |= 1;
        }
    }
    Glv g;
    g.k1[0] = r0;
    g.k1[1] = r1;
    g.k2[0] = q0;
    g.k2[1] = q1;
    return g;
}

struct TauArg8 {
    uint32_t l[8];
};

__device__ __forceinline__ XYZZ30 xyzz30_from_record(const uint4* __restrict__ r, Affine30* p) {
    p->x = load_fq16(r);
    p->y = load_fq16(r + 4);
    XYZZ30 base = xyzz30_inf();
    if (!affine30_is_inf(*p)) {
        base.X = p->x;
        base.Y = p->y;
        base.ZZ = fq_one();
        base.ZZZ = base.ZZ;
    }
    return base;
}

__global__ void __launch_bounds__(kSuThreads) k_srs_update(TauArg8 tau, uint64_t first, uint32_t n,
                                                           const uint4* __restrict__ level0, uint4* __restrict__ out_xyzz) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    // tau arrives as the raw 256-bit integer: times 2^540 over the multiplier's 2^270 it is tau * 2^270, reduced
    const Fr30 t = fr30_mul(fr30_from_limbs(tau.l), fr30_const_r2_540());
    uint64_t e = first + i;
    Fr30 pw = fr30_const_one270();
    Fr30 base = t;
#pragma unroll 1
    while (e) {
        if (e & 1) pw = fr30_mul(pw, base);
        base = fr30_mul(base, base);
        e >>= 1;
    }
    uint32_t k[8];
    fr30_to_limbs(fr30_mul(pw, fr30_small(1)), k);  // canonical
    const Glv g = glv_split_device(k);
    Affine30 p;
    const XYZZ30 pt = xyzz30_from_record(level0 + (size_t)i * kAffineU4, &p);
    store_xyzz30(out_xyzz + (size_t)i * kXyzzU4, g1_mul_glv(pt, g));
}

__device__ __forceinline__ Fq fq_four() {
    const Fq one = fq_one();
    const Fq two = fq_norm(fq_add_raw(one, one));  // one carry pass per doubling: four raw digits could pass 2^31
    return fq_norm(fq_add_raw(two, two));
}
// a == b * c for lazily reduced values below 3.5 p after the subtraction
__device__ __forceinline__ bool fq_eq_prod(const Fq& a, const Fq& b, const Fq& c) {
    return fq_is_zero(fq_norm(fq_sub_raw(a, fq_mul(b, c))));
}

__global__ void __launch_bounds__(kSuThreads) k_srs_check(const uint4* __restrict__ level0, uint32_t n, uint32_t* __restrict__ err) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Affine30 p;
    const XYZZ30 base = xyzz30_from_record(level0 + (size_t)i * kAffineU4, &p);
    if (xyzz30_is_inf(base)) {
        atomicMin(err, i);
        return;
    }
    if (!fq_is_zero(fq_norm(fq_sub_raw(fq_sub_raw(fq_sqr(p.y), fq_mul(fq_sqr(p.x), p.x)), fq_four())))) {
        atomicMin(err + 1, i);  // off the curve: outside G1 all the more
        return;
    }
    // q = [|z|] [|z|] P, one copy of the ladder
    Glv z;
    z.k1[0] = kBlsZAbs;
    z.k1[1] = z.k2[0] = z.k2[1] = 0;
    XYZZ30 q = base;
#pragma unroll 1
    for (int round = 0; round < 2; round++) q = g1_mul_glv(q, z);
    // [z^2] P == (beta^2 x, -y) with beta^2 = -1 - beta: X == -(x + beta x) ZZ and Y == -y ZZZ
    const Fq ex = fq_norm(fq_neg(fq_norm(fq_add_raw(p.x, fq_mul(p.x, fq_beta())))));
    const bool in_g1 = !xyzz30_is_inf(q) && fq_eq_prod(q.X, ex, q.ZZ) && fq_eq_prod(q.Y, fq_neg(p.y), q.ZZZ);
    if (!in_g1) atomicMin(err + 1, i);
}

}  // namespace

void launch_srs_update(hipStream_t s, const uint32_t* tau_raw8, uint64_t first, uint32_t n, const void* d_level0, void* d_out_xyzz) {
    if (!n) return;
    TauArg8 tau;
    for (int i = 0; i < 8; i++) tau.l[i] = tau_raw8[i];
    hipLaunchKernelGGL(k_srs_update, dim3((n + kSuThreads - 1) / kSuThreads), dim3(kSuThreads), 0, s, tau, first, n,
                       (const uint4*)d_level0, (uint4*)d_out_xyzz);
    for (int i = 0; i < 8; i++) ((volatile uint32_t*)tau.l)[i] = 0;
}

void launch_srs_check(hipStream_t s, const void* d_level0, uint32_t n, uint32_t* d_err) {
    if (!n) return;
    hipLaunchKernelGGL(k_srs_check, dim3((n + kSuThreads - 1) / kSuThreads), dim3(kSuThreads), 0, s, (const uint4*)d_level0, n, d_err);
}

}  // namespace kzg
