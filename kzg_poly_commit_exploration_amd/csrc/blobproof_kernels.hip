// blobproof_kernels.hip -- the quotients of a batch of blob-sized polynomials, each at its own point, in ONE launch
// (DESIGN.md section 4.17).
//
// kzg_open_batch runs one launch_quotient per polynomial in stream order, each with ~60 host Fr products behind its kernel
// argument (poly_kernels.hip).  For the openings of blobs (n <= 4096 coefficients, one point per blob: the Fiat-Shamir
// challenge or a point the caller names) the scans are a microsecond of arithmetic each and the launches are the cost.  Here
// workgroup b runs k_poly_single's scan on polynomial b:
//        S[i] = sum_{k >= i} c[k] z^(k-i),     q[i-1] = S[i]  (i >= 1),     S[0] = P(z),
// as chunk Horner over 16 coefficients per lane, a Kogge-Stone suffix scan over the 256 lanes and a replay from the
// neighbour's value.  What differs: the point z_b comes from a device array (the multiplier's form, digits of z * 2^270, as
// fr30_arg_from_mont256 makes them), and the multipliers of the scan -- z^16 and its seven repeated squares -- are derived
// on the device, each lane squaring its own copy between the steps (4 + 8 products on top of the scan's 40, the last one unused): nothing per
// polynomial passes through the kernel arguments and the host prepares one product per point.
// Every value that leaves is an exact field element in its canonical form, so q, P(z) and the flags are bit for bit what
// k_poly_single and the two-launch scan write for the same polynomial and point.
// The helpers below restate the few lines of poly_kernels.hip this unit needs; that unit's text stays as it is (the ISA
// tests pin its kernels' registers).
#include "engine.h"
#include "fr30.hip.h"
#include "fr30_lanes.hip.h"

namespace kzg {

namespace {

#define KZG_DEV __device__ __forceinline__

constexpr int kBpBlock = 256;                              // lanes per workgroup
constexpr uint32_t kBpL = 16;                              // coefficients per lane
static_assert(kBpL * kBpBlock == kBlobProofMaxN, "one workgroup covers a polynomial");
constexpr int kBpScanWords = kBpBlock * kR9;               // LDS words of the exchange

// value = value * multiplier + value (Horner step), carry-normalised
KZG_DEV Fr30 bp_mul_add(const Fr30& h, const Fr30& mult, const Fr30& c) { return fr30_norm(fr30_add_raw(fr30_mul(h, mult), c)); }

}  // namespace

// d_z: batch x kBlobProofZWords words, the first 9 the multiplier digits of z_b.  d_flags: batch x 32 words, written in full:
// [0] = any non-zero coefficient with index >= 1, [8..15] = P_b(z_b), [16..23] = c_0 as it came, zero elsewhere.
// d_q (may be null: values only): n - 1 canonical values per polynomial, polynomial b at word 8 b (n - 1).
__global__ void __launch_bounds__(kBpBlock) k_blobproof_quotients(const uint32_t* __restrict__ d_coeffs, uint32_t n, uint64_t stride,
                                                                  const uint32_t* __restrict__ d_z, uint32_t* __restrict__ d_q,
                                                                  uint32_t* __restrict__ d_flags) {
    __shared__ uint32_t lds[kBpScanWords];
    const uint32_t t = threadIdx.x, b = blockIdx.x;
    const uint32_t* coeffs = d_coeffs + 8 * (size_t)b * stride;
    uint32_t* flags = d_flags + 32 * (size_t)b;
    // the point, through LDS: a value every lane reads from one global address would live in scalar registers, and two
    // such values (the point and the scan's multiplier) beside the modulus are more than the scalar file holds
    if (t < (uint32_t)kR9) lds[t] = d_z[(size_t)b * kBlobProofZWords + t];
    __syncthreads();
    Fr30 z;
#pragma unroll
    for (int i = 0; i < kR9; i++) z.d[i] = (int32_t)lds[i];  // (the scan's first write comes after the barrier below)
    const uint32_t base = t * kBpL;
    Fr30 h = fr30_zero();
    bool nz = false;
#pragma unroll 1
    for (int k = (int)kBpL - 1; k >= 0; k--) {
        const uint32_t idx = base + k;
        Fr30 c = fr30_zero();
        if (idx < n) {
            const uint4* q = reinterpret_cast<const uint4*>(coeffs + (size_t)idx * 8);
            const uint4 lo = q[0], hi = q[1];
            if (idx >= 1 && ((lo.x | lo.y | lo.z | lo.w) | (hi.x | hi.y | hi.z | hi.w)) != 0u) nz = true;
            c = fr30_from_u4(lo, hi);
        }
        h = bp_mul_add(h, z, c);
    }
    const int any_nz = __syncthreads_or(nz ? 1 : 0);
    // Kogge-Stone suffix scan over the lanes: h_t <- sum_{u >= t} h_u (z^16)^(u - t); the step's multiplier (z^16)^(2^s) is
    // squared in place (a product of two multipliers is a multiplier again)
    Fr30 mult = z;
#pragma unroll 1
    for (int i = 0; i < 4; i++) mult = fr30_mul(mult, mult);  // z^16
#pragma unroll 1
    for (int off = 1; off < kBpBlock; off <<= 1) {
#pragma unroll
        for (int i = 0; i < kR9; i++) lds[i * kBpBlock + t] = (uint32_t)h.d[i];
        __syncthreads();
        if (t + off < (uint32_t)kBpBlock) {
            Fr30 o;
#pragma unroll
            for (int i = 0; i < kR9; i++) o.d[i] = (int32_t)lds[i * kBpBlock + t + off];
            h = bp_mul_add(o, mult, h);
        }
        __syncthreads();
        mult = fr30_mul(mult, mult);
    }
    // h = S at the first coefficient of this lane's chunk
#pragma unroll
    for (int i = 0; i < kR9; i++) lds[i * kBpBlock + t] = (uint32_t)h.d[i];
    __syncthreads();
    if (t < 32) {
        uint32_t w = 0;
        if (t == 0) w = any_nz ? 1u : 0u;
        if (t < 8 || (t >= 24)) flags[t] = w;  // (words 8..23 are written below by lane 0)
    }
    if (t == 0) {
        fr30_store(flags + 8, fr30_mul(h, fr30_const_one270()));  // S[0] = P(z), brought under r / 2 by a product with one
        const uint4* q = reinterpret_cast<const uint4*>(coeffs);
        reinterpret_cast<uint4*>(flags + 16)[0] = q[0];
        reinterpret_cast<uint4*>(flags + 16)[1] = q[1];
    }
    if (!d_q || n <= 1) return;
    uint32_t* qout = d_q + 8 * (size_t)b * (n - 1);
    Fr30 carry = fr30_zero();  // S at the first coefficient of the next chunk
    if (t + 1 < (uint32_t)kBpBlock) {
#pragma unroll
        for (int i = 0; i < kR9; i++) carry.d[i] = (int32_t)lds[i * kBpBlock + t + 1];
    }
    h = carry;
#pragma unroll 1
    for (int k = (int)kBpL - 1; k >= 0; k--) {
        const uint32_t idx = base + k;
        if (idx < n) {
            const uint4* q = reinterpret_cast<const uint4*>(coeffs + (size_t)idx * 8);
            h = bp_mul_add(h, z, fr30_from_u4(q[0], q[1]));  // a product plus a canonical coefficient
            if (idx >= 1) fr30_store(qout + (size_t)(idx - 1) * 8, h);
        } else {
            h = fr30_mul(h, z);  // (past the end: h is zero and stays zero)
        }
    }
}

bool launch_blobproof_quotients(hipStream_t s, const uint32_t* d_coeffs, uint32_t n, uint64_t stride, uint32_t batch,
                                const uint32_t* d_z, uint32_t* d_q, uint32_t* d_flags) {
    if (n == 0 || n > kBlobProofMaxN) return false;
    if (batch == 0) return true;
    hipLaunchKernelGGL(k_blobproof_quotients, dim3(batch), dim3(kBpBlock), 0, s, d_coeffs, n, stride, d_z, d_q, d_flags);
    return true;
}

}  // namespace kzg
