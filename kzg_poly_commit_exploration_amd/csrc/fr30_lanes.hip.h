// fr30_lanes.hip.h -- how the Fr kernel units move an Fr30 (fr30.hip.h) between memory and a lane's registers, once: the 32-byte
// load and the canonical store of the ABI's form, an entry of a table of digits, a digit record, a root of unity from the twiddle
// tables, digit planes in LDS and the product scans over a workgroup's lanes.  Device code only; every function is inlined.  The
// arithmetic (fr30_sub and fr30_is_zero among it) is fr30.hip.h's.  A unit's own comments say what ITS values are and why they
// meet the contracts stated here.
#pragma once
#include <hip/hip_runtime.h>

#include "engine.h"
#include "fr30.hip.h"

namespace kzg {

// The ABI's form (a blst_fr image, 8 x u32, any value below 2^256) out of two 16-byte words that are already loaded, as
// carry-normalised digits: digits 0..7 within [-2^29 - 4, 2^29 + 4], the value unchanged -- [0, r) for a canonical input.
__device__ __forceinline__ Fr30 fr30_from_u4(const uint4& lo, const uint4& hi) {
    const uint32_t l[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    return fr30_from_limbs(l);
}
// ... out of the 32 bytes at p, which is 16-byte aligned: two 16-byte loads
__device__ __forceinline__ Fr30 fr30_load(const uint32_t* __restrict__ p) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
    const uint4 a = q[0], b = q[1];
    return fr30_from_u4(a, b);
}
// The canonical residue of v, 8 x u32 in [0, r), to the 32 bytes at p (16-byte aligned): two 16-byte stores.  v is whatever
// fr30_to_limbs canonicalises: a lazy value in (-r, 2r) -- a product (|v| <= 0.5001 r) plus at most one canonical value.
__device__ __forceinline__ void fr30_store(uint32_t* __restrict__ p, const Fr30& v) {
    uint32_t l[8];
    fr30_to_limbs(v, l);
    uint4* q = reinterpret_cast<uint4*>(p);
    q[0] = make_uint4(l[0], l[1], l[2], l[3]);
    q[1] = make_uint4(l[4], l[5], l[6], l[7]);
}

// entry i of a table of digits that the host prepared (twiddles, powers, constants): the nine digits as they are
__device__ __forceinline__ Fr30 fr30_table(const Fr30* __restrict__ t, uint32_t i) {
    Fr30 v;
#pragma unroll
    for (int k = 0; k < kR9; k++) v.d[k] = t[i].d[k];
    return v;
}
// a digit record between two launches: the nine digits of a lazy value as nine words, no reduction either way
__device__ __forceinline__ Fr30 fr30_digits(const uint32_t* __restrict__ p) {
    Fr30 v;
#pragma unroll
    for (int k = 0; k < kR9; k++) v.d[k] = (int32_t)p[k];
    return v;
}
__device__ __forceinline__ void fr30_put_digits(uint32_t* __restrict__ p, const Fr30& v) {
#pragma unroll
    for (int k = 0; k < kR9; k++) p[k] = (uint32_t)v.d[k];
}

// x^e (e < 2^22) in multiplier form from a pair of tables of multipliers, t: lo[i] = x^i then hi[i] = x^(2048 i), kNttTableLen
// entries each -- one product, |v| <= 0.5001 r
__device__ __forceinline__ Fr30 fr30_pow22(const Fr30* __restrict__ t, uint32_t e) {
    return fr30_mul(fr30_table(t + kNttTableLen, e >> 11), fr30_table(t, e & (kNttTableLen - 1)));
}
// w_n^i for n = 2^log_n <= 2^22 and i < n from the NTT's twiddle tables of w = w_(2^22) (tw: the forward tables, or the inverse
// ones for w_n^-i)
__device__ __forceinline__ Fr30 fr30_root(const Fr30* __restrict__ tw, uint32_t i, uint32_t log_n) {
    return fr30_pow22(tw, i << (kNttMaxLog - log_n));
}

// digit planes of N values in LDS: digit k of lane t at d[k][t], so that consecutive lanes touch consecutive banks
template <uint32_t N>
struct Fr30Plane {
    int32_t d[kR9][N];
};
template <uint32_t N>
__device__ __forceinline__ void plane_put(Fr30Plane<N>& p, uint32_t t, const Fr30& v) {
#pragma unroll
    for (int k = 0; k < kR9; k++) p.d[k][t] = v.d[k];
}
template <uint32_t N>
__device__ __forceinline__ Fr30 plane_get(const Fr30Plane<N>& p, uint32_t t) {
    Fr30 v;
#pragma unroll
    for (int k = 0; k < kR9; k++) v.d[k] = p.d[k][t];
    return v;
}
// The two product scans over the N lanes of a workgroup, which all call (log2 N rounds of one barrier, double buffered): on return
// pre[cur] holds the products of mp over lanes [0, t] and suf[cur] the products of ms over lanes [t, N - 1], visible to every
// lane, and mp, ms are the lane's own entries of the two; the return value is cur.  Operand order: pre x own, own x suf.  mp and
// ms are operands of fr30_mul and every entry is a product from the first round on.
template <uint32_t N>
__device__ __forceinline__ uint32_t fr30_scan_products(Fr30Plane<N> (&pre)[2], Fr30Plane<N> (&suf)[2], uint32_t t, Fr30& mp, Fr30& ms) {
    uint32_t cur = 0;
#pragma unroll 1
    for (uint32_t o = 1; o < N; o <<= 1) {
        plane_put(pre[cur], t, mp);
        plane_put(suf[cur], t, ms);
        __syncthreads();
        if (t >= o) mp = fr30_mul(plane_get(pre[cur], t - o), mp);
        if (t + o < N) ms = fr30_mul(ms, plane_get(suf[cur], t + o));
        cur ^= 1;
    }
    plane_put(pre[cur], t, mp);
    plane_put(suf[cur], t, ms);
    __syncthreads();
    return cur;
}

}  // namespace kzg
