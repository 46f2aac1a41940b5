// wire30.hip.h -- decoders for inputs as they travel: 48-byte compressed G1 points (ZCash encoding: reference
// src/curves.rs:99-183) and 32-byte big-endian scalars, as __host__ __device__ functions over field30.hip.h and fr30.hip.h
// (tests/host/wire30_host.cpp compiles them with g++).  The SRS loader (srs_io.hip) and the byte-string entry points of the
// verifiers (wire_kernels.hip) run one of them per lane.
//
// Acceptance of a point is blst_p1_uncompress's: compressed flag set; infinity = flag 0x40 and every other bit zero (the
// sign bit too); otherwise x < p as an integer, x^3 + 4 a square, y chosen by the sign bit against (p - 1) / 2.  No subgroup
// check: that is k_vc_ladder's.  A scalar is accepted when it is below r as an integer.
#pragma once
#include <stdint.h>

#include "field30.hip.h"
#include "fr30.hip.h"

namespace kzg {

constexpr uint32_t kWireInfinity = 1u;  // the encoding of infinity (x = y = 0 in the record form)
constexpr uint32_t kWireBad = 2u;       // not a valid compressed point / not below r

KZG_HD Fq fq_const_2_780() {
    Fq c;
    constexpr int32_t V[13] = {
#include "field30_c780.inc"
    };
#pragma unroll
    for (int i = 0; i < kQ; i++) c.d[i] = V[i];
    return c;
}
KZG_HD Fq fq_const_half() {
    Fq c;
    constexpr int32_t V[13] = {
#include "field30_half.inc"
    };
#pragma unroll
    for (int i = 0; i < kQ; i++) c.d[i] = V[i];
    return c;
}
// plain integer behind a lazy Montgomery value, canonical balanced digits in [0, p)
KZG_HD Fq fq_canonical_integer(const Fq& a) {
    Fq raw_one = fq_zero();
    raw_one.d[0] = 1;
    Fq t = fq_canon_digits(fq_mul(a, raw_one));  // x * 2^390 * 1 / 2^390 = x, |.| < 0.62 p
    int32_t s = 0;
#pragma unroll
    for (int i = 0; i < kQ; i++) s = t.d[i] != 0 ? t.d[i] : s;  // sign = sign of the most significant non-zero digit
    if (s < 0) {
#pragma unroll
        for (int i = 0; i < kQ; i++) t.d[i] += fq_pd(i);
        t = fq_canon_digits(t);
    }
    return t;
}
// a > b for canonical balanced digit vectors of non-negative integers
KZG_HD bool fq_digits_greater(const Fq& a, const Fq& b) {
    int32_t s = 0;
#pragma unroll
    for (int i = 0; i < kQ; i++) {
        const int32_t d = a.d[i] - b.d[i];
        s = d != 0 ? d : s;
    }
    return s > 0;
}

KZG_HD uint32_t wire_bswap32(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24); }

// One compressed point.  raw: its 48 bytes as twelve 32-bit words in memory order (a little-endian load of big-endian
// bytes: byte 0, the flags, is the low byte of raw[0]).  x, y: the table's record form (Montgomery 2^390, carry-normalised;
// both zero for infinity).  Returns kWireInfinity and / or kWireBad, 0 for a finite point on the curve.
KZG_HD uint32_t wire_g1_decode(const uint32_t raw[12], Fq& x, Fq& y) {
    const uint32_t flags = raw[0] & 0xffu;
    const bool compressed = flags & 0x80, infinity = flags & 0x40, y_big = flags & 0x20;
    bool bad = !compressed;
    // big-endian 381-bit x -> twelve little-endian 32-bit words
    uint32_t w[12];
#pragma unroll
    for (int t = 0; t < 12; t++) w[t] = wire_bswap32(raw[11 - t]);
    w[11] &= 0x1fffffffu;
    uint32_t any = 0;
#pragma unroll
    for (int t = 0; t < 12; t++) any |= w[t];
    if (infinity) {
        bad = bad || any != 0 || y_big;
        x = fq_zero();
        y = fq_zero();
        return kWireInfinity | (bad ? kWireBad : 0u);
    }
    // x < p ?
    {
        uint32_t borrow = 0;
#pragma unroll
        for (int t = 0; t < 12; t++) {
            constexpr uint32_t PW[12] = {0xffffaaabu, 0xb9feffffu, 0xb153ffffu, 0x1eabfffeu, 0xf6b0f624u, 0x6730d2a0u,
                                         0xf38512bfu, 0x64774b84u, 0x434bacd7u, 0x4b1ba7b6u, 0x397fe69au, 0x1a0111eau};
            const uint64_t d = (uint64_t)w[t] - PW[t] - borrow;
            borrow = (uint32_t)(d >> 63);
        }
        bad = bad || borrow == 0;  // no borrow: x >= p
    }
    // plain integer x -> signed digits -> Montgomery form: x_digits * 2^780 / 2^390 = x * 2^390
    const Fq c = fq_const_2_780();
    {
        Fq xi;
        uint32_t u[kQ];
#pragma unroll
        for (int k = 0; k < kQ; k++) {
            const int lo = 30 * k;
            const int wi = lo >> 5, sh = lo & 31;
            const uint64_t two = (uint64_t)(wi < 12 ? w[wi] : 0u) | ((uint64_t)(wi + 1 < 12 ? w[wi + 1] : 0u) << 32);
            u[k] = (uint32_t)(two >> sh) & (uint32_t)kQMask;
        }
        int32_t cy = 0;
#pragma unroll
        for (int k = 0; k < kQ - 1; k++) {
            const int32_t t = (int32_t)u[k] + cy;
            cy = (t + (1 << (kQBits - 1))) >> kQBits;
            xi.d[k] = t - (int32_t)((uint32_t)cy << kQBits);
        }
        xi.d[kQ - 1] = (int32_t)u[kQ - 1] + cy;
        x = fq_mul(xi, c);                           // x * 2^780 / 2^390 = x * 2^390
    }
    // t = x^3 + 4
    Fq four = fq_zero();
    four.d[0] = 4;
    four = fq_mul(four, c);  // 4 * 2^390, reduced
    const Fq t = fq_norm(fq_add_raw(fq_mul(fq_sqr(x), x), four));
    // y = t^((p + 1) / 4): p = 3 mod 4, so this is a square root whenever one exists
    constexpr uint64_t E[6] = {0xee7fbfffffffeaabULL, 0x07aaffffac54ffffULL, 0xd9cc34a83dac3d89ULL,
                               0xd91dd2e13ce144afULL, 0x92c6e9ed90d2eb35ULL, 0x0680447a8e5ff9a6ULL};
    y = fq_one();
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll 1
#endif
    for (int k = 378; k >= 0; k--) {
        y = fq_sqr(y);
        if ((E[k >> 6] >> (k & 63)) & 1) y = fq_mul(y, t);
    }
    bad = bad || !fq_is_zero(fq_norm(fq_sub_raw(fq_sqr(y), t)));  // not on the curve
    // the encoding's sign bit: set iff y > (p - 1) / 2 as an integer
    const Fq yi = fq_canonical_integer(y);
    const bool is_big = fq_digits_greater(yi, fq_const_half());
    if (is_big != y_big) y = fq_neg(y);
    y = fq_norm(y);  // (the negation keeps the digits' size; one carry pass for the table's contract)
    return bad ? kWireBad : 0u;
}

// 2^526 mod r, balanced digits of the centred residue: fr30_mul(v, .) = v * 2^526 / 2^270 = v * 2^256, the blst_fr image
KZG_HD constexpr int32_t fr30_c526(int i) {
    constexpr int32_t C[9] = {-0x18e4c406, -0x166efbf5, 0x1a2ce6c8, 0x1c3f74a7, -0x75a93b2, -0x164f06cb, -0x1cf09559, 0xbcf4408, -0x37b9};
    return C[i];
}

// One scalar.  raw: its 32 big-endian bytes as eight 32-bit words in memory order.  out: the blst_fr image (v * 2^256 mod r,
// canonical, 8 x u32 little-endian) the kernels read.  Returns kWireBad when the integer is not below r, else 0.
KZG_HD uint32_t wire_fr_decode(const uint32_t raw[8], uint32_t out[8]) {
    uint32_t l[8];
#pragma unroll
    for (int t = 0; t < 8; t++) l[t] = wire_bswap32(raw[7 - t]);
    uint32_t borrow = 0;
#pragma unroll
    for (int t = 0; t < 8; t++) {
        constexpr uint32_t RW[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};
        const uint64_t d = (uint64_t)l[t] - RW[t] - borrow;
        borrow = (uint32_t)(d >> 63);
    }
    Fr30 c;
#pragma unroll
    for (int i = 0; i < kR9; i++) c.d[i] = fr30_c526(i);
    fr30_to_limbs(fr30_mul(fr30_from_limbs(l), c), out);  // |product| <= 0.5001 r + 2^256 r / 2^271
    return borrow == 0 ? kWireBad : 0u;                    // no borrow: v >= r
}

// bits-bit reversal of i (bits <= 32; 0 for bits = 0)
KZG_HD uint32_t wire_brp(uint32_t i, uint32_t bits) {
#ifdef __HIP_DEVICE_COMPILE__
    return bits ? __brev(i) >> (32 - bits) : 0u;
#endif
    uint32_t r = 0;
    for (uint32_t b = 0; b < bits; b++) r |= ((i >> b) & 1u) << (bits - 1 - b);
    return r;
}

#ifdef __HIPCC__
// the 48 bytes of point i of a 16-byte aligned array / the 32 bytes of a scalar, as words in memory order
__device__ __forceinline__ void load_wire48(const uint4* __restrict__ p, uint32_t raw[12]) {
#pragma unroll
    for (int t = 0; t < 3; t++) {
        const uint4 v = p[t];
        raw[4 * t] = v.x; raw[4 * t + 1] = v.y; raw[4 * t + 2] = v.z; raw[4 * t + 3] = v.w;
    }
}
__device__ __forceinline__ void load_wire32(const uint4* __restrict__ p, uint32_t raw[8]) {
#pragma unroll
    for (int t = 0; t < 2; t++) {
        const uint4 v = p[t];
        raw[4 * t] = v.x; raw[4 * t + 1] = v.y; raw[4 * t + 2] = v.z; raw[4 * t + 3] = v.w;
    }
}
// 13 digits into the first 64 bytes of half a table record
__device__ __forceinline__ void store_digits16(uint4* __restrict__ p, const Fq& a) {
    p[0] = make_uint4((uint32_t)a.d[0], (uint32_t)a.d[1], (uint32_t)a.d[2], (uint32_t)a.d[3]);
    p[1] = make_uint4((uint32_t)a.d[4], (uint32_t)a.d[5], (uint32_t)a.d[6], (uint32_t)a.d[7]);
    p[2] = make_uint4((uint32_t)a.d[8], (uint32_t)a.d[9], (uint32_t)a.d[10], (uint32_t)a.d[11]);
    p[3] = make_uint4((uint32_t)a.d[12], 0u, 0u, 0u);
}
#endif

}  // namespace kzg
