// wire_enc30.hip.h -- encoders for outputs as they travel, the inverses of wire30.hip.h's decoders: an affine table record to
// the 48 bytes of a compressed G1 point (ZCash encoding: reference src/curves.rs:99-183), a blst_fr image to 32 big-endian
// bytes.  __host__ __device__ functions over field30.hip.h and fr30.hip.h (tests/host/wire_enc30_host.cpp compiles them with
// g++); blob_kernels.hip runs one of them per lane.
//
// Every field element has one canonical integer in [0, p) (or [0, r)), so an encoding is unique: what leaves here is byte for
// byte what kzg_g1_compress writes for the same point.
#pragma once
#include <stdint.h>

#include "wire30.hip.h"

namespace kzg {

// One point.  x, y: the table's record form (Montgomery 2^390, any digits fq_mul takes; both all zero for infinity).  raw:
// the 48 bytes as twelve 32-bit words in memory order (byte 0, the flags, is the low byte of raw[0]).
KZG_HD void wire_g1_encode(const Fq& x, const Fq& y, uint32_t raw[12]) {
    int32_t any = 0;
#pragma unroll
    for (int i = 0; i < kQ; i++) any |= x.d[i] | y.d[i];
    const Fq xi = fq_canonical_integer(x);
    const bool y_big = fq_digits_greater(fq_canonical_integer(y), fq_const_half());
    // canonical balanced digits of an integer in [0, p) -> unsigned 30-bit digits -> twelve little-endian words
    uint32_t u[kQ];
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < kQ - 1; i++) {
        const int32_t v = xi.d[i] + c;
        c = v >> kQBits;  // floor
        u[i] = (uint32_t)v & (uint32_t)kQMask;
    }
    u[kQ - 1] = (uint32_t)(xi.d[kQ - 1] + c);
    uint32_t w[12];
#pragma unroll
    for (int t = 0; t < 12; t++) {
        const int lo = 32 * t;
        const int i0 = lo / 30, sh = lo - 30 * i0;
        const uint64_t two = (uint64_t)u[i0] | ((uint64_t)(i0 + 1 < kQ ? u[i0 + 1] : 0u) << 30) |
                             ((uint64_t)(i0 + 2 < kQ ? u[i0 + 2] : 0u) << 60);
        w[t] = (uint32_t)(two >> sh);
    }
    const bool infinity = any == 0;
    w[11] |= 0x80000000u | (infinity ? 0x40000000u : (y_big ? 0x20000000u : 0u));  // x < p < 2^381: the three flag bits are free
#pragma unroll
    for (int t = 0; t < 12; t++) raw[t] = wire_bswap32(w[11 - t]);
}

// One scalar.  in: a blst_fr image (v * 2^256 mod r as 8 x u32, little-endian).  raw: the 32 big-endian bytes of v as eight
// words in memory order.  Returns kWireBad when the image is not below r (its residue is written), else 0.
KZG_HD uint32_t wire_fr_encode(const uint32_t in[8], uint32_t raw[8]) {
    uint32_t borrow = 0;
#pragma unroll
    for (int t = 0; t < 8; t++) {
        constexpr uint32_t RW[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};
        const uint64_t d = (uint64_t)in[t] - RW[t] - borrow;
        borrow = (uint32_t)(d >> 63);
    }
    uint32_t l[8];
    fr30_to_limbs(fr30_mul(fr30_from_limbs(in), fr30_small(1 << 14)), l);  // v * 2^256 * 2^14 / 2^270 = v
#pragma unroll
    for (int t = 0; t < 8; t++) raw[t] = wire_bswap32(l[7 - t]);
    return borrow == 0 ? kWireBad : 0u;  // no borrow: the image >= r
}

}  // namespace kzg
