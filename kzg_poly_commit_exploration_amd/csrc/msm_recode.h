// msm_recode.h -- the scalar recoding of the MSM sort (msm_sort.hip): the fold of a scalar to sign and magnitude, the
// 32-byte record the magnitude is kept in between the two passes of the sort, and the digit loops.  __host__ __device__
// code (plain C++ under g++: tests/host/msm_recode_host.cpp builds it for tests/test_msm_recode_host.py).
#pragma once
#include <stdint.h>

#include <utility>

#include "fr30.hip.h"

namespace kzg {

// The scalar as sign and magnitude of its shortest representative: |k| <= r / 2 (+ r / 2^31) < 2^254 in 8 words, and
// k * P = |k| * (+-P).  Returns true when the point has to be negated.  Besides halving the range this makes the
// reference's "negative" i128 inputs (r - |a|, src/scalar.rs:27-48) as cheap as the positive ones: their upper windows
// become zero digits, which are skipped.
// One product in the signed-digit field (fr30.hip.h) leaves the Montgomery form, reduces and centres at once: the blst_fr
// image is x * 2^256, times the single digit 2^14 over the multiplier's 2^270 is x; canonical little-endian bytes (expected
// below r, any 256-bit value accepted) times 2^270 mod r over 2^270 is the value mod r.  The product of balanced
// Montgomery digits is the centred residue up to r / 2^31 -- which representative is used changes the digits, not the sum.
// (Two calls: with the multiplier a compile-time constant the first is a reduction and nine shifts, not 162 multiply-adds.)
KZG_HD bool recode_fold(const uint32_t in[8], int is_mont, uint32_t k[8]) {
    const Fr30 d = fr30_from_limbs_raw(in);
    const Fr30 v = is_mont ? fr30_mul(d, fr30_small(1 << 14)) : fr30_mul(d, fr30_const_one270());
    return fr30_abs_to_limbs(v, k);
}

// The folded scalar as the sort keeps it between its passes: |k| < 2^254 leaves bits 254 and 255 free, bit 255 takes the
// negate flag.
KZG_HD void recode_pack(uint32_t k[8], bool flip) { k[7] |= flip ? 0x80000000u : 0u; }
KZG_HD bool recode_unpack(uint32_t k[8]) {
    const bool flip = (k[7] >> 31) != 0;
    k[7] &= 0x7fffffffu;
    return flip;
}

// Signed window recoding, low window first: digit in [-2^(c-1)+1, 2^(c-1)], carry into the next
// window.  |k| < 2^254 and W * c >= 255, so the top window absorbs the last carry.
// f(table level, bucket, negative)
template <class F>
KZG_HD void for_each_window_digit(uint32_t k[8], uint32_t c, uint32_t W, F&& f) {
    const uint32_t mask = (1u << c) - 1u;
    const uint32_t half = 1u << (c - 1);
    uint32_t carry = 0;
    for (uint32_t j = 0; j < W; j++) {
        uint32_t v = (k[0] & mask) + carry;
        // k >>= c
#pragma unroll
        for (int t = 0; t < 7; t++) k[t] = (k[t] >> c) | (k[t + 1] << (32 - c));
        k[7] >>= c;
        bool neg = v > half;
        uint32_t mag = neg ? (mask + 1u - v) : v;
        carry = neg ? 1u : 0u;
        if (mag) f(j, mag - 1u, neg);
    }
}

// The same digits at a width known to the compiler, without shifting the scalar: window j starts at bit j * C, a constant
// word and shift (the loop over j is unrolled in the front end, by an index sequence), so its bits are one funnel shift
// (v_alignbit_b32) and one mask -- or one bit-field extract where the window lies inside a word -- instead of the seven
// shifts of `k >>= c`.  Carry and sign exactly as above.
template <uint32_t C, uint32_t J, class F>
KZG_HD void window_digit_fixed(const uint32_t k[8], uint32_t& carry, F& f) {
    constexpr uint32_t mask = (1u << C) - 1u;
    constexpr uint32_t half = 1u << (C - 1);
    constexpr uint32_t w = (J * C) >> 5, s = (J * C) & 31u;
    constexpr bool straddles = s + C > 32u && w < 7u;  // (bits past 255 are zero)
    // (two 32-bit shifts, not one 64-bit one: a 64-bit value put together from k[w] and k[w + 1] becomes ONE 8-byte load of
    // the array, which then stays in memory instead of registers)
    uint32_t bits = k[w] >> s;
    if constexpr (straddles) bits |= k[w + 1u] << (32u - s);
    const uint32_t v = (bits & mask) + carry;
    const bool neg = v > half;
    const uint32_t mag = neg ? (mask + 1u - v) : v;
    carry = neg ? 1u : 0u;
    if (mag) f(J, mag - 1u, neg);
}
template <uint32_t C, class F, uint32_t... J>
KZG_HD void window_digits_fixed(const uint32_t k[8], F& f, std::integer_sequence<uint32_t, J...>) {
    uint32_t carry = 0;
    (window_digit_fixed<C, J>(k, carry, f), ...);
}
template <uint32_t C, class F>
KZG_HD void for_each_window_digit_fixed(const uint32_t k[8], F&& f) {
    static_assert(C >= 2 && C <= 31, "a window is cut out of two adjacent words");
    window_digits_fixed<C>(k, f, std::make_integer_sequence<uint32_t, (255 + C - 1) / C>());
}

// Width-c non-adjacent form, low bit first, without ever shifting the scalar: K' = (k >> pos) + carry is the
// value still to encode.  K' even -> next bit (the carry is unchanged: bit == carry).  K' odd -> the digit is
// v = (c bits of k at pos) + carry (no overflow: an odd K' means bit0 + carry == 1), taken as v - 2^c when
// v > 2^(c-1) (carry 1), and the next c-1 digits are zero.  Words are walked by an unrolled loop so that the
// scalar stays in registers; zero digits are skipped with one ffs per run.  |k| < 2^254 keeps the last digit at
// bit <= 254.  Digits are odd: bucket (|d| - 1) / 2, weight 2 * bucket + 1.
// f(bit position = table level, bucket, negative)
template <class F>
KZG_HD void for_each_naf_digit(const uint32_t k[8], uint32_t c, F&& f) {
    const uint32_t mask = (1u << c) - 1u;
    const uint32_t half = 1u << (c - 1);
    uint32_t carry = 0;
    uint32_t p = 0;  // bit offset inside word t (can exceed 32 after a digit)
#pragma unroll
    for (int t = 0; t < 8; t++) {
        const uint64_t win = ((uint64_t)(t < 7 ? k[t + 1] : 0u) << 32) | k[t];
        while (p < 32) {
            uint32_t x = (uint32_t)(win >> p);
            if (carry) x = ~x;
            // first position at or after p (inside this word) where bit != carry
            uint32_t z = x ? (uint32_t)__builtin_ctz(x) : 32u;
            if (z >= 32u - p) {
                p = 32;
                break;
            }
            p += z;
            uint32_t v = ((uint32_t)(win >> p) & mask) + carry;
            const bool neg = v > half;
            const uint32_t mag = neg ? (mask + 1u - v) : v;
            carry = neg ? 1u : 0u;
            f(32u * (uint32_t)t + p, (mag - 1u) >> 1, neg);
            p += c;
        }
        p -= 32;
    }
}

}  // namespace kzg
