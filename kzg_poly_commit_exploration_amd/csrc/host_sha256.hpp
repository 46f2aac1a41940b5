// host_sha256.hpp -- SHA-256 (FIPS 180-4) in portable C++ for the Fiat-Shamir challenges of blob proofs.
//
// Streaming: init / update / final over a copyable state, so that a caller may hash a long prefix once, keep the midstate
// and finish it later with a suffix (api.hip hashes a blob's domain, degree and bytes while the device works, and appends
// the 48 commitment bytes when they arrive).
// Two block functions: the portable one, and on x86-64 one on the SHA extensions (sha256rnds2 / sha256msg1 / sha256msg2),
// taken when CPUID reports them (5 x the portable rate per thread).  A state keeps the path it was
// initialised for, so a test can run each explicitly.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#if defined(__x86_64__)
#include <cpuid.h>
#include <immintrin.h>
#define KZG_SHA256_X86 1
#endif

namespace kzg_host {

struct Sha256 {
    uint32_t h[8];
    uint64_t len;       // bytes taken so far
    uint8_t buf[64];    // the open block: len % 64 bytes of it are filled
    bool ni;            // the blocks go through the SHA extensions
};
enum Sha256Path : int { kSha256Auto = 0, kSha256Portable = 1, kSha256ShaNi = 2 };

namespace sha256_detail {
// FIPS 180-4 section 4.2.2: the first 32 bits of the fractional parts of the cube roots of the first 64 primes
constexpr uint32_t kK[64] = {
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
    0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
    0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
    0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
    0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
    0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
    0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
    0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
inline uint32_t rotr(uint32_t x, int k) { return (x >> k) | (x << (32 - k)); }
// section 6.2.2 on one 64-byte block
inline void compress(uint32_t h[8], const uint8_t* p) {
    uint32_t w[64];
    for (int t = 0; t < 16; t++)
        w[t] = ((uint32_t)p[4 * t] << 24) | ((uint32_t)p[4 * t + 1] << 16) | ((uint32_t)p[4 * t + 2] << 8) | (uint32_t)p[4 * t + 3];
    for (int t = 16; t < 64; t++) {
        const uint32_t s0 = rotr(w[t - 15], 7) ^ rotr(w[t - 15], 18) ^ (w[t - 15] >> 3);
        const uint32_t s1 = rotr(w[t - 2], 17) ^ rotr(w[t - 2], 19) ^ (w[t - 2] >> 10);
        w[t] = w[t - 16] + s0 + w[t - 7] + s1;
    }
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
    for (int t = 0; t < 64; t++) {
        const uint32_t S1 = rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25);
        const uint32_t ch = (e & f) ^ (~e & g);
        const uint32_t t1 = hh + S1 + ch + kK[t] + w[t];
        const uint32_t S0 = rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22);
        const uint32_t maj = (a & b) ^ (a & c) ^ (b & c);
        const uint32_t t2 = S0 + maj;
        hh = g; g = f; f = e; e = d + t1;
        d = c; c = b; b = a; a = t1 + t2;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}

#ifdef KZG_SHA256_X86
inline bool cpu_has_sha() {
    static const bool has = [] {
        unsigned a = 0, b = 0, c = 0, d = 0;
        if (!__get_cpuid(1, &a, &b, &c, &d) || !((c >> 9) & 1u) || !((c >> 19) & 1u)) return false;  // SSSE3, SSE4.1
        return __get_cpuid_count(7, 0, &a, &b, &c, &d) && ((b >> 29) & 1u);                           // SHA
    }();
    return has;
}
// the same function of (h, block) on the SHA extensions.  The two state registers hold (A, B, E, F) and (C, D, G, H), high
// lane first; sha256rnds2 runs two rounds on the two low lanes of w + k and returns the new (A, B, E, F), the old one being
// the new (C, D, G, H).  The schedule keeps the last sixteen words in four registers: W[t .. t+3] =
// msg2(msg1(W[t-16 ..], W[t-12 ..]) + W[t-7 .. t-4], W[t-4 ..]).
__attribute__((target("sha,sse4.1,ssse3"))) inline void compress_shani(uint32_t h[8], const uint8_t* p, size_t blocks) {
    const __m128i swap = _mm_set_epi64x(0x0c0d0e0f08090a0bULL, 0x0405060700010203ULL);  // big-endian words
    __m128i t = _mm_shuffle_epi32(_mm_loadu_si128(reinterpret_cast<const __m128i*>(h)), 0xB1);       // C D A B
    __m128i s1 = _mm_shuffle_epi32(_mm_loadu_si128(reinterpret_cast<const __m128i*>(h + 4)), 0x1B);  // E F G H
    __m128i s0 = _mm_alignr_epi8(t, s1, 8);                                                          // A B E F
    s1 = _mm_blend_epi16(s1, t, 0xF0);                                                               // C D G H
    for (; blocks; blocks--, p += 64) {
        const __m128i save0 = s0, save1 = s1;
        __m128i m[4];
#pragma unroll
        for (int i = 0; i < 16; i++) {
            if (i < 4) {
                m[i] = _mm_shuffle_epi8(_mm_loadu_si128(reinterpret_cast<const __m128i*>(p + 16 * i)), swap);
            } else {
                const __m128i a = m[i & 3], b = m[(i + 1) & 3], c = m[(i + 2) & 3], d = m[(i + 3) & 3];
                const __m128i x = _mm_add_epi32(_mm_sha256msg1_epu32(a, b), _mm_alignr_epi8(d, c, 4));
                m[i & 3] = _mm_sha256msg2_epu32(x, d);
            }
            __m128i wk = _mm_add_epi32(m[i & 3], _mm_loadu_si128(reinterpret_cast<const __m128i*>(kK + 4 * i)));
            s1 = _mm_sha256rnds2_epu32(s1, s0, wk);
            wk = _mm_shuffle_epi32(wk, 0x0E);
            s0 = _mm_sha256rnds2_epu32(s0, s1, wk);
        }
        s0 = _mm_add_epi32(s0, save0);
        s1 = _mm_add_epi32(s1, save1);
    }
    t = _mm_shuffle_epi32(s0, 0x1B);                                         // F E B A
    s1 = _mm_shuffle_epi32(s1, 0xB1);                                        // D C H G
    _mm_storeu_si128(reinterpret_cast<__m128i*>(h), _mm_blend_epi16(t, s1, 0xF0));      // A B C D in memory order
    _mm_storeu_si128(reinterpret_cast<__m128i*>(h + 4), _mm_alignr_epi8(s1, t, 8));     // E F G H
}
#else
inline bool cpu_has_sha() { return false; }
#endif
inline void blocks(Sha256& s, const uint8_t* p, size_t count) {
#ifdef KZG_SHA256_X86
    if (s.ni) {
        compress_shani(s.h, p, count);
        return;
    }
#endif
    for (; count; count--, p += 64) compress(s.h, p);
}
}  // namespace sha256_detail

inline bool sha256_has_shani() { return sha256_detail::cpu_has_sha(); }

// path: kSha256Auto takes the SHA extensions where the CPU has them; kSha256ShaNi on a CPU without them returns false
inline bool sha256_init(Sha256& s, int path = kSha256Auto) {
    // section 5.3.3: the fractional parts of the square roots of the first eight primes
    static const uint32_t h0[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
    if (path == kSha256ShaNi && !sha256_has_shani()) return false;
    s.ni = path == kSha256ShaNi || (path == kSha256Auto && sha256_has_shani());
    std::memcpy(s.h, h0, sizeof h0);
    s.len = 0;
    return true;
}

inline void sha256_update(Sha256& s, const uint8_t* data, size_t n) {
    size_t fill = (size_t)(s.len & 63);
    s.len += n;
    if (fill) {
        const size_t take = 64 - fill < n ? 64 - fill : n;
        std::memcpy(s.buf + fill, data, take);
        data += take;
        n -= take;
        if (fill + take < 64) return;
        sha256_detail::blocks(s, s.buf, 1);
    }
    if (n >= 64) {
        sha256_detail::blocks(s, data, n / 64);
        data += n & ~(size_t)63;
        n &= 63;
    }
    if (n) std::memcpy(s.buf, data, n);
}

// section 5.1.1: a one bit, zeros, the length in bits as 64 bits big-endian; the state is spent afterwards
inline void sha256_final(Sha256& s, uint8_t out[32]) {
    const uint64_t bits = s.len * 8;
    size_t fill = (size_t)(s.len & 63);
    s.buf[fill++] = 0x80;
    if (fill > 56) {
        std::memset(s.buf + fill, 0, 64 - fill);
        sha256_detail::blocks(s, s.buf, 1);
        fill = 0;
    }
    std::memset(s.buf + fill, 0, 56 - fill);
    for (int i = 0; i < 8; i++) s.buf[56 + i] = (uint8_t)(bits >> (56 - 8 * i));
    sha256_detail::blocks(s, s.buf, 1);
    for (int i = 0; i < 8; i++) {
        out[4 * i] = (uint8_t)(s.h[i] >> 24);
        out[4 * i + 1] = (uint8_t)(s.h[i] >> 16);
        out[4 * i + 2] = (uint8_t)(s.h[i] >> 8);
        out[4 * i + 3] = (uint8_t)s.h[i];
    }
}

}  // namespace kzg_host
