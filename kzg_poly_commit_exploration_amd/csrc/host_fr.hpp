// host_fr.hpp -- scalar field Fr on the host (4 x u64, Montgomery R = 2^256: the blst_fr memory image that crosses
// the C-ABI).  Used by the multi-device context for the K-step carry recurrence of a range-sharded opening
// (multi.hip); everything O(n) stays on the devices.  Mirrors the operations the reference takes from blst through
// `Scalar` (src/scalar.rs:111-117, 192-218): add, sub, mul, pow; the inverse and the barycentric weights of a
// multiproof's points (api.hip: kzg_open_points and kzg_verify_points).
#pragma once
#include <stdint.h>
#include <string.h>

namespace kzg_host {

struct Fr {
    uint64_t l[4];
    bool is_zero() const { return (l[0] | l[1] | l[2] | l[3]) == 0; }
    bool operator==(const Fr& o) const { return memcmp(l, o.l, sizeof l) == 0; }
};

static const Fr kFrMod = {{0xffffffff00000001ULL, 0x53bda402fffe5bfeULL, 0x3339d80809a1d805ULL, 0x73eda753299d7d48ULL}};
static const Fr kFrOne = {{0x00000001fffffffeULL, 0x5884b7fa00034802ULL, 0x998c4fefecbc4ff5ULL, 0x1824b159acc5056fULL}};
static const uint64_t kFrN0 = 0xfffffffeffffffffULL;

inline bool fr_geq(const Fr& a, const Fr& b) {
    for (int i = 3; i >= 0; --i)
        if (a.l[i] != b.l[i]) return a.l[i] > b.l[i];
    return true;
}
inline Fr fr_raw_sub(const Fr& a, const Fr& b, uint64_t& borrow) {
    Fr r;
    borrow = 0;
    for (int i = 0; i < 4; ++i) {
        unsigned __int128 d = (unsigned __int128)a.l[i] - b.l[i] - borrow;
        r.l[i] = (uint64_t)d;
        borrow = (uint64_t)(d >> 64) & 1;
    }
    return r;
}
inline Fr fr_add(const Fr& a, const Fr& b) {
    Fr s;
    unsigned __int128 c = 0;
    for (int i = 0; i < 4; ++i) {
        c += (unsigned __int128)a.l[i] + b.l[i];
        s.l[i] = (uint64_t)c;
        c >>= 64;
    }
    uint64_t br;
    return (c || fr_geq(s, kFrMod)) ? fr_raw_sub(s, kFrMod, br) : s;  // 2r < 2^256: c is always 0
}
inline Fr fr_mul(const Fr& a, const Fr& b) {  // Montgomery product, CIOS
    uint64_t t[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; ++i) {
        unsigned __int128 c = 0;
        for (int j = 0; j < 4; ++j) {
            c += (unsigned __int128)a.l[j] * b.l[i] + t[j];
            t[j] = (uint64_t)c;
            c >>= 64;
        }
        c += t[4];
        t[4] = (uint64_t)c;
        t[5] = (uint64_t)(c >> 64);
        const uint64_t m = t[0] * kFrN0;
        c = ((unsigned __int128)m * kFrMod.l[0] + t[0]) >> 64;
        for (int j = 1; j < 4; ++j) {
            c += (unsigned __int128)m * kFrMod.l[j] + t[j];
            t[j - 1] = (uint64_t)c;
            c >>= 64;
        }
        c += t[4];
        t[3] = (uint64_t)c;
        t[4] = t[5] + (uint64_t)(c >> 64);
    }
    Fr r = {{t[0], t[1], t[2], t[3]}};
    uint64_t br;
    if (t[4] || fr_geq(r, kFrMod)) r = fr_raw_sub(r, kFrMod, br);
    return r;
}
inline Fr fr_pow(Fr base, uint64_t e) {
    Fr acc = kFrOne;
    while (e) {
        if (e & 1) acc = fr_mul(acc, base);
        base = fr_mul(base, base);
        e >>= 1;
    }
    return acc;
}

inline Fr fr_sub(const Fr& a, const Fr& b) {
    uint64_t br;
    Fr d = fr_raw_sub(a, b, br);
    if (br) {
        unsigned __int128 c = 0;
        for (int i = 0; i < 4; ++i) {
            c += (unsigned __int128)d.l[i] + kFrMod.l[i];
            d.l[i] = (uint64_t)c;
            c >>= 64;
        }
    }
    return d;
}
// a^(r-2) = 1/a (0 for a = 0)
inline Fr fr_inv(const Fr& a) {
    static const uint64_t e[4] = {0xfffffffeffffffffULL, 0x53bda402fffe5bfeULL, 0x3339d80809a1d805ULL, 0x73eda753299d7d48ULL};
    Fr acc = kFrOne;
    for (int i = 255; i >= 0; --i) {
        acc = fr_mul(acc, acc);
        if ((e[i >> 6] >> (i & 63)) & 1) acc = fr_mul(acc, a);
    }
    return acc;
}
// w_n for n = 2^log_n (log_n <= 32): 7^((r - 1) / n), 7 the multiplicative generator of blst / c-kzg / EIP-4844.
// r - 1 = 2^32 t with t odd: w_(2^32) = 7^t, then 32 - log_n squarings.
inline Fr fr_domain_root(unsigned log_n) {
    static const uint64_t t[4] = {0xfffe5bfeffffffffULL, 0x09a1d80553bda402ULL, 0x299d7d483339d808ULL, 0x0000000073eda753ULL};
    Fr seven = kFrOne;
    for (int i = 0; i < 6; i++) seven = fr_add(seven, kFrOne);
    Fr acc = kFrOne;
    for (int i = 255; i >= 0; --i) {
        acc = fr_mul(acc, acc);
        if ((t[i >> 6] >> (i & 63)) & 1) acc = fr_mul(acc, seven);
    }
    for (unsigned i = log_n; i < 32; i++) acc = fr_mul(acc, acc);
    return acc;
}
// the barycentric weights of k <= 64 distinct points: w_i = 1 / prod_{j != i} (z_i - z_j).  false when two points coincide.
inline bool fr_point_weights(const Fr* zs, size_t k, Fr* ws) {
    for (size_t i = 0; i < k; ++i) {
        Fr d = kFrOne;
        for (size_t j = 0; j < k; ++j)
            if (j != i) d = fr_mul(d, fr_sub(zs[i], zs[j]));
        if (d.is_zero()) return false;
        ws[i] = d;
    }
    // one inversion for all of them (prefix products)
    Fr run = kFrOne;
    Fr pre[64];
    for (size_t i = 0; i < k; ++i) {
        pre[i] = run;
        run = fr_mul(run, ws[i]);
    }
    Fr inv = fr_inv(run);
    for (size_t i = k; i-- > 0;) {
        const Fr wi = fr_mul(inv, pre[i]);
        inv = fr_mul(inv, ws[i]);
        ws[i] = wi;
    }
    return true;
}
// the coefficients zc[0 .. k] of Z = prod_{i < k} (X - z_i): one factor at a time
inline void fr_vanishing_coeffs(const Fr* zs, size_t k, Fr* zc) {
    const Fr fr0 = {{0, 0, 0, 0}};
    for (size_t j = 1; j <= k; ++j) zc[j] = fr0;
    zc[0] = kFrOne;
    for (size_t i = 0; i < k; ++i) {  // degree i -> i + 1: new[j] = old[j - 1] - z_i old[j]
        for (size_t j = i + 1; j > 0; --j) zc[j] = fr_sub(zc[j - 1], fr_mul(zs[i], zc[j]));
        zc[0] = fr_sub(fr0, fr_mul(zs[i], zc[0]));
    }
}
// the coefficients ic[0 .. k) of the interpolant of (z_i, y_i), I = sum_i (y_i w_i) Z / (X - z_i): synthetic division of Z
// (zc, from fr_vanishing_coeffs) by each root, with the weights of fr_point_weights
inline void fr_interpolant_coeffs(const Fr* zs, const Fr* ws, const Fr* ys, size_t k, const Fr* zc, Fr* ic) {
    const Fr fr0 = {{0, 0, 0, 0}};
    for (size_t j = 0; j < k; ++j) ic[j] = fr0;
    for (size_t i = 0; i < k; ++i) {
        const Fr t = fr_mul(ys[i], ws[i]);
        Fr b = zc[k];  // coefficient k - 1 of Z / (X - z_i)
        for (size_t j = k; j-- > 0;) {
            ic[j] = fr_add(ic[j], fr_mul(t, b));
            if (j) b = fr_add(zc[j], fr_mul(zs[i], b));
        }
    }
}

}  // namespace kzg_host
