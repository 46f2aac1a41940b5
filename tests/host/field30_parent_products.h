// field30_parent_products.h -- the product cores of csrc/field30.hip.h as they stood BEFORE the columns became single
// multiply-add chains (fq_mul, fq_mul_sub, fq_sqr, fq_mul_addc<+-1>, fq_sqr_minus), copied verbatim into a namespace of
// their own.  Test infrastructure only: tests/host/field30_columns_host.cpp compares today's functions with these, digit
// for digit.  Host build only; never edit to follow the library.  The text differs from the originals in three names: the
// two device-only macros (KZG_F30_FENCE, KZG_F30_OPAQUE_UNIT: no-ops on the host) carry a name of this file's, and the two
// calls of fq_mul_addc say which namespace they mean (the argument types would find the library's as well).
#pragma once
#include "../../kzg_poly_commit_exploration_amd/csrc/field30.hip.h"

#if defined(__HIP_DEVICE_COMPILE__)
#error "comparison copies for the host build only"
#endif

namespace kzg_parent {
using kzg::Fq;
using kzg::fq_pd;
using kzg::fq_round_shift;
using kzg::fq_sext30;
using kzg::kQ;
using kzg::kQBits;
using kzg::kQN0;
// the originals' fence and opaque unit: nothing on the host
#define KZG_PARENT_FENCE(acc) ((void)0)
#define KZG_PARENT_OPAQUE_UNIT(s) ((void)0)

// Montgomery product a * b / 2^390 (mod p), product scanning; see the header for the digit contract.
KZG_HD Fq fq_mul(const Fq& a, const Fq& b) {
    int32_t m[kQ];
    Fq r;
    int64_t acc = 0;
#pragma unroll
    for (int k = 0; k < kQ; k++) {
#pragma unroll
        for (int i = 0; i <= k; i++) acc += (int64_t)a.d[i] * b.d[k - i];
#pragma unroll
        for (int j = 0; j < k; j++) acc += (int64_t)m[j] * fq_pd(k - j);
        m[k] = fq_sext30((uint32_t)acc * kQN0);
        acc += (int64_t)m[k] * fq_pd(0);  // low 30 bits are now zero
        acc >>= kQBits;
        KZG_PARENT_FENCE(acc);
    }
#pragma unroll
    for (int k = kQ; k < 2 * kQ - 1; k++) {
#pragma unroll
        for (int i = k - kQ + 1; i < kQ; i++) acc += (int64_t)a.d[i] * b.d[k - i];
#pragma unroll
        for (int j = k - kQ + 1; j < kQ; j++) acc += (int64_t)m[j] * fq_pd(k - j);
        r.d[k - kQ] = fq_sext30((uint32_t)acc);
        acc = fq_round_shift(acc);
        KZG_PARENT_FENCE(acc);
    }
    r.d[kQ - 1] = (int32_t)acc;
    return r;
}

// (a * b - c * d) / 2^390 (mod p) with ONE Montgomery reduction: both digit products are accumulated into the same
// columns.  Column bound: 2 x 12 full products of at most (2^29 + 4)^2 plus the m * p part,
// 6.0 * 2^60 + 1.55 * 2^60 < 2^63 -- so ALL FOUR operands must be weakly normalised (|digit| <= 2^29 + 4; no raw sums
// here), |a b - c d| < 2^771.  Saves 169 multiply-adds and the carry work of one product wherever the group law
// subtracts two products (Y3 = R (Q - X3) - Y1 PPP).
KZG_HD Fq fq_mul_sub(const Fq& a, const Fq& b, const Fq& c, const Fq& d) {
    int32_t m[kQ];
    Fq r;
    int64_t acc = 0;
#pragma unroll
    for (int k = 0; k < kQ; k++) {
#pragma unroll
        for (int i = 0; i <= k; i++) acc += (int64_t)a.d[i] * b.d[k - i];
#pragma unroll
        for (int i = 0; i <= k; i++) acc -= (int64_t)c.d[i] * d.d[k - i];
#pragma unroll
        for (int j = 0; j < k; j++) acc += (int64_t)m[j] * fq_pd(k - j);
        m[k] = fq_sext30((uint32_t)acc * kQN0);
        acc += (int64_t)m[k] * fq_pd(0);
        acc >>= kQBits;
        KZG_PARENT_FENCE(acc);
    }
#pragma unroll
    for (int k = kQ; k < 2 * kQ - 1; k++) {
#pragma unroll
        for (int i = k - kQ + 1; i < kQ; i++) acc += (int64_t)a.d[i] * b.d[k - i];
#pragma unroll
        for (int i = k - kQ + 1; i < kQ; i++) acc -= (int64_t)c.d[i] * d.d[k - i];
#pragma unroll
        for (int j = k - kQ + 1; j < kQ; j++) acc += (int64_t)m[j] * fq_pd(k - j);
        r.d[k - kQ] = fq_sext30((uint32_t)acc);
        acc = fq_round_shift(acc);
        KZG_PARENT_FENCE(acc);
    }
    r.d[kQ - 1] = (int32_t)acc;
    return r;
}

// Montgomery square: cross products once against the doubled operand (91 instead of 169 digit products)
KZG_HD Fq fq_sqr(const Fq& a) {
    int32_t m[kQ], dbl[kQ];
#pragma unroll
    for (int i = 0; i < kQ; i++) dbl[i] = a.d[i] * 2;
    Fq r;
    int64_t acc = 0;
#pragma unroll
    for (int k = 0; k < kQ; k++) {
#pragma unroll
        for (int i = 0; 2 * i < k; i++) acc += (int64_t)dbl[i] * a.d[k - i];
        if ((k & 1) == 0) acc += (int64_t)a.d[k / 2] * a.d[k / 2];
#pragma unroll
        for (int j = 0; j < k; j++) acc += (int64_t)m[j] * fq_pd(k - j);
        m[k] = fq_sext30((uint32_t)acc * kQN0);
        acc += (int64_t)m[k] * fq_pd(0);
        acc >>= kQBits;
        KZG_PARENT_FENCE(acc);
    }
#pragma unroll
    for (int k = kQ; k < 2 * kQ - 1; k++) {
#pragma unroll
        for (int i = k - kQ + 1; 2 * i < k; i++) acc += (int64_t)dbl[i] * a.d[k - i];
        if ((k & 1) == 0) acc += (int64_t)a.d[k / 2] * a.d[k / 2];
#pragma unroll
        for (int j = k - kQ + 1; j < kQ; j++) acc += (int64_t)m[j] * fq_pd(k - j);
        r.d[k - kQ] = fq_sext30((uint32_t)acc);
        acc = fq_round_shift(acc);
        KZG_PARENT_FENCE(acc);
    }
    r.d[kQ - 1] = (int32_t)acc;
    return r;
}

template <int kSign>
KZG_HD Fq fq_mul_addc(const Fq& a, const Fq& b, const Fq& c) {
    static_assert(kSign == 1 || kSign == -1, "a b / 2^390 + c or a b / 2^390 - c");
    int32_t unit = kSign;
    KZG_PARENT_OPAQUE_UNIT(unit);
    int32_t m[kQ];
    Fq r;
    int64_t acc = 0;
#pragma unroll
    for (int k = 0; k < kQ; k++) {
#pragma unroll
        for (int i = 0; i <= k; i++) acc += (int64_t)a.d[i] * b.d[k - i];
#pragma unroll
        for (int j = 0; j < k; j++) acc += (int64_t)m[j] * fq_pd(k - j);
        m[k] = fq_sext30((uint32_t)acc * kQN0);
        acc += (int64_t)m[k] * fq_pd(0);  // low 30 bits are now zero
        acc >>= kQBits;
        KZG_PARENT_FENCE(acc);
    }
#pragma unroll
    for (int k = kQ; k < 2 * kQ - 1; k++) {
#pragma unroll
        for (int i = k - kQ + 1; i < kQ; i++) acc += (int64_t)a.d[i] * b.d[k - i];
#pragma unroll
        for (int j = k - kQ + 1; j < kQ; j++) acc += (int64_t)m[j] * fq_pd(k - j);
        acc += (int64_t)c.d[k - kQ] * unit;
        r.d[k - kQ] = fq_sext30((uint32_t)acc);
        acc = fq_round_shift(acc);
        KZG_PARENT_FENCE(acc);
    }
    r.d[kQ - 1] = (int32_t)acc + kSign * c.d[kQ - 1];
    return r;
}
KZG_HD Fq fq_mul_minus(const Fq& a, const Fq& b, const Fq& c) { return kzg_parent::fq_mul_addc<-1>(a, b, c); }  // a b / 2^390 - c
KZG_HD Fq fq_mul_plus(const Fq& a, const Fq& b, const Fq& c) { return kzg_parent::fq_mul_addc<1>(a, b, c); }    // a b / 2^390 + c
// a^2 / 2^390 - c
KZG_HD Fq fq_sqr_minus(const Fq& a, const Fq& c) {
    int32_t unit = -1;
    KZG_PARENT_OPAQUE_UNIT(unit);
    int32_t m[kQ], dbl[kQ];
#pragma unroll
    for (int i = 0; i < kQ; i++) dbl[i] = a.d[i] * 2;
    Fq r;
    int64_t acc = 0;
#pragma unroll
    for (int k = 0; k < kQ; k++) {
#pragma unroll
        for (int i = 0; 2 * i < k; i++) acc += (int64_t)dbl[i] * a.d[k - i];
        if ((k & 1) == 0) acc += (int64_t)a.d[k / 2] * a.d[k / 2];
#pragma unroll
        for (int j = 0; j < k; j++) acc += (int64_t)m[j] * fq_pd(k - j);
        m[k] = fq_sext30((uint32_t)acc * kQN0);
        acc += (int64_t)m[k] * fq_pd(0);
        acc >>= kQBits;
        KZG_PARENT_FENCE(acc);
    }
#pragma unroll
    for (int k = kQ; k < 2 * kQ - 1; k++) {
#pragma unroll
        for (int i = k - kQ + 1; 2 * i < k; i++) acc += (int64_t)dbl[i] * a.d[k - i];
        if ((k & 1) == 0) acc += (int64_t)a.d[k / 2] * a.d[k / 2];
#pragma unroll
        for (int j = k - kQ + 1; j < kQ; j++) acc += (int64_t)m[j] * fq_pd(k - j);
        acc += (int64_t)c.d[k - kQ] * unit;
        r.d[k - kQ] = fq_sext30((uint32_t)acc);
        acc = fq_round_shift(acc);
        KZG_PARENT_FENCE(acc);
    }
    r.d[kQ - 1] = (int32_t)acc - c.d[kQ - 1];
    return r;
}

}  // namespace kzg_parent
