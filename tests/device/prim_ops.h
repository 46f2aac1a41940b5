// prim_ops.h -- one function per primitive of csrc/field30.hip.h, field30_inv.hip.h, fr30.hip.h and g1_30.hip.h, over
// flat int32 records.  Test infrastructure only: tests/device/prims.hip wraps every function in a kernel (the device
// build of the headers), tests/host/field30_host.cpp and fr30_host.cpp in a loop (the g++ build), and
// tests/prim_cases.py holds the records and their big-integer expectations.  The csrc headers are included unchanged.
//
// PRIM_FQ_OPS / PRIM_FR_OPS list (name, ints per input record, ints per output record); unsigned words travel as int32.
#pragma once
#include <stdint.h>

#ifdef PRIM_CSRC_INCLUDES  // the Makefile's CSRC: another copy of the headers (mutation runs)
#include "field30_inv.hip.h"
#include "fr30.hip.h"
#include "g1_30.hip.h"
#include "wire30.hip.h"
#else
#include "../../kzg_poly_commit_exploration_amd/csrc/field30_inv.hip.h"
#include "../../kzg_poly_commit_exploration_amd/csrc/fr30.hip.h"
#include "../../kzg_poly_commit_exploration_amd/csrc/g1_30.hip.h"
#include "../../kzg_poly_commit_exploration_amd/csrc/wire30.hip.h"
#endif

#ifdef __HIPCC__
#define PRIM_FN __device__ __forceinline__
#else
#define PRIM_FN static inline
#endif

namespace prim {
using namespace kzg;

constexpr int kF = kQ;        // ints per Fq
constexpr int kX = 4 * kQ;    // ints per XYZZ30
constexpr int kChain = 16;    // operands per chain case
constexpr int kLoopOps = 3;   // operands per case of the dense loop shape

PRIM_FN Fq ld_fq(const int32_t* p) {
    Fq r;
    for (int i = 0; i < kQ; i++) r.d[i] = p[i];
    return r;
}
PRIM_FN void st_fq(int32_t* p, const Fq& a) {
    for (int i = 0; i < kQ; i++) p[i] = a.d[i];
}
PRIM_FN XYZZ30 ld_xyzz(const int32_t* p) {
    XYZZ30 a;
    a.X = ld_fq(p);
    a.Y = ld_fq(p + kF);
    a.ZZ = ld_fq(p + 2 * kF);
    a.ZZZ = ld_fq(p + 3 * kF);
    return a;
}
PRIM_FN void st_xyzz(int32_t* p, const XYZZ30& a) {
    st_fq(p, a.X);
    st_fq(p + kF, a.Y);
    st_fq(p + 2 * kF, a.ZZ);
    st_fq(p + 3 * kF, a.ZZZ);
}
PRIM_FN Affine30 ld_affine(const int32_t* p) {
    Affine30 a;
    a.x = ld_fq(p);
    a.y = ld_fq(p + kF);
    return a;
}
PRIM_FN Fr30 ld_fr(const int32_t* p) {
    Fr30 r;
    for (int i = 0; i < kR9; i++) r.d[i] = p[i];
    return r;
}
PRIM_FN void st_fr(int32_t* p, const Fr30& a) {
    for (int i = 0; i < kR9; i++) p[i] = a.d[i];
}

// ---- Fp ------------------------------------------------------------------------------------------------------------
PRIM_FN void pop_fq_mul(const int32_t* in, int32_t* out) { st_fq(out, fq_mul(ld_fq(in), ld_fq(in + kF))); }
PRIM_FN void pop_fq_sqr(const int32_t* in, int32_t* out) { st_fq(out, fq_sqr(ld_fq(in))); }
PRIM_FN void pop_fq_mul_sub(const int32_t* in, int32_t* out) {
    st_fq(out, fq_mul_sub(ld_fq(in), ld_fq(in + kF), ld_fq(in + 2 * kF), ld_fq(in + 3 * kF)));
}
PRIM_FN void pop_fq_norm(const int32_t* in, int32_t* out) { st_fq(out, fq_norm(ld_fq(in))); }
PRIM_FN void pop_fq_norm_wide(const int32_t* in, int32_t* out) { st_fq(out, fq_norm_wide(ld_fq(in))); }
PRIM_FN void pop_fq_neg(const int32_t* in, int32_t* out) { st_fq(out, fq_neg(ld_fq(in))); }
PRIM_FN void pop_fq_cneg(const int32_t* in, int32_t* out) { st_fq(out, fq_cneg(ld_fq(in), in[kF] != 0)); }
PRIM_FN void pop_fq_canon_digits(const int32_t* in, int32_t* out) { st_fq(out, fq_canon_digits(ld_fq(in))); }
PRIM_FN void pop_fq_is_zero(const int32_t* in, int32_t* out) { out[0] = fq_is_zero(ld_fq(in)) ? 1 : 0; }
PRIM_FN void pop_fq_from_u32x12(const int32_t* in, int32_t* out) {
    uint32_t s[12];
    for (int i = 0; i < 12; i++) s[i] = (uint32_t)in[i];
    st_fq(out, fq_from_u32x12(s));
}
PRIM_FN void pop_fq_to_u32x12(const int32_t* in, int32_t* out) {
    uint32_t s[12];
    fq_to_u32x12(ld_fq(in), s);
    for (int i = 0; i < 12; i++) out[i] = (int32_t)s[i];
}
// the plain integer in canonical digits, and whether it is above (p - 1) / 2 (the sign bit of the wire format)
PRIM_FN void pop_fq_canon_half(const int32_t* in, int32_t* out) {
    const Fq c = fq_canonical_integer(ld_fq(in));
    st_fq(out, c);
    out[kF] = fq_digits_greater(c, fq_const_half()) ? 1 : 0;
}
PRIM_FN void pop_fq_inv(const int32_t* in, int32_t* out) { st_fq(out, fq_inv(ld_fq(in))); }
// the products that take a third value into their own carry pass (the accumulation kernel's arithmetic): a, b, c
PRIM_FN void pop_fq_mul_minus(const int32_t* in, int32_t* out) {
    st_fq(out, fq_mul_minus(ld_fq(in), ld_fq(in + kF), ld_fq(in + 2 * kF)));
}
PRIM_FN void pop_fq_mul_plus(const int32_t* in, int32_t* out) {
    st_fq(out, fq_mul_plus(ld_fq(in), ld_fq(in + kF), ld_fq(in + 2 * kF)));
}
PRIM_FN void pop_fq_sqr_minus(const int32_t* in, int32_t* out) { st_fq(out, fq_sqr_minus(ld_fq(in), ld_fq(in + kF))); }
PRIM_FN void pop_fq_maybe_zero(const int32_t* in, int32_t* out) { out[0] = fq_maybe_zero(ld_fq(in)) ? 1 : 0; }

// ---- group law: acc (52) [, operand, flags] -> acc (52) -----------------------------------------------------------------
PRIM_FN void pop_madd(const int32_t* in, int32_t* out) {  // acc, affine point, neg
    XYZZ30 acc = ld_xyzz(in);
    xyzz30_madd(acc, ld_affine(in + kX), in[kX + 2 * kF] != 0);
    st_xyzz(out, acc);
}
// ---- the accumulation kernel's form of the mixed addition (xyzz30_acc_*) -----------------------------------------------
PRIM_FN void pop_acc_head(const int32_t* in, int32_t* out) {  // acc, affine point, neg -> code, P, Rn
    Fq P, Rn;
    out[0] = (int32_t)xyzz30_acc_head(ld_xyzz(in), ld_affine(in + kX), in[kX + 2 * kF] != 0, P, Rn);
    st_fq(out + 1, P);
    st_fq(out + 1 + kF, Rn);
}
PRIM_FN void pop_acc_rare(const int32_t* in, int32_t* out) {  // acc, P, Rn -> whether the tail is to run, acc
    XYZZ30 acc = ld_xyzz(in);
    out[0] = xyzz30_acc_rare(acc, ld_fq(in + kX), ld_fq(in + kX + kF)) ? 1 : 0;
    st_xyzz(out + 1, acc);
}
PRIM_FN void pop_acc_tail(const int32_t* in, int32_t* out) {  // acc, P, Rn -> acc
    XYZZ30 acc = ld_xyzz(in);
    xyzz30_acc_tail(acc, ld_fq(in + kX), ld_fq(in + kX + kF));
    st_xyzz(out, acc);
}
// (xyzz30_acc_set has no record of its own: xyzz30_acc_madd runs it for every accumulator at infinity)
// acc as it stays inside the kernel (X a raw sum of two), then as it leaves it (xyzz30_acc_settle)
PRIM_FN void st_acc_both(int32_t* out, XYZZ30 acc) {
    st_xyzz(out, acc);
    xyzz30_acc_settle(acc);
    st_xyzz(out + kX, acc);
}
PRIM_FN void pop_acc_madd(const int32_t* in, int32_t* out) {  // acc, affine point, neg -> acc unsettled, acc settled
    XYZZ30 acc = ld_xyzz(in);
    xyzz30_acc_madd(acc, ld_affine(in + kX), in[kX + 2 * kF] != 0);
    st_acc_both(out, acc);
}
PRIM_FN void pop_chain_acc_madd(const int32_t* in, int32_t* out) {  // 16 x (point, neg) -> the 16 settled partial sums
    XYZZ30 acc = xyzz30_inf();
    for (int s = 0; s < kChain; s++) {
        const int32_t* r = in + s * (2 * kF + 1);
        xyzz30_acc_madd(acc, ld_affine(r), r[2 * kF] != 0);  // the UNSETTLED accumulator feeds the next step
        XYZZ30 settled = acc;
        xyzz30_acc_settle(settled);
        st_xyzz(out + s * kX, settled);
    }
}
PRIM_FN void pop_add(const int32_t* in, int32_t* out) {
    XYZZ30 acc = ld_xyzz(in);
    xyzz30_add(acc, ld_xyzz(in + kX));
    st_xyzz(out, acc);
}
PRIM_FN void pop_add_call(const int32_t* in, int32_t* out) {
    XYZZ30 acc = ld_xyzz(in);
    const XYZZ30 b = ld_xyzz(in + kX);
#ifdef __HIPCC__
    xyzz30_add_call(&acc, &b);
#else
    xyzz30_add(acc, b);  // the call form exists on the device only
#endif
    st_xyzz(out, acc);
}
PRIM_FN void pop_dbl(const int32_t* in, int32_t* out) {
    XYZZ30 acc = ld_xyzz(in);
    xyzz30_dbl_inplace(acc);
    st_xyzz(out, acc);
}
PRIM_FN void pop_pair_classify(const int32_t* in, int32_t* out) {  // a, b, nega, negb -> kind, den
    Fq den;
    out[0] = (int32_t)pair_classify(ld_affine(in), in[4 * kF] != 0, ld_affine(in + 2 * kF), in[4 * kF + 1] != 0, den);
    st_fq(out + 1, den);
}
PRIM_FN void pop_chain_madd(const int32_t* in, int32_t* out) {  // 16 x (point, neg) -> the 16 partial sums
    XYZZ30 acc = xyzz30_inf();
    for (int s = 0; s < kChain; s++) {
        const int32_t* r = in + s * (2 * kF + 1);
        xyzz30_madd(acc, ld_affine(r), r[2 * kF] != 0);
        st_xyzz(out + s * kX, acc);
    }
}
PRIM_FN void pop_chain_add(const int32_t* in, int32_t* out) {  // 16 x XYZZ -> the 16 partial sums
    XYZZ30 acc = xyzz30_inf();
    for (int s = 0; s < kChain; s++) {
        xyzz30_add(acc, ld_xyzz(in + s * kX));
        st_xyzz(out + s * kX, acc);
    }
}
// pairs lo..hi-1 of `in` (rows a, b, nega, negb) with ONE inversion, as the accumulation kernel chains them:
// out rows (kind, x3, y3); prefix: 13 ints of scratch per pair
PRIM_FN void pop_pair_batch(const int32_t* in, int lo, int hi, int32_t* out, int32_t* prefix) {
    constexpr int kRow = 4 * kF + 2;
    Fq run = fq_one();
    for (int i = lo; i < hi; i++) {
        const int32_t* r = in + (size_t)i * kRow;
        Fq den;
        const uint32_t kind = pair_classify(ld_affine(r), r[4 * kF] != 0, ld_affine(r + 2 * kF), r[4 * kF + 1] != 0, den);
        out[(size_t)i * 27] = (int32_t)kind;
        st_fq(prefix + (size_t)i * kF, run);
        if (kind == kPairAdd || kind == kPairDouble) run = fq_mul(run, den);
    }
    Fq inv = fq_inv(run);
    for (int i = hi - 1; i >= lo; i--) {
        const int32_t* r = in + (size_t)i * kRow;
        int32_t* o = out + (size_t)i * 27;
        for (int j = 1; j < 27; j++) o[j] = 0;
        const uint32_t kind = (uint32_t)o[0];
        if (kind != kPairAdd && kind != kPairDouble) continue;
        const Affine30 a = ld_affine(r), b = ld_affine(r + 2 * kF);
        const bool nega = r[4 * kF] != 0, negb = r[4 * kF + 1] != 0;
        Fq den;
        (void)pair_classify(a, nega, b, negb, den);
        const Fq inv_den = fq_mul(inv, ld_fq(prefix + (size_t)i * kF));
        inv = fq_mul(inv, den);
        const Affine30 s = pair_sum(kind, a, nega, b, negb, inv_den);
        st_fq(o + 1, s.x);
        st_fq(o + 1 + kF, s.y);
    }
}

// ---- Fr ------------------------------------------------------------------------------------------------------------
PRIM_FN void pop_fr30_mul(const int32_t* in, int32_t* out) { st_fr(out, fr30_mul(ld_fr(in), ld_fr(in + kR9))); }
PRIM_FN void pop_fr30_norm(const int32_t* in, int32_t* out) { st_fr(out, fr30_norm(ld_fr(in))); }
PRIM_FN void pop_fr30_from_limbs(const int32_t* in, int32_t* out) {
    uint32_t l[8];
    for (int i = 0; i < 8; i++) l[i] = (uint32_t)in[i];
    st_fr(out, fr30_from_limbs(l));
}
PRIM_FN void pop_fr30_to_limbs(const int32_t* in, int32_t* out) {
    uint32_t l[8];
    fr30_to_limbs(ld_fr(in), l);
    for (int i = 0; i < 8; i++) out[i] = (int32_t)l[i];
}
PRIM_FN void pop_fr30_abs_to_limbs(const int32_t* in, int32_t* out) {  // -> |v| (8 words), sign
    uint32_t l[8];
    out[8] = fr30_abs_to_limbs(ld_fr(in), l) ? 1 : 0;
    for (int i = 0; i < 8; i++) out[i] = (int32_t)l[i];
}
PRIM_FN void pop_fr30_inv(const int32_t* in, int32_t* out) { st_fr(out, fr30_inv(ld_fr(in))); }

}  // namespace prim

// one lane (device) or one loop iteration (host) per record
#define PRIM_FQ_OPS(X)                                                                                           \
    X(fq_mul, 26, 13) X(fq_sqr, 13, 13) X(fq_mul_sub, 52, 13) X(fq_norm, 13, 13) X(fq_norm_wide, 13, 13)          \
    X(fq_neg, 13, 13) X(fq_cneg, 14, 13) X(fq_canon_digits, 13, 13) X(fq_is_zero, 13, 1) X(fq_from_u32x12, 12, 13) \
    X(fq_to_u32x12, 13, 12) X(fq_canon_half, 13, 14) X(fq_inv, 13, 13) X(madd, 79, 52) X(add, 104, 52)            \
    X(add_call, 104, 52) X(dbl, 52, 52) X(pair_classify, 54, 14) X(chain_madd, 16 * 27, 16 * 52)                   \
    X(chain_add, 16 * 52, 16 * 52) X(fq_mul_minus, 39, 13) X(fq_mul_plus, 39, 13) X(fq_sqr_minus, 26, 13)         \
    X(fq_maybe_zero, 13, 1) X(acc_head, 79, 27) X(acc_rare, 78, 53) X(acc_tail, 78, 52) X(acc_madd, 79, 104)       \
    X(chain_acc_madd, 16 * 27, 16 * 52)
#define PRIM_FR_OPS(X)                                                                                     \
    X(fr30_mul, 18, 9) X(fr30_norm, 9, 9) X(fr30_from_limbs, 8, 9) X(fr30_to_limbs, 9, 8) X(fr30_abs_to_limbs, 9, 9) \
    X(fr30_inv, 9, 9)
