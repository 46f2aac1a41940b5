// Host build of the product cores of csrc/field30.hip.h (fq_mul, fq_sqr, fq_mul_sub, fq_mul_minus, fq_mul_plus,
// fq_sqr_minus) beside their definitions of before the single-chain columns (field30_parent_products.h), over a C ABI:
// the case rows of tests/test_field30_columns.py and tests/test_accum_columns_gpu.py, and both sets of results.
// Test infrastructure only.
// With -DF30_COLUMNS_MAIN the file is a stand-alone program (built under -fsanitize=undefined,address by
// tests/test_field30_columns.py): every function on 10^5 random rows and on the edges of its contract, today's digits
// against the earlier definition's, digit for digit.
#include <stdint.h>
#include <string.h>

#include "field30_parent_products.h"

using kzg::Fq;
using kzg::kQ;

namespace {

enum Op { kMul = 0, kSqr, kMulSub, kMulMinus, kMulPlus, kSqrMinus, kOps };
constexpr int kRow = 4 * kQ;  // a, b, c, d
constexpr int32_t kHalf = 1 << 29;
constexpr int32_t kWeak = (1 << 29) + 4;  // |digit| behind fq_norm
constexpr int32_t kCTop = 0x7fffffff;     // |digit| of a value taken into the carry pass

Fq fq_of(const int32_t* a) {
    Fq x;
    memcpy(x.d, a, sizeof x.d);
    return x;
}

template <class MUL, class SQR, class MULSUB, class MINUS, class PLUS, class SQRMINUS>
void apply(int op, const int32_t* row, int32_t* out, MUL mul, SQR sqr, MULSUB mulsub, MINUS minus, PLUS plus, SQRMINUS sqrminus) {
    const Fq a = fq_of(row), b = fq_of(row + kQ), c = fq_of(row + 2 * kQ), d = fq_of(row + 3 * kQ);
    Fq r;
    switch (op) {
        case kMul: r = mul(a, b); break;
        case kSqr: r = sqr(a); break;
        case kMulSub: r = mulsub(a, b, c, d); break;
        case kMulMinus: r = minus(a, b, c); break;
        case kMulPlus: r = plus(a, b, c); break;
        default: r = sqrminus(a, c); break;
    }
    memcpy(out, r.d, sizeof r.d);
}

uint64_t rng_state;
uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}
int32_t sign() { return (rnd() & 1) ? 1 : -1; }
int32_t balanced_digit() { return (int32_t)(rnd() & ((1u << 30) - 1)) - kHalf; }
int32_t top_digit() { return (int32_t)(rnd() & 0x1ffffff) - (1 << 24); }  // |v| < 2^385

void random_value(int32_t* x) {
    for (int i = 0; i < kQ - 1; i++) x[i] = balanced_digit();
    x[kQ - 1] = top_digit();
}
void all_digits(int32_t* x, int32_t mag, int pattern) {  // pattern 0: +, 1: -, 2: alternating, 3: random signs
    for (int i = 0; i < kQ - 1; i++) x[i] = mag * (pattern == 0 ? 1 : pattern == 1 ? -1 : pattern == 2 ? ((i & 1) ? 1 : -1) : sign());
    x[kQ - 1] = top_digit();
}
void raw_sum_of_two(int32_t* x) {  // digit-wise sum of two weakly normalised values, the extremes included
    int32_t u[kQ], v[kQ];
    const int mode = rnd() % 3;
    if (mode == 0) {
        random_value(u);
        random_value(v);
    } else {
        all_digits(u, kWeak, mode == 1 ? 3 : 0);
        memcpy(v, u, sizeof u);
    }
    for (int i = 0; i < kQ; i++) x[i] = u[i] + v[i];
}
void multiple_of_p(int32_t* x, int k) {  // k p in balanced digits
    Fq kp;
    for (int i = 0; i < kQ; i++) kp.d[i] = k * kzg::fq_pd(i);
    kp = kzg::fq_canon_digits(kp);
    memcpy(x, kp.d, sizeof kp.d);
}

// row `i` of function `op`: the edges first, random rows behind them
constexpr int kEdgeRows = 256;
void make_row(int op, int i, int32_t* row) {
    rng_state = 0x9e3779b97f4a7c15ull ^ ((uint64_t)(op + 1) << 40) ^ (uint64_t)(i + 1) * 0x2545f4914f6cdd1dull;
    rnd();
    int32_t *a = row, *b = row + kQ, *c = row + 2 * kQ, *d = row + 3 * kQ;
    for (int f = 0; f < 4; f++) random_value(row + f * kQ);
    const bool fused = op == kMulMinus || op == kMulPlus || op == kSqrMinus;
    const bool raw_ok = op == kMul || op == kMulMinus || op == kMulPlus;  // one multiplicand may be a raw sum of two
    if (i >= kEdgeRows) {
        if (fused && (i & 3) == 0)  // c a raw sum of up to four
            for (int t = 0; t < kQ; t++) c[t] = (t < kQ - 1 ? balanced_digit() + balanced_digit() + balanced_digit() : 0) + c[t];
        if (raw_ok && (i & 7) == 1) raw_sum_of_two((i & 8) ? a : b);
        return;
    }
    const int group = i >> 4, v = i & 15;
    switch (group) {
        case 0:  // every digit at +-2^29
            all_digits(a, kHalf, v & 3);
            all_digits(b, kHalf, (v >> 2) & 3);
            all_digits(d, kHalf, v & 3);
            if (!fused) all_digits(c, kHalf, (v >> 2) & 3);
            break;
        case 1:  // every digit at +-(2^29 + 4)
            all_digits(a, kWeak, v & 3);
            all_digits(b, kWeak, (v >> 2) & 3);
            all_digits(d, kWeak, (v >> 2) & 3);
            if (!fused) all_digits(c, kWeak, v & 3);
            break;
        case 2:  // the same against the other sign pattern in the subtracted product
            all_digits(a, kWeak, v & 3);
            all_digits(b, kWeak, v & 3);
            all_digits(c, fused ? kCTop : kWeak, (v >> 2) & 3);
            all_digits(d, kWeak, ((v >> 2) + 1) & 3);
            break;
        case 3:  // the signs of p's own digits: the largest m p part
            for (int t = 0; t < kQ - 1; t++) a[t] = kzg::fq_pd(t) >= 0 ? kWeak : -kWeak, b[t] = (v & 1) ? kWeak : -kWeak;
            a[kQ - 1] = b[kQ - 1] = 0;
            if (fused) all_digits(c, kCTop, v >> 2);
            break;
        case 4:  // one multiplicand a raw sum of two (where the contract takes one), the other at the edge
            if (raw_ok) {
                raw_sum_of_two((v & 1) ? a : b);
                all_digits((v & 1) ? b : a, kHalf, v >> 2);
            } else {
                all_digits(a, kWeak, v >> 2);
            }
            break;
        case 5:  // subtrahends at +-(2^31 - 1)
            all_digits(c, fused ? kCTop : kWeak, v & 3);
            if (v & 4) all_digits(a, kWeak, v >> 2), all_digits(b, kWeak, (v >> 1) & 3);
            break;
        case 6:  // 0, +-p, +-3p in every place
        case 7: {
            static const int ks[5] = {0, 1, -1, 3, -3};
            multiple_of_p(a, ks[v % 5]);
            if (group == 7 || (v & 1)) multiple_of_p(b, ks[(v / 5 + v) % 5]);
            if (v & 2) multiple_of_p(c, ks[(v + 2) % 5]);
            if (v & 4) multiple_of_p(d, ks[(v + 3) % 5]);
            break;
        }
        default: {  // mixtures: each operand drawn from the forms above
            int32_t* f[4] = {a, b, c, d};
            for (int t = 0; t < 4; t++) {
                const int32_t top = (t == 2 && fused) ? kCTop : kWeak;
                switch (rnd() % 5) {
                    case 0: all_digits(f[t], top, rnd() & 3); break;
                    case 1: all_digits(f[t], kHalf, rnd() & 3); break;
                    case 2: multiple_of_p(f[t], (int)(rnd() % 7) - 3); break;
                    case 3:
                        if ((t == 0 && raw_ok) || (t == 2 && fused)) raw_sum_of_two(f[t]);
                        break;
                    default: break;
                }
            }
            break;
        }
    }
}

}  // namespace

extern "C" {

int f30c_ops() { return kOps; }
int f30c_edge_rows() { return kEdgeRows; }
// rows first .. first + n - 1 of function `op`: 52 ints each (a, b, c, d; what a function does not take is ignored)
void f30c_rows(int op, int first, int n, int32_t* rows) {
    for (int i = 0; i < n; i++) make_row(op, first + i, rows + (size_t)i * kRow);
}
// 13 ints per row: today's functions
void f30c_run(int op, const int32_t* rows, int n, int32_t* out) {
    for (int i = 0; i < n; i++)
        apply(op, rows + (size_t)i * kRow, out + (size_t)i * kQ, kzg::fq_mul, kzg::fq_sqr, kzg::fq_mul_sub, kzg::fq_mul_minus,
              kzg::fq_mul_plus, kzg::fq_sqr_minus);
}
// ... and the definitions of before
void f30c_run_parent(int op, const int32_t* rows, int n, int32_t* out) {
    for (int i = 0; i < n; i++)
        apply(op, rows + (size_t)i * kRow, out + (size_t)i * kQ, kzg_parent::fq_mul, kzg_parent::fq_sqr, kzg_parent::fq_mul_sub,
              kzg_parent::fq_mul_minus, kzg_parent::fq_mul_plus, kzg_parent::fq_sqr_minus);
}

}  // extern "C"

#ifdef F30_COLUMNS_MAIN
#include <stdio.h>

int main() {
    static const char* names[kOps] = {"fq_mul", "fq_sqr", "fq_mul_sub", "fq_mul_minus", "fq_mul_plus", "fq_sqr_minus"};
    const int n = kEdgeRows + 100000;
    int bad = 0;
    for (int op = 0; op < kOps; op++) {
        int differ = 0;
        for (int i = 0; i < n; i++) {
            int32_t row[kRow], now[kQ], before[kQ];
            f30c_rows(op, i, 1, row);
            f30c_run(op, row, 1, now);
            f30c_run_parent(op, row, 1, before);
            if (memcmp(now, before, sizeof now) != 0) {
                if (!differ) printf("%s: row %d differs from the earlier definition\n", names[op], i);
                differ++;
            }
        }
        printf("%s: %d rows, %d differ\n", names[op], n, differ);
        bad += differ;
    }
    printf(bad ? "FAILED\n" : "all rows identical\n");
    return bad ? 1 : 0;
}
#endif
