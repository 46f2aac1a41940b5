// Host build of the accumulation kernel's fused arithmetic for tests/test_field30_fused.py (plain g++; the headers are
// __host__ __device__ code): fq_mul_minus / fq_mul_plus / fq_sqr_minus (csrc/field30.hip.h) and the mixed addition built
// on them (xyzz30_acc_*, csrc/g1_30.hip.h) over a C ABI.  Test infrastructure only.
// With -DF30_FUSED_MAIN the file is a stand-alone program (for a build under -fsanitize=address,undefined): it drives the
// same entry points through the contract's edges and chains of additions and checks them against the unfused routines.
#include <stdint.h>
#include <string.h>

#include "../../kzg_poly_commit_exploration_amd/csrc/g1_30.hip.h"

using namespace kzg;

static Fq fq_of(const int32_t* a) {
    Fq x;
    memcpy(x.d, a, sizeof x.d);
    return x;
}
static XYZZ30 xyzz_of(const int32_t* a) {
    XYZZ30 r;
    r.X = fq_of(a);
    r.Y = fq_of(a + 13);
    r.ZZ = fq_of(a + 26);
    r.ZZZ = fq_of(a + 39);
    return r;
}
static void xyzz_to(int32_t* a, const XYZZ30& r) {
    memcpy(a, r.X.d, sizeof r.X.d);
    memcpy(a + 13, r.Y.d, sizeof r.Y.d);
    memcpy(a + 26, r.ZZ.d, sizeof r.ZZ.d);
    memcpy(a + 39, r.ZZZ.d, sizeof r.ZZZ.d);
}

extern "C" {

void f30f_mul(const int32_t* a, const int32_t* b, int32_t* r) {
    const Fq z = fq_mul(fq_of(a), fq_of(b));
    memcpy(r, z.d, sizeof z.d);
}
void f30f_sqr(const int32_t* a, int32_t* r) {
    const Fq z = fq_sqr(fq_of(a));
    memcpy(r, z.d, sizeof z.d);
}
void f30f_mul_minus(const int32_t* a, const int32_t* b, const int32_t* c, int32_t* r) {
    const Fq z = fq_mul_minus(fq_of(a), fq_of(b), fq_of(c));
    memcpy(r, z.d, sizeof z.d);
}
void f30f_mul_plus(const int32_t* a, const int32_t* b, const int32_t* c, int32_t* r) {
    const Fq z = fq_mul_plus(fq_of(a), fq_of(b), fq_of(c));
    memcpy(r, z.d, sizeof z.d);
}
void f30f_sqr_minus(const int32_t* a, const int32_t* c, int32_t* r) {
    const Fq z = fq_sqr_minus(fq_of(a), fq_of(c));
    memcpy(r, z.d, sizeof z.d);
}
int f30f_maybe_zero(const int32_t* a) { return fq_maybe_zero(fq_of(a)) ? 1 : 0; }
// acc: 52 digits (X, Y, ZZ, ZZZ)
void f30f_acc_madd(int32_t* acc, const int32_t* px, const int32_t* py, int neg) {
    XYZZ30 a = xyzz_of(acc);
    Affine30 p;
    p.x = fq_of(px);
    p.y = fq_of(py);
    xyzz30_acc_madd(a, p, neg != 0);
    xyzz_to(acc, a);
}
void f30f_madd(int32_t* acc, const int32_t* px, const int32_t* py, int neg) {  // the unfused mixed addition
    XYZZ30 a = xyzz_of(acc);
    Affine30 p;
    p.x = fq_of(px);
    p.y = fq_of(py);
    xyzz30_madd(a, p, neg != 0);
    xyzz_to(acc, a);
}
void f30f_acc_settle(int32_t* acc) {
    XYZZ30 a = xyzz_of(acc);
    xyzz30_acc_settle(a);
    xyzz_to(acc, a);
}
void f30f_add(int32_t* acc, const int32_t* b) {  // the tree kernels' general addition, a reader of settled accumulators
    XYZZ30 a = xyzz_of(acc);
    xyzz30_add(a, xyzz_of(b));
    xyzz_to(acc, a);
}
// a == b as group elements (both finite or both at infinity): X1 ZZ2 == X2 ZZ1 and Y1 ZZZ2 == Y2 ZZZ1
int f30f_same_point(const int32_t* pa, const int32_t* pb) {
    const XYZZ30 a = xyzz_of(pa), b = xyzz_of(pb);
    if (xyzz30_is_inf(a) || xyzz30_is_inf(b)) return xyzz30_is_inf(a) && xyzz30_is_inf(b);
    const Fq dx = fq_norm(fq_sub_raw(fq_mul(a.X, b.ZZ), fq_mul(b.X, a.ZZ)));
    const Fq dy = fq_norm(fq_sub_raw(fq_mul(a.Y, b.ZZZ), fq_mul(b.Y, a.ZZZ)));
    return fq_is_zero(dx) && fq_is_zero(dy);
}

// ---- the zero pre-test's false positives through k_bucket_accumulate itself (tests/accum_false_positives.py) ----------------
// the level-0 table digits of blst affine words (12 x u32 per coordinate, Montgomery 2^384, below 2 p), as
// k_affine96_to_table (srs_io.hip) stores them: the same two calls, so the same digits bit for bit
void f30f_table_digits(const uint32_t* words, int n, int32_t* out) {
    for (int i = 0; i < n; i++) {
        const Fq z = fq_mul(fq_from_u32x12(words + 12 * (size_t)i), fq_one());
        memcpy(out + 13 * (size_t)i, z.d, sizeof z.d);
    }
}
// per coordinate x (13 digits): the low 30 bits of x * one -- the U2 of xyzz30_acc_head when the accumulator was just set from
// a point (ZZ = fq_one_cold()) -- and of x itself, the X that is subtracted then
void f30f_low_bits(const int32_t* x, int n, uint32_t* lo_mul, uint32_t* lo_x) {
    const Fq one = fq_one_cold();
    for (int i = 0; i < n; i++) {
        lo_mul[i] = (uint32_t)fq_mul(fq_of(x + 13 * (size_t)i), one).d[0] & (uint32_t)kQMask;
        lo_x[i] = (uint32_t)x[13 * (size_t)i] & (uint32_t)kQMask;
    }
}
// xyzz30_acc_set with the point a (x, y: 26 digits), then xyzz30_acc_head with b: the code; *p_is_zero: whether P is a
// multiple of p (code == kAccMaybeEqual with P != 0 is the pre-test's false positive)
int f30f_set_then_head(const int32_t* a, int nega, const int32_t* b, int negb, int* p_is_zero) {
    XYZZ30 acc = xyzz30_inf();
    Affine30 pa, pb;
    pa.x = fq_of(a);
    pa.y = fq_of(a + 13);
    pb.x = fq_of(b);
    pb.y = fq_of(b + 13);
    xyzz30_acc_set(acc, pa, nega != 0);
    Fq P, Rn;
    const uint32_t code = xyzz30_acc_head(acc, pb, negb != 0, P, Rn);
    *p_is_zero = fq_is_zero(P) ? 1 : 0;
    return (int)code;
}

}  // extern "C"

#ifdef F30_FUSED_MAIN
#include <stdio.h>

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}
static int fails = 0;
#define CHECK(c)                                             \
    do {                                                     \
        if (!(c)) {                                          \
            printf("FAILED line %d: %s\n", __LINE__, #c);    \
            fails++;                                         \
        }                                                    \
    } while (0)

// the generator of G1 in Montgomery (2^390) balanced digits
static const int32_t GX[13] = {349286428, 339185917, -184560077, 465995769, -31315776, 83389090, -376571528,
                               -299317673, 456582938, -19687443, -278352466, 157827279, 536252};
static const int32_t GY[13] = {-103681652, 218354957, 284572517, -231624520, -293097554, 49081114, -444301104,
                               -235775134, 142962186, 535793470, 439681483, 493751000, 1503689};

static bool strict(const int32_t* r) {
    for (int i = 0; i < 12; i++)
        if (r[i] < -(1 << 29) || r[i] >= (1 << 29)) return false;
    return true;
}
// r + sign * c == ref as integers, digit by digit after an exact carry pass (all values are small multiples of p)
static bool same_integer(const int32_t* r, const int32_t* c, int sign, const int32_t* ref) {
    int64_t carry = 0;
    for (int i = 0; i < 13; i++) {
        const int64_t t = (int64_t)r[i] - (int64_t)sign * c[i] - ref[i] + carry;  // r = ref + sign c
        if (i < 12) {
            if (t & ((1 << 30) - 1)) return false;
            carry = t >> 30;
        } else if (t != 0) {
            return false;
        }
    }
    return true;
}

int main() {
    // products: random digits and the contract's edges
    const int32_t big = (1 << 29) + 4;
    for (int it = 0; it < 4000; it++) {
        int32_t a[13], b[13], c[13], r[13], ref[13];
        const int mode = it & 7;
        for (int i = 0; i < 12; i++) {
            a[i] = (int32_t)(rnd() & ((1u << 30) - 1)) - (1 << 29);
            b[i] = (int32_t)(rnd() & ((1u << 30) - 1)) - (1 << 29);
            c[i] = (int32_t)(rnd() & ((1u << 30) - 1)) - (1 << 29);
            if (mode == 1) a[i] = (rnd() & 1) ? big : -big, b[i] = (rnd() & 1) ? big : -big;
            if (mode == 2) c[i] = (rnd() & 1) ? 4 * ((1 << 29) - 1) : -4 * (1 << 29);  // a raw sum of four
            if (mode == 3) a[i] = (rnd() & 1) ? 2 * big : -2 * big, b[i] = (rnd() & 1) ? big : -big;  // a raw sum of two
        }
        a[12] = (int32_t)(rnd() & 0xfffff) - (1 << 19);
        b[12] = (int32_t)(rnd() & 0xfffff) - (1 << 19);
        c[12] = (int32_t)(rnd() & 0xfffff) - (1 << 19);
        f30f_mul(a, b, ref);
        f30f_mul_minus(a, b, c, r);
        CHECK(strict(r) && same_integer(r, c, -1, ref));
        f30f_mul_plus(a, b, c, r);
        CHECK(strict(r) && same_integer(r, c, 1, ref));
        if (mode != 3) {
            f30f_sqr(a, ref);
            f30f_sqr_minus(a, c, r);
            CHECK(strict(r) && same_integer(r, c, -1, ref));
        }
    }
    // group law: the fused addition against the unfused one, through infinity, doubling and cancellation
    int32_t zero[13] = {0};
    int32_t a_new[52] = {0}, a_old[52] = {0};
    // G, G (doubling), -G, -G, -G (through 2G - G, G - G = infinity, then -G), infinity point, then a long chain
    const int script_neg[] = {0, 0, 1, 1, 1, 0, 0, 0};
    for (int s = 0; s < 8; s++) {
        f30f_acc_madd(a_new, GX, GY, script_neg[s]);
        f30f_madd(a_old, GX, GY, script_neg[s]);
        CHECK(f30f_same_point(a_new, a_old));
    }
    f30f_acc_madd(a_new, zero, zero, 0);
    f30f_madd(a_old, zero, zero, 0);
    CHECK(f30f_same_point(a_new, a_old));
    for (int it = 0; it < 200; it++) {
        // a biased walk (two steps up, one down) never returns to infinity for long and meets k G + G = doubling at k = 1
        const int neg = (it % 3) == 2;
        f30f_acc_madd(a_new, GX, GY, neg);
        f30f_madd(a_old, GX, GY, neg);
        CHECK(f30f_same_point(a_new, a_old));
        for (int i = 0; i < 12; i++) CHECK(a_new[i] >= -(1 << 30) && a_new[i] < (1 << 30));
        for (int i = 13; i < 52; i++)
            if (i % 13 != 12) CHECK(a_new[i] >= -big && a_new[i] <= big);
    }
    int32_t settled[52];
    memcpy(settled, a_new, sizeof settled);
    f30f_acc_settle(settled);
    for (int i = 0; i < 12; i++) CHECK(settled[i] >= -big && settled[i] <= big);
    CHECK(f30f_same_point(settled, a_old));
    int32_t sum_new[52], sum_old[52];
    memcpy(sum_new, settled, sizeof settled);
    memcpy(sum_old, a_old, sizeof a_old);
    f30f_add(sum_new, settled);  // equal operands: the doubling branch squares X
    f30f_add(sum_old, a_old);
    CHECK(f30f_same_point(sum_new, sum_old));
    // the exports of the false-positive search: table digits of stored words, their low bits, "set, then head"
    {
        uint32_t words[3 * 12];
        int32_t dig[3 * 13], a[26], b[26];
        uint32_t lo_mul[3], lo_x[3];
        for (int i = 0; i < 3 * 12; i++) words[i] = (i % 12 == 11) ? (rnd() & 0x0fffffffu) : rnd();  // below 2^380 < p
        f30f_table_digits(words, 3, dig);
        for (int i = 0; i < 3; i++) CHECK(strict(dig + 13 * i));
        f30f_low_bits(dig, 3, lo_mul, lo_x);
        for (int i = 0; i < 3; i++) CHECK(lo_x[i] == ((uint32_t)dig[13 * i] & 0x3fffffffu) && lo_mul[i] < (1u << 30));
        memcpy(a, GX, sizeof GX);
        memcpy(a + 13, GY, sizeof GY);
        memcpy(b, a, sizeof a);
        int zero_p = 0;
        CHECK(f30f_set_then_head(a, 0, b, 0, &zero_p) == (int)kAccMaybeEqual && zero_p == 1);  // G, then G
        CHECK(f30f_set_then_head(a, 1, b, 0, &zero_p) == (int)kAccMaybeEqual && zero_p == 1);  // -G, then G
        memset(a_new, 0, sizeof a_new);
        f30f_acc_madd(a_new, GX, GY, 0);
        f30f_acc_madd(a_new, GX, GY, 0);  // 2 G
        memcpy(b, a_new, 13 * 4);        // its X and Y as an "affine" pair of digits: another x than G's
        memcpy(b + 13, a_new + 13, 13 * 4);
        const int code = f30f_set_then_head(a, 0, b, 0, &zero_p);
        CHECK((code == 0 && zero_p == 0) || code == (int)kAccMaybeEqual);
    }
    if (fails) printf("%d checks failed\n", fails);
    else printf("all checks passed\n");
    return fails ? 1 : 0;
}
#endif
